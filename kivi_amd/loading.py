"""Between a checkpoint directory and a filled model: config.json and its save_quantized tags, a loader that
routes the tensors of one *.safetensors file at a time into a built model, one ledger of what is still owed, and save_quantized.

The names taken are those of the Hugging Face checkpoints.  For the sparse blocks three spellings: Mixtral's
`block_sparse_moe.gate.weight` and `block_sparse_moe.experts.{e}.w1 / w3 / w2.weight` (gate / up / down), Qwen3-MoE's
`mlp.experts.{e}.gate_proj / up_proj / down_proj.weight`, and the fused names of transformers 5 (`mlp.experts.gate_up_proj` /
`.down_proj`, also under `block_sparse_moe.`).  kivi_amd/llama.py keeps the family table, make_config and the construction of the
model; kivi_amd/checkpoint.py is something else, the checkpoint of a KV cache."""
from __future__ import annotations

import glob
import json
import os
import re

import torch
import torch.nn as nn

from . import wfp8, wquant
from .moe import Fp8Experts, QuantExperts, SparseMoeBlock

_TAGS = ("kivi_weight_layout", "kivi_weight_bits", "kivi_weight_group", "kivi_expert_bits", "kivi_expert_group")
_EXPERT_NAME = re.compile(r"^(.*\.)(?:block_sparse_moe|mlp)\.experts\.(\d+)\.(w1|w2|w3|gate_proj|up_proj|down_proj)"
                          r"\.(weight|weight_scale_inv)$")
_EXPERT_PART = {"w1": "gate", "gate_proj": "gate", "w3": "up", "up_proj": "up", "w2": "down", "down_proj": "down"}
_STACK_PARTS = {"gate_up_proj": ("gate", "up"), "down_proj": ("down",)}
_TRIPLE = ("qweight", "scales", "mins")
_FP8_PAIR = ("weight", "weight_scale_inv")
_FP8_STACKS = {"gate_up_proj": ("gate_up_proj", "gate_up", "weight"), "gate_up_proj_scale_inv": ("gate_up_proj", "gate_up", "scale"),
               "down_proj": ("down_proj", "down", "weight"), "down_proj_scale_inv": ("down_proj", "down", "scale")}
_FP8_EXPERT_LEAVES = {"gate": "gate_proj", "up": "up_proj", "down": "down_proj"}   # the per-expert names save_quantized writes
_FP8_ACTIVATION = ("input_scale", "activation_scale")      # tensors of a static activation scheme: never served


def _fp8_config(path: str, q: dict, kivi: dict) -> None:
    """A checkpoint's `quantization_config` block with quant_method "fp8" (transformers' FineGrainedFP8Config) -> fp8_weights and the
    skip list among the keywords of make_config.  What the kernels do not serve is refused by name."""
    fmt = q.get("fmt", "e4m3")
    if fmt != "e4m3":
        raise ValueError(f"{path}: quantization_config.fmt {fmt!r}: only e4m3 FP8 weights are served")
    if q.get("scale_fmt") not in (None, "float"):
        raise ValueError(f"{path}: quantization_config.scale_fmt {q['scale_fmt']!r}: only float (fp32) scales are served, not ue8m0")
    block = q.get("weight_block_size")
    if block is not None and list(block) != [wfp8.BLOCK, wfp8.BLOCK]:
        raise ValueError(f"{path}: quantization_config.weight_block_size {block!r}: only [128, 128] blocks and per-tensor scales "
                         f"(null) are served")
    scheme = q.get("activation_scheme", "dynamic")
    if scheme != "dynamic":     # "dynamic" is accepted and not applied: activations stay 16-bit
        raise ValueError(f"{path}: quantization_config.activation_scheme {scheme!r}: static activation scales are not served")
    kivi["fp8_weights"] = True
    if q.get("modules_to_not_convert"):     # added to a list the caller gave: a module either names stays dense
        kivi["fp8_skip_modules"] = list(kivi.get("fp8_skip_modules") or []) + list(q["modules_to_not_convert"])


def read_config(path: str, kivi: dict) -> dict:
    """config.json of the directory `path` without the tags of save_quantized.  Where the layout tag is there, the bits and groups
    it was written with go into `kivi` (the keywords of make_config); another layout than this version's raises.  A
    `quantization_config` block of quant_method "fp8"  is validated, becomes fp8_weights=True plus the skip list
    in `kivi`, and is stripped as well."""
    d = json.load(open(os.path.join(path, "config.json")))
    q = d.get("quantization_config")
    if isinstance(q, dict) and q.get("quant_method") == "fp8":
        _fp8_config(path, q, kivi)
        d = {k: v for k, v in d.items() if k != "quantization_config"}
    if "kivi_weight_layout" in d:                           # a checkpoint of save_quantized: loaded as it is, nothing re-quantised
        if d["kivi_weight_layout"] != wquant.LAYOUT:
            raise ValueError(f"{path}: weight layout {d['kivi_weight_layout']!r} is not one this version reads ({wquant.LAYOUT!r})")
        if d.get("kivi_weight_bits") is not None:
            kivi["weight_bits"], kivi["weight_group"] = d["kivi_weight_bits"], d["kivi_weight_group"]
        if d.get("kivi_expert_bits") is not None:
            kivi["expert_bits"], kivi["expert_group"] = d["kivi_expert_bits"], d["kivi_expert_group"]
        d = {k: v for k, v in d.items() if k not in _TAGS}
    return d


class CheckpointLoader:
    """take(tensors) for the {name: tensor} of every file, in any order, then finish().  A name goes one of four ways:
      a per-expert piece    copied into its rows of the block's dense stack, or quantised -- from its image in `dtype` -- into the
                            expert's slab of a QuantExperts: no second copy of the experts is assembled;
      a fused expert stack  quantised expert by expert where the block holds a QuantExperts (a dense block takes it as any tensor);
      a QuantLinear weight  cast to `dtype` on the module's device and packed into its buffers (section 30), as
                            QuantLinear.from_linear on the loaded model would;
      an FP8 expert tensor  (section 36; the block holds an Fp8Experts, `fp8_experts=True`) per expert -- `...experts.{e}.<proj>.weight`
                            as float8_e4m3fn, `.weight_scale_inv` as fp32 -- or fused (`experts.gate_up_proj`, `.down_proj`, and
                            their `_scale_inv`): checked and copied into the expert's slab as it is, each half filling its own
                            key's slots, from any file in any order; a 16-bit expert weight is quantised and fills both halves.
                            Without the flag such a tensor is refused;
      an Fp8Linear's pair   (section 35) a float8_e4m3fn `weight` is checked for NaN bytes and copied as bytes, a `weight_scale_inv`
                            copied as bits (a per-tensor scalar expanded), each filling its own key, in any order and from any
                            file; a 16-bit `weight` is quantised on the module's device and fills both;
      an FP8 pair of a dense linear   (a shape the kernels do not serve, a module of `modules_to_not_convert`) the one case that
                            holds a tensor across files: the first of `weight` / `weight_scale_inv` waits in `pending` for the
                            other, then the pair is dequantised in torch into the parameter; until then its key stays owed;
      any other             `block_sparse_moe.` spelled `mlp.`, then model.load_state_dict(strict=False) over the file's remainder:
                            a shape that does not fit raises there, a name nothing takes ends in `unexpected`, a tensor that comes
                            again is written again.
    The ledger `owed`: state_dict key -> the slots nothing has filled yet.  A key is one slot; the key of an expert stack -- the
    dense parameter, each of a 4-bit stack's three buffers, or each of an FP8 stack's two -- is one slot per (expert, part), part in gate / up / down, since
    only a set can tell a repeated piece from a missing one.  The tied lm_head.weight owes nothing.  But for that
    waiting half of an FP8 pair nothing here keeps a tensor of a file: it dies with the caller's dict."""

    def __init__(self, model: nn.Module, dtype=torch.float16):
        self.model, self.dtype = model, dtype
        self.unexpected = []
        self.linears = {n: m for n, m in model.named_modules() if isinstance(m, wquant.QuantLinear)}
        self.fp8 = {n: m for n, m in model.named_modules() if isinstance(m, wfp8.Fp8Linear)}
        self.dense = {n: m for n, m in model.named_modules() if isinstance(m, nn.Linear)}
        self.pending = {}           # dense linear -> {"weight" / "weight_scale_inv": tensor}: an FP8 pair waiting for its other half
        blocks = {f"{n}.experts": m for n, m in model.named_modules() if isinstance(m, SparseMoeBlock)}
        self.experts = {owner: m.experts for owner, m in blocks.items()}
        tied = getattr(model.config, "tie_word_embeddings", False)
        self.owed = {k: {None} for k in model.state_dict() if not (tied and k == "lm_head.weight")}
        for owner, m in blocks.items():
            for stack, parts in _STACK_PARTS.items():
                for key in self._keys(owner, stack):
                    self.owed[key] = {(e, p) for e in range(m.num_experts) for p in parts}

    def _keys(self, owner: str, stack: str):
        """The state_dict keys behind the stack `stack` (gate_up_proj / down_proj) of the experts module `owner`."""
        if isinstance(self.experts[owner], QuantExperts):
            return [f"{owner}.{stack}.{b}" for b in _TRIPLE]
        if isinstance(self.experts[owner], Fp8Experts):
            return [f"{owner}.{stack}", f"{owner}.{stack}_scale_inv"]
        return [f"{owner}.{stack}"]

    def _fill(self, keys, slots=None) -> None:
        for k in keys:
            if k in self.owed:
                self.owed[k] = set() if slots is None else self.owed[k] - slots

    def take(self, tensors: dict) -> None:
        rest = {}
        for name, t in tensors.items():
            self._refuse_unserved_fp8(name, t)
            m = _EXPERT_NAME.match(name)
            if m is not None:
                owner = f"{m.group(1)}mlp.experts"
                if isinstance(self.experts.get(owner), Fp8Experts):
                    self._take_fp8_piece(name, owner, int(m.group(2)), _EXPERT_PART[m.group(3)], m.group(4), t)
                elif owner in self.experts and m.group(4) == "weight":
                    self._take_piece(name, owner, int(m.group(2)), _EXPERT_PART[m.group(3)], t)
                else:
                    rest[name] = t                          # load_state_dict reports the name as unexpected
                continue
            new = name.replace(".block_sparse_moe.", ".mlp.")
            owner, _, leaf = new.rpartition(".")
            if leaf in _FP8_STACKS and isinstance(self.experts.get(owner), Fp8Experts):
                self._take_fp8_fused(name, owner, leaf, t)
                continue
            if self._take_fp8(new, owner, leaf, t):
                continue
            if leaf in _STACK_PARTS and isinstance(self.experts.get(owner), QuantExperts):
                self._take_fused(name, owner, leaf, t)
            elif leaf == "weight" and owner in self.linears:
                lin = self.linears[owner]
                lin.pack_(t.to(device=lin.qweight.device, dtype=self.dtype), new)
                self._fill(f"{owner}.{b}" for b in _TRIPLE)
            else:
                rest[new] = t
        if rest:
            _, unexpected = self.model.load_state_dict(rest, strict=False)
            self.unexpected += unexpected
            self._fill(rest.keys() - set(unexpected))

    def _fp8_experts_of(self, name: str):
        """The Fp8Experts module the tensor `name` belongs to, or None."""
        m = _EXPERT_NAME.match(name)
        owner = f"{m.group(1)}mlp.experts" if m is not None else name.replace(".block_sparse_moe.", ".mlp.").rpartition(".")[0]
        ex = self.experts.get(owner)
        return ex if isinstance(ex, Fp8Experts) else None

    def _refuse_unserved_fp8(self, name: str, t: torch.Tensor) -> None:
        """ValueError, by name, for what of the FP8 format nothing here serves: experts of a model built without `fp8_experts`,
        static activation scales, e5m2."""
        leaf = name.rpartition(".")[2]
        if ".experts." in name and (t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2) or leaf.endswith("_scale_inv")) \
                and self._fp8_experts_of(name) is None:
            raise ValueError(f"{name}: FP8 experts are not served (the attention projections and the dense MLP layers are) unless the "
                             f"model is built with fp8_experts=True (from_pretrained(path, fp8_experts=True))")
        if leaf in _FP8_ACTIVATION or leaf.endswith(tuple("_" + a for a in _FP8_ACTIVATION)):
            raise ValueError(f"{name}: a static activation scale (input_scale / activation_scale); activations are not quantised "
                             f"here and the tensor is not served")
        if t.dtype == torch.float8_e5m2:
            raise ValueError(f"{name}: {t.dtype}: only e4m3 FP8 weights are served")

    def _take_fp8(self, name: str, owner: str, leaf: str, t: torch.Tensor) -> bool:
        """The tensors of the FP8 format -> True when `name` was one and has been dealt with."""
        fp8_dtype = t.dtype == torch.float8_e4m3fn
        lin = self.fp8.get(owner)
        if lin is not None and leaf in _FP8_PAIR:
            t = t.to(lin.weight.device)
            if leaf == "weight" and not fp8_dtype:          # a 16-bit weight: quantised here, as from_pretrained(fp8_weights=True) asks
                lin.quantize_(t, name)
                self._fill(f"{owner}.{b}" for b in _FP8_PAIR)
            else:
                lin.load_(**{"weight_fp8" if leaf == "weight" else "scale": t}, name=name)
                self._fill([name])
            return True
        dense = self.dense.get(owner)
        if dense is not None and leaf == "weight" and t.dtype == torch.uint8:
            raise ValueError(f"{name}: a uint8 weight for a linear; FP8 bytes have to come as float8_e4m3fn with their weight_scale_inv")
        if not (fp8_dtype or leaf == "weight_scale_inv"):
            return False
        if dense is None or not (leaf == "weight_scale_inv" or (fp8_dtype and leaf == "weight")):
            raise ValueError(f"{name}: an FP8 tensor whose owner is neither an FP8 linear nor a dense linear of this model")
        have = self.pending.setdefault(owner, {})
        have[leaf] = t
        if len(have) == 2:
            w, O, K = have["weight"].to(dense.weight.device), dense.out_features, dense.in_features
            if tuple(w.shape) != (O, K):
                raise ValueError(f"{owner}.weight: shape {tuple(w.shape)} does not fit ({O}, {K})")
            scale = wfp8.as_scale(have["weight_scale_inv"].to(w.device), O, K, f"{owner}.weight_scale_inv")
            dense.weight.data.copy_(wfp8.dequant_torch(wfp8.as_bytes(w, f"{owner}.weight"), scale, dense.weight.dtype))
            del self.pending[owner]
            self._fill([f"{owner}.weight"])
        return True

    def _take_piece(self, name: str, owner: str, e: int, part: str, t: torch.Tensor) -> None:
        ex, stack = self.experts[owner], "down_proj" if part == "down" else "gate_up_proj"
        if isinstance(ex, QuantExperts):
            if e >= ex.num_experts:
                raise ValueError(f"{name}: expert {e} outside the block's {ex.num_experts}")
            ex.pack_expert_(e, part, t.to(device=ex.down_proj.qweight.device, dtype=self.dtype), name)
        else:
            p = getattr(ex, stack)
            inter = p.shape[2] if part == "down" else p.shape[1] // 2
            want = (p.shape[1], p.shape[2]) if part == "down" else (inter, p.shape[2])
            if e >= p.shape[0] or tuple(t.shape) != want:
                raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit {owner}.{stack} {tuple(p.shape)}")
            rows = p.data[e] if part == "down" else p.data[e, :inter] if part == "gate" else p.data[e, inter:]
            rows.copy_(t)
        self._fill(self._keys(owner, stack), {(e, part)})

    def _take_fp8_piece(self, name: str, owner: str, e: int, part: str, leaf: str, t: torch.Tensor) -> None:
        """One per-expert tensor of a block of FP8 experts: `weight` as float8_e4m3fn or `weight_scale_inv`
        goes into the expert's slab as it is and fills its own key's slot (e, part); a 16-bit `weight` is quantised and fills both."""
        ex, stack = self.experts[owner], "down_proj" if part == "down" else "gate_up_proj"
        t = t.to(ex.down_proj.device)
        if leaf == "weight_scale_inv":
            ex.load_expert_(e, part, scale=t, name=name)
            self._fill([f"{owner}.{stack}_scale_inv"], {(e, part)})
        elif t.dtype == torch.float8_e4m3fn:
            ex.load_expert_(e, part, weight_fp8=t, name=name)
            self._fill([f"{owner}.{stack}"], {(e, part)})
        elif t.is_floating_point():
            ex.quantize_expert_(e, part, t, name)
            self._fill(self._keys(owner, stack), {(e, part)})
        else:
            raise ValueError(f"{name}: {t.dtype} for an expert weight; FP8 bytes have to come as float8_e4m3fn with their "
                             f"weight_scale_inv")

    def _take_fp8_fused(self, name: str, owner: str, leaf: str, t: torch.Tensor) -> None:
        """A fused stack of a block of FP8 experts: `gate_up_proj` / `down_proj` (E, rows, cols) as float8_e4m3fn, their `_scale_inv`
        (E, rows / 128, cols / 128) as fp32 (or one per-tensor scalar), or a 16-bit stack, which is quantised expert by expert."""
        ex = self.experts[owner]
        stack, part, half = _FP8_STACKS[leaf]
        t = t.to(ex.down_proj.device)
        O, K = ex.shape_of(part)
        if half == "scale":
            if t.numel() != 1 and (t.dim() != 3 or t.shape[0] != ex.num_experts):
                raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit the block grids "
                                 f"{(ex.num_experts, O // wfp8.BLOCK, K // wfp8.BLOCK)}")
            for e in range(ex.num_experts):
                ex.load_expert_(e, part, scale=t if t.numel() == 1 else t[e], name=name)
            self._fill([f"{owner}.{stack}_scale_inv"])
            return
        if tuple(t.shape) != (ex.num_experts, O, K):
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit {(ex.num_experts, O, K)}")
        if t.dtype == torch.float8_e4m3fn:
            for e in range(ex.num_experts):
                ex.load_expert_(e, part, weight_fp8=t[e], name=name)
            self._fill([f"{owner}.{stack}"])
        elif t.is_floating_point():
            for e in range(ex.num_experts):
                ex.quantize_expert_(e, part, t[e], f"{name}[{e}]")
            self._fill(self._keys(owner, stack))
        else:
            raise ValueError(f"{name}: {t.dtype} for an expert stack; FP8 bytes have to come as float8_e4m3fn with their _scale_inv")

    def _take_fused(self, name: str, owner: str, stack: str, t: torch.Tensor) -> None:
        q, part = self.experts[owner], "down" if stack == "down_proj" else "gate_up"
        if tuple(t.shape) != (q.num_experts, *q.shape_of(part)):
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit {(q.num_experts, *q.shape_of(part))}")
        for e in range(q.num_experts):
            q.pack_expert_(e, part, t[e].to(device=q.down_proj.qweight.device, dtype=self.dtype), f"{name}[{e}]")
        self._fill(self._keys(owner, stack))

    def finish(self) -> None:
        """KeyError over the state_dict keys that still owe a slot; ValueError over a half of an FP8 pair left waiting."""
        missing = [k for k, slots in self.owed.items() if slots]
        if missing:
            raise KeyError(f"checkpoint lacks {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        if self.pending:            # (its key is filled: the weight came as 16-bit, and this half belongs to nothing)
            stray = [f"{owner}.{leaf}" for owner, have in self.pending.items() for leaf in have]
            raise ValueError(f"{stray[:5]}{' ...' if len(stray) > 5 else ''}: half of an FP8 pair whose other half never came, beside a "
                             f"weight that is not FP8")


def load_weights(model: nn.Module, path: str, device, dtype) -> nn.Module:
    """Every *.safetensors file of `path`, in sorted order, onto `device` and through a CheckpointLoader: one file at a time is
    alive next to the model."""
    from safetensors.torch import load_file
    loader = CheckpointLoader(model, dtype)
    for f in sorted(glob.glob(os.path.join(path, "*.safetensors"))):
        loader.take(load_file(f, device=str(device)))       # no name holds the file's dict: it dies when take returns
    loader.finish()
    return model


def save_quantized(model: nn.Module, path: str) -> None:
    """The body of the models' save_quantized: config.json with the tags read_config strips, and model.safetensors."""
    from safetensors.torch import save_file
    cfg = model.config
    if getattr(cfg, "kivi_fp8_weights", False) or getattr(cfg, "kivi_fp8_experts", False):
        return _save_fp8(model, path)
    wbits, ebits = getattr(cfg, "kivi_weight_bits", None), getattr(cfg, "kivi_expert_bits", None)
    if wbits is None and ebits is None:
        raise ValueError("save_quantized: the model was not built with weight_bits=4 or expert_bits=4")
    os.makedirs(path, exist_ok=True)
    d = dict(cfg.kivi_hf_config, kivi_weight_layout=wquant.LAYOUT)
    if wbits is not None:
        d.update(kivi_weight_bits=wbits, kivi_weight_group=cfg.kivi_weight_group)
    if ebits is not None:
        d.update(kivi_expert_bits=ebits, kivi_expert_group=cfg.kivi_expert_group)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(d, fh, indent=1)
    state = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()
             if not (cfg.tie_word_embeddings and k == "lm_head.weight")}
    save_file(state, os.path.join(path, "model.safetensors"))


def _save_fp8(model: nn.Module, path: str) -> None:
    """save_quantized of a model built with fp8_weights or fp8_experts: transformers' fine-grained FP8 format (DESIGN.md sections 35
    and 36) -- `weight` as float8_e4m3fn and `weight_scale_inv` as float32 under the module names, FP8 experts under the per-expert
    names `mlp.experts.{e}.gate_proj / up_proj / down_proj`, and the `quantization_config` block read_config reads;
    `modules_to_not_convert` lists the linears that stayed dense, lm_head among them.  No tag of this project's."""
    from safetensors.torch import save_file
    cfg = model.config
    os.makedirs(path, exist_ok=True)
    fp8 = {n for n, m in model.named_modules() if isinstance(m, wfp8.Fp8Linear)}
    stacks = {n: m for n, m in model.named_modules() if isinstance(m, Fp8Experts)}
    dense = [n for n, m in model.named_modules() if isinstance(m, nn.Linear)]
    d = dict(cfg.kivi_hf_config, quantization_config=dict(
        quant_method="fp8", fmt="e4m3", activation_scheme="dynamic", weight_block_size=[wfp8.BLOCK, wfp8.BLOCK], scale_fmt="float",
        modules_to_not_convert=dense))
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(d, fh, indent=1)
    state = {}
    for k, v in model.state_dict().items():
        if cfg.tie_word_embeddings and k == "lm_head.weight":
            continue
        owner, _, leaf = k.rpartition(".")
        if owner in stacks:
            if leaf in ("gate_up_proj", "down_proj"):       # (the scales travel with their bytes)
                ex = stacks[owner]
                for e in range(ex.num_experts):
                    for part in ("gate", "up") if leaf == "gate_up_proj" else ("down",):
                        codes, bits = ex.slab(e, part)
                        base = f"{owner}.{e}.{_FP8_EXPERT_LEAVES[part]}"
                        state[f"{base}.weight"] = codes.detach().cpu().contiguous().view(torch.float8_e4m3fn)
                        state[f"{base}.weight_scale_inv"] = bits.detach().cpu().contiguous().view(torch.float32)
            continue
        v = v.detach().cpu().contiguous()
        if owner in fp8 and leaf in _FP8_PAIR:
            v = v.view(torch.float8_e4m3fn if leaf == "weight" else torch.float32)
        state[k] = v
    save_file(state, os.path.join(path, "model.safetensors"))
