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

from . import wquant
from .moe import QuantExperts, SparseMoeBlock

_TAGS = ("kivi_weight_layout", "kivi_weight_bits", "kivi_weight_group", "kivi_expert_bits", "kivi_expert_group")
_EXPERT_NAME = re.compile(r"^(.*\.)(?:block_sparse_moe|mlp)\.experts\.(\d+)\.(w1|w2|w3|gate_proj|up_proj|down_proj)\.weight$")
_EXPERT_PART = {"w1": "gate", "gate_proj": "gate", "w3": "up", "up_proj": "up", "w2": "down", "down_proj": "down"}
_STACK_PARTS = {"gate_up_proj": ("gate", "up"), "down_proj": ("down",)}
_TRIPLE = ("qweight", "scales", "mins")


def read_config(path: str, kivi: dict) -> dict:
    """config.json of the directory `path` without the tags of save_quantized.  Where the layout tag is there, the bits and groups
    it was written with go into `kivi` (the keywords of make_config); another layout than this version's raises."""
    d = json.load(open(os.path.join(path, "config.json")))
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
      any other             `block_sparse_moe.` spelled `mlp.`, then model.load_state_dict(strict=False) over the file's remainder:
                            a shape that does not fit raises there, a name nothing takes ends in `unexpected`, a tensor that comes
                            again is written again.
    The ledger `owed`: state_dict key -> the slots nothing has filled yet.  A key is one slot; the key of an expert stack -- the
    dense parameter, or each of a 4-bit stack's three buffers -- is one slot per (expert, part), part in gate / up / down, since
    only a set can tell a repeated piece from a missing one.  The tied lm_head.weight owes nothing.  Nothing here keeps a tensor
    of a file: it dies with the caller's dict."""

    def __init__(self, model: nn.Module, dtype=torch.float16):
        self.model, self.dtype = model, dtype
        self.unexpected = []
        self.linears = {n: m for n, m in model.named_modules() if isinstance(m, wquant.QuantLinear)}
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
        return [f"{owner}.{stack}"]

    def _fill(self, keys, slots=None) -> None:
        for k in keys:
            if k in self.owed:
                self.owed[k] = set() if slots is None else self.owed[k] - slots

    def take(self, tensors: dict) -> None:
        rest = {}
        for name, t in tensors.items():
            m = _EXPERT_NAME.match(name)
            if m is not None:
                owner = f"{m.group(1)}mlp.experts"
                if owner in self.experts:
                    self._take_piece(name, owner, int(m.group(2)), _EXPERT_PART[m.group(3)], t)
                else:
                    rest[name] = t                          # load_state_dict reports the name as unexpected
                continue
            new = name.replace(".block_sparse_moe.", ".mlp.")
            owner, _, leaf = new.rpartition(".")
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

    def _take_fused(self, name: str, owner: str, stack: str, t: torch.Tensor) -> None:
        q, part = self.experts[owner], "down" if stack == "down_proj" else "gate_up"
        if tuple(t.shape) != (q.num_experts, *q.shape_of(part)):
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not fit {(q.num_experts, *q.shape_of(part))}")
        for e in range(q.num_experts):
            q.pack_expert_(e, part, t[e].to(device=q.down_proj.qweight.device, dtype=self.dtype), f"{name}[{e}]")
        self._fill(self._keys(owner, stack))

    def finish(self) -> None:
        """KeyError over the state_dict keys that still owe a slot."""
        missing = [k for k, slots in self.owed.items() if slots]
        if missing:
            raise KeyError(f"checkpoint lacks {missing[:5]}{' ...' if len(missing) > 5 else ''}")


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
