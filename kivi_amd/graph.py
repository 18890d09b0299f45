"""Decode steps of a whole model replayed from ONE hipGraph (round 4).

A decode step of the reference is ~20 launches and ~40 lines of Python per layer (models/llama_kivi.py:314-399); here it is one
launch per layer, but at small batch the GPU still finishes a layer faster than the host can enqueue the next (0.4-0.5 ms of
enqueue per 32-layer step).  The launches of a step depend on six lengths that change every step, so they cannot simply be
captured -- unless the kernels read the lengths from device memory: `kivi_mf_decode_layer_dyn` (include/kivi_hip.h, kivi_mf_step)
sizes the launch geometry for the step's whole geometry class (same super-block counts, `kivi_mf_step_key`) and the kernels take
Tq / Tv / residual and window lengths from a 32-byte device struct.  All layers of a model share the same lengths, so one struct
serves the model: per step the host uploads six numbers (a one-thread kernel), replays the graph, advances its own copy of the
lengths (`kivi_mf_step_advance`) and -- every residual_length steps -- launches the K flushes (`kivi_kt_pack`), outside the graph.
The graph is re-captured when the geometry class changes (every ~512 steps per side) or a cache had to grow.

Replayed and eager steps agree bit for bit: both follow the launch plan of the step's whole geometry class (kivi_mf_launch_plan --
sized for the class's longest row, ceil(Tq / 512) * 512 + residual_length keys; since round 6 an eager step is planned for that
bound too, and the one-launch caps are whole super-blocks + a full residual, so the bands of round 5 where an eager step ran a block
per row and the replayed one sliced the row are gone: tests/test_graph_gpu.py covers Tq just under 8192 / 9216).

`DecodeGraphs` is what a model keeps for its graphed decode: the static buffers, the dense bodies, and either this whole-step graph
or, for caches in the hook-state layout, per-layer graphs of the dense parts around an eager attention call.  Beside it, as functions
of the model, the calls that drive it (`prepare_graphs`, `decode_graphed`, `generate_graphed`): the model's methods delegate here.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import weakref
from typing import Callable, List, Optional

import torch

from . import _lib, lora
from .attention import _rotate_half, kivi_attention_decode, rope_cos_sin
from .cache_mf import SB, KiviLayerCacheMF
from .generation import _MIN16, bind_suppress, leading_pads, observe_prompts, pack_result, resolve_sampler
from .qkrope import unpad
from .sampling import RowSampler
from .scoring import check_top_k, check_top_logprobs, picked_scores, score_into
from .stopping import StopRows, check_sync_every, resolve_stopping


class MfStepDriver:
    """The shared lengths of the layer caches of one model (all KiviLayerCacheMF, all at the same length)."""

    def __init__(self, caches: List[KiviLayerCacheMF]):
        assert caches and all(isinstance(c, KiviLayerCacheMF) and c.ring for c in caches), "matrix-pipe caches only"
        c0 = caches[0]
        # the caches are held WEAKLY: a driver (and the graph captured over it) kept on a model must not keep a finished request's KV
        # cache alive (advisor r5); whoever steps the driver owns the caches
        self._refs = [weakref.ref(c) for c in caches]
        self.lib = _lib.load()
        self.resync()
        self.dev = torch.zeros(4, dtype=torch.int64, device=c0.kt.device)       # kivi_mf_step in device memory (32 bytes)
        self._ptrs = None

    @property
    def caches(self) -> List[KiviLayerCacheMF]:
        cs = [r() for r in self._refs]
        assert all(c is not None for c in cs), "the caches this driver was built for are gone"
        return cs

    def serves(self, caches) -> bool:
        """True when this driver was built for exactly these (still living) cache objects."""
        return len(caches) == len(self._refs) and all(r() is c for r, c in zip(self._refs, caches))

    def resync(self) -> None:
        """Take the lengths from the caches again (they may have been advanced by eager steps or a new prompt since the last call)."""
        self.host = self.caches[0].host_step()
        for c in self.caches[1:]:
            h = c.host_step()
            assert (h.Tq, h.Tv, h.k_res_len, h.v_res_len, h.v_win_start) == (self.host.Tq, self.host.Tv, self.host.k_res_len, self.host.v_res_len, self.host.v_win_start), \
                "the layers of a model advance together"

    # -- per step, in this order: prepare() [-> capture or replay the launches] -> finish()
    def key(self) -> int:
        c = self.caches[0]
        return int(self.lib.kivi_mf_step_key(ctypes.byref(self.host), c.B, c.nh, c.nh_kv, c.cfg.residual_length, c._flags()))

    def prepare(self, also=()) -> bool:
        """Room for one more token in every cache, lengths uploaded.  Returns True when captured launches are stale: a cache was
        reallocated, the geometry class changed, or an address in `also` (what else the caller's captured step reads: its mask
        buffer) moved since the last call."""
        stale = False
        for c in self.caches:
            c.ensure_room(1)
        # everything a captured launch holds a raw pointer to: the stores, the fp16 residual / window, the per-stream scratch
        ptrs = tuple((c.kt.data_ptr(), c.vt.data_ptr(), c.k_res.data_ptr(), c.v_res.data_ptr()) +
                     tuple(t.data_ptr() for t in c._desc(c.nh, c.kt.device)[4]) for c in self.caches) + (self.key(),) + tuple(also)
        if ptrs != self._ptrs:
            stale, self._ptrs = True, ptrs
        _lib.check(self.lib.kivi_mf_step_upload(ctypes.byref(self.host), self.dev.data_ptr(), _lib.stream_ptr(self.dev)), "kivi_mf_step_upload")
        return stale

    def enqueue(self, i: int, q, k, v, out, attention_mask=None, lead=None):
        """The attend launches of layer i for the prepared step (eagerly, or under stream capture)."""
        if lead is None:
            return self.caches[i].decode_step_dyn(q, k, v, self.host, self.dev, out, attention_mask)
        return self.caches[i].decode_step_dyn(q, k, v, self.host, self.dev, out, attention_mask, lead=lead)

    def finish(self) -> None:
        """Bookkeeping after the step's launches were enqueued (replayed): lengths advanced, K flushed when the residual is full."""
        c0 = self.caches[0]
        rc = self.lib.kivi_mf_step_advance(ctypes.byref(self.host), c0.cfg.residual_length, c0.v_res.shape[2])
        if rc < 0:
            _lib.check(rc, "kivi_mf_step_advance")
        for c in self.caches:
            c.apply_step(self.host)
        if rc == 1:
            for c in self.caches:
                c.flush_k()
            self.host.Tq += c0.cfg.residual_length
            self.host.k_res_len = 0


@contextlib.contextmanager
def no_gc_in_capture():
    """Around a stream capture.  A pass of Python's cycle collector may run at any allocation, also while a capture is open, and
    may then destroy what an earlier request left behind in a reference cycle -- a captured graph with its memory pool, device
    buffers.  The runtime refuses such calls during a capture (the capture mode is global) and the process aborts.  torch's graph
    context does not collect before a capture any more, so: collect now, and keep the collector off until the capture has ended."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class GraphedDecode:
    """`step_fn()` enqueues one whole decode step (dense parts + `driver.enqueue(i, ...)` per layer) on the current stream, reading
    and writing static buffers; `step()` runs it -- the first step of a geometry class eagerly (which also settles everything the
    step allocates lazily), the second one captured into a hipGraph and replayed, the rest replayed."""

    def __init__(self, driver: MfStepDriver, step_fn: Callable[[], None]):
        self.driver, self.step_fn = driver, step_fn
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.warm = False
        self.stream = torch.cuda.Stream(driver.dev.device)      # ONE stream for every capture: the library keeps its scratch per stream
        self.captures = self.replays = self.eager = 0

    def step(self, also=()) -> None:
        cur = torch.cuda.current_stream(self.driver.dev.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            if self.driver.prepare(also):                        # room, lengths of THIS step uploaded; stale: reallocation / new class
                self.graph, self.warm = None, False
            if self.graph is None and not self.warm:
                self.step_fn()
                self.warm = True
                self.eager += 1
            else:
                if self.graph is None:
                    g = torch.cuda.CUDAGraph()
                    with no_gc_in_capture(), torch.cuda.graph(g, stream=self.stream):   # (records, does not execute)
                        self.step_fn()
                    self.graph = g
                    self.captures += 1
                self.graph.replay()
                self.replays += 1
            self.driver.finish()
        cur.wait_stream(self.stream)


class DecodeGraphs:
    """Everything a graphed decode of `model` at batch size B needs; LlamaForCausalLM_KIVI.decode_graphed steps it.

    In eager mode the host needs longer to enqueue the ~30 small launches of a layer's dense part than the GPU to run them.  Here
    they read and write static buffers (`tok`, `cos` / `sin`, `x`, `qkv`, `attn`) through two bodies: `pre(i)`, block input (layer 0:
    the embedding of `tok`) to the rotated q / k / v (with config.kivi_qk_kernel: one kivi_qk_rope launch into `qkv` buffers sized
    for the padded query groups, which post() cuts back), and `post(i)`, attention output to block output
    (last layer: on to the head and
    the next token in `tok`).  Same kernels, same results as forward().  Per-layer form: pre(i) and post(i) are captured once, here,
    and the KIVI step between them stays one eager call per layer (its lengths change every step).  Whole-step form (`whole`: every
    cache in the matrix-pipe layout): the attention launches read their lengths from device memory (MfStepDriver), so GraphedDecode
    captures all layers as ONE graph.  Driver and graph are made for the caches of begin() (held weakly: nothing here keeps a finished
    request's KV cache alive) and serve every call over them; MfStepDriver.prepare() alone finds a capture stale.
    `padded`: cos / sin hold one position per row (`pos`), and `mask` is a static additive (B, 1, 1, pitch) fp16 buffer, pitch >= the
    cache capacity, that the attention of every step reads (its new column is 0: new tokens are real).
    `lead` (config.kivi_decode_lead, padded only): a static (B,) int32 buffer beside the mask, refreshed in place
    by begin() from the same 2D mask; the steps hand it to the attention (the captured ones call kivi_mf_decode_layer_dyn_lead), so a
    changed lead replays what was captured.
    `sampler`: the last post() draws into `tok` with it instead of argmax.  The captured call holds what the sampler's key() names:
    a Sampler's parameters and state buffer, a RowSampler's row count and two buffers -- other parameter values in the same
    RowSampler (set_row, another request mix) replay the graphs that exist, another key builds them again.
    `logprobs`: None, or k >= 0 -- the last post() also scores the token it has just written into `tok` under
    the logits it has in hand, inside the captured step and after the draw, into the static buffers `lp` (B, 1) and, for k > 0,
    `top_ids` / `top_lp` (B, 1, k): one kivi_token_logprob (k == 0) or kivi_token_top_logprobs launch.  The warm-up scores too, so
    that a capture sees the launch; k is part of what matches() compares.
    `stopper`: a kivi_amd.stopping.StopRows of B rows -- the last post() runs it on `tok` after the draw and
    before the scores: one kivi_stop_rows launch, which counts the token of every live row, writes the pad over a finished row's
    and leaves the number of live rows in the stopper's `n_live`.  Not in the `draw=False` warm-up, which may not advance the
    state any more than it may consume a draw.  matches() compares the stopper's key(): its buffers, not its records.
    `stats`: (eager steps, captures, replays) of the whole-step form, cumulative over the calls on one set of caches."""

    def __init__(self, model, B: int, device, whole: bool = False, padded: bool = False, sampler=None, lead: bool = False,
                 logprobs: Optional[int] = None, stopper=None):
        cfg, layers = model.config, model.model.layers
        nh, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        D, dt = layers[0].self_attn.head_dim, model.lm_head.weight.dtype

        def zeros(*shape, dtype=dt):
            return torch.zeros(shape, dtype=dtype, device=device)

        self.model, self.B, self.whole, self.padded, self.sampler = model, B, whole, padded, sampler
        self.sampler_key = None if sampler is None else sampler.key()
        self.stopper, self.stopper_key = stopper, None if stopper is None else stopper.key()
        self.lora_key = lora.graph_key(model)       # the LoRA binding the captured steps read, or None
        self.tok = zeros(B, 1, dtype=torch.long)
        # a model that is not fp16: x stays in its dtype; q / k / v, the attention output and the mask are fp16 as
        # ever, cos / sin fp32, and pre() crosses with one kivi_qkv_rope_bf16 launch, post() back in the copy that feeds o_proj
        self.boundary = dt != torch.float16
        self.cos, self.sin = (zeros(B if padded else 1, 1, 1, D, dtype=torch.float32 if self.boundary else dt) for _ in range(2))
        self.x = [zeros(B, 1, cfg.hidden_size) for _ in range(len(layers) + 1)]
        nhp = layers[0].self_attn.cache_heads       # nh, or nh_kv * the padded ratio (config.kivi_qk_kernel)
        f16 = torch.float16 if self.boundary else dt
        self.attn = zeros(B, nhp, 1, D, dtype=f16)
        self.qkv = [(zeros(B, nhp, 1, D, dtype=f16), zeros(B, nkv, 1, D, dtype=f16), zeros(B, nkv, 1, D, dtype=f16)) for _ in layers]
        self.mask = self.pos = self.driver = self.graphed = self.stats = None
        self.lead = zeros(B, dtype=torch.int32) if padded and lead else None
        self.logprobs = logprobs
        self.lp = self.top_ids = self.top_lp = None
        if logprobs is not None:
            self.lp = zeros(B, 1, dtype=torch.float32)
            if logprobs:
                self.top_ids, self.top_lp = zeros(B, 1, logprobs, dtype=torch.long), zeros(B, 1, logprobs, dtype=torch.float32)
        if not whole:
            self._capture_layers()

    def matches(self, B: int, whole: bool, padded: bool, sampler_key, lead: bool = False, logprobs: Optional[int] = None,
                stopper_key=None, lora_key=None) -> bool:
        return ((self.B, self.whole, self.padded, self.sampler_key, self.lead is not None, self.logprobs, self.stopper_key,
                 self.lora_key) == (B, whole, padded, sampler_key, bool(lead), logprobs, stopper_key, lora_key))

    def pre(self, i: int) -> None:
        layer = self.model.model.layers[i]
        a, (q, k, v) = layer.self_attn, self.qkv[i]
        if i == 0:
            self.x[0].copy_(self.model.model.embed_tokens(self.tok))
        h = layer.input_layernorm(self.x[i])
        if self.boundary:                            # one kivi_qkv_rope_bf16 launch: q, k and v cross into fp16
            a.boundary_qkv(a.q_proj(h).view(self.B, 1, -1, a.head_dim), a.k_proj(h).view(self.B, 1, -1, a.head_dim),
                           a.v_proj(h).view(self.B, 1, -1, a.head_dim), self.cos.view(-1, 1, a.head_dim),
                           self.sin.view(-1, 1, a.head_dim), q.shape[1], q, k, v)
            return
        if a.qk_kernel or a.q_norm is not None:      # one kivi_qk_rope launch: head norm, RoPE, the padded head layout
            v.copy_(a.v_proj(h).view(self.B, 1, -1, a.head_dim).transpose(1, 2))
            a.prepare_qk(a.q_proj(h).view(self.B, 1, -1, a.head_dim), a.k_proj(h).view(self.B, 1, -1, a.head_dim),
                         self.cos.view(-1, 1, a.head_dim), self.sin.view(-1, 1, a.head_dim), q.shape[1], q, k)
            return
        for dst, proj in ((q, a.q_proj), (k, a.k_proj), (v, a.v_proj)):
            t = proj(h).view(self.B, 1, -1, a.head_dim).transpose(1, 2)
            dst.copy_(t if dst is v else t * self.cos + _rotate_half(t) * self.sin)

    def post(self, i: int, draw: bool = True) -> None:
        """`draw=False`: the next token by argmax whatever the sampler (a warm-up must not consume a draw)."""
        layer = self.model.model.layers[i]
        a = layer.self_attn
        if self.boundary:
            x = self.x[i] + a.o_proj(unpad(self.attn, a.num_key_value_heads, a.num_key_value_groups, self.x[i].dtype))
        elif self.attn.shape[1] != a.num_heads:     # padded query groups: the pad heads' outputs stay behind
            x = self.x[i] + a.o_proj(unpad(self.attn, a.num_key_value_heads, a.num_key_value_groups))
        else:
            x = self.x[i] + a.o_proj(self.attn.transpose(1, 2).reshape(self.B, 1, -1))
        self.x[i + 1].copy_(x + layer.mlp(layer.post_attention_layernorm(x)))
        if i == len(self.x) - 2:
            logits = self.model.lm_head(self.model.model.norm(self.x[i + 1]))
            if self.sampler is None or not draw:
                self.tok.copy_(logits.argmax(-1))
            else:
                self.sampler(logits, out=self.tok)
            if self.stopper is not None and draw:
                self.stopper(self.tok)
            if self.logprobs is not None:
                score_into(logits, self.tok, self.lp, self.top_ids, self.top_lp)

    def _capture_layers(self) -> None:
        device, n = self.tok.device, len(self.qkv)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):          # warm-up outside capture (library workspaces, autotuning)
            for i in range(n):
                self.pre(i)
                self.post(i, draw=False)
        torch.cuda.current_stream(device).wait_stream(side)
        self.pre_graphs, self.post_graphs, pool = [], [], None
        with no_gc_in_capture():
            for i in range(n):
                for fn, dst in ((self.pre, self.pre_graphs), (self.post, self.post_graphs)):
                    cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cg, pool=pool):
                        fn(i)
                    pool = pool or cg.pool()
                    dst.append(cg)
        self.tok.zero_()

    def _whole_step(self) -> None:
        for i in range(len(self.qkv)):
            self.pre(i)
            self.driver.enqueue(i, *self.qkv[i], self.attn, self.mask, self.lead)
            self.post(i)

    def _grow_mask(self, caches) -> None:
        """Room for a token in every cache, a mask buffer as wide as their capacity (whole: the stores', so that it moves with them)."""
        for c in caches:
            c.ensure_room(1)
        need = caches[0].n_sb * SB if self.whole else ((caches[0].cap + 7) // 8) * 8
        if self.mask is None or self.mask.shape[3] < need:
            old, self.mask = self.mask, torch.zeros((self.B, 1, 1, need), dtype=torch.float16, device=self.tok.device)
            if old is not None:
                self.mask[..., : old.shape[3]].copy_(old)

    def begin(self, tok: torch.Tensor, caches, attention_mask: Optional[torch.Tensor] = None) -> None:
        """Decode steps from `tok` over `caches` follow; padded: HF's 2D mask (B, kv_len + 1) fills the mask buffer and positions."""
        self.tok.copy_(tok)
        self._caches = [weakref.ref(c) for c in caches]
        if self.padded:
            self._grow_mask(caches)
            self.mask.zero_()
            self.mask[..., : attention_mask.shape[1]].masked_fill_((attention_mask == 0)[:, None, None, :], _MIN16)
            self.pos = attention_mask.long().sum(-1) - 1                 # (B,): position of `tok`
            if self.lead is not None:
                self.lead.copy_(leading_pads(attention_mask))            # in place: the captured step keeps its pointer
        if self.whole:
            if self.driver is not None and self.driver.serves(caches):   # the same caches again: replay what was captured instead of
                self.driver.resync()                                     # paying an eager step and a capture of every layer again
            else:
                self.driver = MfStepDriver(caches)
                self.graphed = GraphedDecode(self.driver, self._whole_step)

    def step(self, position: int) -> None:
        """One decode step from `tok` at `position` (padded: every row's own); the next token is left in `tok`."""
        a0 = self.model.model.layers[0].self_attn
        inv_freq = a0.inv_freq_exact(self.cos.device) if self.boundary else a0.inv_freq
        for dst, src in zip((self.cos, self.sin), rope_cos_sin(inv_freq, self.pos if self.padded else position)):
            dst.copy_(src.view(-1, 1, 1, src.shape[-1]))
        caches = [c() for c in self._caches]
        if self.padded:
            self.pos += 1
            self._grow_mask(caches)
        if self.whole:
            self.graphed.step((self.mask.data_ptr(),) if self.padded else ())
            self.stats = (self.graphed.eager, self.graphed.captures, self.graphed.replays)
            return
        mask = self.mask[..., : caches[0].kv_seq_len + 1] if self.padded else None
        for i, (q, k, v) in enumerate(self.qkv):
            self.pre_graphs[i].replay()
            if self.lead is None:
                kivi_attention_decode(q, k, v, caches[i], attention_mask=mask, out=self.attn)
            else:
                kivi_attention_decode(q, k, v, caches[i], attention_mask=mask, out=self.attn, lead=self.lead)
            self.post_graphs[i].replay()

    def end(self) -> None:
        """The caches of begin() die with their request: so does what was captured over them (buffers and per-layer graphs stay)."""
        self.driver = self.graphed = None


# ------------------------------------------------------------------ the graphed calls of a model (its methods of the same names)
def prepare_graphs(model, batch: int, device, whole, padded, sampler, logprobs, stopper) -> None:
    """LlamaForCausalLM_KIVI.prepare_graphs: model.graphs serves this step, built anew only when one of the seven fields differs."""
    model._refuse_capture("prepare_graphs")
    key, stop_key = (None if x is None else x.key() for x in (sampler, stopper))
    lead = padded and bool(getattr(model.config, "kivi_decode_lead", False))
    if model.graphs is None or not model.graphs.matches(batch, whole, padded, key, lead, logprobs, stop_key, lora.graph_key(model)):
        model.graphs = DecodeGraphs(model, batch, device, whole, padded, sampler, lead, logprobs, stopper)


@torch.no_grad()
def decode_graphed(model, tok, past_key_values, position, steps, attention_mask, sampler, sampling, logprobs, stopper, sync_every):
    """LlamaForCausalLM_KIVI.decode_graphed (its docstring is the reference): the checks, the graphs of the step, the step loop."""
    model._refuse_capture("decode_graphed")
    if logprobs is not None and logprobs != 0:
        check_top_k(logprobs, model.config.vocab_size, "logprobs")
    if stopper is not None:
        if not isinstance(stopper, StopRows) or stopper.B != tok.shape[0]:
            raise ValueError(f"decode_graphed(stopper=) takes a StopRows of {tok.shape[0]} rows")
        check_sync_every(sync_every)
    if sampling is not None:
        if sampler is not None:
            raise ValueError("pass either sampler= or sampling=, not both")
        if not isinstance(sampling, RowSampler):
            raise ValueError("decode_graphed(sampling=) takes a RowSampler")
        if sampling.B != tok.shape[0]:
            raise ValueError(f"the RowSampler holds {sampling.B} rows, the step has {tok.shape[0]}")
        sampler = sampling
    caches = [p.layer for p in past_key_values]
    whole = all(isinstance(c, KiviLayerCacheMF) for c in caches)      # the whole step as one graph, else per-layer graphs
    B, kv0 = tok.shape[0], caches[0].kv_seq_len
    padded = attention_mask is not None and model._padded(attention_mask, B, kv0 + 1, kv0)
    model.prepare_graphs(B, tok.device, whole, padded, sampler, logprobs, stopper)
    g = model.graphs
    g.begin(tok, caches, attention_mask)
    # the static buffers the host clones: the token a step is fed, before the step; the scores of the token it produced, after it
    bufs = (g.tok,) + (() if logprobs is None else (g.lp,) + ((g.top_ids, g.top_lp) if logprobs else ()))
    cols = [[] for _ in bufs]
    for s in range(steps):
        if stopper is not None and sync_every is not None and s % sync_every == 0 and int(stopper.n_live) == 0:
            break
        cols[0].append(g.tok.clone())
        g.step(position + s)
        for col, buf in zip(cols[1:], bufs[1:]):
            col.append(buf.clone())
    res = tuple(torch.cat(col, dim=1) if col else buf.new_empty((B, 0) + buf.shape[2:]) for col, buf in zip(cols, bufs))
    return res[0] if logprobs is None else res


def kept_stopper(model, params, device, pad_token_id: int) -> StopRows:
    """The model's own finish tracker for (rows, device, pad), its rows bound to `params`: the buffers stay from call to call, so
    the graphs captured over them are replayed whatever the stops of the next call are."""
    kept, key = model._stoppers, (len(params), str(device), pad_token_id)
    if key in kept:
        kept[key].rebind(params)
    else:
        kept[key] = StopRows(params, device, pad_token_id=pad_token_id)
    return kept[key]


@torch.no_grad()
def generate_graphed(model, input_ids, max_new_tokens, attention_mask, num_beams, do_sample, temperature, top_k, top_p, min_p, seed,
                     sampling, repetition_penalty, presence_penalty, frequency_penalty, return_logprobs, top_logprobs, eos_token_id,
                     pad_token_id, stop_token_ids, stop_sequences, stopping, sync_every, logit_bias, allowed_token_ids, min_new_tokens):
    """LlamaForCausalLM_KIVI.generate_graphed (its docstring is the reference).  One flow; finish conditions change, in explicit
    branches, how many steps run and which tokens come back, and the cut to the tracker's lengths with the masking behind them."""
    model._refuse_capture("generate_graphed")
    if sampling is None and num_beams != 1 and not do_sample:
        raise ValueError(f"generate_graphed is greedy only (num_beams={num_beams}); use generate(num_beams=...)")
    vocab = model.config.vocab_size
    check_top_logprobs(top_logprobs, return_logprobs, num_beams, vocab)
    pick, _ = resolve_sampler(input_ids.device, input_ids.shape[0], 1, num_beams, do_sample, temperature, top_k, top_p, min_p,
                              seed, sampling, repetition_penalty, presence_penalty, frequency_penalty, vocab, logit_bias,
                              allowed_token_ids, min_new_tokens)
    check_sync_every(sync_every)
    stops = resolve_stopping(input_ids.shape[0], max_new_tokens, eos_token_id, pad_token_id, stop_token_ids, stop_sequences,
                             stopping, 1, vocab, torch_eos=False)
    bind_suppress(pick, sampling, stops, eos_token_id)
    logits, pasts = model.forward(input_ids, padding_mask=attention_mask)
    observe_prompts(pick, input_ids, attention_mask)
    if attention_mask is not None:
        attention_mask = torch.cat([attention_mask, torch.ones_like(attention_mask[:, :1])], dim=1)
    tok = logits.argmax(-1) if pick is None else pick(logits)
    k = top_logprobs if return_logprobs else None
    if stops is None or max_new_tokens <= 0:
        # every step runs and the tokens FED come back: the caches end max_new_tokens tokens on, a sampler one draw more, as generate()
        stopper, steps, how = None, max_new_tokens, {} if k is None else dict(logprobs=k)
    else:
        # the first token goes through the tracker eagerly, the steps may end early, and the last token is the one PRODUCED
        stopper = stops if isinstance(stops, StopRows) else kept_stopper(model, stops, input_ids.device, pad_token_id)
        before = stopper.length.clone()                 # (a caller's StopRows may have counted earlier tokens)
        stopper(tok)
        steps, how = max_new_tokens - 1, dict(logprobs=k, stopper=stopper, sync_every=sync_every)
    firsts = picked_scores(logits, tok, k)
    res = model.decode_graphed(tok, pasts, input_ids.shape[1], steps, attention_mask, pick, **how)
    new, scores = (res, ()) if k is None else (res[0], res[1:])
    if stopper is not None:
        new = torch.cat([new, model.graphs.tok], dim=1)
    model.graphs.end()                                  # the caches of this request die with it: so does the graph captured over them
    n = new.shape[1]
    if stopper is not None:                             # all finished: up to the longest row, as generate()
        own, reason = torch.stack([stopper.length - before, stopper.reason]).tolist()
        n = n if 0 in reason else max(max(own), 1)
    # step s scores the token it produced, new[:, s + 1]: the first token's score in front, what lies past the width off
    scores = tuple(torch.cat([f, sc], dim=1)[:, :n] for f, sc in zip(firsts, scores))
    if stopper is not None and scores:                  # the scores of a finished row's pads: logprob 0, id -1, value 0
        pads = torch.arange(n, device=new.device)[None, :] >= torch.tensor(own, device=new.device)[:, None]
        scores = tuple(sc.masked_fill(pads if sc.dim() == 2 else pads.unsqueeze(-1), fill) for sc, fill in zip(scores, (0.0, -1, 0.0)))
    return pack_result(input_ids, new[:, :n], scores)
