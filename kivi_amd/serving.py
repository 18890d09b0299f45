"""Continuous batching over a queue of requests: `generate_continuous`, the scheduler above
LlamaForCausalLM_KIVI.admit_.

generate() decodes a batch until its slowest row has finished; a row that is done keeps feeding pad tokens, and a waiting request
is served only by a new prompt pass over a new batch.  Here a finished row is taken over by the next waiting request between two
steps: its prompt, left-padded to the living caches' length, runs as a prompt pass of its own and is put into the row in place
(kivi_cache_admit); the other rows, every buffer and every captured graph stay as they are.

The policy is fixed (tests restate it):
  * B = min(batch_size, number of requests); the first B requests form the initial batch, left-padded to L0, the longest prompt of
    ALL requests of the call -- every later admission (at a length >= L0) then fits.
  * Every iteration picks a token for every row from the logits the row has; a live row records it.  A row is finished when the
    token is `eos_token_id` or the request holds its `max_new_tokens` (the one synchronisation of a step: the tokens are read).
    In full: the rule of kivi_amd/stopping.py -- stop ids (the eos ids first), stop sequences over the
    request's own tokens, the limit -- run in Python on the tokens the scheduler has read anyway (StopState.push); there is no
    device tracker here, a launch would buy nothing where the host already holds the tokens, and the captured step stays as it is.
  * Finished rows take the next waiting requests, lowest row first and in FIFO order, through ONE admit_ at the current length.
    An admitted request's first token is picked from its prompt logits and replaces the row's token before the step; should that
    token already finish the request, the row is free again and the admission repeats at the same length.
  * `compact=n` (None: never): after the tokens were recorded and before the admissions,
    room = min(leading pads of the live rows (no live row: L), L - the longest waiting prompt (none: 0), rebase_limit) and
    drop = room rounded down to rebase_quantum; if drop >= n, model.rebase_ drops the first `drop` tokens of every row, the 2D mask
    loses its first `drop` columns and L falls by `drop`.  The leading pads are kept on the host: admission length - prompt
    length - the drops since.
  * `short_admissions=True` (default False): an admission runs its prompt pass at a short length instead of L.
    off = admission_offset(L, the longest prompt of the group admitted together, residual_length, rebase_quantum): the prompts are
    left-padded to L - off, model.admit_(..., offset=off) puts them into tokens [off, L) of the rows and zeroes the blocks below, the
    rows' 2D mask is off zeros followed by the short mask.  Still ONE admit_ per group; the leading pads kept on the host are
    L - prompt length as before, so `compact=` works unchanged; no buffer or length changes, so the graphed mode replays the captured
    step.  An offset-admitted row is NOT bit-identical to an L-padded one: the K groups that mix pads and real tokens quantise
    other pad values (the pads' hidden states depend on how many pads precede them), and the prompt's SDPA runs at another length
    (another reduction order).  Both are the differences two L-padded admissions at different L already have; tokens can differ
    from short_admissions=False, which is why the default stays off.
  * Rows with nothing to do feed `pad_token_id`.  The call ends when every request is done: no step runs after the last pick.
  * Token i of a request is draw i of its own seed with Philox stream 0, whichever row and step it lands on:
    the first token is drawn by a RowSampler of the admitted rows alone, then the batch's RowSampler row is bound with
    set_row(..., draw_index=1).
  * Penalties: when a request's SamplingParams carry one, both samplers get a history table.  The
    first-token sampler of an admission has the admitted prompts marked; the batch's row is bound with
    set_row(..., draw_index=1, prompt=<the prompt>, generated=[the first token]), which clears what the row's last request left.
    The table is indexed by token id, not by cache position: a rebase and an admission offset do not touch it.
  * `return_logprobs` / `top_logprobs=k`: every recorded token is scored under the raw logits it was picked
    from -- the batch's step logits, or the admission's prompt logits for a first token -- by one kivi_token_logprob /
    kivi_token_top_logprobs launch beside the pick (graphed: inside the captured step).  The values are read where the tokens are
    read, so a step keeps its one synchronisation.  Eager, the rows with nothing to do score the ignore index; the captured step
    scores every row and the host drops what no request owns.
  * Constraints: when a request's SamplingParams carry a logit_bias, allowed_token_ids or min_new_tokens, or
    an `allowed_fn` is given, both samplers get constraint state.  The ids a request's min_new_tokens suppresses are its stop ids
    (the eos ids first); the batch's row is bound with set_row(..., draw_index=1, generated=[the first token], suppress=<those>), so
    its suppression ends min_new_tokens draws after the request's first.  Before every pick the scheduler calls a request's
    `allowed_fn` with the tokens the request has so far -- it holds them on the host anyway -- and uploads the answer with
    set_allowed; the captured step reads the mask buffer and is not captured again.
"""
from __future__ import annotations

import contextlib
from typing import List, Optional

import torch

from . import lora
from .generation import decode_key_row, left_pad, padding_key_row
from .sampling import RowSampler, SamplingParams
from .scoring import check_top_logprobs, picked_scores
from .stopping import LIVE, StopParams, StopState, stop_ids


def _positive_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool) and x >= 1


def check_arguments(prompts, max_new_tokens, batch_size, eos_token_id, pad_token_id, sampling, vocab_size: Optional[int] = None,
                    compact: Optional[int] = None, short_admissions: bool = False, allowed_fn=None):
    """-> (prompts as 1-D int64 CPU tensors, max_new_tokens per request, bound SamplingParams per request or None); ValueError for
    anything generate_continuous cannot serve (no device work)."""
    if compact is not None and not _positive_int(compact):
        raise ValueError(f"compact has to be None or a positive integer (the fewest tokens worth reclaiming), got {compact!r}")
    if not isinstance(short_admissions, bool):
        raise ValueError(f"short_admissions has to be a bool (admit at an offset, DESIGN.md section 19), got {short_admissions!r}")
    if not isinstance(prompts, (list, tuple)) or not prompts:
        raise ValueError("prompts has to be a non-empty list of token id sequences")
    seqs = [torch.as_tensor(p, dtype=torch.long).flatten().cpu() for p in prompts]
    N = len(seqs)
    for r, s in enumerate(seqs):
        if not s.numel():
            raise ValueError(f"prompt {r} is empty")
        if vocab_size is not None and (int(s.min()) < 0 or int(s.max()) >= vocab_size):
            raise ValueError(f"prompt {r} holds token ids outside the vocabulary [0, {vocab_size})")
    if not _positive_int(batch_size):
        raise ValueError(f"batch_size has to be a positive integer, got {batch_size!r}")
    if _positive_int(max_new_tokens):
        limits = [max_new_tokens] * N
    elif isinstance(max_new_tokens, (list, tuple)) and all(_positive_int(m) for m in max_new_tokens):
        limits = list(max_new_tokens)
        if len(limits) != N:
            raise ValueError(f"{len(limits)} max_new_tokens for {N} requests")
    else:
        raise ValueError(f"max_new_tokens has to be a positive integer or one per request, got {max_new_tokens!r}")
    if eos_token_id is not None and pad_token_id is None:
        raise ValueError("eos_token_id needs a pad_token_id for the rows that have nothing to do")
    if sampling is None:
        params = None
    else:
        if isinstance(sampling, SamplingParams):
            sampling = [sampling] * N
        elif not isinstance(sampling, (list, tuple)) or not all(isinstance(p, SamplingParams) for p in sampling):
            raise ValueError("sampling has to be None (greedy), a SamplingParams, or a list with one SamplingParams per request")
        if len(sampling) != N:
            raise ValueError(f"{len(sampling)} SamplingParams for {N} requests")
        for p in sampling:
            p.check_vocab(vocab_size)
        params = [RowSampler._bind(p) for p in sampling]          # one seed per request, whichever row it lands on
    if allowed_fn is not None:
        fns = [allowed_fn] * N if callable(allowed_fn) else allowed_fn
        if not isinstance(fns, (list, tuple)) or not all(f is None or callable(f) for f in fns):
            raise ValueError("allowed_fn has to be None, a callable, or a list with one callable or None per request")
        if len(fns) != N:
            raise ValueError(f"{len(fns)} allowed_fn entries for {N} requests")
        if params is None:                                        # greedy requests: the masks still need a RowSampler
            params = [RowSampler._bind(SamplingParams(do_sample=False)) for _ in range(N)]
    return seqs, limits, params


def check_stopping(limits, eos_token_id, pad_token_id, stopping, vocab_size: Optional[int] = None):
    """The finish conditions of every request as one StopParams each (kivi_amd/stopping.py): the ids of `eos_token_id` (None, an int
    or a list) in front of the request's own stop ids, its stop sequences, and the smaller of its two limits.  `stopping`: None, one
    StopParams, or one per request.  ValueError (no device work) for anything else."""
    N = len(limits)
    if stopping is None:
        stopping = [StopParams()] * N
    elif isinstance(stopping, StopParams):
        stopping = [stopping] * N
    elif not isinstance(stopping, (list, tuple)) or not all(isinstance(p, StopParams) for p in stopping):
        raise ValueError("stopping has to be None, a StopParams, or a list with one StopParams per request")
    if len(stopping) != N:
        raise ValueError(f"{len(stopping)} StopParams for {N} requests")
    if pad_token_id is None and any(p.stop_token_ids or p.stop_sequences for p in stopping):
        raise ValueError("stop ids and stop sequences need a pad_token_id for the rows that have nothing to do")
    eos = stop_ids(eos_token_id, None)
    out = []
    for p, limit in zip(stopping, limits):
        p = StopParams(eos + p.stop_token_ids, p.stop_sequences, min(limit, p.limit))
        p.check_vocab(vocab_size)
        out.append(p)
    return out


def compact_drop(leads, L: int, longest_waiting: int, limit: int, quantum: int) -> int:
    """The tokens to drop from the front of every row of living caches at length L: `leads`, the leading pads of the LIVE rows (none:
    the whole length counts); `longest_waiting`, the longest prompt still in the queue (0: none), which has to fit into the new
    length; `limit` and `quantum`, what the caches take (rebase_limit, rebase_quantum)."""
    room = min(min(leads, default=L), L - longest_waiting, limit)
    return max(room, 0) // quantum * quantum


def admission_offset(L: int, longest_prompt: int, R: int, quantum: int) -> int:
    """The offset of an admission into living caches at length L (host arithmetic): the prompt pass runs over L - offset tokens,
    which has to hold the longest prompt of the group admitted together and at least R = residual_length tokens; the offset is a
    multiple of `quantum` (rebase_quantum).  0: the admission runs at L, as without short_admissions."""
    return max(L - max(longest_prompt, R), 0) // quantum * quantum


@torch.no_grad()
def generate_continuous(model, prompts, max_new_tokens, batch_size: int, eos_token_id: Optional[int] = None,
                        pad_token_id: Optional[int] = 0, sampling=None, graphed: bool = False,
                        compact: Optional[int] = None, short_admissions: bool = False, return_logprobs: bool = False,
                        top_logprobs: int = 0, stopping=None, return_finish: bool = False, allowed_fn=None, adapters=None):
    """`prompts`: a list of token id sequences, possibly more than `batch_size`; `max_new_tokens`: an int or one per request;
    `sampling`: None (greedy), one SamplingParams, or one per request.  -> the generated tokens of every request as 1-D int64
    tensors, in request order, ending with `eos_token_id` where it was produced.  The policy: the module docstring.
    `graphed=True`: the steps go through decode_graphed(..., attention_mask=, sampling=) over the same living caches; the 2D mask
    with the replaced rows is passed again after an admission and the captured step is replayed, not captured again (unless the
    mask buffer has to grow, or the first pad of the call arrives with an admission).  Same tokens as graphed=False.
    `compact`: None -- the caches' length only grows --, or the fewest tokens worth reclaiming: at the top of every iteration the
    leading tokens no live row and no waiting prompt needs are dropped from the living caches (model.rebase_), if there are at least
    that many.
    `short_admissions`: False -- every admission is a prompt pass at the caches' length --, or True: at about the prompts' length,
    admitted at an offset (the module docstring; tokens can differ from False).
    `return_logprobs`: -> (tokens, logprobs), the second a list of fp32 tensors of the tokens' lengths: the log-probability of every
    token under the raw distribution it was picked from; with `top_logprobs=k` also top_ids (n, k) int64 and top_logprobs (n, k)
    fp32 per request, the k most likely tokens of each of those distributions.
    `eos_token_id`: an int or a list of ids; `stopping`: None, one StopParams or one per request -- stop ids (after the eos ids),
    stop sequences, and a max_new_tokens of its own (the smaller of the two limits holds).  A request's tokens end with the stop that
    finished it.  `return_finish=True`: the result (a tuple in any case then) gains a last element, a list of (reason, index) per
    request -- kivi_amd.stopping: TOKEN / SEQUENCE / LENGTH and the position of the id or sequence that matched (-1 for LENGTH).
    Constraints come with `sampling`: a request's logit_bias, allowed_token_ids and min_new_tokens, which
    holds back the request's eos and stop token ids (not its stop sequences).  `allowed_fn`: None, one callable, or one callable or
    None per request -- before every pick it is called with the list of the request's generated ids and answers token ids, an int32
    bitmask (RowSampler.set_allowed) or None (the request's own allowed_token_ids, or no mask): the mask of that one pick.
    `adapters`: None, one LoRA slot for every request, or one int or None per request.  The batch owns one
    RowBinding: the first prompt pass and every step run under it; an admission runs its prompt pass under a binding of the admitted
    rows alone (admit_(adapters=)) and then set_row()s the batch's, so the captured step is replayed; a finished row goes back to -1."""
    prompts, limits, params = check_arguments(prompts, max_new_tokens, batch_size, eos_token_id, pad_token_id, sampling,
                                              model.config.vocab_size, compact, short_admissions, allowed_fn)
    stops = check_stopping(limits, eos_token_id, pad_token_id, stopping, model.config.vocab_size)
    finish = [StopState(p) for p in stops]
    fns = None if allowed_fn is None else ([allowed_fn] * len(prompts) if callable(allowed_fn) else list(allowed_fn))
    check_top_logprobs(top_logprobs, return_logprobs, 1, model.config.vocab_size)
    k = top_logprobs
    pad = 0 if pad_token_id is None else pad_token_id
    use_lead = bool(getattr(model.config, "kivi_decode_lead", False))
    N, device = len(prompts), model.lm_head.weight.device
    B = min(batch_size, N)
    L = max(p.numel() for p in prompts)

    lset = getattr(model, "lora", None)
    slot_of = lora.resolve_adapters(adapters, N, None if lset is None else lset.S)
    if isinstance(slot_of, lora.RowBinding):
        raise ValueError("generate_continuous(adapters=) takes slots per request, not a RowBinding: the batch owns its binding")
    binding = None if slot_of is None else lora.RowBinding(B, device, slot_of[:B])
    bound = contextlib.nullcontext() if binding is None else lset.bound(binding)
    with bound:
        return _continuous(model, prompts, params, stops, finish, fns, k, pad, use_lead, N, device, B, L,
                           graphed, compact, short_admissions, return_logprobs, return_finish, slot_of, binding)


def _continuous(model, prompts, params, stops, finish, fns, k, pad, use_lead, N, device, B, L, graphed, compact,
                short_admissions, return_logprobs, return_finish, slot_of, binding):
    """The scheduler of generate_continuous behind its checks; `binding`: the batch's LoRA binding (active for the whole call) or
    None, `slot_of`: the slot of every request."""
    ids, mask = left_pad(prompts[:B], pad, device, length=L)
    logits, pasts = model.forward(ids, padding_mask=mask)
    con = params is not None and (fns is not None or any(p.constrained for p in params))
    table = model.config.vocab_size if params is not None and (con or any(p.penalised for p in params)) else None
    sampler = None if params is None else RowSampler(params[:B], device, vocab_size=table, constraints=con,
                                                     suppress=[stops[r].stop_token_ids for r in range(B)])
    if table is not None:
        sampler.observe_prompt(ids, attention_mask=mask)

    def pick(lg, rows_sampler):
        return lg.argmax(-1) if rows_sampler is None else rows_sampler(lg)

    def score(lg, t, skip=()):
        """The scores of the picked tokens t (n, 1) under lg (n, 1, V), as device tensors (read later, with the tokens)."""
        if skip:
            t = t.clone()
            t[list(skip)] = -100
        return picked_scores(lg, t, k)

    out: List[List[int]] = [[] for _ in range(N)]

    def bind_masks(rows_sampler, pairs) -> None:
        """Every (row of `rows_sampler`, request) pair whose request has an allowed_fn gets the mask of its next pick."""
        for b, r in pairs:
            if fns is not None and fns[r] is not None:
                answer = fns[r](list(out[r]))
                rows_sampler.set_allowed(b, params[r].allowed_token_ids if answer is None else answer)

    bind_masks(sampler, [(b, b) for b in range(B)])
    tok = pick(logits, sampler)
    scores = score(logits, tok) if return_logprobs else None
    mask2d = torch.ones((B, 2 * L + 64), dtype=torch.long, device=device)      # column t: 1 = cache token t of the row is real
    mask2d[:, :L] = mask
    owner: List[Optional[int]] = list(range(B))                                # the request of every row (None: nothing to do)
    lead = [L - prompts[r].numel() for r in range(B)]                          # leading pads of every row (host side, no device read)
    out_scores: List[List[list]] = [[[] for _ in range(N)] for _ in range(3)]      # logprob, top ids, top logprobs of every token
    waiting = B

    def record(b: int, t: int, sc=None, i: int = 0) -> None:
        """Row b's request takes token t; sc: the host copies of score()'s tensors, i the row of them that belongs to b."""
        r = owner[b]
        out[r].append(t)
        if sc is not None:
            for dst, v in zip(out_scores, sc):
                dst[r].append(v[i])
        if finish[r].push(t) != LIVE:              # the rule of kivi_amd/stopping.py on the request's own tokens
            owner[b] = None
            if binding is not None and binding.host[b] != -1:
                binding.set_row(b, -1)                 # an idle row runs the base model

    while True:
        toks = tok.view(-1).tolist()                                           # the one synchronisation of a step
        sc = None if scores is None else [v.squeeze(1).tolist() for v in scores]
        for b, t in enumerate(toks):
            if owner[b] is not None:
                record(b, t, sc, b)
        if compact is not None:
            drop = compact_drop([lead[b] for b in range(B) if owner[b] is not None], L,
                                max((prompts[r].numel() for r in range(waiting, N)), default=0),
                                model.rebase_limit(pasts), model.rebase_quantum(pasts))
            if drop >= compact:
                pasts = model.rebase_(pasts, drop)
                mask2d = torch.cat([mask2d[:, drop:], torch.ones_like(mask2d[:, :drop])], dim=1)
                L -= drop
                lead = [n - drop for n in lead]
        while waiting < N and None in owner:
            rows = [b for b in range(B) if owner[b] is None][: N - waiting]
            reqs = list(range(waiting, waiting + len(rows)))
            waiting += len(rows)
            off = 0
            if short_admissions:
                off = admission_offset(L, max(prompts[r].numel() for r in reqs), pasts[0].layer.cfg.residual_length,
                                       model.rebase_quantum(pasts))
            new_ids, new_mask = left_pad([prompts[r] for r in reqs], pad, device, length=L - off)
            own = {} if binding is None else dict(adapters=[slot_of[r] for r in reqs])     # the admitted rows' slots alone
            lg, pasts = model.admit_(pasts, rows, new_ids, new_mask, offset=off, **own)
            if off:
                mask2d[rows, :off] = 0                                             # the zeroed lead is masked like any pad
            mask2d[rows, off:L] = new_mask
            first_sampler = None if params is None else RowSampler([params[r] for r in reqs], device, vocab_size=table, constraints=con,
                                                                   suppress=[stops[r].stop_token_ids for r in reqs])
            if table is not None:
                first_sampler.observe_prompt(new_ids, attention_mask=new_mask)
            bind_masks(first_sampler, list(enumerate(reqs)))
            first = pick(lg, first_sampler)                                                                 # draw 0 of each
            first_scores = score(lg, first) if return_logprobs else None
            tok[rows] = first
            firsts = first.view(-1).tolist()
            fsc = None if first_scores is None else [v.squeeze(1).tolist() for v in first_scores]
            for i, (b, r, t) in enumerate(zip(rows, reqs, firsts)):
                owner[b] = r
                lead[b] = L - prompts[r].numel()
                if binding is not None:
                    binding.set_row(b, slot_of[r])
                if sampler is not None:
                    sampler.set_row(b, params[r], draw_index=1, prompt=prompts[r], generated=[t],
                                    suppress=stops[r].stop_token_ids if con else None)
                record(b, t, fsc, i)
        if all(r is None for r in owner):
            break
        idle = [b for b in range(B) if owner[b] is None]
        if idle:
            tok[idle] = pad
        if L + 1 > mask2d.shape[1]:
            mask2d = torch.cat([mask2d, torch.ones_like(mask2d)], dim=1)
        m = mask2d[:, : L + 1]                                                 # the fed token is real in every row
        bind_masks(sampler, [(b, owner[b]) for b in range(B) if owner[b] is not None])
        if graphed:
            res = model.decode_graphed(tok, pasts, L, 1, attention_mask=m, sampling=sampler, logprobs=k if return_logprobs else None)
            scores = res[1:] if return_logprobs else None
            tok = model.graphs.tok.clone()
        else:
            # (config.kivi_decode_lead: the row travels with the leading zeros of the SAME mask -- what an admission rewrote and
            # a rebase dropped is in it)
            logits, pasts = model._forward(tok, pasts, decode_key_row(m, use_lead), m.sum(-1, keepdim=True) - 1, True, True)
            tok = pick(logits, sampler)
            if return_logprobs:
                scores = score(logits, tok, idle)
        L += 1
    if graphed and model.graphs is not None:
        model.graphs.end()           # the caches of this call die with it: so does the graph captured over them
    tokens = [torch.tensor(o, dtype=torch.long, device=device) for o in out]
    finished = ([(f.reason, f.index) for f in finish],) if return_finish else ()
    if not return_logprobs:
        return (tokens,) + finished if return_finish else tokens
    res = (tokens, [torch.tensor(o, dtype=torch.float32, device=device) for o in out_scores[0]])
    if k:
        res += ([torch.tensor(o, dtype=torch.long, device=device) for o in out_scores[1]],
                [torch.tensor(o, dtype=torch.float32, device=device) for o in out_scores[2]])
    return res + finished
