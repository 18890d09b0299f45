"""GPU: finish conditions end to end on the tiny model of tests/test_extend_gpu.py, both cache layouts:
generate() against a free run cut by reference_stop, the list form of eos_token_id against today's torch path, generate_graphed()
against generate(), and generate_continuous() against the rule."""
import pytest
import torch

from kivi_amd.stopping import LENGTH, LIVE, SEQUENCE, TOKEN, StopParams, StopRows, reference_stop
from test_extend_gpu import _model
from test_score_gpu import _layouts
from test_top_logprobs_gpu import SAMPLED, _bits_equal, _layout_of

pytestmark = pytest.mark.gpu

PAD, N = 0, 40                  # 40 new tokens: more than residual_length = 32, a K flush lies inside
NEVER = 319                     # the batches below hold ids in [1, 319): no prompt holds it; the runs assert that no output does


def _batch(seed=4, lens=(21, 14, 9)):
    from kivi_amd.llama import left_pad
    g = torch.Generator().manual_seed(seed)
    return left_pad([torch.randint(1, 319, (n,), generator=g).tolist() for n in lens], PAD, "cuda")


def _cut(new, stops, n=N):
    """The rows of a free run, each cut by reference_stop under its StopParams capped at n and padded -> (tensor, results)."""
    res = [reference_stop(row, p.capped(n)) for row, p in zip(new.tolist(), stops)]
    width = max(r[0] for r in res) if all(r[1] != LIVE for r in res) else n
    out = torch.full((len(res), width), PAD, dtype=torch.long)
    for b, (length, _, _) in enumerate(res):
        out[b, :length] = new[b, :length].cpu()
    return out.cuda(), res


def _stops_from(new):
    """A token of row 0, a bigram of row 1, nothing reachable for row 2."""
    assert not bool((new == NEVER).any())
    return [StopParams([int(new[0, 5])]), StopParams((), [[NEVER, NEVER], new[1, 9:11].tolist()]), StopParams([NEVER], [[NEVER, 5]])]


@pytest.mark.parametrize("kw", [dict(), SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_and_generate_graphed_against_the_cut_free_run(layout, kw, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 71)
    assert _layout_of(model) == layout
    ids, mask = _batch()
    T = ids.shape[1]
    free = model.generate(ids, N, attention_mask=mask, **kw)
    new = free[:, T:]
    stops = _stops_from(new)
    want, res = _cut(new, stops)
    assert res[0][1] == TOKEN and res[0][0] <= 6 and res[1][1:] == (SEQUENCE, 1) and res[1][0] <= 11
    assert res[2] == (N, LENGTH, -1) and want.shape[1] == N                      # row 2 runs to the limit
    args = dict(attention_mask=mask, stopping=stops, pad_token_id=PAD, **kw)
    got = model.generate(ids, N, **args)
    assert torch.equal(got[:, :T], ids) and torch.equal(got[:, T:], want), (layout, kw)
    # a ready StopRows is used as it is and reads out why every row ended
    tracker = StopRows([p.capped(N) for p in stops], "cuda", model.config.vocab_size, PAD)
    assert torch.equal(model.generate(ids, N, attention_mask=mask, stopping=tracker, pad_token_id=PAD, **kw), got)
    assert list(zip(tracker.length.tolist(), tracker.reason.tolist(), tracker.index.tolist())) == res
    assert tracker.n_live.tolist() == [0]
    # the keyword form: the same conditions for every row
    both = StopParams([int(new[0, 5])], [new[1, 9:11].tolist()])
    want_kw, _ = _cut(new, [both] * 3)
    kwargs = dict(attention_mask=mask, stop_token_ids=[int(new[0, 5])], stop_sequences=[new[1, 9:11].tolist()], pad_token_id=PAD, **kw)
    got_kw = model.generate(ids, N, **kwargs)
    assert torch.equal(got_kw[:, T:], want_kw)
    # the graphed call returns exactly that, however often it looks
    for sync_every in (1, 4, 16):
        assert torch.equal(model.generate_graphed(ids, N, sync_every=sync_every, **args), got), (layout, kw, sync_every)
        assert torch.equal(model.generate_graphed(ids, N, sync_every=sync_every, **kwargs), got_kw), (layout, kw, sync_every)
    assert torch.equal(model.generate_graphed(ids, N, sync_every=None, **args), got)
    if layout == "mfma":
        assert model.graphs.stats[1] >= 1 and model.graphs.stats[2] >= N // 2      # captured, then replayed


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_eos_list_equals_the_torch_path_of_one_eos(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 72)
    ids, mask = _batch(6)
    T, n = ids.shape[1], 12
    for kw in (dict(), SAMPLED):
        free = model.generate(ids, n, attention_mask=mask, **kw)
        e = int(free[0, T + 3])
        a = model.generate(ids, n, attention_mask=mask, eos_token_id=e, pad_token_id=PAD, **kw)
        b = model.generate(ids, n, attention_mask=mask, eos_token_id=[e], pad_token_id=PAD, **kw)
        assert torch.equal(a, b) and bool((a[0, T:] == e).any()), (layout, kw)
        a = model.generate(ids, n, attention_mask=mask, eos_token_id=e, pad_token_id=PAD, return_logprobs=True, top_logprobs=5, **kw)
        b = model.generate(ids, n, attention_mask=mask, eos_token_id=[e], pad_token_id=PAD, return_logprobs=True, top_logprobs=5, **kw)
        assert torch.equal(a[0], b[0]) and _bits_equal(a[1], b[1]) and torch.equal(a[2], b[2]) and _bits_equal(a[3], b[3])
        g = model.generate_graphed(ids, n, attention_mask=mask, eos_token_id=e, pad_token_id=PAD, return_logprobs=True,
                                   top_logprobs=5, **kw)
        assert torch.equal(a[0], g[0]) and _bits_equal(a[1], g[1]) and torch.equal(a[2], g[2]) and _bits_equal(a[3], g[3])
        # every row ends on e: the width is the longest row, in all three
        rows = [free[r, T:].tolist() for r in range(3)]
        ends = [int(free[r, T + 2 + r]) for r in range(3)]
        stops = [StopParams([t]) for t in ends]
        width = max(reference_stop(row, p)[0] for row, p in zip(rows, stops))
        a = model.generate(ids, n, attention_mask=mask, stopping=stops, pad_token_id=PAD, return_logprobs=True, **kw)
        g = model.generate_graphed(ids, n, attention_mask=mask, stopping=stops, pad_token_id=PAD, return_logprobs=True, **kw)
        assert a[0].shape[1] == T + width < T + n and a[1].shape == (3, width)
        assert torch.equal(a[0], g[0]) and _bits_equal(a[1], g[1])


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_graphed_equals_eager_with_penalties_and_scores(layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 73)
    ids, mask = _batch(8)
    T = ids.shape[1]
    rows = [SamplingParams(temperature=0.8, top_k=40, seed=5, repetition_penalty=1.3),
            SamplingParams(do_sample=False, frequency_penalty=0.4, presence_penalty=0.2), SamplingParams(temperature=1.2, top_k=0, seed=6)]
    free = model.generate(ids, N, attention_mask=mask, sampling=rows)
    stops = _stops_from(free[:, T:])
    want, res = _cut(free[:, T:], stops)
    args = dict(attention_mask=mask, sampling=rows, stopping=stops, pad_token_id=PAD, return_logprobs=True, top_logprobs=3)
    eager = model.generate(ids, N, **args)
    assert torch.equal(eager[0][:, T:], want) and eager[1].shape == (3, N) and eager[2].shape == (3, N, 3)
    for b, (length, _, _) in enumerate(res):                                     # the pads of a finished row: 0 and id -1
        assert bool((eager[1][b, length:] == 0).all()) and bool((eager[2][b, length:] == -1).all())
        assert bool((eager[3][b, length:] == 0).all()) and bool((eager[2][b, :length] >= 0).all())
    for sync_every in (1, 4, 16):
        got = model.generate_graphed(ids, N, sync_every=sync_every, **args)
        assert torch.equal(got[0], eager[0]) and _bits_equal(got[1], eager[1]), (layout, sync_every)
        assert torch.equal(got[2], eager[2]) and _bits_equal(got[3], eager[3]), (layout, sync_every)
    two = model.generate_graphed(ids, N, attention_mask=mask, sampling=rows, stopping=stops, pad_token_id=PAD, return_logprobs=True)
    assert len(two) == 2 and torch.equal(two[0], eager[0]) and _bits_equal(two[1], eager[1])


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_early_finish_replay_and_no_stale_stopper(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 74)
    ids, mask = _batch(9)
    T = ids.shape[1]
    free = model.generate(ids, N, attention_mask=mask)
    new = free[:, T:]
    # every row stops at its 2nd token: 2 new columns, although the host looks only every 16 steps
    stops = [StopParams((), [new[b, :2].tolist()]) for b in range(3)]
    eager = model.generate(ids, N, attention_mask=mask, stopping=stops, pad_token_id=PAD)
    early = model.generate_graphed(ids, N, attention_mask=mask, stopping=stops, pad_token_id=PAD, sync_every=16)
    assert eager.shape[1] == T + 2 and torch.equal(eager, free[:, : T + 2]) and torch.equal(early, eager)
    one = model.generate_graphed(ids, N, attention_mask=mask, stopping=StopParams(max_new_tokens=1), pad_token_id=PAD)
    assert torch.equal(one, free[:, : T + 1])
    # other stop keywords find the same DecodeGraphs: the tracker's buffers are the model's, only its records change
    held = model.graphs
    layers = None if layout == "mfma" else (held.pre_graphs, list(held.pre_graphs), list(held.post_graphs))
    key = held.stopper.key()
    a = model.generate_graphed(ids, N, attention_mask=mask, eos_token_id=int(new[0, 7]), pad_token_id=PAD)
    assert model.graphs is held and held.stopper.key() == key
    assert held.matches(3, layout == "mfma", True, None, False, None, key) and not held.matches(3, layout == "mfma", True, None)
    assert torch.equal(a, model.generate(ids, N, attention_mask=mask, eos_token_id=int(new[0, 7]), pad_token_id=PAD))
    b = model.generate_graphed(ids, N, attention_mask=mask, stop_sequences=[new[2, 3:6].tolist()], stop_token_ids=[int(new[1, 4])],
                               pad_token_id=PAD)
    assert model.graphs is held
    assert torch.equal(b, model.generate(ids, N, attention_mask=mask, stop_sequences=[new[2, 3:6].tolist()],
                                         stop_token_ids=[int(new[1, 4])], pad_token_id=PAD))
    if layers is None:
        assert held.stats[2] >= 1                                                   # the whole-step form replays
    else:
        assert held.pre_graphs is layers[0] and all(x is y for x, y in zip(held.pre_graphs, layers[1]))
        assert all(x is y for x, y in zip(held.post_graphs, layers[2]))            # the per-layer graphs were not built again
    # a call without any stop argument after one with: nothing stale is replayed
    assert torch.equal(model.generate_graphed(ids, 8, attention_mask=mask), model.generate(ids, 8, attention_mask=mask))
    assert model.graphs is not held and model.graphs.stopper is None
    assert torch.equal(model.generate_graphed(ids, 8), model.generate(ids, 8))


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_finishes_by_the_rule(layout, monkeypatch):
    from kivi_amd.serving import check_stopping
    from test_admit_gpu import LENS, _prompts
    _layouts(monkeypatch, layout)
    model = _model(4, 75)
    prompts = _prompts(5, LENS)
    limits = [14] * 7
    free = [t.tolist() for t in model.generate_continuous(prompts, limits, 3)]
    assert all(len(f) == 14 for f in free)
    # requests 0-2 form the first batch: whatever the others do, their tokens are a prefix of the free run's.  The eos ids come
    # from the later requests and occur in none of the three
    early = set(free[0] + free[1] + free[2])
    eos = [t for r in (3, 4, 5, 6) for t in free[r][2:6] if t not in early][:2]
    assert len(eos) == 2
    stops = [StopParams([int(free[0][4])]), StopParams((), [free[1][5:7]]), StopParams(max_new_tokens=5)] + [StopParams()] * 3 + \
            [StopParams([NEVER], [[NEVER]], 3)]
    full = check_stopping(limits, eos, PAD, stops, model.config.vocab_size)
    runs = []
    for graphed in (False, True):
        toks, finish = model.generate_continuous(prompts, limits, 3, eos_token_id=eos, pad_token_id=PAD, stopping=stops,
                                                 graphed=graphed, return_finish=True)
        runs.append(([t.tolist() for t in toks], finish))
        for r, (t, f) in enumerate(zip(toks, finish)):
            t = t.tolist()
            length, why, index = reference_stop(t, full[r])
            assert why != LIVE and length == len(t) and f == (why, index), (layout, graphed, r)   # at the last token, not before
        assert toks[0].tolist() == free[0][: len(toks[0])] and finish[0][0] == TOKEN and finish[0][1] == 2
        assert toks[1].tolist() == free[1][: len(toks[1])] and finish[1] == (SEQUENCE, 0) and len(toks[1]) <= 7
        assert toks[2].tolist() == free[2][:5] and finish[2] == (LENGTH, -1) and finish[6][0] in (TOKEN, LENGTH)
    assert runs[0] == runs[1]                                                       # graphed equals eager
    # with scores the finish list comes last
    out = model.generate_continuous(prompts, limits, 3, eos_token_id=eos, pad_token_id=PAD, stopping=stops, return_logprobs=True,
                                    return_finish=True)
    assert len(out) == 3 and [t.tolist() for t in out[0]] == runs[0][0] and out[2] == runs[0][1]
    assert all(lp.shape == t.shape for lp, t in zip(out[1], out[0]))


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_graphed_equals_generate_at_the_edge_lengths(layout, n, monkeypatch):
    """max_new_tokens 1 and 2 -- no graphed step and one with finish conditions, one and two without --, scores and lists with them;
    with the conditions row 0 ends at its first token, so at n = 2 its second column is a pad with masked scores."""
    _layouts(monkeypatch, layout)
    model = _model(4, 76)
    ids, mask = _batch(10)
    T = ids.shape[1]
    first = int(model.generate(ids, 1, attention_mask=mask)[0, T])
    stops = [StopParams([first]), StopParams(), StopParams([NEVER])]
    for how in (dict(), dict(stopping=stops, pad_token_id=PAD)):
        args = dict(attention_mask=mask, return_logprobs=True, top_logprobs=3, **how)
        eager, got = model.generate(ids, n, **args), model.generate_graphed(ids, n, **args)
        assert eager[0].shape == (3, T + n) and eager[1].shape == (3, n) and eager[2].shape == eager[3].shape == (3, n, 3)
        assert torch.equal(got[0], eager[0]) and _bits_equal(got[1], eager[1]), (layout, n, how)
        assert torch.equal(got[2], eager[2]) and _bits_equal(got[3], eager[3]), (layout, n, how)
        assert torch.equal(model.generate_graphed(ids, n, attention_mask=mask, **how), eager[0])
        if how and n == 2:
            assert eager[0][0, T:].tolist() == [first, PAD] and eager[1][0, 1] == 0 and eager[2][0, 1].tolist() == [-1] * 3
