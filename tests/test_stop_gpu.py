"""GPU: kivi_stop_rows against reference_stop (kivi_amd/stopping.py), integer for integer after every step."""
import random

import pytest
import torch

from kivi_amd.stopping import LENGTH, LIVE, SEQUENCE, TOKEN, StopParams, StopRows, StopState

pytestmark = pytest.mark.gpu

V, STEPS, PAD = 6, 40, 77


def _params(rng, kind):
    tok = lambda: rng.randrange(V)                                                    # noqa: E731
    limit = rng.choice([None, None, rng.randrange(1, STEPS + 6)])
    if kind == 0:
        return StopParams()                                                           # no stops at all: never finishes
    if kind == 1:                                                                     # 16 ids, one of them reachable, at any position
        ids = [100 + j for j in range(16)]
        ids[rng.randrange(16)] = tok()
        return StopParams(ids, (), limit)
    if kind == 2:                                                                     # 8 sequences of lengths 1, 2 and 16
        lens = [16, 2, 16, 2, 1, 2, 16, 2]
        rng.shuffle(lens)
        seqs = [[tok() for _ in range(m)] for m in lens]
        for s in seqs:
            if len(s) == 1:
                s[0] = V + 3                                                          # (a reachable 1-sequence would end every such row at once)
        return StopParams((), seqs, limit)
    if kind == 3:
        return StopParams([tok()] if rng.random() < 0.3 else [V + 1],
                          [[tok() for _ in range(rng.choice([2, 3, 3, 4, 5]))] for _ in range(rng.randrange(1, 4))], limit)
    return StopParams((), (), rng.randrange(1, STEPS + 6))                            # a limit alone


def _case(B, seed):
    """Streams, parameters and the reference's trace: per step the token buffer after the call and (produced, reason, index) of
    every row, and n_live.  Rows 1-3 (B > 3) get planted sequences that end across the ring's wrap."""
    rng = random.Random(seed)
    streams = [[rng.randrange(V) for _ in range(STEPS)] for _ in range(B)]
    params = [_params(rng, rng.randrange(5) if b else 2) for b in range(B)]
    if B > 3:
        params[1] = StopParams((), [[V + 2], streams[1][14:18]])                      # tokens 15-18: slots 14, 15, 0, 1
        params[2] = StopParams((), [streams[2][5:21]])                                # 16 tokens ending at token 21
        params[3] = StopParams((), [[V + 1, V + 1], streams[3][31:34]], 39)           # across the second wrap
    states = [StopState(p) for p in params]
    trace = []
    for s in range(STEPS):
        toks = []
        for b, st in enumerate(states):
            toks.append(streams[b][s] if st.reason == LIVE else PAD)
            st.push(streams[b][s])
        trace.append((toks, [(st.produced, st.reason, st.index) for st in states], sum(st.reason == LIVE for st in states)))
    return streams, params, trace


def _straddles(params, final):
    """Rows whose matched sequence lies across a multiple of 16 produced tokens (the ring's wrap)."""
    return [b for b, (p, why, j) in enumerate(final)
            if why == SEQUENCE and (p - len(params[b].stop_sequences[j])) // 16 != (p - 1) // 16]


def test_the_reference_run_is_not_vacuous():
    """On the CPU side alone: the B = 70 case holds every reason, a live row at the end and matches across the ring's wrap."""
    _, params, trace = _case(70, 10)
    final = trace[-1][1]
    reasons = [why for _, why, _ in final]
    assert {LIVE, TOKEN, SEQUENCE, LENGTH} <= set(reasons) and trace[-1][2] >= 1
    assert {1, 2, 3} <= set(_straddles(params, final))
    assert final[2] == (21, SEQUENCE, 0) and final[1] == (18, SEQUENCE, 1) and final[3] == (34, SEQUENCE, 1)
    assert any(len(p.stop_token_ids) == 16 and why == TOKEN and j > 0 for p, (_, why, j) in zip(params, final))
    assert any(len(p.stop_sequences) == 8 and why == SEQUENCE for p, (_, why, _) in zip(params, final))
    assert any(len(p.stop_sequences[j]) == 2 and n > 16 for p, (n, why, j) in zip(params, final) if why == SEQUENCE)


@pytest.mark.parametrize("B,seed,stride", [(70, 10, 1), (70, 10, 3), (1, 12, 1), (1, 13, 1)])
def test_random_streams_against_the_reference(B, seed, stride):
    streams, params, trace = _case(B, seed)
    tracker = StopRows(params, "cuda", vocab_size=200, pad_token_id=PAD)
    assert tracker.n_live.tolist() == [B]
    feed = torch.tensor(streams, dtype=torch.long, device="cuda")                    # (B, STEPS)
    buf = torch.full((B, stride), -5, dtype=torch.long, device="cuda")
    tok = buf[:, :1]
    for s, (toks, rows, n_live) in enumerate(trace):
        tok.copy_(feed[:, s: s + 1])
        assert tracker(tok) is tok
        state = tracker.state.cpu()
        assert tok[:, 0].tolist() == toks, s
        assert [tuple(r) for r in state[:, :3].tolist()] == rows, s
        assert tracker.n_live.tolist() == [n_live], s
        assert torch.equal(tracker.length.cpu(), state[:, 0]) and torch.equal(tracker.reason.cpu(), state[:, 1])
        assert torch.equal(tracker.index.cpu(), state[:, 2])
        if stride > 1:
            assert bool((buf[:, 1:] == -5).all())
    tracker.reset()
    assert tracker.n_live.tolist() == [B] and tracker.reason.tolist() == [0] * B and tracker.length.tolist() == [0] * B
    tok.copy_(feed[:, :1])
    tracker(tok)
    assert [tuple(r) for r in tracker.state[:, :3].tolist()] == trace[0][1] and tracker.n_live.tolist() == [trace[0][2]]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_rows_map(dtype):
    a = 4
    params = [StopParams([a]), StopParams((), [[1, 2]]), StopParams(max_new_tokens=2), StopParams([a], max_new_tokens=9), StopParams()]
    tracker = StopRows(params, "cuda", pad_token_id=PAD)
    ref = [StopState(p) for p in params]

    def step(rows, toks):
        before = tracker.state.clone()
        tok = torch.tensor(toks, dtype=torch.long, device="cuda").view(-1, 1)
        tracker(tok, torch.tensor(rows, dtype=dtype, device="cuda"))
        want = list(toks)
        for i, (r, t) in enumerate(zip(rows, toks)):
            if 0 <= r < len(params):
                if ref[r].reason != LIVE:
                    want[i] = PAD
                ref[r].push(t)
        assert tok[:, 0].tolist() == want
        assert [tuple(x) for x in tracker.state[:, :3].tolist()] == [(s.produced, s.reason, s.index) for s in ref]
        assert tracker.n_live.tolist() == [sum(s.reason == LIVE for s in ref)]        # the whole table, not the n entries
        untouched = [b for b in range(len(params)) if b not in rows]
        assert torch.equal(tracker.state[untouched], before[untouched])               # bit-identical, ring included
        return tok[:, 0].tolist()

    step([3, 0, 4], [1, a, 2])                    # a permuted subset, n = 3 of B = 5: row 0 stops, row 3 does not (its token is 1)
    assert [s.reason for s in ref] == [TOKEN, LIVE, LIVE, LIVE, LIVE]
    assert step([3, 7, 1], [a, 3, 1]) == [a, 3, 1]          # entry 1 is out of range: its token stays, no row sees it
    assert step([0, -1, 1], [2, 3, 2]) == [PAD, 3, 2]       # row 0 had finished; row 1 completes [1, 2]
    assert [s.reason for s in ref] == [TOKEN, SEQUENCE, LIVE, TOKEN, LIVE]
    step([2, 4, 0], [0, 0, 0])
    step([4, 2, 1], [0, 0, 0])
    assert [(s.produced, s.reason) for s in ref] == [(1, TOKEN), (2, SEQUENCE), (2, LENGTH), (2, TOKEN), (3, LIVE)]
    with pytest.raises(ValueError):
        tracker(torch.zeros((3, 1), dtype=torch.long, device="cuda"), torch.zeros(2, dtype=dtype, device="cuda"))
    with pytest.raises(ValueError):
        tracker(torch.zeros((6, 1), dtype=torch.long, device="cuda"))


def test_set_row_between_steps():
    a, b = 2, 3
    tracker = StopRows([StopParams((), [[a, b]]), StopParams([5])], "cuda", vocab_size=8, pad_token_id=PAD)

    def feed(t0, t1):
        tok = torch.tensor([[t0], [t1]], device="cuda")
        tracker(tok)
        return tok[:, 0].tolist()

    assert feed(1, 5) == [1, 5] and feed(a, 0) == [a, PAD]
    assert tracker.reason.tolist() == [LIVE, TOKEN] and tracker.n_live.tolist() == [1]
    tracker.set_row(0, StopParams((), [[a, b]]))            # the next request of the row has the same sequence
    assert tracker.length.tolist() == [0, 1] and tracker.n_live.tolist() == [1]
    assert feed(b, 0) == [b, PAD]                           # ..., a | b: no match across the binding
    assert tracker.state[0, :3].tolist() == [1, LIVE, -1]
    assert feed(a, 0) == [a, PAD] and feed(b, 0) == [b, PAD]
    assert tracker.state[0, :3].tolist() == [3, SEQUENCE, 0] and tracker.n_live.tolist() == [0]
    tracker.set_row(1, StopParams(max_new_tokens=2))        # a finished row that is rebound is live again
    assert tracker.n_live.tolist() == [1] and tracker.state[1, :3].tolist() == [0, LIVE, -1]
    assert feed(9, 5) == [PAD, 5] and feed(9, 5) == [PAD, 5]
    assert tracker.state[1, :3].tolist() == [2, LENGTH, -1] and tracker.n_live.tolist() == [0]
    tracker.rebind([StopParams([1]), StopParams([1])])
    assert tracker.n_live.tolist() == [2] and feed(1, 0) == [1, 0] and tracker.reason.tolist() == [TOKEN, LIVE]


def test_replayed_from_a_graph_equals_eager():
    """The launch is capturable: no host read, no allocation; set_row between replays is seen by the replay."""
    tracker = StopRows([StopParams([4]), StopParams((), [[1, 1]]), StopParams(max_new_tokens=3)], "cuda", pad_token_id=PAD)
    tok = torch.zeros((3, 1), dtype=torch.long, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tracker(tok)
    torch.cuda.current_stream().wait_stream(side)
    assert tracker.length.tolist() == [0, 0, 0]             # a capture records, it does not run
    ref = [StopState(p) for p in tracker.rows]
    for toks in ([1, 1, 1], [4, 1, 1], [0, 0, 0], [0, 0, 0]):
        tok.copy_(torch.tensor(toks, device="cuda").view(3, 1))
        graph.replay()
        want = [t if s.reason == LIVE else PAD for t, s in zip(toks, ref)]
        for s, t in zip(ref, toks):
            s.push(t)
        assert tok[:, 0].tolist() == want
        assert [tuple(x) for x in tracker.state[:, :3].tolist()] == [(s.produced, s.reason, s.index) for s in ref]
    assert tracker.n_live.tolist() == [0]
    tracker.set_row(2, StopParams([0]))
    tok.fill_(0)
    graph.replay()
    assert tracker.state[2, :3].tolist() == [1, TOKEN, 0] and tok[:, 0].tolist() == [PAD, PAD, 0]
