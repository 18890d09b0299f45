"""CPU: the finish tracker without a device -- the C entry's declaration and refusals, the validation of
StopParams / StopRows and of the generate calls, reference_stop on hand-written streams, and decode_loop driven by a fake tracker."""
import ctypes

import pytest
import torch

from kivi_amd.generation import decode_loop
from kivi_amd.stopping import LENGTH, LIVE, SEQUENCE, TOKEN, StopParams, StopRows, StopState, reference_stop


# ------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_is_declared_exported_and_additive(lib):
    from test_abi_cpu import _declared_symbols
    from kivi_amd import _lib
    assert "kivi_stop_rows" in _declared_symbols() and "kivi_stop_rows" in _lib.SIGNATURES and hasattr(lib, "kivi_stop_rows")
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    assert (_lib.STOP_MAX_IDS, _lib.STOP_MAX_SEQS, _lib.STOP_MAX_LEN) == (16, 8, 16)
    from kivi_amd import stopping
    assert ctypes.sizeof(stopping.StopParamsRecord) == 624 and ctypes.sizeof(stopping.StopStateRecord) == 80
    import os
    import re
    from helpers import ROOT
    header = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    for name, value in (("KIVI_STOP_MAX_IDS", 16), ("KIVI_STOP_MAX_SEQS", 8), ("KIVI_STOP_MAX_LEN", 16)):
        assert re.search(rf"#define {name} {value}\b", header)


def test_entry_refuses_before_any_device_call(lib):
    """Pointers that are never dereferenced: every refusal happens before a HIP call."""
    P, S, T, L, R = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000        # params, state, tokens, n_live, rows: aligned, never read

    def call(tok=T, stride=1, params=P, state=S, rows=None, rows_bytes=4, n=2, B=4, n_live=L):
        return lib.kivi_stop_rows(tok, stride, params, state, rows, rows_bytes, n, B, 0, n_live, None)

    for kw, word in ((dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"), (dict(n=-1), b"n=-1"), (dict(n=5), b"without a rows map"),
                     (dict(rows=R, rows_bytes=2), b"rows_bytes=2"), (dict(stride=0), b"tok_stride"),
                     (dict(params=None), b"null"), (dict(state=None), b"null"), (dict(n_live=None), b"null"),
                     (dict(tok=None), b"null tokens")):
        assert call(**kw) == -1, kw
        assert word in lib.kivi_last_error(), (kw, lib.kivi_last_error())
    for kw in (dict(tok=T + 4), dict(params=P + 4), dict(state=S + 4), dict(n_live=L + 2), dict(rows=R + 4, rows_bytes=8),
               dict(rows=R + 2, rows_bytes=4)):
        assert call(**kw) == -2, kw
        assert b"misaligned" in lib.kivi_last_error()


# ------------------------------------------------------------------ validation
def test_stop_params_validation():
    p = StopParams([3, 4], [[1, 2], (5,)], 7)
    assert p.stop_token_ids == (3, 4) and p.stop_sequences == ((1, 2), (5,)) and p.max_new_tokens == 7 and p.limit == 7
    assert StopParams().limit == 2 ** 31 - 1 and hash(p) == hash(StopParams((3, 4), ((1, 2), (5,)), 7))
    StopParams(list(range(16)), [list(range(16))] * 8)                                   # the caps themselves
    for bad in (dict(stop_token_ids=list(range(17))), dict(stop_sequences=[[1]] * 9), dict(stop_sequences=[list(range(17))]),
                dict(stop_sequences=[[1], []]), dict(stop_token_ids=[-1]), dict(stop_sequences=[[2, -3]]),
                dict(stop_token_ids=[1.5]), dict(stop_token_ids=[True]), dict(max_new_tokens=0), dict(max_new_tokens=-2),
                dict(max_new_tokens=2.0), dict(stop_sequences=5)):
        with pytest.raises(ValueError):
            StopParams(**bad)
    with pytest.raises(dataclasses_error()):
        p.max_new_tokens = 3
    rec = p.record()
    assert rec.shape == (156,) and rec[:4].tolist() == [2, 2, 7, 0] and rec[4:6].tolist() == [3, 4]
    assert rec[20:22].tolist() == [2, 1] and rec[28:30].tolist() == [1, 2] and rec[44] == 5


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_stop_rows_validation_without_a_device():
    rows = StopRows([StopParams([1]), StopParams(stop_sequences=[[2, 3]], max_new_tokens=4)], "cpu", vocab_size=10)
    assert rows.B == 2 and rows.params.shape == (2, 156) and rows.state.shape == (2, 20) and rows.n_live.tolist() == [2]
    assert rows.reason.tolist() == [0, 0] and rows.index.tolist() == [-1, -1] and rows.length.tolist() == [0, 0]
    assert rows.key()[:2] == ("stop", 2) and StopRows(StopParams(), "cpu", B=3).B == 3
    for bad in (dict(params=[]), dict(params=[StopParams(), 3]), dict(params=StopParams(), B=0),
                dict(params=[StopParams()], B=2), dict(params=StopParams([10]), vocab_size=10),
                dict(params=StopParams(stop_sequences=[[1, 11]]), vocab_size=10), dict(params=StopParams(), vocab_size=0),
                dict(params=StopParams(), pad_token_id=None)):
        with pytest.raises(ValueError):
            StopRows(device="cpu", **bad)
    for b, p in ((2, StopParams()), (-1, StopParams()), (0, None), (0, StopParams([10]))):
        with pytest.raises(ValueError):
            rows.set_row(b, p)
    with pytest.raises(ValueError):
        rows.rebind([StopParams()])
    from kivi_amd._lib import KiviHipError
    with pytest.raises(KiviHipError):                    # no CPU path: a call on CPU buffers is an error, not a torch fallback
        rows(torch.zeros((2, 1), dtype=torch.long))


def _cpu_model():
    from kivi_amd.attention import LlamaAttention_KIVI
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64), residual_length=32)
    return LlamaForCausalLM_KIVI(cfg, LlamaAttention_KIVI)


def test_generate_calls_refuse_before_any_device_work():
    model = _cpu_model()
    ids = torch.zeros((2, 5), dtype=torch.long)
    sp = StopParams([3])
    for gen in (model.generate, model.generate_graphed):
        with pytest.raises(ValueError, match="cannot be combined"):
            gen(ids, 3, stopping=sp, stop_sequences=[[1, 2]], pad_token_id=0)
        with pytest.raises(ValueError, match="cannot be combined"):
            gen(ids, 3, stopping=sp, eos_token_id=1, pad_token_id=0)
        with pytest.raises(ValueError, match="pad_token_id"):
            gen(ids, 3, stop_sequences=[[1, 2]])
        with pytest.raises(ValueError, match="pad_token_id"):
            gen(ids, 3, eos_token_id=[1, 2])
        with pytest.raises(ValueError, match="pad_token_id"):
            gen(ids, 3, stopping=sp)
        with pytest.raises(ValueError, match="vocabulary"):
            gen(ids, 3, stop_token_ids=[64], pad_token_id=0)
        with pytest.raises(ValueError, match="for a batch of 2"):
            gen(ids, 3, stopping=[sp] * 3, pad_token_id=0)
        with pytest.raises(ValueError, match="at most 16"):
            gen(ids, 3, eos_token_id=list(range(9)), stop_token_ids=list(range(8)), pad_token_id=0)
        with pytest.raises(ValueError, match="holds 3 rows"):
            gen(ids, 3, stopping=StopRows(sp, "cpu", B=3), pad_token_id=0)
    with pytest.raises(ValueError, match="sync_every"):
        model.generate_graphed(ids, 3, eos_token_id=1, pad_token_id=0, sync_every=0)
    with pytest.raises(ValueError, match="beam search"):
        model.generate(ids, 3, num_beams=2, stop_sequences=[[1, 2]], pad_token_id=0)
    with pytest.raises(ValueError, match="beam search"):
        model.generate(ids, 3, num_beams=2, stopping=sp, pad_token_id=0)
    with pytest.raises(ValueError, match="beam search"):
        model.generate(ids, 3, num_beams=2, eos_token_id=[1, 2], pad_token_id=0)


def test_generate_continuous_refusals():
    from kivi_amd.serving import check_stopping
    model = _cpu_model()
    prompts = [[1, 2, 3], [4, 5], [6]]
    with pytest.raises(ValueError, match="2 StopParams for 3 requests"):
        model.generate_continuous(prompts, 4, 2, stopping=[StopParams([1])] * 2)
    with pytest.raises(ValueError, match="StopParams"):
        model.generate_continuous(prompts, 4, 2, stopping=[StopParams([1]), 5, None])
    with pytest.raises(ValueError, match="vocabulary"):
        model.generate_continuous(prompts, 4, 2, stopping=StopParams([64]))
    with pytest.raises(ValueError, match="pad_token_id"):
        model.generate_continuous(prompts, 4, 2, pad_token_id=None, stopping=StopParams([1]))
    with pytest.raises(ValueError, match="at most 16"):
        model.generate_continuous(prompts, 4, 2, eos_token_id=[1, 2], stopping=StopParams(list(range(15))))
    got = check_stopping([4, 9, 2], [7, 8], 0, [StopParams([1], [[2, 3]], 6), StopParams(), StopParams(max_new_tokens=5)], 64)
    assert [p.stop_token_ids for p in got] == [(7, 8, 1), (7, 8), (7, 8)] and [p.limit for p in got] == [4, 9, 2]
    assert got[0].stop_sequences == ((2, 3),)


# ------------------------------------------------------------------ the rule on hand-written streams
def test_reference_stop_priorities_and_edges():
    a, b, c = 1, 2, 3
    assert reference_stop([5, 6, 7], StopParams()) == (3, LIVE, -1)
    # stop id and limit on the same token: the id wins; two ids: the lowest position in the list
    assert reference_stop([5, 6, a, 9], StopParams([4, a], max_new_tokens=3)) == (3, TOKEN, 1)
    assert reference_stop([5, 6, 7, 9], StopParams([4, a], max_new_tokens=3)) == (3, LENGTH, -1)
    # an id beats a sequence that ends on the same token; a sequence beats the limit
    assert reference_stop([b, a], StopParams([a], [[b, a]])) == (2, TOKEN, 0)
    assert reference_stop([b, a], StopParams((), [[b, a]], 2)) == (2, SEQUENCE, 0)
    # two sequences ending on the same token: the lowest index
    assert reference_stop([c, b, a], StopParams((), [[c, b, a], [b, a], [a]])) == (3, SEQUENCE, 0)
    assert reference_stop([c, b, a, a], StopParams((), [[c, c], [b, a], [a]])) == (3, SEQUENCE, 1)
    # a sequence that overlaps itself
    assert reference_stop([a, a, a, b, 7], StopParams((), [[a, a, b]])) == (4, SEQUENCE, 0)
    # m > produced: the sequence's tail alone is no match, and a prompt never takes part
    assert reference_stop([b], StopParams((), [[a, b]])) == (1, LIVE, -1)
    assert reference_stop([b, a, b], StopParams((), [[a, b]])) == (3, SEQUENCE, 0)
    # limit = 1
    assert reference_stop([9, 9], StopParams(max_new_tokens=1)) == (1, LENGTH, -1)
    assert reference_stop([a, 9], StopParams([a], max_new_tokens=1)) == (1, TOKEN, 0)


def test_reference_stop_sixteen_tokens_across_the_ring_wrap():
    seq = list(range(20, 36))                                            # 16 tokens
    p = StopParams((), [seq])
    assert reference_stop(seq + [1], p) == (16, SEQUENCE, 0)            # ends at token 16: the ring is exactly full
    assert reference_stop([7] + seq + [1], p) == (17, SEQUENCE, 0)      # ends at token 17: the ring has wrapped by one
    assert reference_stop([7] * 21 + seq, p) == (37, SEQUENCE, 0)       # wrapped twice
    assert reference_stop(seq[1:] + [1], p) == (16, LIVE, -1)           # 15 of the 16


def test_nothing_after_the_finish_changes_the_result():
    p = StopParams([4], [[2, 3]], 6)
    for stream in ([1, 2, 3], [4], [1, 1, 1, 1, 1, 1]):
        want = reference_stop(stream, p)
        assert want[1] != LIVE and want[0] == len(stream)
        for tail in ([4], [2, 3], [9] * 20):
            assert reference_stop(stream + tail, p) == want
        st = StopState(p)
        for t in stream + [4, 2, 3]:
            st.push(t)
        assert (st.produced, st.reason, st.index) == want


# ------------------------------------------------------------------ decode_loop with a tracker (scripted logits, as tests/test_generation_cpu.py)
B, V, N, PAD = 2, 5, 4, 9
SCRIPT = [(1, 2), (3, 2), (4, 0), (0, 1), (2, 2)]


def _logits(toks):
    lg = torch.zeros((B, 1, V))
    for b, t in enumerate(toks):
        lg[b, 0, t] = 1.0
    return lg


class _Driver:
    def __init__(self, script=SCRIPT):
        self.script, self.fed, self.picks = script, [], 0

    def step(self, tok):
        assert tok.shape == (B, 1) and tok.dtype == torch.int64
        self.fed.append(tok[:, 0].tolist())
        return _logits(self.script[len(self.fed)])

    def pick(self, logits):
        self.picks += 1
        return logits.argmax(-1)


class _FakeTracker:
    """The protocol decode_loop asks of a tracker, on CPU tensors, over the Python rule."""

    def __init__(self, params):
        self.states, self.calls, self.reads = [StopState(p) for p in params], 0, 0

    @property
    def reason(self):
        return torch.tensor([s.reason for s in self.states], dtype=torch.int32)

    @property
    def n_live(self):
        self.reads += 1
        return torch.tensor([sum(s.reason == LIVE for s in self.states)], dtype=torch.int32)

    def __call__(self, tok):
        self.calls += 1
        for b, s in enumerate(self.states):
            if s.reason != LIVE:
                tok[b, 0] = PAD
            else:
                s.push(int(tok[b, 0]))
        return tok


def _run(params, script=SCRIPT, n=N):
    d, tr = _Driver(script), _FakeTracker(params)
    toks, lps = decode_loop(_logits(script[0]), d.step, d.pick, n, want_logprobs=False, stopper=tr)
    assert lps is None and toks.dtype == torch.int64
    return toks.tolist(), d, tr


def test_loop_feeds_pads_and_stops_when_no_row_is_live():
    # row 0 stops on token 3 (its second), row 1 on the sequence [2, 0] (its third): two steps, no pass after the last token
    toks, d, tr = _run([StopParams([3]), StopParams((), [[2, 0]])])
    assert toks == [[1, 3, PAD], [2, 2, 0]]
    assert d.fed == [[1, 2], [3, 2]] and d.picks == 3 and tr.calls == 3 and tr.reads == 3      # one read per token
    assert [(s.produced, s.reason, s.index) for s in tr.states] == [(2, TOKEN, 0), (3, SEQUENCE, 0)]


def test_loop_with_a_live_row_runs_the_pass_after_the_last_token():
    toks, d, tr = _run([StopParams([3]), StopParams()])                  # row 1 has no condition at all
    assert toks == [[1, 3, PAD, PAD], [2, 2, 0, 1]]
    assert d.fed == [[1, 2], [3, 2], [PAD, 0], [PAD, 1]] and d.picks == N + 1 and tr.calls == N
    assert tr.states[1].produced == N                                    # the trailing pick is not counted


def test_length_is_a_finish_like_any_other():
    toks, d, tr = _run([StopParams(max_new_tokens=N)] * 2)
    assert toks == [[1, 3, 4, 0], [2, 2, 0, 1]] and len(d.fed) == N - 1 and d.picks == N
    assert [s.reason for s in tr.states] == [LENGTH, LENGTH]
    toks, d, tr = _run([StopParams(max_new_tokens=1), StopParams(max_new_tokens=2)])
    assert toks == [[1, PAD], [2, 2]] and d.fed == [[1, 2]]


def test_tracker_and_eos_exclude_each_other():
    d = _Driver()
    with pytest.raises(ValueError, match="not both"):
        decode_loop(_logits(SCRIPT[0]), d.step, d.pick, 2, eos_token_id=3, pad_token_id=PAD, stopper=_FakeTracker([StopParams()] * 2))


def test_finished_rows_score_the_ignore_index(monkeypatch):
    """want_logprobs: a row that was not live before its token scores target -100 (the scorer is replaced: it needs the GPU)."""
    import kivi_amd.scoring as S
    seen = []
    monkeypatch.setattr(S, "token_logprobs", lambda lg, tgt: seen.append(tgt[:, 0].tolist()) or torch.zeros(tgt.shape))
    d, tr = _Driver(), _FakeTracker([StopParams([3]), StopParams(max_new_tokens=4)])
    toks, lps = decode_loop(_logits(SCRIPT[0]), d.step, d.pick, N, want_logprobs=True, stopper=tr)
    assert toks.tolist() == [[1, 3, PAD, PAD], [2, 2, 0, 1]] and lps.shape == (B, N)
    assert seen == [[1, 2], [3, 2], [-100, 0], [-100, 1]]
