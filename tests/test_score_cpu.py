"""No GPU: the fp64 restatement of kivi_token_logprob (kivi_amd/scoring.py), the argument checks of the ABI entry point, and the
argument checks of score() / perplexity() / generate(return_logprobs=True) that must come before any device work."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_reference_equals_log_softmax_gather():
    from kivi_amd.scoring import reference_token_logprobs
    g = torch.Generator().manual_seed(0)
    for x in (torch.randn((7, 33), generator=g), (torch.randn((3, 5, 320), generator=g) * 30).half(),
              torch.randn((4, 1), generator=g)):
        t = torch.randint(0, x.shape[-1], x.shape[:-1], generator=g)
        lp, lse, rank = reference_token_logprobs(x, t)
        ref = torch.log_softmax(x.double(), -1)
        assert lp.dtype == lse.dtype == torch.float64 and rank.dtype == torch.int64
        assert (lp - ref.gather(-1, t.unsqueeze(-1)).squeeze(-1)).abs().max().item() <= 1e-12
        assert (lse - torch.logsumexp(x.double(), -1)).abs().max().item() <= 1e-12
        assert torch.equal(rank == 0, x.double().argmax(-1) == t)
    # -inf logits weigh nothing; a target on one gives -inf, never NaN
    x = torch.tensor([[0.0, -float("inf"), 1.0, -float("inf")]])
    lp, lse, rank = reference_token_logprobs(x.expand(4, 4), torch.arange(4))
    assert lp[1] == lp[3] == -float("inf") and not lp.isnan().any()
    assert abs(lse[0].item() - torch.log1p(torch.exp(torch.tensor(1.0, dtype=torch.float64))).item()) <= 1e-12
    assert rank.tolist() == [1, 2, 0, 3]


def test_reference_rank_tie_rule_is_argmax():
    from kivi_amd.scoring import reference_token_logprobs
    x = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, -0.0, 0.0]]).half()
    t = torch.arange(7)
    _, _, rank = reference_token_logprobs(x.expand(7, 7), t)
    # the three 3.0 rank 0, 1, 2 in vocabulary order (argmax takes the first), then 1.0, then 0.5, then -0 and +0 (one tie class)
    assert rank.tolist() == [3, 0, 1, 4, 2, 5, 6]
    assert int(x[0].argmax()) == 1
    # a planted tie before the target costs a rank, one after it does not
    y = torch.tensor([[2.0, 5.0, 1.0, 5.0]])
    assert reference_token_logprobs(y, torch.tensor([3]))[2].item() == 1
    assert reference_token_logprobs(y, torch.tensor([1]))[2].item() == 0


def test_reference_ignore_index_and_out_of_range():
    from kivi_amd.scoring import reference_token_logprobs
    g = torch.Generator().manual_seed(1)
    x = torch.randn((6, 50), generator=g)
    t = torch.tensor([3, -100, 50, -1, 49, 7])
    lp, lse, rank = reference_token_logprobs(x, t)
    full = torch.log_softmax(x.double(), -1)
    assert lp[1].item() == 0.0 and rank[1].item() == -1
    assert lp[2].isnan() and lp[3].isnan() and rank[2].item() == rank[3].item() == -1
    for r in (0, 4, 5):                                         # the neighbours are unaffected
        assert abs(lp[r].item() - full[r, t[r]].item()) <= 1e-12 and rank[r].item() >= 0
    assert (lse - torch.logsumexp(x.double(), -1)).abs().max().item() <= 1e-12          # lse of every row, scored or not
    # another ignore_index, inside the vocabulary
    lp, _, rank = reference_token_logprobs(x, t, ignore_index=7)
    assert lp[5].item() == 0.0 and rank[5].item() == -1 and lp[1].isnan()


def test_argument_validation_without_device(lib):
    """Every rejected argument returns a negative code before any HIP call (pointers are never dereferenced)."""
    from kivi_amd._lib import KiviHipError, check
    f = lib.kivi_token_logprob
    p = ctypes.c_void_p
    lg, tg, out = p(0x10000), p(0x20000), p(0x30000)           # plausible, aligned, never dereferenced

    def call(logits=lg, bits=16, row_stride=320, N=4, V=320, targets=tg, target_stride=1, ignore=-100, o=out, lse=None,
             rank=None):
        return f(logits, bits, row_stride, N, V, targets, target_stride, ignore, o, lse, rank, None)

    for kw, word in ((dict(bits=8), b"logits_bits"), (dict(bits=64), b"logits_bits"), (dict(N=0), b"N="), (dict(N=-3), b"N="),
                     (dict(V=0), b"V="), (dict(V=(1 << 20) + 1, row_stride=1 << 21), b"V="), (dict(row_stride=319), b"row_stride"),
                     (dict(target_stride=0), b"target_stride"), (dict(logits=None), b"null"), (dict(targets=None), b"null"),
                     (dict(o=None), b"null")):
        assert call(**kw) == -1, kw
        assert word in lib.kivi_last_error(), (kw, lib.kivi_last_error())
    for kw in (dict(logits=p(0x10001)), dict(logits=p(0x10002), bits=32), dict(targets=p(0x20004)), dict(o=p(0x30002)),
               dict(lse=p(0x40001)), dict(rank=p(0x50003))):
        assert call(**kw) == -2, kw
        assert b"misaligned" in lib.kivi_last_error()
    with pytest.raises(KiviHipError):
        check(call(bits=12), "kivi_token_logprob")


def test_token_logprobs_has_no_cpu_fallback():
    from kivi_amd._lib import KiviHipError
    from kivi_amd.scoring import token_logprobs
    with pytest.raises(KiviHipError):
        token_logprobs(torch.randn(3, 10), torch.zeros(3, dtype=torch.long))


def _tiny():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=1,
                           intermediate_size=512, vocab_size=100))
    return LlamaForCausalLM_KIVI(cfg)


def test_score_and_generate_refuse_bad_arguments_before_device_work():
    """On the CPU any device work would raise KiviHipError (no CPU path), so a ValueError shows the check came first."""
    m = _tiny()
    ids = torch.randint(0, 100, (2, 12))
    for fn in (m.score, m.perplexity):
        with pytest.raises(ValueError, match="T >= 2"):
            fn(ids[:, :1])
        for fc in (0, 13, -1):
            with pytest.raises(ValueError, match="first_chunk"):
                fn(ids, first_chunk=fc)
        for cs in (0, -4):
            with pytest.raises(ValueError, match="chunk_size"):
                fn(ids, first_chunk=4, chunk_size=cs)
    bad = ids.clone()
    bad[1, 3] = 100
    with pytest.raises(ValueError, match="vocabulary"):
        m.score(bad)
    bad[1, 3] = -1
    with pytest.raises(ValueError, match="vocabulary"):
        m.score(bad, first_chunk=4, chunk_size=2)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(ids, 4, num_beams=2, return_logprobs=True)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(ids, 4, num_beams=3, return_logprobs=True, do_sample=True)


def test_score_plan_covers_every_token_once():
    from kivi_amd.scoring import score_plan
    ids = torch.zeros((1, 50), dtype=torch.long)
    assert score_plan(ids, None, None) == [(0, 50)]
    assert score_plan(ids, 50, 7) == [(0, 50)]
    assert score_plan(ids, 40, None) == [(0, 40), (40, 50)]
    assert score_plan(ids, 40, 7) == [(0, 40), (40, 47), (47, 50)]
    assert score_plan(ids, 1, 1) == [(i, i + 1) for i in range(50)]
    assert _tiny()._score_plan(ids, 40, 7) == score_plan(ids, 40, 7)           # the model still answers to the name it had


def test_row_stride_collapse():
    from kivi_amd.scoring import _row_stride
    x = torch.zeros((3, 10, 16))
    assert _row_stride(x) == 16 and _row_stride(x[:, :, :8]) == 16 and _row_stride(x[:, 2:3]) == 160
    assert _row_stride(x[:1, 2:7]) == 16 and _row_stride(x[:, 2:7]) is None and _row_stride(x[0, 0]) == 16
    assert _row_stride(x[:, 0]) == 160 and _row_stride(x.transpose(0, 1)) is None
