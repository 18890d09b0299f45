"""CPU: the decode loop of kivi_amd/generation.py driven by a scripted step (no model, no library).

`step` returns fixed logits whose argmax is the scripted next token of every row; `pick` is argmax.  What the loop does around them
is observable to callers: which tokens come out, how often the model is stepped (the caches end that many tokens on) and how often
`pick` runs (a sampler ends that many draws on).  Log-probabilities need the GPU kernel: want_logprobs=False throughout."""
import torch

from kivi_amd.generation import decode_loop

B, V, N = 2, 5, 4
# the tokens (row 0, row 1) that the logits of pass i point at: pass 0 is the prompt pass, pass i the step on token i
SCRIPT = [(1, 2), (3, 2), (4, 0), (0, 1), (2, 2)]
PAD = 9


def _logits(toks):
    lg = torch.zeros((B, 1, V))
    for b, t in enumerate(toks):
        lg[b, 0, t] = 1.0
    return lg


class _Driver:
    """The two callables of a run, counting: `step` replays `script` and records its inputs, `pick` is argmax."""

    def __init__(self, script=SCRIPT):
        self.script, self.fed, self.picks = script, [], 0

    def step(self, tok):
        assert tok.shape == (B, 1) and tok.dtype == torch.int64
        self.fed.append(tok[:, 0].tolist())
        return _logits(self.script[len(self.fed)])

    def pick(self, logits):
        self.picks += 1
        return logits.argmax(-1)

    def run(self, n=N, **kw):
        toks, lps = decode_loop(_logits(self.script[0]), self.step, self.pick, n, want_logprobs=False, **kw)
        assert lps is None and toks.dtype == torch.int64 and toks.shape[0] == B
        return toks.tolist()


def test_without_eos_the_pass_after_the_last_token_runs():
    d = _Driver()
    assert d.run() == [[1, 3, 4, 0], [2, 2, 0, 1]]
    assert len(d.fed) == N                                  # every emitted token is stepped: the caches end N tokens on
    assert d.fed == [[1, 2], [3, 2], [4, 0], [0, 1]]
    assert d.picks == N + 1                                 # and its logits are picked over: a sampler ends N + 1 draws on
    # an eos that never comes changes nothing
    e = _Driver()
    assert e.run(eos_token_id=V + 1, pad_token_id=PAD) == [[1, 3, 4, 0], [2, 2, 0, 1]] and len(e.fed) == N and e.picks == N + 1


def test_every_row_finished_breaks_before_the_pass():
    d = _Driver([(1, 2), (3, 3), (4, 0), (0, 1), (2, 2)])   # both rows produce 3 as their second token
    assert d.run(eos_token_id=3, pad_token_id=PAD) == [[1, 3], [2, 3]]
    assert d.fed == [[1, 2]] and d.picks == 2               # one step: the eos tokens themselves are not stepped


def test_finished_row_emits_pad_while_the_other_continues():
    d = _Driver()                                           # row 0 produces 3 as its second token, row 1 never does
    assert d.run(eos_token_id=3, pad_token_id=PAD) == [[1, 3, PAD, PAD], [2, 2, 0, 1]]
    assert d.fed == [[1, 2], [3, 2], [PAD, 0], [PAD, 1]]    # the finished row is stepped on its pads; a live row keeps the loop going
    assert d.picks == N + 1


def test_no_new_tokens_still_picks_once():
    d = _Driver()
    toks, lps = decode_loop(_logits(SCRIPT[0]), d.step, d.pick, 0, want_logprobs=False)
    assert toks.shape == (B, 0) and toks.dtype == torch.int64 and lps is None         # the prompt alone: nothing to append to it
    assert torch.equal(torch.cat([torch.zeros((B, 3), dtype=torch.long), toks], dim=1), torch.zeros((B, 3), dtype=torch.long))
    assert d.fed == [] and d.picks == 1
