"""StreamingRecognizer on the beam search (beam_width=): the 8 recorded windows of tests/golden/streaming.npz on test_frontend_gpu.py's model -
222 decoded frames, 91 tokens, more than max_history (40) and more than the label encoder's table (16), so both clamps of the streaming
label-history rule are exercised.

A beam of one is the greedy recogniser: the same tokens, breaks and frames (on the float64 oracle the smallest gap between the two largest
logits over those 222 frames is 4.5e-3, against an f32 error of 2.8e-6 at max|logit| 5.8, so identity is a fair demand), log-probabilities
within 1e-5 + 4 * 2^-23 * max|logit| per term, the score within that times the frame count.  A beam of four is, as Python objects, the
BeamSearch(history="stream") fed the recorded encoder windows; what feed() commits is never retracted."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_beam_gpu import _well_formed
from test_frontend_gpu import _streaming_model

pytestmark = pytest.mark.gpu

N_FRAMES = 222


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "streaming.npz"))


@pytest.fixture(scope="module")
def model(z):
    prev = os.environ.pop("TTMI_PRECISION", None)
    try:
        yield _streaming_model(z)
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def _feed_all(rec, z, each=None):
    n = int(z["n_windows"])
    out = []
    for i in range(n):
        out.append(rec.feed(z["win%d" % i], last=(i == n - 1)))
        if each is not None:
            each(i)
    return out


@pytest.fixture(scope="module")
def greedy(model, z):
    from ttmi.streaming import StreamingRecognizer
    rec = StreamingRecognizer(model, details=True)
    _feed_all(rec, z)
    assert rec.result == z["tokens"].tolist() and rec.pos == N_FRAMES
    return rec


def _bound(model, rec):
    """1e-5 + 4 * 2^-23 * max|logit| over the lattice of the greedy tokens under the streaming label-history rule: every row either decoder scores"""
    frames = torch.cat([w[4][0, w[2]:w[4].shape[1] - w[3]] for w in rec.windows if w[3]], 0)
    assert frames.shape[0] == N_FRAMES
    with torch.no_grad():
        states = [model.decoder(torch.zeros(1, 1, dtype=torch.long, device="cuda"))[:, -1, :]]
        for n in range(1, len(rec.result) + 1):
            states.append(model.decoder(torch.tensor([rec.result[max(0, n - rec.max_history):n]], device="cuda"))[:, -1, :])
        logits = model.joint(frames[None].contiguous(), torch.cat(states, 0)[None].contiguous())
    return 1e-5 + 4 * 2.0 ** -23 * float(logits.float().abs().max())


def test_beam_of_one_is_the_greedy_recogniser(model, z, greedy):
    from ttmi.streaming import StreamingRecognizer
    rec = StreamingRecognizer(model, beam_width=1, details=True)
    per_window = _feed_all(rec, z)
    assert rec.result == z["tokens"].tolist()
    assert sum(per_window, []) == rec.result
    assert rec.breaks == [31, 58, 76] == greedy.breaks
    assert rec.frames == greedy.frames and rec.partial == rec.result and len(rec.nbest_results) == 1
    bound = _bound(model, greedy)
    worst = max(abs(a - b) for a, b in zip(rec.logprobs, greedy.logprobs))
    print("beam of one against greedy: max |logprob diff| = %.3e (bound %.3e), |score diff| = %.3e (bound %.3e)"
          % (worst, bound, abs(rec.score - greedy.score), N_FRAMES * bound))
    assert worst <= bound and abs(rec.score - greedy.score) <= N_FRAMES * bound
    plain = StreamingRecognizer(model, beam_width=1)
    assert sum(_feed_all(plain, z), []) == rec.result and not hasattr(plain, "frames")


def test_beam_of_four_is_the_resumable_search(model, z):
    from ttmi.streaming import StreamingRecognizer
    rec = StreamingRecognizer(model, beam_width=4)
    history = []

    def each(i):
        assert rec.partial[:len(rec.result)] == rec.result
        history.append(list(rec.result))
    per_window = _feed_all(rec, z, each)
    assert all(b[:len(a)] == a for a, b in zip(history, history[1:]))                  # nothing committed is retracted
    assert 0 < len(history[3]) < len(history[-1])                                      # ... and something is committed on the way
    assert sum(per_window, []) == rec.result == rec.nbest_results[0].tokens
    _well_formed(rec.nbest_results, N_FRAMES)
    assert len(rec.nbest_results) == 4 and rec.biases == [0.0] * 4 and rec.lm_totals == [0.0] * 4
    search = model.beam_search_state(1, 4, history="stream", max_history=rec.max_history)
    for w in rec.windows:
        left, right, enc = w[2], w[3], w[4]
        search.advance(enc[0, left:-right][None])                                      # (the last window's slice `[left:-0]` is empty)
    assert search.clock == [N_FRAMES] and search.finish() == [rec.nbest_results]
    two = StreamingRecognizer(model, beam_width=4, nbest=2)
    _feed_all(two, z)
    assert two.nbest_results == rec.nbest_results[:2]


def test_hotword_in_the_stream(model, z):
    from ttmi.context import ContextGraph
    from ttmi.streaming import StreamingRecognizer
    tokens = z["tokens"].tolist()
    phrase, boost = tokens[40:43], 2.0
    rec = StreamingRecognizer(model, beam_width=4, context=ContextGraph([phrase], boost=boost))
    per_window = _feed_all(rec, z)
    best = rec.nbest_results[0].tokens
    assert sum(per_window, []) == rec.result == best
    n = sum(best[i:i + 3] == phrase for i in range(len(best)))
    print("phrase %s: %d occurrence(s) in the best hypothesis, bias %.1f" % (phrase, n, rec.biases[0]))
    assert n >= 1 and rec.biases[0] == boost * len(phrase) * n


def test_without_a_beam_width_no_search_is_built(model, z, monkeypatch):
    import ttmi.beam
    from ttmi.streaming import StreamingRecognizer

    def refuse(*a, **k):
        raise AssertionError("the greedy path built a BeamSearch")
    monkeypatch.setattr(ttmi.beam.BeamSearch, "__init__", refuse)
    rec = StreamingRecognizer(model)
    for i in range(2):
        rec.feed(z["win%d" % i])
    assert rec.search is None and rec.result and not hasattr(rec, "nbest_results")
