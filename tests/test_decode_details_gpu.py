"""Decode details through the whole model: Transducer.decode_batch / decode / recognize(details=True) and StreamingRecognizer(details=True)
against a per-frame Python restatement of the reference's greedy loop (tt/model.py:70-90) that calls the joint on one frame at a time, takes
argmax and float64 log_softmax on the CPU and re-runs the label encoder on the history.  The tiny model of
test_batched_greedy_decode_equals_one_utterance_at_a_time in the fp32 mode, B = 3 with ragged lengths around 40 frames and blocks of 8
frames: blocks repeat within a symbol step and the batch shrinks.

Tolerance: log_softmax moves by at most twice the sup-norm change of its input, so a term may differ by 2 * delta + 1e-5 and the score of an
utterance by T_b times that; delta is measured here on existing code, as the largest difference between model.joint on a block of 8 frames
and on the same frames one at a time."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [40, 37, 29]
BLOCK = 8


def _model():
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=2, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    torch.manual_seed(9)
    model = Transducer(cfg).cuda().eval()
    with torch.no_grad():
        model.joint.project_layer.bias[0] += 0.9             # some blank frames between the emissions
    return model


@torch.no_grad()
def _restate(model, enc, T):
    """the reference loop on one utterance -> (tokens, frames, logprobs, score): one joint call per frame, CPU argmax, float64 log_softmax"""
    toks, frames, lps, score = [0], [], [], 0.0
    dstate = model.decoder(torch.tensor([toks], device="cuda"))[:, -1, :]
    for t in range(T):
        z = model.joint(enc[t].view(-1), dstate.view(-1)).float().cpu()
        ls = torch.log_softmax(z.double(), dim=0)
        pred = int(torch.argmax(z))
        score += float(ls[pred])
        if pred != 0:
            toks.append(pred)
            frames.append(t)
            lps.append(float(ls[pred]))
            dstate = model.decoder(torch.tensor([toks], device="cuda"))[:, -1, :]
    return toks[1:], frames, lps, score


@pytest.fixture(scope="module")
def ctx():
    """model, inputs, encoder states, the restatement of every utterance and the measured delta: computed once, read by every test"""
    import os
    prev = os.environ.pop("TTMI_PRECISION", None)            # the fp32 mode, as the batched-decode tests run (the default)
    try:
        model = _model()
        x = torch.randn(3, 40, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        with torch.no_grad():
            enc = model.encoder(x)
            want = [_restate(model, enc[b], LENS[b]) for b in range(3)]
            delta = 0.0
            dstate = model.decoder(torch.zeros(1, 1, dtype=torch.long, device="cuda"))[:, -1:, :]
            for b in range(3):
                for t0 in range(0, LENS[b] - BLOCK + 1, BLOCK):
                    blk = model.joint(enc[b, t0:t0 + BLOCK].unsqueeze(0), dstate)[0, :, 0, :].float()
                    one = torch.stack([model.joint(enc[b, t].view(-1), dstate.view(-1)).float() for t in range(t0, t0 + BLOCK)])
                    delta = max(delta, float((blk - one).abs().max()))
        print("delta (joint on a block of %d frames vs one frame at a time) = %.3e" % (BLOCK, delta))
        yield dict(model=model, x=x, enc=enc, want=want, tol=2 * delta + 1e-5)
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def _check(res, want, T, tol, what=""):
    from tt.model import DecodeResult
    tokens, frames, lps, score = want
    assert isinstance(res, DecodeResult)
    assert res.tokens == tokens and res.frames == frames, (what, res, want)
    assert all(a < b for a, b in zip(res.frames, res.frames[1:])) and all(0 <= f < T for f in res.frames), what
    assert len(res.logprobs) == len(tokens)
    for got, w in zip(res.logprobs, lps):
        assert abs(got - w) <= tol, (what, got, w, tol)
    print("%s score %.6f (restatement %.6f), max logprob difference %.3e, bound per term %.3e"
          % (what, res.score, score, max([abs(g - w) for g, w in zip(res.logprobs, lps)] or [0.0]), tol))
    assert abs(res.score - score) <= T * tol, (what, res.score, score, T * tol)


def test_details_match_the_per_frame_restatement(ctx):
    model, enc, want, tol = ctx["model"], ctx["enc"], ctx["want"], ctx["tol"]
    assert all(0 < len(w[0]) < T for w, T in zip(want, LENS)) and len({len(w[0]) for w in want}) > 1       # blank frames, and the batch shrinks
    plain = model.decode_batch(enc, LENS, block=BLOCK)
    res = model.decode_batch(enc, LENS, block=BLOCK, details=True)
    assert [r.tokens for r in res] == plain == [model.decode(enc[b], LENS[b]) for b in range(3)]
    assert plain == [w[0] for w in want]
    for b in range(3):
        _check(res[b], want[b], LENS[b], tol, "utterance %d" % b)
        assert isinstance(res[b].score, float) and all(isinstance(v, float) for v in res[b].logprobs)
        assert all(isinstance(v, int) for v in res[b].tokens + res[b].frames)
    assert model.decode_batch(enc, LENS, block=BLOCK) == plain           # details leave nothing behind that changes a plain run
    again = model.decode_batch(enc, LENS, block=BLOCK, details=True)
    assert again == res                                                  # no atomics in the sums: the same floats in every run


@pytest.mark.parametrize("graphs,shrink", [(True, True), (False, True), (True, False), (False, False)])
def test_details_with_and_without_graphs_and_shrinking(ctx, graphs, shrink):
    model, enc, want, tol = ctx["model"], ctx["enc"], ctx["want"], ctx["tol"]
    model.config["decode_batch_graphs"], model.config["decode_batch_shrink"] = graphs, shrink
    try:
        for block in (BLOCK, 64):
            res = model.decode_batch(enc, LENS, block=block, details=True)
            for b in range(3):
                _check(res[b], want[b], LENS[b], tol, "graphs=%s shrink=%s block=%d utterance %d" % (graphs, shrink, block, b))
    finally:
        model.config["decode_batch_graphs"] = model.config["decode_batch_shrink"] = None


def test_decode_and_recognize_with_details(ctx):
    model, x, enc, want, tol = ctx["model"], ctx["x"], ctx["enc"], ctx["want"], ctx["tol"]
    batch = model.decode_batch(enc, LENS, block=BLOCK, details=True)
    for b in range(3):
        one = model.decode(enc[b], LENS[b], block=BLOCK, details=True)
        assert one.tokens == batch[b].tokens and one.frames == batch[b].frames
        _check(one, want[b], LENS[b], tol, "decode, utterance %d" % b)
    lens = torch.tensor(LENS)
    res = model.recognize(x, lens, details=True)
    assert [r.tokens for r in res] == model.recognize(x, lens)
    for b in range(3):
        _check(res[b], want[b], LENS[b], tol, "recognize, utterance %d" % b)
    # a batch of one goes through the batched path too; its encoder run is its own, so it is compared with that run's own decode
    with torch.no_grad():
        enc1 = model.encoder(x[:1])
    ref1 = _restate(model, enc1[0], LENS[0])
    res1 = model.recognize(x[:1], lens[:1], details=True)
    assert len(res1) == 1 and res1[0].tokens == model.recognize(x[:1], lens[:1])[0]
    _check(res1[0], ref1, LENS[0], tol, "recognize, batch of one")
    model.config["batched_decode"] = False                               # one decode(details=True) per utterance
    try:
        res = model.recognize(x, lens, details=True)
    finally:
        model.config["batched_decode"] = None
    for b in range(3):
        _check(res[b], want[b], LENS[b], tol, "recognize, batched_decode off, utterance %d" % b)


def test_details_in_the_bf16_mode_structure(ctx, monkeypatch):
    """bf16 logits: no restatement to compare with (its own rounding differs per call shape); the structure must hold"""
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    model, x = ctx["model"], ctx["x"]
    with torch.no_grad():
        enc = model.encoder(x)
    plain = model.decode_batch(enc, LENS, block=BLOCK)
    res = model.decode_batch(enc, LENS, block=BLOCK, details=True)
    assert [r.tokens for r in res] == plain and any(plain)
    for b, r in enumerate(res):
        assert len(r.frames) == len(r.logprobs) == len(r.tokens)
        assert all(a < c for a, c in zip(r.frames, r.frames[1:])) and all(0 <= f < LENS[b] for f in r.frames)
        assert all(math.isfinite(v) and v <= 0.0 for v in r.logprobs)
        assert math.isfinite(r.score) and r.score <= sum(r.logprobs) + 1e-9      # the blank frames' terms are <= 0 too


def test_streaming_recogniser_with_details():
    """a short synthetic recording (seeded random log-mel windows, seeded random weights; blocks of 5 frames): same tokens as the details-off
    run, one frame and one log-probability per token, frames strictly increasing absolute indices below the number of frames decoded"""
    from tt.model import Transducer
    from tt.utils import AttrDict
    from ttmi.streaming import StreamingRecognizer
    cfg = AttrDict(dict(enc=dict(n_layer=2, d_model=512, n_head=2, d_head=8, d_inner=16, max_input_length=48, left_context=6, right_context=2),
                        dec=dict(n_layer=1, d_model=512, n_head=2, d_head=8, d_inner=16, max_target_length=16),
                        joint=dict(input_size=1024, inner_size=16), vocab_size=40, dropout=0.0))
    torch.manual_seed(21)
    model = Transducer(cfg).cuda().eval()
    with torch.no_grad():
        model.joint.project_layer.bias[0] += 0.3
    g = torch.Generator().manual_seed(22)
    windows = [torch.randn(103, 128, generator=g) for _ in range(4)]
    off, on = StreamingRecognizer(model, block=5), StreamingRecognizer(model, block=5, details=True)
    assert not hasattr(off, "frames")
    for rec in (off, on):
        emitted = [rec.feed(w, last=(i == len(windows) - 1)) for i, w in enumerate(windows)]
        assert sum(emitted, []) == rec.result
    assert on.result == off.result and len(on.result) > 0 and on.pos == off.pos and on.breaks == off.breaks
    assert len(on.frames) == len(on.logprobs) == len(on.result)
    assert all(a < b for a, b in zip(on.frames, on.frames[1:])) and all(0 <= f < on.pos for f in on.frames)
    assert all(math.isfinite(v) and v <= 0.0 for v in on.logprobs)
    assert math.isfinite(on.score) and on.score <= sum(on.logprobs) + 1e-9
    on.reset()
    assert on.frames == [] and on.logprobs == [] and on.score == 0.0 and on.result == []
