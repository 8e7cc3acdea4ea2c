"""Transducer.align_ctc on the tiny two-layer Transducer of tests/test_ctc_gpu.py (golden weights, a fresh CTC head): it is ttmi.ctc.ctc_align on
the head's logits; a module without the head refuses; and after a few optimiser steps on one batch the spans of the transcript are ordered
and inside the utterance.  The kernels themselves are tested raw in tests/test_ctc_align_gpu.py."""
import numpy as np
import pytest
import torch

import ctc_align_oracle as A
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _tiny(ctc_weight):
    from tt.model import Transducer
    from tt.utils import AttrDict
    z, sd = load_golden("tiny_kshort")
    side = dict(n_layer=2, d_model=96, n_head=4, d_head=24, d_inner=160)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=sd["encoder.layers.0.r_emb"].shape[0]),
                        dec=dict(side, max_target_length=sd["decoder.layers.0.r_emb"].shape[0]),
                        joint=dict(input_size=192, inner_size=80), vocab_size=48, dropout=0.0, ctc_weight=ctc_weight))
    torch.manual_seed(5)
    model = Transducer(cfg).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)
    return z, model


def _batch(z):
    x = torch.tensor(z["inputs"], device="cuda")
    y = torch.tensor(z["targets"], device="cuda")
    tl = torch.tensor(z["full/act_lens"], device="cuda").int().clone()
    ul = torch.tensor(z["full/label_lens"], device="cuda").int().clone()
    if tl.numel() > 1:
        tl[-1] = max(int(tl[-1]) - 3, int(ul[-1]) * 2 + 1)                         # one ragged utterance
    return x, y, tl, ul


def _head_logits(model, x):
    """the head's logits by the route align_ctc takes (the library's GEMM into a row-padded buffer), so that the comparison is exact"""
    from ttmi import ops
    from tt.transformer import default_precision
    with torch.no_grad():
        enc = model.encoder(x, model._audio_mask(x)).contiguous()
        B, T, d = enc.shape
        V = model.ctc_head.out_features
        buf, logits = ops.padded_empty((B, T, V), torch.float32, enc.device)
        ops.weights_fresh()
        ops.linear_nt(enc.reshape(B * T, d), model.ctc_head.weight.detach(), buf.view(B * T, buf.shape[-1])[:, :V],
                      bias=model.ctc_head.bias.detach(), prec=default_precision())
    return logits


def test_align_ctc_is_ctc_align_on_the_heads_logits(monkeypatch):
    from ttmi.ctc import CTCAlignment, ctc_align
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    z, model = _tiny(0.3)
    x, y, tl, ul = _batch(z)
    got = model.align_ctc(x, tl, y, ul, stats=True)
    assert isinstance(got, CTCAlignment)
    logits = _head_logits(model, x)
    want = ctc_align(logits, y, tl, ul, blank=0, stats=True)
    B, T, U = x.shape[0], logits.shape[1], y.shape[1]
    assert got.path.shape == (B, T) and got.spans.shape == (B, U, 2) and got.score.shape == (B,) and got.expected.shape == (B, U)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    plain = model.align_ctc(x, tl, y, ul)
    assert plain.expected is None and plain.mass is None and plain.duration is None and torch.equal(plain.path, got.path)
    # and against the float64 reference on those logits: a valid alignment, optimal within the project's tolerance, healthy statistics
    seen, yh = logits.double().cpu().numpy(), y.cpu().numpy()
    path, spans, score, mass = (v.cpu().numpy() for v in (got.path, got.spans, got.score, got.mass))
    for b in range(B):
        Tb, Ub = int(tl[b]), int(ul[b])
        lp, _, skip = A.tables(seen[b], yh[b], Tb, Ub)
        best = A.viterbi_ref(lp, skip)[1]
        assert A.valid_path(path[b, :Tb], skip) and np.array_equal(spans[b, :Ub], A.spans_of(path[b, :Tb], Ub))
        mine = A.path_score(lp, path[b, :Tb])
        assert best - mine <= TOL * abs(best) and abs(score[b] - mine) <= TOL * abs(mine), (b, best, mine, score[b])
        assert np.abs(mass[b, :Ub] - 1.0).max(initial=0.0) <= TOL


def test_align_ctc_without_a_head_raises():
    z, model = _tiny(0.0)
    x, y, tl, ul = _batch(z)
    assert getattr(model, "ctc_head", None) is None
    with pytest.raises(ValueError, match="no CTC head: build it with config.ctc_weight > 0"):
        model.align_ctc(x, tl, y, ul)
    z, model = _tiny(0.3)
    with pytest.raises(ValueError, match="GPU"):
        model.align_ctc(x.cpu(), tl, y, ul)


def test_spans_after_a_few_steps_are_ordered_and_inside_the_utterance(monkeypatch):
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    z, model = _tiny(0.3)
    x, y, tl, ul = _batch(z)
    before = model.align_ctc(x, tl, y, ul).score.clone()
    opt = torch.optim.SGD(list(model.encoder.parameters()) + list(model.ctc_head.parameters()), lr=0.01)
    for _ in range(4):
        opt.zero_grad()
        model.ctc_loss(x, tl, y, ul).backward()
        opt.step()
    res = model.align_ctc(x, tl, y, ul, stats=True)
    torch.cuda.synchronize()
    spans, score, expected, duration = (v.cpu().numpy() for v in (res.spans, res.score, res.expected, res.duration))
    print("best-alignment score before", before.cpu().numpy(), "after four steps", score)
    assert np.isfinite(score).all()
    for b in range(x.shape[0]):
        Tb, Ub = int(tl[b]), int(ul[b])
        s = spans[b, :Ub]
        assert (s >= 0).all() and (s < Tb).all() and (s[:, 0] <= s[:, 1]).all() and (s[1:, 0] > s[:-1, 1]).all(), (b, s)
        assert (spans[b, Ub:] == -1).all()
        assert (np.diff(expected[b, :Ub]) > 0).all() and (duration[b, :Ub] >= 1.0 - TOL).all()
