"""The monotonic lattice through the alignment surfaces: Transducer.align_monotonic, warprnnt_pytorch.rnnt_align(topology="monotonic") on
the DeferredLogits handle and on materialised logits, on the tiny two-layer Transducer of tests/test_mono_model_gpu.py; and the tie with the greedy decoder, whose
DecodeResult.frames / .score live on the same lattice.  The three forms run the same kernels on the same states and must agree within the
project's 1e-4; every form's frames are scored by the float64 oracle (tests/mono_align_oracle.py) on the materialised logits and have to be
optimal there - identical frames are not required across numerically different routes.

T is 24 and not the 12 of tests/test_mono_model_gpu.py: in the bf16 mode ttmi_joint_fwd adds the second term of the weights' and label states'
bf16 split only when a call's T (U + 1) lattice rows give its workspace room for it (rows >= the joint's input width, 128 here), so a chunk of
ONE 72-row utterance would get other logits than a chunk of two or three (1.6e-4 of the cost, measured) - a property of the joint on shapes
this small, on the standard lattice too, and none of the chunk loop under test.  At 144 rows per utterance every chunk size takes one route."""
import numpy as np
import pytest
import torch

import mono_align_oracle as A

pytestmark = pytest.mark.gpu
TOL = 1e-4
B, T, U, D, V = 3, 24, 5, 64, 29
ACT, LAB = [24, 19, 7], [5, 3, 0]


def _model():
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=2, d_model=D, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=V, dropout=0.0))
    torch.manual_seed(9)
    return Transducer(cfg).cuda().eval()


def _batch():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, D, generator=g).cuda()
    y = torch.randint(1, V, (B, U), generator=g).cuda()
    return x, y, torch.tensor(ACT, dtype=torch.int32, device="cuda"), torch.tensor(LAB, dtype=torch.int32, device="cuda")


def _host(res):
    return [None if v is None else v.cpu().numpy() for v in res]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_three_forms_agree(prec, monkeypatch):
    import tt.model as TM
    from warprnnt_pytorch import rnnt_align
    monkeypatch.setenv("TTMI_PRECISION", prec)
    model = _model()
    x, y, al, ll = _batch()
    forms = {}
    with torch.no_grad():
        monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
        logits = model(x, y)
        assert not isinstance(logits, TM.DeferredLogits)
        forms["materialised"] = _host(rnnt_align(logits, y.int(), al, ll, check_lengths=False, stats=True, topology="monotonic"))
        monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1")
        handle = model(x, y)
        assert isinstance(handle, TM.DeferredLogits)
        forms["deferred"] = _host(rnnt_align(handle, y.int(), al, ll, check_lengths=False, stats=True, topology="monotonic"))
        assert not handle.is_materialized                                           # the chunk form ran on the handle
        for chunk in (1, 2, None):
            forms["align chunk %s" % chunk] = _host(model.align_monotonic(x, al, y, ll, chunk=chunk, check_lengths=False, stats=True))
    seen = logits.double().cpu().numpy()
    yh = y.cpu().numpy()
    ref = forms["materialised"]
    for name, (frames, score, cost, expected, mass) in forms.items():
        assert frames.shape == (B, U) and frames.dtype == np.int32 and expected.shape == (B, U) and mass.shape == (B, U)
        for b in range(B):
            Tb, Ub = ACT[b], LAB[b]
            lpb, lpl = A.tables(seen[b], yh[b], Tb, Ub)
            best = A.viterbi_ref(lpb, lpl)[1]
            f = frames[b, :Ub]
            assert (frames[b, Ub:] == -1).all() and all(f[i] < f[i + 1] for i in range(Ub - 1))
            path = A.path_score(lpb, lpl, f)
            print("%s %s utt %d: cost %.6f score %.6f, oracle best %.6f, path of the frames %.6f" % (prec, name, b, cost[b], score[b], best, path))
            assert best - path <= TOL * abs(best), (name, b)
            assert abs(cost[b] - ref[2][b]) <= TOL * abs(ref[2][b]) and abs(score[b] - ref[1][b]) <= TOL * abs(ref[1][b]), (name, b)
            assert score[b] <= -cost[b] + TOL * abs(cost[b])
            assert np.abs(mass[b, :Ub] - 1.0).max(initial=0.0) <= TOL and (mass[b, Ub:] == 0).all() and (expected[b, Ub:] == -1).all()
            assert np.abs(expected[b, :Ub] - ref[3][b, :Ub]).max(initial=0.0) <= TOL * Tb, (name, b)
    if prec == "fp32":                                      # fp32 logits: the kernel's score against the oracle's best itself
        for b in range(B):
            lpb, lpl = A.tables(seen[b], yh[b], ACT[b], LAB[b])
            best = A.viterbi_ref(lpb, lpl)[1]
            assert abs(ref[1][b] - best) <= TOL * abs(best)


def test_default_topology_is_the_standard_lattice(monkeypatch):
    """rnnt_align with the keyword left out and with topology="rnnt" return equal tensors (Transducer.align has no such keyword: its
    parameter list is pinned by tests/test_align.py, and align_monotonic is the model-level entry of the other lattice)"""
    from warprnnt_pytorch import rnnt_align
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    x, y, al, ll = _batch()
    a = model.align(x, al, y, ll, check_lengths=False, stats=True)
    with torch.no_grad():
        logits = model(x, y)
    b = rnnt_align(logits, y.int(), al, ll, check_lengths=False, stats=True)
    c = rnnt_align(logits, y.int(), al, ll, check_lengths=False, stats=True, topology="rnnt")
    m = model.align_monotonic(x, al, y, ll, check_lengths=False, stats=True)
    for u, v in zip(b, c):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert abs(float((a.cost - b.cost).abs().max())) <= TOL * float(b.cost.abs().max())
    assert not torch.equal(a.cost, m.cost)                  # and the monotonic lattice is another one
    with pytest.raises(ValueError, match="more labels than frames"):
        model.align_monotonic(x[:, :4].contiguous(), torch.tensor([4, 4, 4]), y, torch.tensor([5, 3, 0]))


def test_decoder_score_is_bounded_by_the_alignment_score(monkeypatch):
    """fp32 mode: the greedy decoder's path is a path of the monotonic lattice, so for the tokens it returned the forced alignment's score is at
    least the decoder's, and the two are equal where the decoder's frames are the aligned frames.  The decoder reaches its logits by another
    route (label states one step at a time, the joint on single rows) than the loss; `bound` starts at TOL |score| and, when the two routes
    disagree by more than that on the SAME path - the decoder's score against the oracle's path_score of the decoder's frames on
    model(x, tokens)'s logits - becomes twice that measured disagreement."""
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    with torch.no_grad():
        model.joint.project_layer.bias[0] += 0.9             # some blank frames between the emissions (tests/test_decode_details_gpu.py)
    n, Tn, LENS = 3, 40, [40, 37, 29]
    x = torch.randn(n, Tn, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    lens = torch.tensor(LENS)
    results = model.recognize(x, lens, details=True)
    Un = max(1, max(len(r.tokens) for r in results))
    y = torch.zeros(n, Un, dtype=torch.long)
    for b, r in enumerate(results):
        y[b, :len(r.tokens)] = torch.tensor(r.tokens, dtype=torch.long)
    y = y.cuda()
    ul = torch.tensor([len(r.tokens) for r in results], dtype=torch.int32, device="cuda")
    res = model.align_monotonic(x, lens, y, ul, check_lengths=False)
    with torch.no_grad():
        seen = model(x, y).double().cpu().numpy()
    frames, score = res.frames.cpu().numpy(), res.score.cpu().numpy()
    assert sum(len(r.tokens) for r in results) > 0, "the decoder emitted nothing: the test compares no label"
    for b, r in enumerate(results):
        Ub = len(r.tokens)
        lpb, lpl = A.tables(seen[b], y[b].cpu().numpy(), LENS[b], Ub)
        route = abs(r.score - A.path_score(lpb, lpl, r.frames))
        bound = TOL * abs(r.score)
        if route > bound:
            bound = 2 * route
        same = list(frames[b, :Ub]) == list(r.frames)
        print("utt %d: %d tokens, decoder score %.6f, aligned score %.6f, same frames %s, decode route against loss route on the decoder's path %.3e "
              "(relative %.3e)" % (b, Ub, r.score, score[b], same, route, route / abs(r.score)))
        assert score[b] >= r.score - bound, (b, score[b], r.score)
        if same:
            assert abs(score[b] - r.score) <= bound, (b, score[b], r.score)
