"""topology="monotonic" through the Python layers: warprnnt_pytorch.RNNTLoss on materialised logits and on the DeferredLogits handle,
Transducer.loss and Transducer.mwer_loss, on the tiny two-layer Transducer of tests/test_decode_details_gpu.py.  The three forms run the same
kernels on the same states and must agree within the project's 1e-4 (conftest.rel_err); the materialised form is held to the float64 oracle
(tests/mono_oracle.py) chained through torch autograd on float64 copies of the joint network."""
import numpy as np
import pytest
import torch

import mono_oracle as M
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
B, T, U, D, V = 3, 12, 5, 64, 29
ACT, LAB = [12, 10, 7], [5, 3, 0]


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


def _grads(model, xi):
    return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in model.parameters()]).double().cpu().numpy()


def _three_forms(model, monkeypatch, **kw):
    """-> [(loss, gradients)] of RNNTLoss on materialised logits, RNNTLoss on the deferred handle, Transducer.loss"""
    import tt.model as TM
    from warprnnt_pytorch import RNNTLoss
    x, y, al, ll = _batch()
    crit = RNNTLoss(check_lengths=False, topology="monotonic", **kw)
    out = []
    for form in ("materialised", "deferred", "fused"):
        monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1" if form == "deferred" else "0")
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        if form == "fused":
            loss = model.loss(xi, al, y, ll, check_lengths=False, topology="monotonic", **kw)
        else:
            lg = model(xi, y)
            assert isinstance(lg, TM.DeferredLogits) == (form == "deferred")
            loss = crit(lg, y.int(), al, ll)
            if form == "deferred":
                assert not lg.is_materialized                                       # the fused chunk form ran on the handle
        # an upstream factor scales everything.  A power of two: in the bf16 mode the materialised form rounds d logits to bf16 AFTER the
        # factor and the fused forms before it, which is the same bits only for a factor that is exact in bf16 arithmetic
        (loss * 4.0).sum().backward()
        out.append((loss.detach().double().cpu().numpy(), _grads(model, xi)))
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_three_forms_agree(prec, monkeypatch):
    monkeypatch.setenv("TTMI_PRECISION", prec)
    model = _model()
    res = _three_forms(model, monkeypatch)
    for name, (loss, grads) in zip(("deferred", "fused"), res[1:]):
        print("%s %s: loss %.7f against %.7f, gradient rel err %.2e" % (prec, name, loss[0], res[0][0][0], rel_err(grads, res[0][1])))
        assert loss.shape == (1,) and rel_err(loss, res[0][0]) < TOL, name
        assert rel_err(grads, res[0][1]) < TOL, name
    assert np.isfinite(res[0][1]).all() and np.abs(res[0][1]).max() > 0


def test_gradients_against_the_oracle_through_the_joint(monkeypatch):
    """fp32 mode: the encoder states of the model go through a float64 torch copy of the joint network, the oracle gives the cost and its
    gradient w.r.t. those logits, torch autograd chains it into the states and the joint's parameters"""
    from warprnnt_pytorch import RNNTLoss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    x, y, al, ll = _batch()
    with torch.no_grad():
        enc, dec = model._encode(x, y)
    j = model.joint
    e, d = enc.clone().requires_grad_(True), dec.clone().requires_grad_(True)
    model.zero_grad()
    loss = RNNTLoss(check_lengths=False, topology="monotonic")(j(e, d), y.int(), al, ll)
    loss.backward()
    got = [e.grad, d.grad, j.forward_layer.weight.grad, j.forward_layer.bias.grad, j.project_layer.weight.grad, j.project_layer.bias.grad]
    e64, d64, wf, bf, wp, bp = (t.detach().double().cpu().requires_grad_(True)
                                for t in (enc, dec, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias))
    h = torch.tanh((e64 @ wf[:, :D].t())[:, :, None, :] + (d64 @ wf[:, D:].t())[:, None, :, :] + bf)
    z = h @ wp.t() + bp
    want_c, want_g = M.mono_loss(z.detach().numpy(), y.cpu().numpy(), ACT, LAB)
    z.backward(torch.tensor(want_g / B))
    print("loss %.7f, oracle %.7f" % (float(loss.detach()), want_c.mean()))
    assert abs(float(loss.detach()) - want_c.mean()) <= TOL * want_c.mean()
    for name, a, b in zip(("enc", "dec", "wf", "bf", "wp", "bp"), got, (e64, d64, wf, bf, wp, bp)):
        print("  d %s rel err %.2e" % (name, rel_err(a.cpu().numpy(), b.grad.numpy())))
        assert rel_err(a.cpu().numpy(), b.grad.numpy()) < TOL, name


def test_utterance_weights_and_reduction_none(monkeypatch):
    """as on the standard lattice: reduction='none' gives the per-utterance costs (and, on materialised logits, takes per-utterance upstream
    gradients); utterance_weights w makes the fused loss sum_b w_b cost_b with the gradients of that sum"""
    from warprnnt_pytorch import RNNTLoss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    x, y, al, ll = _batch()
    w = torch.tensor([1.75, 0.0, -0.5], device="cuda")
    model.zero_grad()
    xi = x.clone().requires_grad_(True)
    costs = RNNTLoss(reduction="none", check_lengths=False, topology="monotonic")(model(xi, y), y.int(), al, ll)
    assert costs.shape == (B,)
    (costs * w).sum().backward()
    ref = _grads(model, xi)
    with torch.no_grad():
        none = model.loss(x, al, y, ll, reduction="none", check_lengths=False, topology="monotonic")
        mean = model.loss(x, al, y, ll, check_lengths=False, topology="monotonic")
    assert none.shape == (B,) and rel_err(none.cpu().numpy(), costs.detach().cpu().numpy()) < TOL
    assert abs(float(mean) - float(costs.mean())) <= TOL * float(costs.mean())
    for reduction, div in (("sum", 1.0), ("mean", float(B))):
        for chunk in (1, 2):
            model.zero_grad()
            xi = x.clone().requires_grad_(True)
            got = model.loss(xi, al, y, ll, reduction=reduction, chunk=chunk, check_lengths=False, utterance_weights=w, topology="monotonic")
            want = float((costs.detach() * w).sum()) / div
            assert got.shape == (1,) and abs(float(got) - want) <= TOL * abs(want)
            got.backward()
            assert rel_err(_grads(model, xi) * div, ref) < TOL, (reduction, chunk)
    with pytest.raises(ValueError):
        model.loss(x, al, y, ll, reduction="none", check_lengths=False, utterance_weights=w, topology="monotonic")


def test_ctc_weight_still_adds_its_term(monkeypatch):
    from tt.model import Transducer
    from tt.utils import AttrDict
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    side = dict(n_layer=1, d_model=D, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=V, dropout=0.0, ctc_weight=0.3))
    torch.manual_seed(3)
    model = Transducer(cfg).cuda().eval()
    x, y, al, ll = _batch()
    with torch.no_grad():
        both = float(model.loss(x, al, y, ll, check_lengths=False, topology="monotonic"))
        plain = float(model.loss(x, al, y, ll, check_lengths=False, topology="monotonic", ctc_weight=0))
        ctc = float(model.ctc_loss(x, al, y, ll))
    assert abs((both - plain) - 0.3 * ctc) <= TOL * 0.3 * ctc


def test_default_topology_is_bit_identical(monkeypatch):
    """topology="rnnt" and a call without the keyword: the same bits from the loss kernels (costs and d logits, which have no atomics); the
    fused form's weight gradients are f32 atomic sums that differ from run to run (tests/test_mwer_gpu.py), so they are held to 1e-6"""
    from warprnnt_pytorch import RNNTLoss, rnnt_loss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    x, y, al, ll = _batch()
    with torch.no_grad():
        logits = model(x, y)
    res = []
    for kw in ({}, {"topology": "rnnt"}):
        for fe in (0.0, 0.01):
            lg = logits.clone().requires_grad_(True)
            loss = RNNTLoss(check_lengths=False, fastemit_lambda=fe, **kw)(lg, y.int(), al, ll)
            loss.backward()
            fn = rnnt_loss(logits, y.int(), al, ll, 0, "none", False, fastemit_lambda=fe, **kw)
            res.append((loss.detach(), lg.grad, fn))
    for a, b in zip(res[:2], res[2:]):
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    fused = []
    for kw in ({}, {"topology": "rnnt"}):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        loss = model.loss(xi, al, y, ll, check_lengths=False, **kw)
        loss.backward()
        fused.append((loss.detach(), _grads(model, xi)))
    assert torch.equal(fused[0][0].view(torch.int32), fused[1][0].view(torch.int32))
    assert rel_err(fused[1][1], fused[0][1]) < 1e-6
    # ... and the monotonic lattice is a different model: its cost is not the standard one's
    mono = RNNTLoss(check_lengths=False, topology="monotonic")(logits, y.int(), al, ll)
    assert abs(float(mono) - float(res[0][0])) > 1e-3 * float(res[0][0])


def test_option_contract(monkeypatch):
    from warprnnt_pytorch import RNNTLoss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _model()
    x, y, al, ll = _batch()
    with pytest.raises(ValueError, match="topology"):
        model.loss(x, al, y, ll, check_lengths=False, topology="ctc")
    with pytest.raises(ValueError, match="exp"):
        model.loss(x, al, y, ll, check_lengths=False, topology="monotonic", exp_domain=True)
    with pytest.raises(ValueError, match="fastemit"):
        model.loss(x, al, y, ll, check_lengths=False, topology="monotonic", fastemit_lambda=0.01)
    with pytest.raises(ValueError, match="topology"):
        model.mwer_loss(x, al, y, ll, topology="x")
    # the length check also rejects more labels than frames; with the check off that utterance costs +inf and adds no gradient
    full_al, full_ll = torch.tensor([12, 12, 4], dtype=torch.int32, device="cuda"), torch.tensor([5, 5, 5], dtype=torch.int32, device="cuda")
    model.loss(x, full_al, y, full_ll, topology="rnnt")
    with pytest.raises(ValueError, match="more labels than frames"):
        model.loss(x, full_al, y, full_ll, topology="monotonic")
    with torch.no_grad():
        logits = model(x, y)
    with pytest.raises(ValueError, match="more labels than frames"):
        RNNTLoss(topology="monotonic")(logits, y.int(), full_al, full_ll)
    lg = logits.clone().requires_grad_(True)
    costs = RNNTLoss(reduction="none", check_lengths=False, topology="monotonic")(lg, y.int(), full_al, full_ll)
    assert torch.isposinf(costs[2]) and torch.isfinite(costs[:2]).all()
    costs[:2].sum().backward()
    assert torch.isfinite(lg.grad).all() and float(lg.grad[2].abs().max()) == 0.0


def test_mwer_on_the_monotonic_lattice(monkeypatch):
    """both passes take the topology: the hypothesis costs are Transducer.loss(reduction='none', topology='monotonic') on the same rows, the
    value and every gradient are finite, and they differ from the standard lattice's"""
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _model()
    x, y, al, ll = _batch()
    al = torch.tensor([12, 10, 7], dtype=torch.int32, device="cuda")
    ul = torch.tensor([5, 3, 2], dtype=torch.int32, device="cuda")
    hyps = [[[int(v) for v in y[0]], [int(v) for v in y[0, :3]]], [[int(v) for v in y[1, :3]], [4, 9], []], [[7, 7], [int(y[2, 0])]]]
    model.zero_grad()
    xi = x.clone().requires_grad_(True)
    loss, det = model.mwer_loss(xi, al, y, ul, hypotheses=hyps, rnnt_weight=0.1, details=True, topology="monotonic")
    loss.backward()
    assert torch.isfinite(loss).all() and torch.isfinite(xi.grad).all() and float(xi.grad.abs().max()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    flat = [h for hs in hyps for h in hs]
    rows = torch.tensor([b for b, hs in enumerate(hyps) for _ in hs], device="cuda")
    lab = torch.zeros(len(flat), U, dtype=torch.long, device="cuda")
    for i, h in enumerate(flat):
        lab[i, :len(h)] = torch.tensor(h, dtype=torch.long)
    hl = torch.tensor([len(h) for h in flat], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        want = model.loss(x[rows], al[rows], lab, hl, reduction="none", check_lengths=False, topology="monotonic")
        std = model.mwer_loss(x, al, y, ul, hypotheses=hyps, rnnt_weight=0.1, details=True)[1].costs
    got = det.costs[:len(flat)]
    print("hypothesis costs", got.cpu().numpy(), "loss(reduction='none')", want.cpu().numpy())
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < TOL
    assert rel_err(got.cpu().numpy(), std[:len(flat)].cpu().numpy()) > 1e-3
