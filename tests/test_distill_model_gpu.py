"""Distillation on collapsed lattice posteriors through the Python layers, on the tiny two-layer Transducer of
tests/test_decode_details_gpu.py: Transducer.lattice_posteriors against ops.kd_collapse on materialised logits, Transducer.loss(distill=...)
against the two-call form model(...) + RNNTLoss + w * lattice_kd_loss, and against the float64 oracles (tests/distill_oracle.py for the KD
term, oracle.tt_oracle / tests/mono_oracle.py for the transducer term) chained through tests/joint_oracle.py's exact joint.

Bounds: the project's 1e-4 (conftest.rel_err) wherever both sides run the same arithmetic or one of them is the float64 oracle.  One
comparison cannot be held to it: in the bf16 mode the two-call form rounds d logits to bf16 three times (the transducer gradient, the KD
gradient, and autograd's sum of the two) where the fused form rounds twice (the transducer gradient, then the sum formed in f32), so the two
d logits differ by up to five half-ulps of bf16 (2^-9 each) per element and everything downstream of them inherits that: 5 * 2^-9.

And one comparison is not made: in the bf16 mode a chunk of another size than the two-call form's batch.  The bf16 joint chooses how it
splits its operands by its row count (tests/joint_oracle.py, `resid`: the second bf16 term of the input weight is added only when the
chunk has at least de + dd rows), so one utterance alone gets other - equally valid - bf16 logits than the same utterance inside the batch,
and their difference (measured: 1.1e-4 of the loss, 1e-3 of a posterior) is the joint's rounding, not this feature's.  Chunking is compared
in the fp32 mode, where the joint is exact at every size; lattice_posteriors at chunk 1 and 2 is held in the bf16 mode to what two bf16
roundings of a logit allow, 2 * 2^-9 of the largest logit."""
import numpy as np
import pytest
import torch

import distill_oracle as DO
import joint_oracle as JO
import mono_oracle as M
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_BF16_ROUNDINGS = 5 * 2.0 ** -9
B, T, U, D, V = 3, 12, 5, 64, 29
ACT, LAB = [12, 10, 7], [5, 3, 0]
W = 0.75


def _model(seed=9):
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=2, d_model=D, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=V, dropout=0.0))
    torch.manual_seed(seed)
    return Transducer(cfg).cuda().eval()


def _batch():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, D, generator=g).cuda()
    y = torch.randint(1, V, (B, U), generator=g).cuda()
    return x, y, torch.tensor(ACT, dtype=torch.int32, device="cuda"), torch.tensor(LAB, dtype=torch.int32, device="cuda")


def _grads(model, xi):
    return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in model.parameters()]).double().cpu().numpy()


def _teacher_post(x, y, al, ll, **kw):
    return _model(seed=21).lattice_posteriors(x, al, y, ll, **kw)


def _node_err(got, want):
    """posteriors [B, T, U1, 3]: the same NEG / zero pattern, the rest within the node's largest magnitude -> worst relative error"""
    got, want = got.double().cpu().numpy(), want.double().cpu().numpy()
    assert np.array_equal(got == DO.NEG, want == DO.NEG) and np.array_equal(got == 0, want == 0)
    live = np.where(want == DO.NEG, 0.0, np.abs(want))
    den = live.max(-1, keepdims=True)
    return float((np.where(want == DO.NEG, 0.0, np.abs(got - want)) / np.where(den > 0, den, 1.0)).max())


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_lattice_posteriors_equal_kd_collapse_of_the_logits(prec, monkeypatch):
    from ttmi import distill, ops
    monkeypatch.setenv("TTMI_PRECISION", prec)
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _model()
    x, y, al, ll = _batch()
    with torch.no_grad():
        logits = model(x, y)
    want = ops.kd_collapse(logits if ops.row_pitch(logits) is not None else logits.contiguous(), y.int().contiguous(), al, ll, 0)
    assert want.shape == (B, T, U + 1, 3)
    zmax = float(logits.float().abs().max())
    for chunk in (1, 2, None):
        got = model.lattice_posteriors(x, al, y, ll, chunk=chunk)
        assert got.shape == want.shape and got.dtype == torch.float32 and not got.requires_grad
        print("%s chunk %s: worst node error %.2e, worst absolute difference %.2e (largest logit %.2f)"
              % (prec, chunk, _node_err(got, want), float((got - want)[want != DO.NEG].abs().max()), zmax))
        if prec == "fp32" or chunk is None:
            assert _node_err(got, want) < TOL
        else:                                                            # other bf16 logits (module docstring): the logit and the row's lse, one rounding each
            _node_err(got, want)
            assert float((got - want)[want != DO.NEG].abs().max()) <= 2 * 2.0 ** -9 * zmax
    assert _node_err(distill.lattice_posteriors(logits, y, al, ll), want) == 0.0
    # a handle is materialised like any other use of it
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1")
    import tt.model as TM
    with torch.no_grad():
        lg = model(x, y)
    assert isinstance(lg, TM.DeferredLogits)
    assert _node_err(distill.lattice_posteriors(lg, y, al, ll), want) < TOL
    for b in range(B):                                                   # exact zeros outside the ragged lattice, NEG at u == U_b
        assert float(want[b, ACT[b]:].abs().max() if ACT[b] < T else 0.0) == 0.0
        assert bool((want[b, :ACT[b], LAB[b], 1] == DO.NEG).all())


CONFIGS = [("rnnt", 0.0), ("rnnt", 0.01), ("monotonic", 0.0)]


@pytest.mark.parametrize("topology,fe", CONFIGS, ids=["rnnt", "rnnt-fastemit", "monotonic"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_form_equals_the_two_call_form(prec, topology, fe, monkeypatch):
    from ttmi.distill import LatticeKDLoss, lattice_kd_loss
    from warprnnt_pytorch import RNNTLoss
    monkeypatch.setenv("TTMI_PRECISION", prec)
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    x, y, al, ll = _batch()
    post = _teacher_post(x, y, al, ll)
    model = _model()
    gtol = TOL if prec == "fp32" else TOL_BF16_ROUNDINGS
    for reduction in ("mean", "sum"):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        lg = model(xi, y)
        two = RNNTLoss(reduction=reduction, check_lengths=False, fastemit_lambda=fe, topology=topology)(lg, y.int(), al, ll) \
            + W * lattice_kd_loss(lg, post, y.int(), al, ll, reduction=reduction)
        two.backward()
        want = (two.detach().double().cpu().numpy(), _grads(model, xi))
        for chunk in ((None, 1) if prec == "fp32" else (None,)):
            model.zero_grad()
            xi = x.clone().requires_grad_(True)
            got = model.loss(xi, al, y, ll, reduction=reduction, chunk=chunk, check_lengths=False, fastemit_lambda=fe, topology=topology,
                             distill=post, distill_weight=W)
            got.backward()
            gerr = rel_err(_grads(model, xi), want[1])
            print("%s %s fe %g %s chunk %s: loss %.7f against %.7f, gradient rel err %.2e"
                  % (prec, topology, fe, reduction, chunk, float(got.detach()), float(want[0][0]), gerr))
            assert got.shape == (1,) and rel_err(got.detach().double().cpu().numpy(), want[0]) < TOL
            assert gerr < gtol
    with torch.no_grad():
        lg = model(x, y)
        two = RNNTLoss(reduction="none", check_lengths=False, fastemit_lambda=fe, topology=topology)(lg, y.int(), al, ll) \
            + W * LatticeKDLoss(reduction="none")(lg, post, y.int(), al, ll)
        got = model.loss(x, al, y, ll, reduction="none", check_lengths=False, fastemit_lambda=fe, topology=topology, distill=post, distill_weight=W)
        plain = model.loss(x, al, y, ll, reduction="none", check_lengths=False, fastemit_lambda=fe, topology=topology)
    assert got.shape == (B,) and rel_err(got.cpu().numpy(), two.cpu().numpy()) < TOL
    assert bool((got > plain).all())                                     # the KD term of another model is positive


@pytest.mark.parametrize("topology", ["rnnt", "monotonic"])
def test_gradients_against_the_oracles_through_the_exact_joint(topology, monkeypatch):
    """fp32 mode: the model's encoder states and joint weights go through joint_oracle's float64 joint; the float64 oracles give the costs and
    d logits of the transducer term and of the KD term; joint_oracle's backward chains their weighted sum into the states and the weights"""
    from oracle import tt_oracle as O
    from tt.model import _JointLossFn
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    x, y, al, ll = _batch()
    post = _teacher_post(x, y, al, ll)
    model = _model()
    with torch.no_grad():
        enc, dec = model._encode(x, y)
    j = model.joint
    e, d = enc.clone().requires_grad_(True), dec.clone().requires_grad_(True)
    model.zero_grad()
    loss = _JointLossFn.apply(e, d, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias,
                              y.int().contiguous(), al, ll, 0, 2, "mean", None, True, 0, 0.0, None, topology, post, W)
    loss.backward()
    U1, J = U + 1, 48
    case = dict(B=B, T=T, U1=U1, de=D, dd=D, J=J, V=V, blank=0)
    for k, t in (("enc", enc), ("dec", dec), ("wf", j.forward_layer.weight), ("bf", j.forward_layer.bias), ("wp", j.project_layer.weight),
                 ("bp", j.project_layer.bias)):
        case[k] = t.detach().double().cpu()
    fwd = JO.joint_fwd_ref(case)
    z = fwd["logits"].reshape(B, T, U1, V).numpy()
    labels = y.int().cpu().numpy()
    if topology == "monotonic":
        c_t, g_t = M.mono_loss(z, labels, ACT, LAB)
    else:
        c_t, _, g_t = O.rnnt_loss(z, labels, np.asarray(ACT, dtype=np.int32), np.asarray(LAB, dtype=np.int32), blank=0, reduction="none",
                                  lattice=lambda lpb, lpl: O.rnnt_lattice_diag(lpb.astype(np.float64), lpl.astype(np.float64)))
    c_k, g_k, _ = DO.kd_loss(z, post.double().cpu().numpy(), labels, ACT, LAB)
    want_loss = (np.asarray(c_t).sum() + W * c_k.sum()) / B
    dz = torch.from_numpy(np.ascontiguousarray((np.asarray(g_t) + W * g_k) / B)).reshape(B * T * U1, V)
    ref = JO.joint_bwd_ref(case, fwd, dz)
    print("%s: loss %.7f, oracle %.7f (KD part %.7f)" % (topology, float(loss.detach()), want_loss, W * c_k.sum() / B))
    assert abs(float(loss.detach()) - want_loss) <= TOL * want_loss
    gwf = j.forward_layer.weight.grad
    got = dict(denc=e.grad.reshape(B * T, D), ddec=d.grad.reshape(B * U1, D), g_wp=j.project_layer.weight.grad, g_wf_e=gwf[:, :D],
               g_wf_d=gwf[:, D:], g_bf=j.forward_layer.bias.grad, g_bp=j.project_layer.bias.grad)
    for k, g in got.items():
        err = rel_err(g.double().cpu().numpy(), ref[k].numpy())
        print("  %s rel err %.2e" % (k, err))
        assert err < TOL, k


@pytest.mark.parametrize("topology", ["rnnt", "monotonic"])
def test_a_student_given_its_own_posteriors_trains_on_the_plain_loss(topology, monkeypatch):
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _model()
    x, y, al, ll = _batch()
    own = model.lattice_posteriors(x, al, y, ll)
    res = []
    for kw in ({}, dict(distill=own, distill_weight=W)):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        loss = model.loss(xi, al, y, ll, check_lengths=False, topology=topology, **kw)
        loss.backward()
        res.append((float(loss.detach()), _grads(model, xi)))
    print("%s: plain %.7f, with its own posteriors %.7f, gradient rel err %.2e" % (topology, res[0][0], res[1][0], rel_err(res[1][1], res[0][1])))
    assert abs(res[1][0] - res[0][0]) <= TOL * res[0][0]
    assert rel_err(res[1][1], res[0][1]) < TOL


def test_without_a_teacher_the_call_is_todays(monkeypatch):
    """distill=None and distill_weight=0.0: the call issues the library calls of a call without the arguments, the same ones in the same
    order with the same `inplace` (no KD kernel among them), and its loss has the same bits.  The parameter gradients cannot be held to their
    bits: the joint's weight gradients are f32 atomic sums (tests/test_mono_model_gpu.py, tests/test_mwer_gpu.py) that differ in the last
    bit between two identical calls of the parent commit too - seen here as well, one element of one gradient one ulp apart - so they are
    held to 1e-6 as they are there, and the identical call sequence is what shows that the same code ran."""
    import inspect
    from ttmi import ops
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _model()
    x, y, al, ll = _batch()
    post = _teacher_post(x, y, al, ll)

    calls = []

    def traced(name, fn):
        def f(*a, **k):
            assert not name.startswith("kd_"), "a KD call without a teacher: %s" % name
            calls.append((name, k.get("inplace")))
            return fn(*a, **k)
        return f
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if not name.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, name, traced(name, fn))

    def run(**kw):
        del calls[:]
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        loss = model.loss(xi, al, y, ll, check_lengths=False, **kw)
        loss.backward()
        return [loss.detach(), xi.grad] + [p.grad.clone() for p in model.parameters()], list(calls)
    for base in ({}, dict(topology="monotonic"), dict(fastemit_lambda=0.01)):
        a, seq = run(**base)
        assert any(n in ("rnnt_loss_bwd", "mono_loss_bwd") and inplace for n, inplace in seq), seq
        for kw in (dict(distill=None), dict(distill_weight=0.0), dict(distill=post, distill_weight=0.0), dict(distill=None, distill_weight=0.5)):
            got, seq_kw = run(**base, **kw)
            assert seq_kw == seq, (base, kw)
            assert torch.equal(got[0].view(torch.int32), a[0].view(torch.int32)), (base, kw)
            for p, q in zip(got[1:], a[1:]):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)) or rel_err(p.cpu().numpy(), q.cpu().numpy()) < 1e-6, (base, kw)


def test_option_contract(monkeypatch):
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _model()
    x, y, al, ll = _batch()
    post = _teacher_post(x, y, al, ll)
    with pytest.raises(ValueError, match="distill"):
        model.loss(x, al, y, ll, check_lengths=False, exp_domain=True, distill=post, distill_weight=W)
    with pytest.raises(ValueError, match="shape"):
        model.loss(x, al, y, ll, check_lengths=False, distill=post[:2], distill_weight=W)
    with pytest.raises(ValueError, match="float32"):
        model.loss(x, al, y, ll, check_lengths=False, distill=post.double(), distill_weight=W)
    with pytest.raises(ValueError, match="GPU"):
        model.loss(x, al, y, ll, check_lengths=False, distill=post.cpu(), distill_weight=W)
    with pytest.raises(ValueError, match="fastemit"):
        model.loss(x, al, y, ll, check_lengths=False, topology="monotonic", fastemit_lambda=0.01, distill=post, distill_weight=W)
    # the KD term is not multiplied by utterance_weights, like the CTC term
    w = torch.tensor([1.75, 0.0, -0.5], device="cuda")
    with torch.no_grad():
        both = float(model.loss(x, al, y, ll, reduction="sum", check_lengths=False, utterance_weights=w, distill=post, distill_weight=W))
        plain = float(model.loss(x, al, y, ll, reduction="sum", check_lengths=False, utterance_weights=w))
        none = model.loss(x, al, y, ll, reduction="none", check_lengths=False, distill=post, distill_weight=W) \
            - model.loss(x, al, y, ll, reduction="none", check_lengths=False)
    assert abs((both - plain) - float(none.sum())) <= TOL * abs(float(none.sum()))
