"""FastEmit on the GPU, every loss path against the float64 reference of tests/test_fastemit.py: the plain loss on f32 and on row-padded bf16
logits, the bf16x3 gradient planes, the exp-domain fused joint + loss (through `_JointLossFn` and through train.py's unchanged call sequence),
lambda = 0 bit for bit, and a captured training step."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_fastemit import fastemit_ref
from test_fused_loss_gpu import _run, _training_sized

pytestmark = pytest.mark.gpu


def _loss(x, y, tl, ul, blank, reduction, lam=None, upstream=None):
    from warprnnt_pytorch import RNNTLoss
    acts = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    kw = {} if lam is None else {"fastemit_lambda": lam}
    loss = RNNTLoss(blank=blank, reduction=reduction, **kw)(
        acts, torch.tensor(y, dtype=torch.int32, device="cuda"), torch.tensor(tl, dtype=torch.int32, device="cuda"),
        torch.tensor(ul, dtype=torch.int32, device="cuda"))
    if reduction == "none":
        loss.backward(torch.tensor(upstream, dtype=torch.float32, device="cuda"))
    else:
        loss.backward()
    return loss.detach().cpu().numpy(), acts.grad.cpu().numpy()


@pytest.mark.parametrize("lam", [1e-3, 0.5])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("B,T,U,V", [(3, 17, 9, 11), (4, 33, 70, 37), (5, 64, 63, 130), (2, 7, 600, 5)])
def test_plain_loss_f32(B, T, U, V, reduction, lam):
    """random ragged sizes as in test_rnnt_gpu.py::test_random_vs_float64_oracle, a non-zero blank and one label equal to it"""
    rng = np.random.default_rng(B * 1000 + T + U + V)
    x = (rng.normal(size=(B, T, U + 1, V)) * 2).astype(np.float32)
    blank = V // 2
    y = rng.integers(0, V, size=(B, U))
    y[0, 1] = blank
    tl, ul = np.full(B, T), np.full(B, U)
    tl[1:] = rng.integers(1, T + 1, size=B - 1)
    ul[1:] = rng.integers(0, U + 1, size=B - 1)
    upstream = 1.0 + 0.25 * np.arange(B)
    g_b = {"mean": np.full(B, 1.0 / B), "sum": np.ones(B), "none": upstream}[reduction]
    cost0, _ = _loss(x, y, tl, ul, blank, reduction, upstream=upstream)
    cost, g = _loss(x, y, tl, ul, blank, reduction, lam, upstream=upstream)
    assert np.array_equal(cost, cost0)                                # the cost is the plain NLL, bit for bit
    want_costs, want = fastemit_ref(x, y, tl, ul, blank, lam, g_b)
    assert rel_err(cost if reduction == "none" else cost.sum(), want_costs if reduction == "none" else (g_b * want_costs).sum()) < 1e-4
    assert rel_err(g, want) < 1e-4
    assert np.abs(g.astype(np.float64).sum(-1)).max() < 2e-5          # every row sums to zero
    for b in range(B):
        assert np.all(g[b, tl[b]:] == 0) and np.all(g[b, :, ul[b] + 1:] == 0)


@pytest.mark.parametrize("B,T,U,V", [(2, 24, 7, 300), (1, 9, 3, 4334)])
def test_bf16_row_padded_logits(B, T, U, V):
    from warprnnt_pytorch import RNNTLoss
    lam = 0.5
    rng = np.random.default_rng(V + 1)
    Vp = (V + 63) // 64 * 64
    buf = torch.zeros(B, T, U + 1, Vp, device="cuda", dtype=torch.bfloat16)
    buf[..., :V] = torch.tensor(rng.normal(size=(B, T, U + 1, V)) * 2, device="cuda").to(torch.bfloat16)
    buf[..., V:] = 77.0                                     # poison the pad: must never be read
    acts = buf[..., :V].detach().requires_grad_(True)
    y = rng.integers(1, V, size=(B, U))
    tl, ul = np.full(B, T, dtype=np.int32), np.full(B, U, dtype=np.int32)
    if B > 1:
        tl[1], ul[1] = T - 4, U - 2
    raw = []
    acts.register_hook(raw.append)
    loss = RNNTLoss(fastemit_lambda=lam)(acts, torch.tensor(y, dtype=torch.int32, device="cuda"), torch.tensor(tl, device="cuda"),
                                         torch.tensor(ul, device="cuda"))
    loss.backward()
    g = raw[0]
    assert g.dtype is torch.bfloat16 and g.stride(-2) == Vp
    want_costs, want = fastemit_ref(buf[..., :V].float().cpu().numpy(), y, tl, ul, 0, lam, np.full(B, 1.0 / B))
    assert abs(float(loss) - want_costs.mean()) / want_costs.mean() < 1e-5
    assert rel_err(g.float().cpu().numpy(), want) < 6e-3
    full = torch.as_strided(g, (B, T, U + 1, Vp), g.stride())
    assert float(full[..., V:].float().abs().max()) == 0


def _states(model, x, y):
    with torch.no_grad():
        return model._encode(x, y)


def _fused(model, enc_s, dec_s, y, al, ll, prec, chunk, st, lam):
    """_JointLossFn on the given encoder states (mean reduction) -> (loss, {denc, ddec, joint parameter gradients})"""
    from tt.model import _JointLossFn
    j = model.joint
    enc_l, dec_l = enc_s.clone().requires_grad_(True), dec_s.clone().requires_grad_(True)
    model.zero_grad()
    loss = _JointLossFn.apply(enc_l, dec_l, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias,
                              y.int().contiguous(), al, ll, prec, chunk, "mean", st, True, 0, lam)
    loss.backward()
    torch.cuda.synchronize()
    out = {"denc": enc_l.grad.double().cpu().numpy(), "ddec": dec_l.grad.double().cpu().numpy()}
    for k, p in j.named_parameters():
        out["g_" + k] = p.grad.double().cpu().numpy()
    return float(loss.detach()), out


def _oracle_joint_grads(model, enc_s, dec_s, y, al, ll, lam, delta):
    """the reference through oracle.joint_fwd / joint_bwd (float64) on the same encoder states; delta: grad(lam) - grad(0) only"""
    from oracle import tt_oracle as O
    j = model.joint
    sd = {"joint." + k: v.detach().double().cpu().numpy() for k, v in j.state_dict().items()}
    z, cache = O.joint_fwd(enc_s.double().cpu().numpy(), dec_s.double().cpu().numpy(), sd)
    B = z.shape[0]
    costs, dz = fastemit_ref(z, y.int().cpu().numpy(), al.cpu().numpy(), ll.cpu().numpy(), 0, lam, np.full(B, 1.0 / B), delta=delta)
    del z
    grads = {}
    denc, ddec = O.joint_bwd(dz, cache, sd, grads)
    out = {"denc": denc, "ddec": ddec}
    for k in ("forward_layer.weight", "forward_layer.bias", "project_layer.weight", "project_layer.bias"):
        out["g_" + k] = grads["joint." + k]
    return costs, out


def test_bf16x3_planes(monkeypatch):
    """TTMI_PRECISION=bf16x3 at the C2 joint size: the gradient planes with lambda equal the unsplit f32 gradient with the same lambda
    (2e-6) and the float64 reference through oracle.joint_bwd (1e-4)"""
    import ttmi.ops as ops
    lam = 0.5
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16x3")
    seen = []
    inner = ops.rnnt_loss_bwd_split
    monkeypatch.setattr(ops, "rnnt_loss_bwd_split", lambda *a, **k: (seen.append(k.get("fastemit_lambda")), inner(*a, **k))[1])
    planes = _run(model, x, y, al, ll, chunk=4, fastemit_lambda=lam)
    assert seen == [lam, lam]                                 # two chunks, both through the split form, both with lambda
    monkeypatch.setenv("TTMI_X3_SPLIT_GRAD", "0")
    plain = _run(model, x, y, al, ll, chunk=4, fastemit_lambda=lam)
    assert len(seen) == 2
    assert planes[0] == plain[0]
    for n in plain[2]:
        assert rel_err(planes[2][n], plain[2][n]) < 2e-6, n
    monkeypatch.delenv("TTMI_X3_SPLIT_GRAD")
    enc_s, dec_s = _states(model, x, y)
    loss, got = _fused(model, enc_s, dec_s, y, al, ll, 2, 4, None, lam)
    assert len(seen) == 4
    costs, want = _oracle_joint_grads(model, enc_s, dec_s, y, al, ll, lam, delta=False)
    assert abs(loss - costs.mean()) < 1e-4 * costs.mean()
    errs = {k: rel_err(got[k], want[k]) for k in want}
    print("bf16x3 planes, lambda %g, vs float64: %s" % (lam, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < 1e-4, (k, e)


# the FastEmit part of the exp-domain gradients against the reference's.  First measurement (lambda 0.5; C2 / C4 joint sizes): ddec 1.3e-2 /
# 1.2e-2, joint biases 1.6e-2 / 1.8e-2 and 6.3e-3 / 3.4e-3, project weight 1.6e-2 / 1.6e-2 - bf16 class; d enc 6.1e-2 / 8.9e-2 and the forward
# layer's weight 1.4e-1 / 1.0e-1: a sum over only U + 1 = 21 lattice rows per frame of a difference that is a small part of the gradient, so the
# bf16 rounding of P, Wp and the bf16 row factors does not average out.  In logit space (srow * P, the loss kernel's own output) the difference
# is within 3.2e-2 / 3.6e-2: the softmax of logits formed from bf16 operands, which the lambda = 0 gradient of this form carries as well.
EXP_DELTA_TOL = {"denc": 2.5e-1, "g_forward_layer.weight": 2.5e-1}
EXP_DELTA_TOL_DEFAULT = 3e-2
EXP_LOGIT_DELTA_TOL = 6e-2


@pytest.mark.parametrize("J,V", [(1024, 4334), (2048, 6485)])          # C2 and C4 joint dimensions
def test_exp_domain_difference_vs_reference(monkeypatch, J, V):
    """the exp-domain fused form: its bf16 gradient error (about 1e-2) would hide a small FastEmit term, so the FastEmit PART of every
    gradient, grad(0.5) - grad(0) from this path, is compared with the reference's grad(0.5) - grad(0) (linear in d logits: joint_bwd of
    the delta).  Both runs start from the same shift."""
    import ttmi.ops as ops
    lam = 0.5
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16", J, V)
    enc_s, dec_s = _states(model, x, y)
    B = enc_s.shape[0]
    st = model.joint.exp_shift_state(x.device)
    calls = []
    orig = ops.rnnt_loss_bwd_exp
    monkeypatch.setattr(ops, "rnnt_loss_bwd_exp", lambda *a, **k: (calls.append(k.get("fastemit_lambda")), orig(*a, **k))[1])
    st.set(0.0)
    loss0, g0 = _fused(model, enc_s, dec_s, y, al, ll, 1, B, st, 0.0)
    st.set(0.0)
    loss1, g1 = _fused(model, enc_s, dec_s, y, al, ll, 1, B, st, lam)
    assert calls == [0.0, lam], "the exp-domain kernels did not run"
    assert int(st.flag) == 0
    assert loss1 == loss0                                     # the cost is the plain NLL
    _, want = _oracle_joint_grads(model, enc_s, dec_s, y, al, ll, lam, delta=True)
    errs = {k: rel_err(g1[k] - g0[k], want[k]) for k in want}
    print("exp-domain FastEmit difference (J=%d V=%d, lambda %g) vs float64: %s" % (J, V, lam, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < EXP_DELTA_TOL.get(k, EXP_DELTA_TOL_DEFAULT), (k, e)
    # d logits = srow * P as the loss kernel leaves it, with and without lambda, against the reference's FastEmit part, utterance by utterance
    from oracle import tt_oracle as O
    j = model.joint
    wf, bf, wp, bp = (t.detach() for t in (j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias))
    lab = y.int().contiguous()
    shift = torch.zeros(1, device="cuda")
    P, rowsum, _, emis = ops.joint_fwd_exp(enc_s, dec_s, wf, bf, wp, bp, 1, shift, lab, 0)
    ws = ops.rnnt_workspace(*P.shape[:3], P.device)
    ops.rnnt_loss_fwd_exp(P, rowsum, lab, al, ll, 0, ws, shift, None, emis, None)
    dl = []
    for lam_ in (0.0, lam):
        Pc = P.clone()
        srow, _ = orig(Pc, lab, al, ll, 0, ws, torch.ones(1, device="cuda"), 0, 1.0 / B, fastemit_lambda=lam_)
        dl.append(srow.view(P.shape[:3])[..., None] * Pc.float())
    got = (dl[1] - dl[0]).double().cpu().numpy()
    del dl, P, rowsum, emis
    sd = {"joint." + k: v.detach().double().cpu().numpy() for k, v in j.state_dict().items()}
    num = den = 0.0
    for b in range(B):
        zb, _ = O.joint_fwd(enc_s[b:b + 1].double().cpu().numpy(), dec_s[b:b + 1].double().cpu().numpy(), sd)
        _, wb = fastemit_ref(zb, lab[b:b + 1].cpu().numpy(), al[b:b + 1].cpu().numpy(), ll[b:b + 1].cpu().numpy(), 0, lam, [1.0 / B], delta=True)
        num += float(((got[b:b + 1] - wb) ** 2).sum())
        den += float((wb ** 2).sum())
    e_logits = (num / den) ** 0.5
    print("exp-domain FastEmit difference in logit space (srow * P): %.2e" % e_logits)
    assert e_logits < EXP_LOGIT_DELTA_TOL


def test_train_py_call_sequence_keeps_the_fused_path(monkeypatch):
    """criterion = RNNTLoss(fastemit_lambda=lam); criterion(model(x, y), ...) in bf16 mode: the exp-domain projection runs, no logits are
    formed, and the gradients are those of Transducer.loss(..., exp_domain=True, fastemit_lambda=lam)"""
    import tt.model as M
    import ttmi.ops as ops
    from warprnnt_pytorch import RNNTLoss
    lam = 0.5
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16")
    crit = RNNTLoss(check_lengths=False, fastemit_lambda=lam)
    calls = {"exp": 0, "plain": 0}
    orig_exp, orig_plain = ops.joint_fwd_exp, ops.joint_fwd
    monkeypatch.setattr(ops, "joint_fwd_exp", lambda *a, **k: (calls.__setitem__("exp", calls["exp"] + 1), orig_exp(*a, **k))[1])
    monkeypatch.setattr(ops, "joint_fwd", lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), orig_plain(*a, **k))[1])

    def grads(xi):
        return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    def two_call(c):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        logits = model(xi, y)
        loss = c(logits, y.int(), al, ll)
        loss.backward()
        assert isinstance(logits, M.DeferredLogits) and not logits.is_materialized
        return float(loss.detach()), grads(xi)

    def explicit(lam_):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        loss = model.loss(xi, al, y, ll, check_lengths=False, exp_domain=True, fastemit_lambda=lam_)
        loss.backward()
        return float(loss.detach()), grads(xi)

    two_call(crit)                                           # first use: the plain fused form seeds the shift
    assert calls == {"exp": 0, "plain": 1}
    a = two_call(crit)
    assert calls == {"exp": 1, "plain": 1}
    b = explicit(lam)
    assert calls == {"exp": 2, "plain": 1}
    assert a[0] == b[0] and rel_err(a[1], b[1]) < 1e-3
    z = explicit(0.0)
    assert abs(z[0] - a[0]) < 1e-6 * a[0] and rel_err(a[1], z[1]) > 1e-2     # lambda reached the kernels: the gradient moved, the cost did not


def test_zero_lambda_is_bit_identical_on_every_path(monkeypatch):
    """fastemit_lambda=0.0 against the argument omitted, at the three loss-gradient kernels' outputs (deterministic: no atomics)"""
    import ttmi.ops as ops
    from warprnnt_pytorch import RNNTLoss
    rng = np.random.default_rng(5)
    B, T, U, V = 3, 20, 6, 40
    x = torch.tensor(rng.normal(size=(B, T, U + 1, V)) * 2, dtype=torch.float32, device="cuda")
    y = torch.tensor(rng.integers(1, V, size=(B, U)), dtype=torch.int32, device="cuda")
    tl = torch.tensor([T, T - 3, 11], dtype=torch.int32, device="cuda")
    ul = torch.tensor([U, 2, U - 1], dtype=torch.int32, device="cuda")
    # the public surface, f32 and bf16 logits
    for dt in (torch.float32, torch.bfloat16):
        outs = []
        for kw in ({}, {"fastemit_lambda": 0.0}):
            a = x.detach().clone().to(dt).requires_grad_(True)
            loss = RNNTLoss(**kw)(a, y, tl, ul)
            loss.backward()
            outs.append((loss.detach(), a.grad))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the bf16x3 planes
    planes = []
    for kw in ({}, {"fastemit_lambda": 0.0}):
        buf, lg = ops.padded_empty((B, T, U + 1, V), torch.float32, "cuda")
        buf.zero_()
        lg.copy_(x)
        ws = ops.rnnt_workspace(B, T, U + 1, x.device)
        ops.rnnt_loss_fwd(lg, y, tl, ul, 0, ws)
        ops.rnnt_loss_bwd_split(lg, y, tl, ul, 0, ws, torch.ones(1, device="cuda"), 0, 0.5, **kw)
        planes.append(buf.clone())
    assert torch.equal(planes[0], planes[1])
    # the exp-domain row factors and patched P, on a joint-sized problem
    model, xs, ys, al, ll = _training_sized(monkeypatch, "bf16")
    enc_s, dec_s = _states(model, xs, ys)
    j = model.joint
    wf, bf, wp, bp = (t.detach() for t in (j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias))
    lab = ys.int().contiguous()
    shift = torch.zeros(1, device="cuda")
    P, rowsum, _, emis = ops.joint_fwd_exp(enc_s, dec_s, wf, bf, wp, bp, 1, shift, lab, 0)
    ws = ops.rnnt_workspace(*P.shape[:3], P.device)
    ops.rnnt_loss_fwd_exp(P, rowsum, lab, al, ll, 0, ws, shift, None, emis, None)
    res = []
    for kw in ({}, {"fastemit_lambda": 0.0}, {"fastemit_lambda": 0.5}):
        Pc = P.clone()
        srow, srow16 = ops.rnnt_loss_bwd_exp(Pc, lab, al, ll, 0, ws, torch.ones(1, device="cuda"), 0, 0.125, **kw)
        res.append((Pc, srow.clone(), srow16.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][1], res[2][1])              # lambda > 0 moves the row factors


def _graph_setup(monkeypatch, lam):
    """test_graph_gpu.py's step (bench.py's sizes at which the exp-domain kernels, grouped weight gradients and weight shadows run) with lambda"""
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    from test_dp_nccl_gpu import _bench_cfg, _bench_data
    from tt.model import Transducer
    from ttmi.train import FlatModel, FusedOptimizer, GradSync
    dev = torch.device("cuda", 0)
    cfg = _bench_cfg()
    cfg["dropout"] = 0.0
    torch.manual_seed(1)
    model = Transducer(cfg).to(dev).train()
    flat = FlatModel(model)
    flat.enable_grouped_wgrads()
    flat.enable_shadows()
    sync = GradSync(flat)
    opt = FusedOptimizer(flat, kind="sgd", lr=0.00025, momentum=0.9, max_grad_norm=200.0)
    x, y = _bench_data(0, 0)
    x, y = x.to(dev), y.to(dev)
    il = torch.full((8,), 512, dtype=torch.int32, device=dev)
    tl = torch.full((8,), 7, dtype=torch.int32, device=dev)

    def step():
        flat.zero_grad()
        sync.start_step()
        loss = model.loss(x, il, y, tl, exp_domain=True, fastemit_lambda=lam)
        loss.backward()
        sync.finish()
        opt.step()
        return loss.detach()

    return model, flat, opt, step, dev


def test_graphed_step_with_fastemit_follows_the_eager_trajectory(monkeypatch):
    """a GraphedStep captured with lambda > 0 walks the eager trajectory with the same lambda (as test_graph_gpu.py's test does at 0), and
    that trajectory is not the lambda = 0 one"""
    from test_graph_gpu import _teardown
    from ttmi.train import GraphedStep
    lam = 0.5

    def eager(lam_):
        torch.manual_seed(11)
        model, flat, opt, step, dev = _graph_setup(monkeypatch, lam_)
        w0[:] = [flat.flat.cpu().numpy().copy()]
        for _ in range(6):
            step()
        torch.cuda.synchronize()
        w = flat.flat.cpu().numpy().copy()
        _teardown(flat)
        return w

    w0 = [None]
    want, plain = eager(lam), eager(0.0)
    torch.manual_seed(11)
    model, flat, opt, step, dev = _graph_setup(monkeypatch, lam)
    g = GraphedStep(step, device=dev, warmup=3, exp_state=model.joint.exp_shift_state(dev), optimizer=opt)
    losses = [float(g()) for _ in range(3)]                      # 3 eager warm-up steps + 3 replays = the 6 steps above
    torch.cuda.synchronize()
    got = flat.flat.cpu().numpy().copy()
    _teardown(flat)
    assert g.captures == 1 and all(np.isfinite(losses))
    moved = rel_err(want - w0[0], plain - w0[0])           # how far lambda moved the six updates
    print("graphed FastEmit trajectory: rel err vs eager %.2e; updates with lambda %g vs 0 differ by %.2e" % (rel_err(got, want), lam, moved))
    assert rel_err(got, want) < 5e-6                              # (test_graph_gpu.py's bound at lambda = 0; measured 2.8e-6 here)
    assert moved > 2e-3                                           # (measured 7.9e-3: three orders above the replay's own error)
