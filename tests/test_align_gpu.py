"""Forced alignment (ttmi_rnnt_align) and emission statistics (ttmi_rnnt_emit_stats) on the GPU, against the float64 reference of
tests/test_align.py evaluated on the logits the kernel saw (bf16 logits are rounded to bf16 first, then taken to float64)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_align import GPU_PLANTED_CASES, emit_stats_ref, path_score, planted_batch, planted_gap, viterbi_ref
from test_model_gpu import build

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's fp32 tolerance for the loss against the oracle (README round 1, tests/test_rnnt_gpu.py)


def _dev(logits, labels, al, ll, dtype):
    x = torch.tensor(logits, device="cuda").to(dtype)
    seen = x.double().cpu().numpy()                      # what the kernel saw, in float64
    return x, seen, torch.tensor(labels, device="cuda"), torch.tensor(al, device="cuda"), torch.tensor(ll, device="cuda")


def _random_batch(seed, B, T, U, V, scale=2.0):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, U + 1, V)) * scale).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U)).astype(np.int32)
    al = rng.integers(1, T + 1, size=B).astype(np.int32)
    ll = rng.integers(0, U + 1, size=B).astype(np.int32)
    al[0], ll[0] = T, U
    return logits, labels, al, ll


@pytest.fixture
def placement(request):
    from ttmi import ops
    ops.set_option(23, request.param)
    yield request.param
    ops.set_option(23, 0)


# ----------------------------------------------------------------------------- 1. planted paths, exact
@pytest.mark.parametrize("placement", [0, 1], ids=["lds_by_shape", "global_forced"], indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GPU_PLANTED_CASES, ids=[c[0] for c in GPU_PLANTED_CASES])
def test_planted_paths_exact(case, dtype, placement):
    """placement 0: decision words in LDS where an utterance's words fit 128 KB (every case but u1_1024, which is in global memory by its
    shape); placement 1: in the caller's workspace whatever the shape"""
    from warprnnt_pytorch import rnnt_align
    _, seed, B, T, U = case
    logits, labels, al, ll, planted = planted_batch(seed, B, T, U)
    x, seen, y, tl, ul = _dev(logits, labels, al, ll, dtype)
    res = rnnt_align(x, y, tl, ul)
    frames, score = res.frames.cpu().numpy(), res.score.cpu().numpy()
    assert frames.shape == (B, U) and frames.dtype == np.int32 and score.shape == (B,)
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        if dtype is torch.bfloat16:          # the rounded logits still plant the same path, far from a tie
            ref_frames, _ = viterbi_ref(seen[b], labels[b], Tb, Ub)
            assert list(ref_frames) == list(planted[b, :Ub]) and planted_gap(seen[b], labels[b], Tb, Ub, planted[b]) > 1.0
        assert list(frames[b, :Ub]) == list(planted[b, :Ub]), (b, Tb, Ub)
        assert (frames[b, Ub:] == -1).all()
        want = path_score(seen[b], labels[b], Tb, Ub, planted[b, :Ub])
        assert abs(score[b] - want) <= TOL * abs(want), (b, score[b], want)


# ----------------------------------------------------------------------------- 2. random logits, optimality
RANDOM_CASES = [(31, 4, 60, 12, 16), (32, 3, 500, 50, 16), (33, 3, 300, 200, 8), (34, 2, 7, 600, 8), (35, 3, 1, 9, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", RANDOM_CASES, ids=["B%d_T%d_U%d" % c[1:4] for c in RANDOM_CASES])
def test_random_logits_optimality(case, dtype):
    from warprnnt_pytorch import rnnt_align
    seed, B, T, U, V = case
    logits, labels, al, ll = _random_batch(seed, B, T, U, V)
    x, seen, y, tl, ul = _dev(logits, labels, al, ll, dtype)
    res = rnnt_align(x, y, tl, ul)
    frames, score = res.frames.cpu().numpy(), res.score.cpu().numpy()
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        f = frames[b, :Ub]
        assert (frames[b, Ub:] == -1).all()
        assert all(0 <= f[i] < Tb for i in range(Ub)) and all(f[i] <= f[i + 1] for i in range(Ub - 1)), (b, f)
        _, best = viterbi_ref(seen[b], labels[b], Tb, Ub)
        got = path_score(seen[b], labels[b], Tb, Ub, f)
        print("utt %d: best %.6f, returned path %.6f (gap %.3e), kernel score %.6f" % (b, best, got, best - got, score[b]))
        assert best - got <= TOL * abs(best), (b, best, got)
        assert abs(score[b] - got) <= TOL * abs(got), (b, score[b], got)


# ----------------------------------------------------------------------------- 3. emission statistics
def _check_stats(seen, labels, al, ll, expected, mass):
    B, U = labels.shape
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        want_e, want_m, _ = emit_stats_ref(seen[b], labels[b], Tb, Ub)
        assert (mass[b, Ub:] == 0).all() and (expected[b, Ub:] == -1).all()
        if Ub:
            em, ee = np.abs(mass[b, :Ub] - 1.0).max(), np.abs(expected[b, :Ub] - want_e).max()
            print("utt %d (T_b %d, U_b %d): |mass - 1| max %.2e, |expected - ref| max %.2e frames" % (b, Tb, Ub, em, ee))
            assert np.abs(want_m - 1.0).max() < 1e-9
            assert em <= TOL and ee <= TOL * Tb, (b, em, ee)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", GPU_PLANTED_CASES, ids=[c[0] for c in GPU_PLANTED_CASES])
def test_emission_statistics(case, dtype):
    from warprnnt_pytorch import rnnt_align
    _, seed, B, T, U = case
    logits, labels, al, ll, _ = planted_batch(seed, B, T, U)
    logits = (logits * 0.5).astype(np.float32)           # softer than the planted +8, so that the posteriors are spread over several frames
    x, seen, y, tl, ul = _dev(logits, labels, al, ll, dtype)
    res = rnnt_align(x, y, tl, ul, stats=True)
    assert res.expected_frames.shape == (B, U) and res.mass.shape == (B, U)
    _check_stats(seen, labels, al, ll, res.expected_frames.cpu().numpy(), res.mass.cpu().numpy())


def test_emission_statistics_c5_lattice():
    """C5's lattice size once: B 8, T 2000, U 200 (a small vocabulary keeps the logits at 100 MB; the lattice is the same)"""
    from warprnnt_pytorch import rnnt_align
    logits, labels, al, ll = _random_batch(41, 8, 2000, 200, 8, scale=1.0)
    x, seen, y, tl, ul = _dev(logits, labels, al, ll, torch.float32)
    res = rnnt_align(x, y, tl, ul, stats=True)
    _check_stats(seen, labels, al, ll, res.expected_frames.cpu().numpy(), res.mass.cpu().numpy())
    frames = res.frames.cpu().numpy()
    for b in (0, 1):
        Tb, Ub = int(al[b]), int(ll[b])
        _, best = viterbi_ref(seen[b], labels[b], Tb, Ub)
        got = path_score(seen[b], labels[b], Tb, Ub, frames[b, :Ub])
        assert best - got <= TOL * abs(best) and abs(float(res.score[b]) - got) <= TOL * abs(got)


# ----------------------------------------------------------------------------- 4. cost is the loss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cost_is_the_loss(dtype):
    from warprnnt_pytorch import RNNTLoss, rnnt_align
    logits, labels, al, ll = _random_batch(51, 5, 40, 11, 29)
    x, _, y, tl, ul = _dev(logits, labels, al, ll, dtype)
    want = RNNTLoss(reduction="none")(x, y, tl, ul)
    res = rnnt_align(x, y, tl, ul)
    assert torch.equal(res.cost, want)
    assert res.expected_frames is None and res.mass is None
    assert (res.score <= -res.cost + 1e-4 * res.cost.abs()).all()       # one path cannot weigh more than all of them


# ----------------------------------------------------------------------------- 5. the loss does not notice
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_backward_after_align_gives_the_same_bits(dtype):
    from ttmi import ops
    logits, labels, al, ll = _random_batch(52, 4, 50, 70, 16)
    x, _, y, tl, ul = _dev(logits, labels, al, ll, dtype)
    B, T, U1, _ = x.shape
    go = torch.ones(B, device="cuda")
    grads, spaces = [], []
    for with_align in (False, True):
        ws = ops.rnnt_workspace(B, T, U1, x.device)
        ops.rnnt_loss_fwd(x, y, tl, ul, 0, ws)
        before = ws.clone()
        if with_align:
            ops.rnnt_align(ws, tl, ul, B, T, U1)
            ops.rnnt_emit_stats(ws, tl, ul, B, T, U1)
            assert torch.equal(ws.view(torch.int32), before.view(torch.int32))       # the loss workspace is read-only here
        grads.append(ops.rnnt_loss_bwd(x, y, tl, ul, 0, ws, go, 1, 1.0))
    assert torch.equal(grads[0].view(torch.int16 if dtype is torch.bfloat16 else torch.int32),
                       grads[1].view(torch.int16 if dtype is torch.bfloat16 else torch.int32))


# ----------------------------------------------------------------------------- 6. fused path = two-call path (fp32 mode)
@pytest.mark.parametrize("name", ["tiny_klong", "tiny_kshort"])
def test_fused_path_equals_two_call_path(name, monkeypatch):
    from warprnnt_pytorch import rnnt_align
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    z, sd = load_golden(name)
    model = build(sd)
    inp, tgt = torch.tensor(z["inputs"], device="cuda"), torch.tensor(z["targets"], device="cuda")
    al, ll = torch.tensor(z["ragged/act_lens"], device="cuda"), torch.tensor(z["ragged/label_lens"], device="cuda")
    assert inp.shape[0] > 1
    fused = model.align(inp, al, tgt, ll, chunk=1, check_lengths=False, stats=True)
    with torch.no_grad():
        two = rnnt_align(model(inp, tgt), tgt.int(), al, ll, check_lengths=False, stats=True)
    assert torch.equal(fused.frames, two.frames)
    for a, b in ((fused.score, two.score), (fused.cost, two.cost), (fused.expected_frames, two.expected_frames), (fused.mass, two.mass)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the handle of the bf16 pipeline goes through the same loop instead of being materialised
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1")
    with torch.no_grad():
        h = model(inp, tgt)
    got = rnnt_align(h, tgt.int(), al, ll, check_lengths=False)
    assert not h.is_materialized
    want = model.align(inp, al, tgt, ll, check_lengths=False)
    assert torch.equal(got.frames, want.frames) and torch.equal(got.cost, want.cost)


# ----------------------------------------------------------------------------- 7. exp-domain form (bf16 mode)
def _training_sized(monkeypatch, prec, seed, J=1024, V=4334):
    from tt.model import Transducer
    from tt.utils import AttrDict
    monkeypatch.setenv("TTMI_PRECISION", prec)
    side = dict(n_layer=1, d_model=512, n_head=8, d_head=64, d_inner=256)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=64), dec=dict(side, max_target_length=16),
                        joint=dict(input_size=1024, inner_size=J), vocab_size=V, dropout=0.0))
    torch.manual_seed(seed)
    model = Transducer(cfg).cuda().train()
    B, T, U = 8, 200, 20
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    x = torch.randn(B, T, 512, device="cuda", generator=g)
    y = torch.randint(1, V, (B, U), device="cuda", generator=g)
    al = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ll = torch.full((B,), U, dtype=torch.int32, device="cuda")
    al[2], ll[2] = 150, 11
    return model, x, y, al, ll


# twice the worst gap measured over the test's seeds (docstring of test_exp_domain_form).  The measured worst value is 0, so the factor of two
# leaves NO head-room: the test demands that the bf16 exp-domain form returns exactly the float64-optimal path of the fp32-mode logits for
# all 16 utterances, and a rebuild of the GEMM library that flips one near-tie would turn it red.  That is the bound the feature's issue sets
# (twice the measured value, nothing wider); a failure here is to be read as "re-measure and explain", not as a defect by itself.
EXP_GAP_BOUND = 2 * 0.0


def _step(model, x, y, al, ll):
    model.zero_grad()
    loss = model.loss(x, al, y, ll, check_lengths=False, chunk=x.shape[0], exp_domain=True)
    loss.backward()
    return loss.detach().clone()


@pytest.mark.parametrize("seed", [2, 7])
def test_exp_domain_form(monkeypatch, seed):
    """B 8, T 200, U 20, J 1024, V 4334 in one chunk (33600 lattice rows), bf16 mode, after one training step has made the shift valid.
    The returned path is scored in float64 on the FP32-MODE logits of the same model and inputs and compared with the float64 optimum on
    those logits: gap = (best - score of the returned path) / |best|.
    MEASURED on one MI355X over both seeds and all 16 utterances: worst gap 0.0 - the exp-domain bf16 form returned the float64-optimal
    path of the fp32-mode logits for every utterance (best-path scores -1264 ... -1794; the kernel's own bf16-mode scores differ from them
    by up to 2.5e-2 absolute, 1.4e-5 relative).  The asserted bound is twice the measured worst value, i.e. 0 (the project's bound for one
    utterance's bf16 loss, 3e-4, was not approached; see the note at EXP_GAP_BOUND on what a zero bound means).  The exp-domain result is
    the one that is kept: the plain joint forward is not called inside the align call.  The module's _ExpShift (cur, nxt, flag, valid) is unchanged by the call
    and a training step after it gives the same loss bits as without it."""
    import ttmi.ops as ops
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16", seed)
    assert ops.joint_exp_supported(8, 200, 21, 1024, 4334, 1, fwd_only=True)
    st = model.joint.exp_shift_state(x.device)
    _step(model, x, y, al, ll)                               # plain form, seeds the shift
    assert st.valid
    torch.cuda.synchronize()
    snap = (st.cur.clone(), st.nxt.clone(), st.flag.clone(), st.valid, st.gen, len(st.pending))
    calls = []
    orig = ops.joint_fwd_exp
    plain_calls = []
    orig_plain = ops.joint_fwd
    monkeypatch.setattr(ops, "joint_fwd_exp", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    monkeypatch.setattr(ops, "joint_fwd", lambda *a, **k: (plain_calls.append(1), orig_plain(*a, **k))[1])
    res = model.align(x, al, y, ll, check_lengths=False, chunk=8, exp_domain=True, stats=True)
    torch.cuda.synchronize()
    assert calls, "the exp-domain kernels did not run"
    assert not plain_calls, "the exp-domain chunk was run again in the plain form: its result was not the one returned"
    monkeypatch.setattr(ops, "joint_fwd_exp", orig)
    monkeypatch.setattr(ops, "joint_fwd", orig_plain)
    assert torch.equal(st.cur, snap[0]) and torch.equal(st.nxt, snap[1]) and torch.equal(st.flag, snap[2])
    assert (st.valid, st.gen, len(st.pending)) == snap[3:]
    after = _step(model, x, y, al, ll)                       # the exp-domain training step that follows
    # the same two steps on an identical model without the align call in between
    model2, x2, y2, al2, ll2 = _training_sized(monkeypatch, "bf16", seed)
    _step(model2, x2, y2, al2, ll2)
    want = _step(model2, x2, y2, al2, ll2)
    assert torch.equal(after.view(torch.int32), want.view(torch.int32))
    # the reference's terms: fp32-mode logits of the same model and inputs
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    with torch.no_grad():
        logits = model(x, y)
    frames = res.frames.cpu().numpy()
    yl, tl, ul = y.cpu().numpy(), al.cpu().numpy(), ll.cpu().numpy()
    worst = 0.0
    for b in range(x.shape[0]):
        Tb, Ub = int(tl[b]), int(ul[b])
        z = logits[b].double().cpu().numpy()
        f = frames[b, :Ub]
        assert all(0 <= f[i] < Tb for i in range(Ub)) and all(f[i] <= f[i + 1] for i in range(Ub - 1)) and (frames[b, Ub:] == -1).all()
        _, best = viterbi_ref(z, yl[b], Tb, Ub)
        got = path_score(z, yl[b], Tb, Ub, f)
        gap = (best - got) / abs(best)
        worst = max(worst, gap)
        print("seed %d utt %d: best %.5f, returned path %.5f, gap %.3e; kernel score %.5f; |mass - 1| max %.2e"
              % (seed, b, best, got, gap, float(res.score[b]), float((res.mass[b, :Ub] - 1).abs().max())))
    print("seed %d: worst gap %.3e" % (seed, worst))
    assert worst <= EXP_GAP_BOUND, worst


def test_exp_domain_form_falls_back_when_the_shift_does_not_fit(monkeypatch):
    """the fallback branch of the forward-only loop: with a shift far above the logits every exp(logit - shift) underflows, the loss
    kernel raises THIS CALL'S flag (not the module's), and the chunk is run again in the plain form - the result is the plain form's bit
    for bit, and the module's flag / valid / nxt are untouched.  The shift is put back afterwards."""
    import ttmi.ops as ops
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16", 2)
    st = model.joint.exp_shift_state(x.device)
    _step(model, x, y, al, ll)                               # plain form, seeds the shift
    assert st.valid
    want = model.align(x, al, y, ll, check_lengths=False, chunk=8, exp_domain=False, stats=True)
    torch.cuda.synchronize()
    keep = st.cur.clone()
    snap = (st.nxt.clone(), st.flag.clone(), st.valid, st.gen, len(st.pending))
    counts = {"exp": 0, "plain": 0}
    orig_exp, orig_plain = ops.joint_fwd_exp, ops.joint_fwd
    monkeypatch.setattr(ops, "joint_fwd_exp", lambda *a, **k: (counts.__setitem__("exp", counts["exp"] + 1), orig_exp(*a, **k))[1])
    monkeypatch.setattr(ops, "joint_fwd", lambda *a, **k: (counts.__setitem__("plain", counts["plain"] + 1), orig_plain(*a, **k))[1])
    try:
        st.cur.fill_(1.0e4)                                  # exp(logit - 1e4) == 0 in every row
        got = model.align(x, al, y, ll, check_lengths=False, chunk=8, exp_domain=True, stats=True)
        torch.cuda.synchronize()
    finally:
        st.cur.copy_(keep)
        monkeypatch.setattr(ops, "joint_fwd_exp", orig_exp)
        monkeypatch.setattr(ops, "joint_fwd", orig_plain)
    assert counts == {"exp": 1, "plain": 1}, counts
    assert torch.equal(st.nxt, snap[0]) and torch.equal(st.flag, snap[1]) and int(st.flag) == 0
    assert (st.valid, st.gen, len(st.pending)) == snap[2:]
    assert torch.equal(got.frames, want.frames)
    for a, b in ((got.score, want.score), (got.cost, want.cost), (got.expected_frames, want.expected_frames), (got.mass, want.mass)):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- 8. graph capture
def test_graph_capture():
    from ttmi import ops
    B, T, U = 3, 40, 10
    la, labels, al, ll, _ = planted_batch(61, B, T, U)
    lb, _, _, _, _ = planted_batch(62, B, T, U)
    lb = (lb * 0.5).astype(np.float32)
    y, tl, ul = torch.tensor(labels, device="cuda"), torch.tensor(al, device="cuda"), torch.tensor(ll, device="cuda")
    static = torch.tensor(la, device="cuda")
    U1 = U + 1
    ws = ops.rnnt_workspace(B, T, U1, static.device)

    def run(x, w):
        cost = ops.rnnt_loss_fwd(x, y, tl, ul, 0, w)
        frames, score = ops.rnnt_align(w, tl, ul, B, T, U1)
        expected, mass = ops.rnnt_emit_stats(w, tl, ul, B, T, U1)
        return cost, frames, score, expected, mass

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static, ws)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static, ws)
    static.copy_(torch.tensor(lb, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    eager = run(torch.tensor(lb, device="cuda"), ops.rnnt_workspace(B, T, U1, static.device))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (outs[1][0] >= 0).all() and abs(float(outs[4][0, 0]) - 1.0) < 1e-4
