"""The two per-row walks every lattice loss shares (csrc/lattice.h: row_lse, row_map), driven through ttmi.ops by all four losses - rnnt, mono,
kd (csrc/distill.hip) and ctc - forward and backward at ONE tiny ragged lattice, over the row layouts at which a walk can go wrong:

    V 3                      smaller than a vector: head only
    V 37, pitch 37           the row heads cycle through every 16-byte phase
    V 37, pitch 40           aligned rows; tails of 1 (f32) and 5 (bf16) elements
    V 300, pitch 304, + 1    the buffer starts one element into its allocation: head = NV - 1, and 74 (f32) / 37 (bf16) whole vectors, so
                             the f32 walk's lanes take a second trip
    V 600, bf16              75 whole vectors: a second trip in bf16 too

each with the blank in the first and in the last column and with three gradient targets: a buffer of the logits' pitch and 16-byte phase
(vectors), the logits themselves (in place), and a dense buffer (pitch V) whose rows do not share the logits' 16-byte phase (scalar walk;
only where the layout has such a buffer: pitch != V).  Every byte of a gradient buffer starts as garbage: the pad columns [V, pitch) and
the rows outside the ragged lattice must come back as exact zeros, the guards behind (and before) it must keep their fill.

Expected values are the float64 oracles and the tolerances are those of each loss's own GPU test for the same dtype:
    rnnt   oracle/rnnt_c.py; f32: 1e-4 on costs and through rel_err on gradients (tests/test_rnnt_gpu.py:12, 49-50); bf16: 1e-5 on costs, 6e-3
           through rel_err on gradients (tests/test_rnnt_gpu.py:156-157)
    mono   tests/mono_oracle.py; 1e-4 on costs and through rel_err on gradients, bf16: the oracle's gradient is rounded to bf16 first
           (tests/test_mono_gpu.py:5-7, 20, 71-72)
    kd     tests/distill_oracle.py; post_ok, grad_ok and 1e-4 on costs (tests/test_distill_gpu.py:92-119, 156), data() and its kappa <= 100
           condition on the oracle (tests/test_distill_gpu.py:34-47, 153)
    ctc    torch.nn.functional.ctc_loss in float64 (tests/test_ctc_gpu.py:15-28); 1e-4 on costs and through rel_err on gradients
           (tests/test_ctc_gpu.py:12, 63-65); f32 only, as the kernels are"""
import ctypes

import numpy as np
import pytest
import torch

import distill_oracle as D
import mono_oracle as M
from conftest import rel_err
from oracle.rnnt_c import rnnt_loss_c
from test_ctc_gpu import oracle as ctc_oracle
from test_distill_gpu import data as kd_data, grad_ok as kd_grad_ok, post_ok as kd_post_ok

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64                     # elements behind every buffer that must keep their fill
FILL = 7.0
B, T, U1 = 2, 3, 3             # ctc: U = U1 - 1 = 2
TL, UL = [3, 2], [2, 1]
GO, SCALE = np.array([0.5, -2.0]), 0.25
LOSSES = ["rnnt", "mono", "kd", "ctc"]
F32, BF16 = torch.float32, torch.bfloat16
#        V, pitch, offset of the buffer in its allocation (elements), dtypes
CASES = [(3, 3, 0, (F32, BF16)), (37, 37, 0, (F32, BF16)), (37, 40, 0, (F32, BF16)), (300, 304, 1, (F32, BF16)), (600, 600, 0, (BF16,))]
TARGETS = ["pitch", "inplace", "dense"]

_ref = {}


def logits_and_labels(loss, V, blank):
    """-> (x f32 [B, T, U1, V] ([B, T, V] for ctc), teacher logits (kd) or None, labels int32 [B, U1 - 1])"""
    if loss == "kd":
        # labels over the whole vocabulary: some equal `blank`.  (Seed offset 4: the first at which no node of any case here is near
        # ill-conditioned on the oracle, kappa <= 31 against the 100 that check() asserts; tests/test_distill_gpu.py: data())
        return kd_data(1000 * V + 4, V, (B, T, U1), blank)
    rng = np.random.default_rng(V)
    shape = (B, T, V) if loss == "ctc" else (B, T, U1, V)
    x = (1.5 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, V - 1, (B, U1 - 1)).astype(np.int32)
    return x, None, y + (y >= blank)                             # no label equals `blank`


def reference(loss, V, dtype, blank):
    """the float64 oracle on the values the kernels see (bf16: rounded, then widened), computed once per (loss, V, dtype, blank) and only
    read afterwards -> dict"""
    key = (loss, V, dtype, blank)
    if key in _ref:
        return _ref[key]
    x, xt, y = logits_and_labels(loss, V, blank)
    xq = torch.tensor(x).to(dtype)
    x64 = xq.double().numpy()
    r = {"x": xq, "labels": y}
    if loss == "rnnt":
        _, r["costs"], r["grad"] = rnnt_loss_c(xq.float().numpy(), y, TL, UL, blank, reduction="none")
    elif loss == "mono":
        r["costs"], r["grad"] = M.mono_loss(x64, y, TL, UL, blank)
    elif loss == "ctc":
        r["costs"], r["grad"] = ctc_oracle(x64, y, TL, UL, blank)
    else:
        r["xt"] = torch.tensor(xt).to(dtype)
        r["post"] = D.collapse(r["xt"].double().numpy(), y, TL, UL, blank)
    if loss != "kd":
        r["grad"] = np.asarray(r["grad"], dtype=np.float64) * (np.float32(SCALE) * GO.astype(np.float32)).astype(np.float64).reshape(
            (B,) + (1,) * (x.ndim - 1))
    _ref[key] = r
    return r


def to_dev(xt, ld, off):
    """xt [..., V] on the host -> (flat, buf [..., ld], logits view [..., :V]): a pitch-ld buffer `off` elements into its allocation, pad
    columns and both ends filled with FILL (the pattern of tests/test_distill_gpu.py: to_dev)"""
    n = xt[..., 0].numel() * ld
    flat = torch.full((off + n + GUARD,), FILL, dtype=xt.dtype, device="cuda")
    buf = flat[off:off + n].view(*xt.shape[:-1], ld)
    buf[..., :xt.shape[-1]] = xt.cuda()
    return flat, buf, buf[..., :xt.shape[-1]]


def guards_ok(flat, off, n):
    return bool((flat[:off] == FILL).all()) and bool((flat[off + n:] == FILL).all())


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda")


def backward_into(loss, logits, ld, y, tlg, ulg, blank, ws, go, gbuf, ldg):
    """ttmi.ops allocates the gradient it returns; a buffer of the test's own (garbage in every byte) goes through the same library entry"""
    from ttmi import lib, ops
    c_int, c_long, P = ctypes.c_int, ctypes.c_long, lambda t: ctypes.c_void_p(t.data_ptr())
    dims = [c_int(v) for v in logits.shape[:2]] + [c_int(y.shape[1] + (loss != "ctc")), c_int(logits.shape[-1])]
    args = [P(logits)] + ([c_int(0 if logits.dtype is F32 else 1)] if loss != "ctc" else []) + [c_long(ld), P(y), P(tlg), P(ulg)] + dims
    args += [c_int(blank), P(ws), P(go), c_int(1), ctypes.c_float(SCALE), P(gbuf), c_long(ldg)] + ([c_int(0)] if loss == "kd" else [])
    name = "ttmi_%s_loss_bwd" % loss
    ops.check(getattr(lib(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def run(loss, V, ld, off, dtype, blank, target):
    """one forward and one backward -> dict of host tensors: costs [B], grad (the whole gradient buffer [..., ldg]), post (kd), and what a
    caller needs to go on from the workspace (ws, y, tlg, ulg: device tensors)"""
    from ttmi import ops
    r = reference(loss, V, dtype, blank)
    xq = r["x"]
    rows = xq[..., 0].numel()
    flat, buf, logits = to_dev(xq, ld, off)
    y, tlg, ulg = i32(r["labels"]), i32(TL), i32(UL)
    go = torch.tensor(GO, dtype=torch.float32, device="cuda")
    out = {"y": y, "tlg": tlg, "ulg": ulg}
    if loss == "kd":
        post = ops.kd_collapse(to_dev(r["xt"], ld, off)[2], y, tlg, ulg, blank)
        out["post"] = post.cpu()
        ws = ops.kd_workspace(B, T, U1, "cuda")
        costs = ops.kd_loss_fwd(logits, y, tlg, ulg, blank, post, ws)
    else:
        ws = getattr(ops, loss + "_workspace")(B, T, U1 - 1 if loss == "ctc" else U1, "cuda")
        costs = getattr(ops, loss + "_loss_fwd")(logits, y, tlg, ulg, blank, ws)
    if target == "inplace":
        g = getattr(ops, loss + "_loss_bwd")(logits, y, tlg, ulg, blank, ws, go, 1, SCALE, inplace=True)
        assert g.data_ptr() == logits.data_ptr()
        full = buf
    else:
        # "pitch": the logits' pitch and offset, so that the rows share their 16-byte phase; "dense": pitch V at offset 0, which they do not
        ldg, goff = (ld, off) if target == "pitch" else (V, 0)
        es = xq.element_size()
        shared = (off - goff) * es % 16 == 0 and (ld - ldg) * es % 16 == 0
        assert shared == (target == "pitch"), "the case does not reach the walk it is meant for"
        gflat = torch.full((goff + rows * ldg + GUARD,), FILL, dtype=dtype, device="cuda")
        full = gflat[goff:goff + rows * ldg].view(*xq.shape[:-1], ldg)
        backward_into(loss, logits, ld, y, tlg, ulg, blank, ws, go, full, ldg)
        torch.cuda.synchronize()
        assert guards_ok(gflat, goff, rows * ldg), "guards around the gradient buffer"
        assert torch.equal(logits.cpu(), xq), "out of place: the logits are untouched"
    torch.cuda.synchronize()
    assert guards_ok(flat, off, rows * ld), "guards around the logits"
    out.update(costs=costs.cpu(), grad=full.cpu(), ws=ws)
    return out


def check(loss, V, ld, off, dtype, blank, target):
    r = reference(loss, V, dtype, blank)
    out = run(loss, V, ld, off, dtype, blank, target)
    costs, full = out["costs"].double().numpy(), out["grad"].double().numpy()
    g = full[..., :V]
    if loss == "kd":
        perr = kd_post_ok(out["post"].double().numpy(), r["post"], TL, UL)
        # the student's oracle takes the teacher's posteriors as the kernels computed them (tests/test_distill_gpu.py:148)
        want_c, want_g, _ = D.kd_loss(r["x"].double().numpy(), out["post"].double().numpy(), r["labels"], TL, UL, blank)
        x64 = r["x"].double().numpy()
        smax = np.exp(x64.max(-1) - np.log(np.exp(x64 - x64.max(-1, keepdims=True)).sum(-1)) - x64.max(-1))
        kappa = max((smax[b, :TL[b], :UL[b] + 1] / np.abs(want_g[b, :TL[b], :UL[b] + 1]).max(-1)).max() for b in range(B))
        assert kappa <= 100.0, "the case has an ill-conditioned node (its data, not the kernel): kappa = %.1e" % kappa
        want_g = want_g * (np.float32(SCALE) * GO.astype(np.float32)).astype(np.float64)[:, None, None, None]
        cerr = (np.abs(costs - want_c) / np.abs(want_c)).max()
        gerr = kd_grad_ok(g, want_g, dtype, target)
        print("kd   V %d ld %d off %d %s blank %d %s: post %.2e cost %.2e grad %.2e%s"
              % (V, ld, off, str(dtype)[6:], blank, target, perr, cerr, gerr, " (bf16: ulps)" if dtype is BF16 else ""))
        assert cerr <= TOL
    else:
        want_c, want_g = np.asarray(r["costs"], dtype=np.float64), r["grad"]
        ctol, gtol = TOL, TOL
        if dtype is BF16 and loss == "rnnt":
            ctol, gtol = 1e-5, 6e-3
        if dtype is BF16 and loss == "mono":
            want_g = torch.tensor(want_g).to(BF16).double().numpy()
        cerr = (np.abs(costs - want_c) / np.abs(want_c)).max()
        gerr = rel_err(g, want_g)
        print("%-4s V %d ld %d off %d %s blank %d %s: cost %.2e grad %.2e" % (loss, V, ld, off, str(dtype)[6:], blank, target, cerr, gerr))
        assert np.isfinite(want_c).all() and cerr <= ctol
        assert np.isfinite(g).all() and gerr < gtol
    assert np.all(full[..., V:] == 0), "pad columns"
    for b in range(B):                                           # outside the ragged lattice: exact zeros, pad columns included
        assert np.all(full[b, TL[b]:] == 0), b
        if loss != "ctc":
            assert np.all(full[b, :, UL[b] + 1:] == 0), b


def targets(V, ld):
    return TARGETS if ld != V else TARGETS[:2]                   # pitch == V: the dense buffer IS the buffer of the logits' pitch


def dtypes_of(loss, case):
    return [d for d in case[3] if loss != "ctc" or d is F32]     # the ctc kernels take f32 logits only


SWEEP = [(loss, case) for loss in LOSSES for case in CASES if dtypes_of(loss, case)]


@pytest.mark.parametrize("loss,case", SWEEP, ids=["%s_V%d_ld%d_off%d" % ((s[0],) + s[1][:3]) for s in SWEEP])
def test_row_walks(loss, case):
    V, ld, off, _ = case
    for dtype in dtypes_of(loss, case):
        for blank in (0, V - 1):
            for target in targets(V, ld):
                check(loss, V, ld, off, dtype, blank, target)
