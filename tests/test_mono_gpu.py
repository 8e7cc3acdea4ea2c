"""The monotonic RNN-T loss kernels (csrc/mono.hip) driven raw through ttmi.ops against the float64 reference of tests/mono_oracle.py, and
against the beam step (csrc decode kernels): two independently written kernels walk the same lattice, so the beam's merged score of a transcript,
with nothing pruned, is minus this loss.

Tolerance: the project's 1e-4 (tests/test_rnnt_gpu.py, tests/test_ctc_gpu.py) on costs, relative to the cost, and on gradients through
conftest.rel_err.  bf16 logits: the oracle is evaluated on the bf16-rounded values widened to float64, and its gradient is rounded to bf16
before the comparison (the kernel's last step); the bound stays 1e-4.  Utterances without a path (U_b > T_b) are not compared with the oracle:
cost +inf and all-zero rows are asserted."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import mono_oracle as M
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64                     # elements behind the gradient buffer / floats behind the workspace that must keep their fill
FILL, WS_FILL = 7.0, 12345.0
GO, SCALE = np.array([0.5, -2.0, 3.0]), 0.25


def ws_floats_used(B, T, U1):
    """the bytes the documented layout occupies (alpha, beta [B, T+1, U1] f64, ll [B] f64, lse / lpb / lpl [B, T, U1] f32), in floats"""
    return (8 * (2 * B * (T + 1) * U1 + B) + 4 * 3 * B * T * U1) // 4


def run_hip(xt, labels, tl, ul, blank=0, ld=None, go=None, scale=1.0, inplace=False):
    """xt: torch f32 / bf16 [B, T, U1, V] on the host.  The logits live in a pitch-ld buffer whose pad columns start as garbage; in place the
    buffer is followed by guard elements.  The workspace is followed by guard floats.  -> (costs [B], full gradient buffer [B, T, U1, ld] f64)"""
    from ttmi import ops
    B, T, U1, V = xt.shape
    ld = V if ld is None else ld
    n = B * T * U1 * ld
    flat = torch.full((n + GUARD,), FILL, dtype=xt.dtype, device="cuda")
    buf = flat[:n].view(B, T, U1, ld)
    buf[..., :V] = xt.cuda()
    logits = buf[..., :V]
    y = torch.tensor(np.asarray(labels).reshape(B, -1), dtype=torch.int32, device="cuda")
    tlg, ulg = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (tl, ul))
    nws = ops.mono_workspace(B, T, U1, "cuda").numel()
    used = ws_floats_used(B, T, U1)
    assert used <= nws
    wsg = torch.full((nws + GUARD,), WS_FILL, dtype=torch.float32, device="cuda")
    ws = wsg[:nws]
    costs = ops.mono_loss_fwd(logits, y, tlg, ulg, blank, ws)
    g = torch.ones(B, device="cuda") if go is None else torch.tensor(np.asarray(go), dtype=torch.float32, device="cuda")
    grad = ops.mono_loss_bwd(logits, y, tlg, ulg, blank, ws, g, 1, scale, inplace=inplace)
    torch.cuda.synchronize()
    if inplace:
        assert grad.data_ptr() == logits.data_ptr()
        full = buf
    else:
        assert torch.equal(buf[..., :V].cpu(), xt)                                  # out of place: the logits are untouched
        full = torch.as_strided(grad, (B, T, U1, ld), (T * U1 * ld, U1 * ld, ld, 1))
    assert bool((flat[n:] == FILL).all()), "guard behind the gradient buffer"
    assert bool((wsg[used:] == WS_FILL).all()), "guard behind the workspace"
    return costs.cpu().numpy(), full.double().cpu().numpy()


def check(x, labels, tl, ul, blank=0, ld=None, dtype=torch.float32, inplace=False, go=None, scale=1.0):
    """one batch against the oracle -> (costs, gradient [B, T, U1, V])"""
    B, T, U1, V = x.shape
    xt = torch.tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    want_c, want_g = M.mono_loss(xt.double().numpy(), labels, tl, ul, blank)
    gov = np.ones(B) if go is None else np.asarray(go, dtype=np.float64)
    want_g = want_g * (np.float32(scale) * gov.astype(np.float32)).astype(np.float64)[:, None, None, None]
    if dtype is torch.bfloat16:
        want_g = torch.tensor(want_g).to(torch.bfloat16).double().numpy()
    costs, full = run_hip(xt, labels, tl, ul, blank, ld, go, scale, inplace)
    g = full[..., :V]
    dead = np.asarray(ul) > np.asarray(tl)
    assert np.array_equal(np.isposinf(want_c), dead)
    cerr = np.abs(costs[~dead] - want_c[~dead]) / np.abs(want_c[~dead])
    print("B %d T %d U1 %d V %d ld %s %s blank %d inplace %d: cost rel err %.2e, grad rel err %.2e"
          % (B, T, U1, V, ld, str(dtype)[6:], blank, inplace, cerr.max() if cerr.size else 0.0, rel_err(g, want_g)))
    assert np.all(np.isposinf(costs[dead])), costs                                  # no path: +inf ...
    for b in np.nonzero(dead)[0]:
        assert np.all(full[b] == 0), b                                              # ... and zero rows, never NaN
    assert np.all(cerr <= TOL), (costs, want_c)
    assert np.isfinite(g).all()
    assert rel_err(g, want_g) < TOL
    for b in range(B):
        assert np.all(full[b, tl[b]:] == 0) and np.all(full[b, :, ul[b] + 1:] == 0), b      # outside the lattice: exact zeros
    assert np.all(full[..., V:] == 0)                                               # pad columns
    if dtype is torch.float32:
        # a row is g * (softmax * occ - patches): two sets of at most V f32 terms that each add up to occ <= 1, so the sum's rounding error is
        # a few f32 ulps of |g| per addend pair at the worst - 1e-5 |g| leaves room for V = 4334 (tests/test_ctc_gpu.py)
        gmax = np.abs(np.float32(scale) * gov).max()
        assert np.abs(g.sum(-1)).max() < 1e-5 * gmax
    return costs, g


def ragged(T, U1):
    """three utterances on [T, U1]: the longest (all labels, or U_b = T_b when the label axis is longer than the frames), one with one label
    more than frames where the label axis allows it (no path), one in the middle (U_b = 0 when T is 1 or 2)"""
    t1, t2 = max(1, T - 2), max(1, T - 1)
    return [T, t1, t2], [min(U1 - 1, T), min(U1 - 1, t1 + 1), min(U1 - 1, t2 // 2)]


def case(seed, B, T, U1, V, scale=1.5):
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((B, T, U1, V))).astype(np.float32)
    labels = rng.integers(0, V, (B, max(U1 - 1, 1))).astype(np.int32)               # the whole vocabulary: some labels equal `blank`
    return x, labels


# ----------------------------------------------------------------------------- shapes: lane and slot seams, prefetch chunk, ragged lengths
U1S = [1, 2, 64, 65, 129]
TS = [1, 2, 3, 5, 7, 8, 9]     # the prefetch chunk is 8 frames up to U1 = 128 and 4 from U1 = 129: 7 / 8 / 9 and 3 / 5 sit on either side
VS = [2, 5, 67, 131]


def pitches(V):
    return [V, V + 3, (V + 63) // 64 * 64]


@pytest.mark.parametrize("U1", U1S)
@pytest.mark.parametrize("T", TS)
def test_shapes(T, U1):
    """every (T, U1); vocabulary, pitch, dtype, blank and aliasing rotate through their values with the case number"""
    i = TS.index(T) * len(U1S) + U1S.index(U1)
    V = VS[i % 4]
    ld = pitches(V)[(i // 4) % 3]
    dtype = (torch.float32, torch.bfloat16)[(i // 2) % 2]
    blank = (0, V - 1)[(i // 3) % 2]
    x, labels = case(1000 + i, 3, T, U1, V)
    tl, ul = ragged(T, U1)
    check(x, labels, tl, ul, blank, ld, dtype, inplace=bool(i % 2), go=GO, scale=SCALE)


LIVE = [(64, 66, 5), (65, 67, 5), (129, 131, 3), (300, 302, 3)]


@pytest.mark.parametrize("U1,T,V", LIVE, ids=["U1_%d" % c[0] for c in LIVE])
def test_live_cells_cross_the_seams(U1, T, V):
    """T > U: paths run through labels 63 | 64, 127 | 128, 255 | 256 (lane 63 of one slot to lane 0 of the next) in one, two, four and eight
    slots per lane; the second utterance ends one label before the seam's far side, the third has no label.

    f32 logits only.  The lattice kernel under test here never sees the logits' dtype (it reads the f32 emission tables), and the two row
    kernels that do never see the lattice's length: they are covered in bf16 by test_shapes and the vocabulary / pitch matrix below.  On a
    lattice this long the bf16 comparison stops measuring the kernel: alpha and beta carry about 3e-7 of absolute error after 300 steps of
    lae's f32 correction term (the gradient's rel_err is 5.6e-7 in f32), a handful of cells hold most of the gradient's norm, and when one
    of those lands within that error of a bf16 rounding boundary it comes out one bf16 ulp (2^-8 relative) from the rounded oracle.  Measured
    on U1 = 300, T = 302 with bf16 logits: 4 of 815 400 elements differ, ONE of them gives rel_err 1.32e-4 by itself; the same figure comes
    out of a CPU emulation of the kernel's arithmetic with exact alpha / beta perturbed by 3e-7, and 1e-10 with them unperturbed."""
    x, labels = case(U1, 3, T, U1, V)
    check(x, labels, [T, T - 1, T - 3], [U1 - 1, U1 - 2, 0], blank=V - 1, ld=V + 3, inplace=True, go=GO, scale=SCALE)


@pytest.mark.parametrize("V", VS)
def test_vocabulary_pitch_dtype_blank_aliasing(V):
    """every combination at one small ragged shape (T 4, U1 5): the 16-byte walk's head, body and tail at each row alignment"""
    x, labels = case(V, 3, 4, 5, V)
    tl, ul = [4, 3, 2], [4, 1, 3]
    for ld, dtype, blank, inplace in itertools.product(pitches(V), (torch.float32, torch.bfloat16), (0, V - 1), (False, True)):
        check(x, labels, tl, ul, blank, ld, dtype, inplace, go=GO, scale=SCALE)


def test_corner_utterances():
    """U_b = 0 (every frame blank), U_b = T_b (every frame emits), U_b = T_b + 1 (no path) in one batch, against their closed forms too"""
    x, labels = case(7, 3, 5, 7, 6)
    costs, g = check(x, labels, [5, 5, 5], [0, 5, 6], blank=2)
    lp = M.log_softmax(x)
    assert abs(costs[0] + lp[0, :, 0, 2].sum()) <= TOL * abs(costs[0])
    assert abs(costs[1] + sum(lp[1, t, t, labels[1, t]] for t in range(5))) <= TOL * abs(costs[1])
    assert np.isposinf(costs[2]) and np.all(g[2] == 0)


def test_every_label_equal_to_blank():
    """both patches land on one column; the row still sums to zero"""
    x, _ = case(8, 2, 6, 4, 5)
    labels = np.full((2, 3), 4, dtype=np.int32)
    for dtype in (torch.float32, torch.bfloat16):
        check(x, labels, [6, 4], [3, 2], blank=4, dtype=dtype, go=GO[:2], scale=SCALE)


def test_lengths_and_labels_are_clamped():
    """T_b to [1, T], U_b to [0, U1 - 1], labels to [0, V - 1]: the same bits as the clamped call"""
    x, labels = case(9, 3, 4, 4, 5)
    xt = torch.tensor(x)
    wild = labels.copy()
    wild[0, 0], wild[1, 1] = -3, 99
    a = run_hip(xt, wild, [9, 0, -2], [7, -1, 3])
    b = run_hip(xt, np.clip(wild, 0, 4), [4, 1, 1], [3, 0, 3])
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("T,Ub", [(3, 3), (1026, 1023)], ids=["T3", "live"])
def test_longest_label_axis(T, Ub):
    """U1 = 1024, sixteen slots per lane: T = 3 (almost every cell outside the lattice), and one utterance whose paths cross all fifteen seams"""
    V = 2 if T > 3 else 5
    x, labels = case(T, 1 if T > 3 else 2, T, 1024, V)
    if T > 3:
        check(x, labels, [T], [Ub], blank=1, inplace=True)
    else:
        check(x, labels, [3, 2], [3, 1], blank=0, ld=8)


def test_long_utterance_range():
    """T 1500, U 20, logits scaled until the cost is in the thousands: what the fp64 frontier is for"""
    x, labels = case(11, 1, 1500, 21, 8, scale=6.0)
    costs, _ = check(x, labels, [1500], [20], inplace=True)
    assert costs[0] > 1000.0


# ----------------------------------------------------------------------------- reproducibility, graph capture
def test_two_runs_give_identical_bits():
    x, labels = case(12, 3, 40, 70, 19)
    for dtype in (torch.float32, torch.bfloat16):
        xt = torch.tensor(x).to(dtype)
        runs = [run_hip(xt, labels, [40, 33, 70 - 40], [39, 33, 12], go=GO, scale=SCALE) for _ in range(2)]
        assert np.array_equal(runs[0][0].view(np.int32), runs[1][0].view(np.int32))
        assert np.array_equal(runs[0][1], runs[1][1])


def _hip_runtime():
    """the HIP runtime this process already holds (torch's), for the two graph queries torch does not wrap"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


def _graph_shape(raw):
    """-> (nodes, edges as index pairs) of a captured hipGraph_t"""
    hip = _hip_runtime()
    g = ctypes.c_void_p(int(raw))
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    if e.value:
        assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    idx = {nodes[i]: i for i in range(n.value)}
    return n.value, [(idx[src[i]], idx[dst[i]]) for i in range(e.value)]


def test_graph_capture_forward_and_backward():
    from ttmi import ops
    rng = np.random.default_rng(14)
    B, T, U1, V = 3, 11, 7, 37
    xa, xb = (rng.standard_normal((B, T, U1, V)).astype(np.float32) for _ in range(2))
    yh = rng.integers(0, V, (B, U1 - 1)).astype(np.int32)
    y = torch.tensor(yh, device="cuda")
    tl, ul = torch.tensor([11, 9, 4], dtype=torch.int32, device="cuda"), torch.tensor([6, 4, 0], dtype=torch.int32, device="cuda")
    go = torch.tensor([1.0, 2.0, -1.0], device="cuda")

    def run(x, w):
        costs = ops.mono_loss_fwd(x, y, tl, ul, 0, w)
        return costs, ops.mono_loss_bwd(x, y, tl, ul, 0, w, go, 1, 0.5)

    static = torch.tensor(xa, device="cuda")
    ws = ops.mono_workspace(B, T, U1, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static, ws)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static, ws)
    static.copy_(torch.tensor(xb, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    eager = run(torch.tensor(xb, device="cuda"), ops.mono_workspace(B, T, U1, "cuda"))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want_c, _ = M.mono_loss(xb, yh, [11, 9, 4], [6, 4, 0])
    assert rel_err(outs[0].cpu().numpy(), want_c) < TOL
    # the capture is ONE chain: three kernel nodes (log-sum-exp, lattice, gradient), each hanging off the one before - no memset node, no
    # parallel branch.  A second capture that keeps its hipGraph_t is looked at and never replayed.
    kept = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(kept):
        run(static, ws)
    n, edges = _graph_shape(kept.raw_cuda_graph())
    print("captured nodes %d, edges %s" % (n, edges))
    assert n == 3 and len(edges) == n - 1
    assert len({a for a, _ in edges}) == n - 1 and len({b for _, b in edges}) == n - 1       # nobody has two successors or two predecessors
    del kept


# ----------------------------------------------------------------------------- the beam step walks the same lattice
def _beam_score(lg, y, T, W=32, blank=0):
    """drive ops.beam_step frame by frame over ONE utterance with a synthetic scorer: a hypothesis spelling y[:u] gets lg[t, u, :], any other
    one fixed pseudo-random rows -> the f64 score of the slot whose tokens are y"""
    from ttmi import ops
    V, ldh = lg.shape[-1], T + 2
    dev = "cuda"

    def beam():
        return (torch.full((1, W), -np.inf, dtype=torch.float64, device=dev), torch.zeros(1, W, dtype=torch.int32, device=dev),
                torch.zeros(1, W, ldh, dtype=torch.long, device=dev), None, None)
    cur, nxt = beam(), beam()
    cur[0][0, 0] = 0.0
    parent, fresh = (torch.zeros(1, W, dtype=torch.int32, device=dev) for _ in range(2))
    T_len = torch.tensor([T], dtype=torch.int32, device=dev)

    def tokens(b):
        score, n, hist = b[0][0].cpu().numpy(), b[1][0].cpu().numpy(), b[2][0].cpu().numpy()
        return [None if not score[w] > -np.inf else [int(v) for v in hist[w, 1:1 + n[w]]] for w in range(W)]
    for t in range(T):
        rows = np.zeros((1, W, V), dtype=np.float32)
        for w, tk in enumerate(tokens(cur)):
            if tk is None:
                continue
            if tk == list(y[:len(tk)]):
                rows[0, w] = lg[t, len(tk)]
            else:
                rows[0, w] = np.random.default_rng([77, t] + tk).standard_normal(V)
        ops.beam_step(torch.tensor(rows, device=dev), torch.tensor([t], dtype=torch.int32, device=dev), T_len, cur, nxt, parent, fresh, blank)
        cur, nxt = nxt, cur
    torch.cuda.synchronize()
    final = tokens(cur)
    assert sum(tk is not None for tk in final) <= 31                               # nothing was pruned: the beam never filled
    slot = [w for w, tk in enumerate(final) if tk == list(y)]
    assert len(slot) == 1
    return float(cur[0][0, slot[0]])


def test_beam_step_merged_score_is_minus_the_cost():
    """V 3, T 4, W 32: at most 1 + 2 + 4 + 8 + 16 = 31 distinct sequences exist, so the beam holds every one of them and its merged score of y is
    the sum over all of y's monotonic paths"""
    rng = np.random.default_rng(21)
    B, T, U1, V = 3, 4, 5, 3
    x = (1.5 * rng.standard_normal((B, T, U1, V))).astype(np.float32)
    labels = rng.integers(1, V, (B, U1 - 1)).astype(np.int32)
    tl, ul = [T, T, T], [0, 2, 4]
    costs, _ = run_hip(torch.tensor(x), labels, tl, ul, blank=0)
    for b in range(B):
        score = _beam_score(x[b], labels[b, :ul[b]], T)
        print("U_b %d: beam score %.7f, -cost %.7f" % (ul[b], score, -costs[b]))
        assert abs(score + float(costs[b])) <= TOL * abs(float(costs[b]))
