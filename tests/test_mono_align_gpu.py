"""Forced alignment (ttmi_mono_align) and emission statistics (ttmi_mono_emit_stats) on the monotonic lattice, driven raw on the GPU against
the float64 reference of tests/mono_align_oracle.py evaluated on the logits the kernel saw (bf16 logits are rounded to bf16 first, then taken
to float64).  TOL is the project's fp32 bound (tests/test_align_gpu.py): relative on scores, absolute on the emission mass, times T_b on the
expected frames.  Frames of planted paths are compared exactly (tests/test_mono_align_oracle.py checks the planted path's gap); on random
logits the returned path is scored by the oracle and has to be optimal, not identical."""
import ctypes

import numpy as np
import pytest
import torch

import mono_align_oracle as A

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64                     # elements behind every output and behind the align workspace that must keep their fill
FR_FILL, F_FILL, AWS_FILL = -77, 12345.0, 0x5A5A5A5A5A5A5A5A


@pytest.fixture
def placement(request):
    from ttmi import ops
    ops.set_option(23, request.param)
    yield request.param
    ops.set_option(23, 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_hip(x, labels, al, ll, blank=0, stats=True):
    """x: device logits [B, T, U1, V] -> dict of host arrays: cost, frames [B, U1-1], score, expected, mass (None without stats).  The library
    is called through its C entry points on buffers of this test's own, each followed by guard elements; the monotonic workspace is compared
    byte for byte before and after the two calls."""
    import ttmi
    from ttmi import ops
    L = ttmi.lib()
    B, T, U1, _ = x.shape
    n = B * (U1 - 1)
    y, tl, ul = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (labels, al, ll))
    ws = ops.mono_workspace(B, T, U1, "cuda")
    ws.fill_(0.0)                                            # (entries outside the ragged lattice are never written: a fixed fill keeps two runs comparable)
    cost = ops.mono_loss_fwd(x, y, tl, ul, blank, ws)
    before = ws.clone()
    f = L.ttmi_mono_align_workspace_bytes
    f.restype = ctypes.c_size_t
    nw = (f(B, T, U1) + 7) // 8
    assert nw > 0
    aws = torch.full((nw + GUARD,), AWS_FILL, dtype=torch.int64, device="cuda")
    fr = torch.full((n + GUARD,), FR_FILL, dtype=torch.int32, device="cuda")
    sc = torch.full((B + GUARD,), F_FILL, dtype=torch.float32, device="cuda")
    ex = torch.full((n + GUARD,), F_FILL, dtype=torch.float32, device="cuda")
    ms = torch.full((n + GUARD,), F_FILL, dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ttmi.check(L.ttmi_mono_align(_ptr(ws), _ptr(tl), _ptr(ul), B, T, U1, _ptr(aws), _ptr(fr), _ptr(sc), st), "ttmi_mono_align")
    if stats:
        ttmi.check(L.ttmi_mono_emit_stats(_ptr(ws), _ptr(tl), _ptr(ul), B, T, U1, _ptr(ex), _ptr(ms), st), "ttmi_mono_emit_stats")
    torch.cuda.synchronize()
    assert torch.equal(ws.view(torch.int32), before.view(torch.int32)), "the monotonic workspace is read only"
    assert bool((aws[nw:] == AWS_FILL).all()), "guard behind the align workspace"
    assert bool((fr[n:] == FR_FILL).all()) and bool((sc[B:] == F_FILL).all()), "guard behind frames / score"
    assert bool((ex[n:] == F_FILL).all()) and bool((ms[n:] == F_FILL).all()), "guard behind expected / mass"
    out = dict(cost=cost.cpu().numpy(), frames=fr[:n].view(B, U1 - 1).cpu().numpy(), score=sc[:B].cpu().numpy(), expected=None, mass=None,
               ws=ws, y=y, tl=tl, ul=ul)
    if stats:
        out["expected"], out["mass"] = ex[:n].view(B, U1 - 1).cpu().numpy(), ms[:n].view(B, U1 - 1).cpu().numpy()
    return out


def _dev(logits, dtype):
    x = torch.tensor(logits, device="cuda").to(dtype)
    return x, x.double().cpu().numpy()                       # the device logits, and what the kernel saw in float64


# ----------------------------------------------------------------------------- the seam batches
U1S = [1, 2, 64, 65, 66, 128, 129, 257]


def prefetch_chunk(U1):
    """the (R, PF) ladder of csrc/mono.hip: frames per prefetch chunk"""
    return 8 if U1 <= 128 else 4 if U1 <= 256 else 2 if U1 <= 512 else 1


def seam_lengths(U1):
    """(T, act_lens, label_lens) of one ragged batch on a U1-wide lattice: T_b on both sides of the prefetch chunk (1, PF-1, PF, PF+1, 2 PF+1),
    alternately with U_b = T_b and U_b = T_b // 2; U_b = 0; U_b = 63, 64, 65 and U1-1 where the lattice is that wide, each with three frames to
    spare (the path crosses lane 63 -> 0 and a ballot-word boundary) and U1-1 once more with U_b = T_b; and one utterance with more labels than
    frames between two healthy ones.  Every T_b but the longest is below T."""
    PF, Umax = prefetch_chunk(U1), U1 - 1
    pairs = []
    for i, Tb in enumerate(sorted({1, PF - 1, PF, PF + 1, 2 * PF + 1} - {0})):
        pairs.append((Tb, min(Umax, Tb if i % 2 == 0 else Tb // 2)))
    pairs.append((5, 0))
    if Umax >= 2:
        pairs.insert(2, (min(Umax, 4) - 1, min(Umax, 4)))               # no path
    for Ub in sorted({63, 64, 65, Umax}):
        if 0 < Ub <= Umax:
            pairs.append((Ub + 3, Ub))
    if Umax > 0:
        pairs.append((Umax, Umax))
    T = max(p[0] for p in pairs)
    return T, [p[0] for p in pairs], [p[1] for p in pairs]


def check_planted(seed, T, U, al, ll, dtype, stats=False):
    logits, labels, al, ll, planted = A.planted_batch(seed, T, U, al, ll)
    x, seen = _dev(logits, dtype)
    got = run_hip(x, labels, al, ll, stats=stats)
    B = len(al)
    assert got["frames"].shape == (B, U) and got["frames"].dtype == np.int32
    worst = 0.0
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        fr, sc = got["frames"][b], got["score"][b]
        if Ub > Tb:
            assert np.isneginf(sc) and (fr == -1).all() and np.isposinf(got["cost"][b]), (b, sc, fr)
            continue
        lpb, lpl = A.tables(seen[b], labels[b], Tb, Ub)
        if dtype is torch.bfloat16:
            assert np.array_equal(A.viterbi_ref(lpb, lpl)[0], planted[b, :Ub])      # the rounded logits still plant the same path
        assert np.array_equal(fr[:Ub], planted[b, :Ub]), (b, Tb, Ub, fr[:Ub], planted[b, :Ub])
        assert (fr[Ub:] == -1).all()
        want = A.path_score(lpb, lpl, planted[b, :Ub])
        worst = max(worst, abs(sc - want) / abs(want))
        assert abs(sc - want) <= TOL * abs(want), (b, Tb, Ub, sc, want)
        if Ub == Tb or Ub == 0:                              # one path: the best path is the whole likelihood
            assert abs(sc + got["cost"][b]) <= TOL * abs(got["cost"][b]), (b, sc, got["cost"][b])
        assert sc <= -got["cost"][b] + TOL * abs(got["cost"][b])
    print("B %d T %d U1 %d %s: score rel err max %.2e" % (B, T, U + 1, str(dtype)[6:], worst))
    return got, seen, labels


@pytest.mark.parametrize("placement", [0, 1], ids=["lds_by_shape", "global_forced"], indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("U1", U1S)
def test_planted_paths_exact(U1, dtype, placement):
    T, al, ll = seam_lengths(U1)
    assert any(u > t for t, u in zip(al, ll)) == (U1 >= 3) and any(u == t for t, u in zip(al, ll)) == (U1 >= 2) and 0 in ll
    check_planted(500 + U1, T, U1 - 1, al, ll, dtype)


@pytest.mark.parametrize("placement", [0, 1], ids=["lds_by_shape", "global_forced"], indirect=True)
def test_planted_paths_u1_1024(placement):
    """the sixteen-slot instantiation (prefetch chunk 1): T_b 1, 2, 3 and 40, and an utterance with 1023 labels on 40 frames between them"""
    check_planted(1024, 40, 1023, [40, 1, 40, 2, 3, 38], [40, 1, 1023, 0, 3, 17], torch.float32)


def test_planted_path_in_global_memory_by_shape():
    """B 1, T 1030, U1 1024: 1030 * 16 decision words are 131 840 bytes, over the 128 KB kept in LDS; the path crosses every slot seam"""
    check_planted(1030, 1030, 1023, [1030], [1023], torch.float32)


# ----------------------------------------------------------------------------- random logits: optimality, not identity
RANDOM_CASES = [(31, 4, 60, 12, 16), (32, 3, 500, 50, 16), (33, 3, 300, 200, 8), (34, 2, 7, 6, 8), (35, 3, 1, 1, 16)]


def random_batch(seed, B, T, U, V, scale=2.0):
    """U_b <= T_b everywhere but in utterance 1 of the batches that can hold an utterance without a path (B >= 3, U >= 2)"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, U + 1, V)) * scale).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U)).astype(np.int32)
    al = rng.integers(1, T + 1, size=B).astype(np.int32)
    al[0] = T
    ll = np.array([rng.integers(0, min(U, t) + 1) for t in al], dtype=np.int32)
    ll[0] = min(U, T)
    if B >= 3 and U >= 2:
        al[1], ll[1] = U - 1, U
    return logits, labels, al, ll


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", RANDOM_CASES, ids=["B%d_T%d_U%d" % c[1:4] for c in RANDOM_CASES])
def test_random_logits_optimality(case, dtype):
    seed, B, T, U, V = case
    logits, labels, al, ll = random_batch(seed, B, T, U, V)
    x, seen = _dev(logits, dtype)
    got = run_hip(x, labels, al, ll, stats=False)
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        fr, sc = got["frames"][b], got["score"][b]
        assert (fr[Ub:] == -1).all()
        if Ub > Tb:
            assert np.isneginf(sc) and (fr == -1).all()
            continue
        f = fr[:Ub]
        assert all(0 <= f[i] < Tb for i in range(Ub)) and all(f[i] < f[i + 1] for i in range(Ub - 1)), (b, f)      # STRICTLY increasing
        lpb, lpl = A.tables(seen[b], labels[b], Tb, Ub)
        _, best = A.viterbi_ref(lpb, lpl)
        path = A.path_score(lpb, lpl, f)
        print("utt %d (T_b %d, U_b %d): best %.6f, returned path %.6f (gap %.3e), kernel score %.6f" % (b, Tb, Ub, best, path, best - path, sc))
        assert best - path <= TOL * abs(best), (b, best, path)
        assert abs(sc - path) <= TOL * abs(sc), (b, sc, path)
        assert sc <= -got["cost"][b] + TOL * abs(got["cost"][b])


# ----------------------------------------------------------------------------- all-equal logits: the tie rule, exactly
@pytest.mark.parametrize("placement", [0, 1], ids=["lds_by_shape", "global_forced"], indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_all_equal_logits_tie_goes_to_blank(dtype, placement):
    al, ll = [70, 70, 9, 66, 5, 130], [65, 64, 4, 0, 5, 129]
    B, T, U, V = len(al), 130, 129, 8
    x = torch.zeros(B, T, U + 1, V, dtype=dtype, device="cuda")
    got = run_hip(x, np.ones((B, U), dtype=np.int32), al, ll, stats=False)
    for b in range(B):
        assert np.array_equal(got["frames"][b, :ll[b]], np.arange(ll[b])), (b, got["frames"][b, :ll[b]])
        assert (got["frames"][b, ll[b]:] == -1).all()
        assert abs(got["score"][b] + al[b] * np.log(V)) <= TOL * al[b] * np.log(V)


# ----------------------------------------------------------------------------- emission statistics
def check_stats(got, seen, labels, al, ll):
    B = len(al)
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        mass, expected = got["mass"][b], got["expected"][b]
        if Ub > Tb:
            assert (mass == 0).all() and (expected == -1).all(), b               # no path: 0 / -1 in every entry
            continue
        assert (mass[Ub:] == 0).all() and (expected[Ub:] == -1).all(), b
        if Ub:
            lpb, lpl = A.tables(seen[b], labels[b], Tb, Ub)
            want_e, want_m = A.emit_stats_ref(lpb, lpl)
            em, ee = np.abs(mass[:Ub] - 1.0).max(), np.abs(expected[:Ub] - want_e).max()
            print("utt %d (T_b %d, U_b %d): |mass - 1| max %.2e, |expected - ref| max %.2e frames" % (b, Tb, Ub, em, ee))
            assert np.abs(want_m - 1.0).max() < 1e-9
            assert em <= TOL and ee <= TOL * Tb, (b, em, ee)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("U1", U1S[1:])
def test_emission_statistics(U1, dtype):
    T, al, ll = seam_lengths(U1)
    logits, labels, al, ll, _ = A.planted_batch(500 + U1, T, U1 - 1, al, ll)
    logits = (logits * 0.5).astype(np.float32)               # softer than the planted +8, so that the posteriors are spread over several frames
    x, seen = _dev(logits, dtype)
    got = run_hip(x, labels, al, ll)
    check_stats(got, seen, labels, al, ll)


def test_emission_statistics_c5_lattice():
    """C5's lattice size once: B 8, T 2000, U 200 (a small vocabulary keeps the logits at 100 MB; the lattice is the same)"""
    seed, B, T, U, V = 41, 8, 2000, 200, 8
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, U + 1, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U)).astype(np.int32)
    al = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(0, U + 1, size=B).astype(np.int32)
    al[0], ll[0] = T, U
    x, seen = _dev(logits, torch.float32)
    got = run_hip(x, labels, al, ll)
    check_stats(got, seen, labels, al, ll)
    for b in range(B):                                       # and the alignment at that size: optimal and strictly increasing
        Tb, Ub = int(al[b]), int(ll[b])
        lpb, lpl = A.tables(seen[b], labels[b], Tb, Ub)
        f = got["frames"][b, :Ub]
        assert all(f[i] < f[i + 1] for i in range(Ub - 1))
        best, path = A.viterbi_ref(lpb, lpl)[1], A.path_score(lpb, lpl, f)
        assert best - path <= TOL * abs(best) and abs(got["score"][b] - path) <= TOL * abs(path)


# ----------------------------------------------------------------------------- the cost, the read-only workspace, determinism
def test_cost_bits_backward_bits_and_two_runs():
    from ttmi import ops
    from warprnnt_pytorch import RNNTLoss, rnnt_align
    T, al, ll = seam_lengths(66)
    logits, labels, al, ll, planted = A.planted_batch(77, T, 65, al, ll)
    logits = (logits * 0.5).astype(np.float32)
    B = len(al)
    for dtype in (torch.float32, torch.bfloat16):
        x, _ = _dev(logits, dtype)
        a, b = run_hip(x, labels, al, ll), run_hip(x, labels, al, ll)
        for k in ("cost", "score", "expected", "mass"):
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k      # two runs, the same bits
        assert np.array_equal(a["frames"], b["frames"])
        y, tl, ul = a["y"], a["tl"], a["ul"]
        want = RNNTLoss(reduction="none", topology="monotonic", check_lengths=False)(x, y, tl, ul).detach().cpu().numpy()
        assert np.array_equal(a["cost"].view(np.int32), want.view(np.int32))
        res = rnnt_align(x, y, tl, ul, check_lengths=False, stats=True, topology="monotonic")
        assert np.array_equal(res.cost.cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(res.frames.cpu().numpy(), a["frames"]) and res.frames.dtype is torch.int32
        for k, v in (("score", res.score), ("expected", res.expected_frames), ("mass", res.mass)):
            assert np.array_equal(v.cpu().numpy().view(np.int32), a[k].view(np.int32)), k
        with pytest.raises(ValueError, match="more labels than frames"):
            rnnt_align(x, y, tl, ul, check_lengths=True, topology="monotonic")
        # a backward issued after align + emit_stats: the bits of one issued straight after the forward
        go = torch.linspace(0.5, 2.0, B, device="cuda")
        ws = ops.mono_workspace(B, T, 66, "cuda")
        ws.fill_(0.0)
        ops.mono_loss_fwd(x, y, tl, ul, 0, ws)
        g0 = ops.mono_loss_bwd(x, y, tl, ul, 0, ws, go, 1, 0.5)
        g1 = ops.mono_loss_bwd(x, y, tl, ul, 0, a["ws"], go, 1, 0.5)
        torch.cuda.synchronize()
        assert torch.equal(g0.view(torch.int16 if dtype is torch.bfloat16 else torch.int32),
                           g1.view(torch.int16 if dtype is torch.bfloat16 else torch.int32))


def test_no_backtrace_option_leaves_the_label_frames_alone():
    """ttmi_set_option(23, 2), the measurement switch: the forward walk alone - score as always, frames of real labels not written"""
    from ttmi import ops
    logits, labels, al, ll, _ = A.planted_batch(5, 20, 6, [20, 11], [6, 3])
    x, _ = _dev(logits, torch.float32)
    full = run_hip(x, labels, al, ll, stats=False)
    ops.set_option(23, 2)
    try:
        walk = run_hip(x, labels, al, ll, stats=False)
    finally:
        ops.set_option(23, 0)
    assert np.array_equal(walk["score"].view(np.int32), full["score"].view(np.int32))
    assert (walk["frames"][0] == FR_FILL).all() and (walk["frames"][1, :3] == FR_FILL).all() and (walk["frames"][1, 3:] == -1).all()


# ----------------------------------------------------------------------------- graph capture
def _hip_runtime():
    """the HIP runtime this process already holds (torch's), for the graph queries torch does not wrap"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


def _node_types(raw):
    """-> the hipGraphNodeType of every node of a captured hipGraph_t (0 = kernel, 1 = memcpy, 2 = memset)"""
    hip = _hip_runtime()
    g = ctypes.c_void_p(int(raw))
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kinds = []
    for i in range(n.value):
        k = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(k)) == 0
        kinds.append(k.value)
    return kinds


def test_graph_capture():
    from ttmi import ops
    T, al, ll = seam_lengths(65)
    B, U1 = len(al), 65
    la, labels, al, ll, _ = A.planted_batch(61, T, 64, al, ll)
    lb = (A.planted_batch(62, T, 64, al, ll)[0] * 0.5).astype(np.float32)
    y, tl, ul = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (labels, al, ll))
    static = torch.tensor(la, device="cuda")
    ws = ops.mono_workspace(B, T, U1, "cuda")
    ws.fill_(0.0)

    def run(x, w):
        cost = ops.mono_loss_fwd(x, y, tl, ul, 0, w)
        frames, score = ops.mono_align(w, tl, ul, B, T, U1)
        expected, mass = ops.mono_emit_stats(w, tl, ul, B, T, U1)
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
    eager = run(torch.tensor(lb, device="cuda"), ops.mono_workspace(B, T, U1, "cuda"))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    healthy = [b for b in range(B) if 0 < ll[b] <= al[b]]
    assert all(bool((outs[1][b, :ll[b]] >= 0).all()) and abs(float(outs[4][b, 0]) - 1.0) < TOL for b in healthy)
    # four kernel nodes (log-sum-exp, lattice, Viterbi, statistics) and nothing else: no memset node.  A second capture that keeps its
    # hipGraph_t is looked at and never replayed.
    kept = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(kept):
        run(static, ws)
    kinds = _node_types(kept.raw_cuda_graph())
    print("captured node types", kinds)
    assert kinds == [0, 0, 0, 0]
    del kept
