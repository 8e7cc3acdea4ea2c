"""Forced alignment (ttmi_ctc_align) and emission statistics (ttmi_ctc_emit_stats) on the CTC lattice, driven raw on the GPU against the float64
reference of tests/ctc_align_oracle.py evaluated on the f32 logits the kernels saw.

TOL is the 1e-4 of tests/test_ctc_gpu.py: relative on `score`, absolute on |mass - 1|, and on `expected` / `duration` relative with an absolute
floor of one frame's worth (|got - want| <= TOL * max(1, |want|): a duration is at least 1, an expected onset may be 0).  Paths and spans are
compared exactly on planted inputs only - the planted symbol leads every frame by 8 and the oracle asserts a gap above 1.0 to the runner-up
alignment first; on random logits the returned path has to be a valid alignment of the labels whose float64 score is the optimum within TOL,
and `spans` has to agree with `path`."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_align_oracle as A

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64                     # elements behind every output and behind the align workspace that must keep their fill
I_FILL, F_FILL, AWS_FILL = -77, 12345.0, 0x5A5A5A5A5A5A5A5A


@pytest.fixture
def placement(request):
    from ttmi import ops
    ops.set_option(23, request.param)
    yield request.param
    ops.set_option(23, 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_hip(x, labels, al, ll, blank=0, ld=None, stats=True):
    """x: host logits [B, T, V] -> dict of host arrays: cost, path [B, T], spans [B, U, 2], score, expected / mass / duration [B, U] (None
    without stats).  The library is called through its C entry points on buffers of this test's own, each followed by guard elements; the
    loss workspace is compared byte for byte before and after the two calls."""
    import ttmi
    from ttmi import ops
    L = ttmi.lib()
    x = np.asarray(x, dtype=np.float32)
    B, T, V = x.shape
    ld = V if ld is None else ld
    buf = torch.full((B, T, ld), 7.0, dtype=torch.float32, device="cuda")       # pad columns start as garbage
    buf[..., :V] = torch.tensor(x)
    logits = buf[..., :V]
    y = torch.tensor(np.asarray(labels).reshape(B, -1), dtype=torch.int32, device="cuda")
    U = y.shape[1]
    tl, ul = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (al, ll))
    ws = ops.ctc_workspace(B, T, U, "cuda")
    ws.fill_(0.0)                                            # (entries outside the ragged lattice are never written: a fixed fill keeps two runs comparable)
    cost = ops.ctc_loss_fwd(logits, y, tl, ul, blank, ws)
    before = ws.clone()
    f = L.ttmi_ctc_align_workspace_bytes
    f.restype = ctypes.c_size_t
    nw = (f(B, T, U) + 7) // 8
    assert nw > 0
    n = B * U
    aws = torch.full((nw + GUARD,), AWS_FILL, dtype=torch.int64, device="cuda")
    pa = torch.full((B * T + GUARD,), I_FILL, dtype=torch.int32, device="cuda")
    sp = torch.full((2 * n + GUARD,), I_FILL, dtype=torch.int32, device="cuda")
    sc = torch.full((B + GUARD,), F_FILL, dtype=torch.float32, device="cuda")
    ex, ms, du = (torch.full((n + GUARD,), F_FILL, dtype=torch.float32, device="cuda") for _ in range(3))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ttmi.check(L.ttmi_ctc_align(_ptr(ws), _ptr(y), _ptr(tl), _ptr(ul), B, T, U, V, blank, _ptr(aws), _ptr(pa), _ptr(sp), _ptr(sc), st),
               "ttmi_ctc_align")
    if stats:
        ttmi.check(L.ttmi_ctc_emit_stats(_ptr(ws), _ptr(y), _ptr(tl), _ptr(ul), B, T, U, V, blank, _ptr(ex), _ptr(ms), _ptr(du), st),
                   "ttmi_ctc_emit_stats")
    torch.cuda.synchronize()
    assert torch.equal(ws.view(torch.int32), before.view(torch.int32)), "the loss workspace is read only"
    assert bool((aws[nw:] == AWS_FILL).all()), "guard behind the align workspace"
    assert bool((pa[B * T:] == I_FILL).all()) and bool((sp[2 * n:] == I_FILL).all()) and bool((sc[B:] == F_FILL).all()), "guard behind path / spans / score"
    for t in (ex, ms, du):
        assert bool((t[n:] == F_FILL).all()), "guard behind expected / mass / duration"
    out = dict(cost=cost.cpu().numpy(), path=pa[:B * T].view(B, T).cpu().numpy(), spans=sp[:2 * n].view(B, U, 2).cpu().numpy(),
               score=sc[:B].cpu().numpy(), expected=None, mass=None, duration=None, ws=ws, logits=logits, y=y, tl=tl, ul=ul)
    if stats:
        out["expected"], out["mass"], out["duration"] = (t[:n].view(B, U).cpu().numpy() for t in (ex, ms, du))
    return out


def check_infeasible(got, b):
    assert np.isneginf(got["score"][b]) and np.isposinf(got["cost"][b]), (b, got["score"][b], got["cost"][b])
    assert (got["path"][b] == -1).all() and (got["spans"][b] == -1).all(), b
    if got["mass"] is not None:
        assert (got["mass"][b] == 0).all() and (got["expected"][b] == -1).all() and (got["duration"][b] == 0).all(), b


def check_stats(got, b, lp, skip, Tb, Ub):
    mass, expected, duration = got["mass"][b], got["expected"][b], got["duration"][b]
    assert (mass[Ub:] == 0).all() and (expected[Ub:] == -1).all() and (duration[Ub:] == 0).all(), b
    if Ub == 0:
        return
    we, wm, wd, wblank = A.emit_stats_ref(lp, skip)
    assert np.abs(wm - 1.0).max() < 1e-9 and abs(wd.sum() + wblank - Tb) < 1e-9 * Tb
    em = np.abs(mass[:Ub] - 1.0).max()
    ee = (np.abs(expected[:Ub] - we) / np.maximum(1.0, np.abs(we))).max()
    ed = (np.abs(duration[:Ub] - wd) / np.maximum(1.0, np.abs(wd))).max()
    print("utt %d (T_b %d, U_b %d): |mass - 1| max %.2e, expected err %.2e, duration err %.2e" % (b, Tb, Ub, em, ee, ed))
    assert em <= TOL and ee <= TOL and ed <= TOL, (b, em, ee, ed)


def check_common(got, b, Tb, Ub, skip):
    """what holds of every feasible utterance: the path is an alignment of the labels, -1 past T_b, and spans says what the path says"""
    path, spans = got["path"][b], got["spans"][b]
    assert (path[Tb:] == -1).all() and (spans[Ub:] == -1).all(), b
    assert A.valid_path(path[:Tb], skip), (b, path[:Tb])
    assert np.array_equal(spans[:Ub], A.spans_of(path[:Tb], Ub)), (b, spans[:Ub])
    assert all(spans[u, 0] <= spans[u, 1] for u in range(Ub)) and all(spans[u, 1] < spans[u + 1, 0] for u in range(Ub - 1))


def check_random(x, labels, al, ll, blank=0, ld=None):
    got = run_hip(x, labels, al, ll, blank, ld)
    labels = np.asarray(labels).reshape(len(al), -1)
    for b in range(len(al)):
        Tb, Ub = int(al[b]), int(ll[b])
        lp, ext, skip = A.tables(np.asarray(x, dtype=np.float32)[b], labels[b], Tb, Ub, blank)
        want_path, best = A.viterbi_ref(lp, skip)
        if not np.isfinite(best):
            check_infeasible(got, b)
            continue
        check_common(got, b, Tb, Ub, skip)
        mine, sc = A.path_score(lp, got["path"][b, :Tb]), got["score"][b]
        print("utt %d (T_b %d, U_b %d): best %.6f, returned path %.6f (gap %.3e), kernel score %.6f" % (b, Tb, Ub, best, mine, best - mine, sc))
        assert best - mine <= TOL * abs(best), (b, best, mine)
        assert abs(sc - mine) <= TOL * abs(mine), (b, sc, mine)
        assert sc <= -got["cost"][b] + TOL * abs(got["cost"][b])              # one alignment is no more likely than all of them
        check_stats(got, b, lp, skip, Tb, Ub)
    return got


def check_planted(seed, T, U, al, ll, labels=None, stats=True):
    x, labels, al, ll, planted = A.planted_batch(seed, T, U, al, ll, labels=labels)
    got = run_hip(x, labels, al, ll, stats=stats)
    B = len(al)
    assert got["path"].shape == (B, T) and got["spans"].shape == (B, U, 2) and got["path"].dtype == np.int32
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        lp, ext, skip = A.tables(x[b], labels[b], Tb, Ub)
        if (planted[b] == -1).all():
            assert not np.isfinite(A.viterbi_ref(lp, skip)[1])
            check_infeasible(got, b)
            continue
        want, best = A.viterbi_ref(lp, skip)
        assert np.array_equal(want, planted[b, :Tb])
        assert best - A.runner_up(lp, skip, want) > 1.0, b                   # the planted path is the optimum by a margin no f32 table can close
        check_common(got, b, Tb, Ub, skip)
        assert np.array_equal(got["path"][b, :Tb], want), (b, Tb, Ub, got["path"][b, :Tb], want)
        assert abs(got["score"][b] - best) <= TOL * abs(best), (b, got["score"][b], best)
        if stats:
            check_stats(got, b, lp, skip, Tb, Ub)
    return got


# ----------------------------------------------------------------------------- smallest lattices
SMALL = [("T1_U0", 1, []), ("T1_U1", 1, [2]), ("T2_U1", 2, [3]), ("T5_U0", 5, []), ("aa_T3_min_feasible", 3, [2, 2]), ("aa_T2_infeasible", 2, [2, 2])]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_smallest_lattices(case):
    name, T, lab = case
    rng = np.random.default_rng(len(lab) * 10 + T)
    x = rng.standard_normal((1, T, 5)).astype(np.float32)
    got = check_random(x, np.array(lab, dtype=np.int32).reshape(1, -1), [T], [len(lab)])
    if name == "aa_T2_infeasible":
        check_infeasible(got, 0)
    if name == "aa_T3_min_feasible":
        assert got["path"][0].tolist() == [1, 2, 3] and got["spans"][0].tolist() == [[0, 0], [2, 2]]
    if not lab:
        assert (got["path"][0] == 0).all()


# ----------------------------------------------------------------------------- wave edges, planted, both placements
def wave_edge_batch(U):
    """T = U + 3.  Utterance 0: three symbols and two adjacent repeats, feasible from U + 2 frames on; 1: no repeat on exactly U frames (one
    alignment); 2: U - 2 labels on T - 1 frames; 3: no labels; 4: one symbol U times on T frames - needs 2 U - 1, infeasible"""
    T = U + 3
    labels = np.zeros((5, U), dtype=np.int32)
    labels[0] = 1 + (np.arange(U) % 3)
    labels[0, 5], labels[0, U - 1] = labels[0, 4], labels[0, U - 2]
    labels[1] = 1 + (np.arange(U) % 2)
    labels[2] = 1 + (np.arange(U) % 5)
    labels[3] = 3
    labels[4] = 4
    return T, labels, [T, U, T - 1, 5, T], [U, U, U - 2, 0, U]


@pytest.mark.parametrize("placement", [0, 1], ids=["lds_by_shape", "global_forced"], indirect=True)
@pytest.mark.parametrize("U", [63, 64, 127, 128])
def test_wave_edges_planted_exact(U, placement):
    T, labels, al, ll = wave_edge_batch(U)
    got = check_planted(700 + U, T, U, al, ll, labels=labels)
    assert got["path"][1, :U].tolist() == list(range(1, 2 * U, 2))             # the one alignment of U distinct neighbours on U frames


def test_both_placements_give_identical_output():
    from ttmi import ops
    T, labels, al, ll = wave_edge_batch(128)
    x = np.random.default_rng(21).standard_normal((5, T, 8)).astype(np.float32)
    runs = []
    for bits in (0, 1):
        ops.set_option(23, bits)
        try:
            runs.append(run_hip(x, labels, al, ll))
        finally:
            ops.set_option(23, 0)
    for k in ("path", "spans"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    for k in ("score", "expected", "mass", "duration"):
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), k


def test_u1023_decision_words_in_global_memory_by_shape():
    """B 1, T 1030, U 1023: 1030 * 16 * 3 decision words are 395 520 bytes, over the 128 KB kept in LDS; sixteen waves, every wave seam crossed"""
    U = 1023
    labels = (1 + (np.arange(U) % 3)).astype(np.int32).reshape(1, U)
    check_planted(1030, 1030, U, [1030], [U], labels=labels)


def test_decision_words_above_the_default_lds_limit():
    """T 700, U 300: 700 * 5 * 3 words are 84 000 bytes - in LDS, above the 64 KB a kernel gets without asking"""
    U = 300
    labels = np.stack([1 + (np.arange(U) % 4), 1 + (np.arange(U) % 7)]).astype(np.int32)
    check_planted(300, 700, U, [700, 512], [U, 257], labels=labels, stats=False)


# ----------------------------------------------------------------------------- random logits: optimality, not identity
def test_ragged_batch_random_logits():
    """B 4, T 12, U 5, V 7, repeated labels, lengths that include U_b = 0 and T_b = 1, pitch 64 (the batch of tests/test_ctc_gpu.py)"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 12, 7)).astype(np.float32)
    labels = np.array([[1, 1, 2, 2, 1], [3, 4, 3, 3, 6], [5, 5, 5, 1, 1], [2, 6, 6, 1, 3]], dtype=np.int32)
    check_random(x, labels, [12, 9, 1, 7], [5, 3, 0, 2], ld=64)
    check_random(x, labels, [12, 9, 1, 7], [5, 3, 1, 2], ld=64)


def test_workload_lattice_random_logits():
    """T 500, U 50, V 16: the CTC head's lattice on the training workload, ragged, once dense and once on a padded row pitch"""
    rng = np.random.default_rng(2)
    B, T, U, V = 3, 500, 50, 16
    x = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    check_random(x, labels, [T, 431, 77], [U, 37, 50])
    check_random(x, labels, [T, 431, 77], [U, 37, 50], ld=24)


@pytest.mark.parametrize("blank", [0, 3])
def test_label_equal_to_blank(blank):
    """l' is built literally: a label equal to `blank` is one more state that emits the blank symbol (no skip into it, ties by construction -
    so optimality and validity, not identity)"""
    rng = np.random.default_rng(4 + blank)
    B, T, U, V = 3, 20, 6, 9
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(0, V, (B, U)).astype(np.int32)
    labels[0, 2] = labels[1, 0] = labels[1, 1] = labels[2, 5] = blank
    check_random(x, labels, [T, 17, 13], [U, 5, 6], blank=blank)


def test_all_equal_logits_tie_rule():
    """every alignment scores the same: the predecessor order s, s-1, s-2 and the final rule decide alone.  The oracle's path for [1, 2] on five
    frames is worked by hand in tests/test_ctc_align_oracle.py; here 70 labels cross the wave seam"""
    al, ll = [5, 5, 140, 75, 4], [2, 2, 70, 64, 0]
    B, T, U, V = 5, 140, 70, 8
    labels = np.zeros((B, U), dtype=np.int32)
    labels[0, :2], labels[1, :2] = [1, 2], [1, 1]
    labels[2], labels[3] = 1 + (np.arange(U) % 3), 1 + (np.arange(U) % 2)
    got = run_hip(np.zeros((B, T, V), dtype=np.float32), labels, al, ll, stats=False)
    assert got["path"][0, :5].tolist() == [1, 3, 4, 4, 4] and got["path"][1, :5].tolist() == [1, 2, 3, 4, 4]
    for b in range(B):
        lp, _, skip = A.tables(np.zeros((T, V)), labels[b], al[b], ll[b])
        want, score = A.viterbi_ref(lp, skip)
        assert np.array_equal(got["path"][b, :al[b]], want), (b, got["path"][b, :al[b]], want)
        assert np.array_equal(got["spans"][b, :ll[b]], A.spans_of(want, ll[b]))
        assert abs(got["score"][b] - score) <= TOL * abs(score)


# ----------------------------------------------------------------------------- determinism, the read-only workspace, options
def test_two_runs_and_backward_bits():
    from ttmi import ops
    from ttmi.ctc import ctc_align
    T, labels, al, ll = wave_edge_batch(64)
    x = np.random.default_rng(31).standard_normal((5, T, 8)).astype(np.float32)
    a, b = run_hip(x, labels, al, ll), run_hip(x, labels, al, ll)
    for k in ("cost", "score", "expected", "mass", "duration"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k           # two runs, the same bits
    assert np.array_equal(a["path"], b["path"]) and np.array_equal(a["spans"], b["spans"])
    # the public wrapper gives what the raw entries gave
    res = ctc_align(a["logits"], a["y"], a["tl"], a["ul"], stats=True)
    assert res.path.dtype is torch.int32 and np.array_equal(res.path.cpu().numpy(), a["path"]) and np.array_equal(res.spans.cpu().numpy(), a["spans"])
    for k, v in (("score", res.score), ("expected", res.expected), ("mass", res.mass), ("duration", res.duration)):
        assert np.array_equal(v.cpu().numpy().view(np.int32), a[k].view(np.int32)), k
    plain = ctc_align(a["logits"], a["y"], a["tl"], a["ul"])
    assert plain.expected is None and plain.mass is None and plain.duration is None and torch.equal(plain.path, res.path)
    # a backward issued after align + emit_stats: the bits of one issued straight after the forward
    B = len(al)
    go = torch.linspace(0.5, 2.0, B, device="cuda")
    ws = ops.ctc_workspace(B, T, 64, "cuda")
    ws.fill_(0.0)
    ops.ctc_loss_fwd(a["logits"], a["y"], a["tl"], a["ul"], 0, ws)
    g0 = ops.ctc_loss_bwd(a["logits"], a["y"], a["tl"], a["ul"], 0, ws, go, 1, 0.5)
    g1 = ops.ctc_loss_bwd(a["logits"], a["y"], a["tl"], a["ul"], 0, a["ws"], go, 1, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))


def test_no_backtrace_option_leaves_the_path_alone():
    """ttmi_set_option(23, 2), the measurement switch: the forward walk alone - score as always, frames and labels the utterance has not written"""
    from ttmi import ops
    x, labels, al, ll, _ = A.planted_batch(5, 20, 6, [20, 11], [6, 3])
    full = run_hip(x, labels, al, ll, stats=False)
    ops.set_option(23, 2)
    try:
        walk = run_hip(x, labels, al, ll, stats=False)
    finally:
        ops.set_option(23, 0)
    assert np.array_equal(walk["score"].view(np.int32), full["score"].view(np.int32))
    assert (walk["path"][0] == I_FILL).all() and (walk["path"][1, :11] == I_FILL).all() and (walk["path"][1, 11:] == -1).all()
    assert (walk["spans"][0] == I_FILL).all() and (walk["spans"][1, :3] == I_FILL).all() and (walk["spans"][1, 3:] == -1).all()


# ----------------------------------------------------------------------------- graph capture
def test_graph_capture():
    from ttmi import ops
    T, labels, al, ll = wave_edge_batch(64)
    B, U, V = 5, 64, 8
    rng = np.random.default_rng(41)
    xa, xb = (rng.standard_normal((B, T, V)).astype(np.float32) for _ in range(2))
    y, tl, ul = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (labels, al, ll))
    static = torch.tensor(xa, device="cuda")
    ws = ops.ctc_workspace(B, T, U, "cuda")
    ws.fill_(0.0)
    aws = ops.ctc_align_workspace(B, T, U, "cuda")

    def run(x, w, scratch):
        cost = ops.ctc_loss_fwd(x, y, tl, ul, 0, w)
        path, spans, score = ops.ctc_align(w, y, tl, ul, B, T, V, 0, align_workspace=scratch)
        expected, mass, duration = ops.ctc_emit_stats(w, y, tl, ul, B, T, V, 0)
        return cost, path, spans, score, expected, mass, duration

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static, ws, aws)                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static, ws, aws)
    static.copy_(torch.tensor(xb, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    ws2 = ops.ctc_workspace(B, T, U, "cuda")
    ws2.fill_(0.0)
    eager = run(torch.tensor(xb, device="cuda"), ws2, ops.ctc_align_workspace(B, T, U, "cuda"))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool((outs[1][0, :T] >= 0).all()) and abs(float(outs[5][0, 0]) - 1.0) < TOL and bool(torch.isneginf(outs[3][4]))
