"""The CTC hypothesis scorer (ttmi_ctc_score_hyps) driven through ttmi.ops on the GPU against the float64 reference of tests/ctc_score_oracle.py
evaluated on the f32 logits the kernels saw, and against the loss it restates: float32(-score) must be ttmi_ctc_loss_fwd's cost of the same
pair on the gathered [P, T, V] batch, bit for bit.

TOL is the 1e-4 (relative) of tests/test_ctc_gpu.py.  The logits sit on a padded row pitch behind a base pointer that is 4 bytes off a 16-byte
boundary: every row walk has a scalar head, then vectors (V 37, 260) and a scalar tail.  The gathered batch of the loss gets the same
placement, because the order in which a row's log-sum-exp is added up - and with it the last bit - depends on where the row's first 16-byte
boundary falls (expand_route).  Workspace and score are followed by guard words."""
import numpy as np
import pytest
import torch

import ctc_score_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64
F_FILL, D_FILL, PAD_TOKEN = 12345.0, -4321.0, 1 << 40


def pitch_of(V, odd=False):
    """a padded row pitch: a multiple of four elements, so that every row starts 4 bytes past a 16-byte boundary like the base pointer (the
    placement the comparison with the loss needs, see run_hip) - or, odd, V + 3: the rows' phases then differ from row to row"""
    return V + 3 if odd else (V + 3) // 4 * 4 + 4


def place_logits(x, ld):
    """[B, T, V], host array or device tensor -> a device view with row pitch ld whose first element is 4 bytes past a 16-byte boundary; the
    pad columns hold garbage"""
    B, T, V = x.shape
    flat = torch.full((B * T * ld + 5,), 7.0, dtype=torch.float32, device="cuda")
    off = 1 + (-(flat.data_ptr() // 4) % 4)
    buf = flat[off:off + B * T * ld].view(B, T, ld)
    assert buf.data_ptr() % 16 == 4
    buf[..., :V] = x if torch.is_tensor(x) else torch.tensor(x)
    return buf[..., :V]


def hyp_arrays(hyps, U, lens=None):
    """P token lists -> (int64 [P, U] view of a [P, U + 3] buffer whose unused entries hold a token far outside the vocabulary, int32 [P])"""
    P = len(hyps)
    buf = torch.full((P, U + 3), PAD_TOKEN, dtype=torch.int64)
    for p, h in enumerate(hyps):
        assert len(h) <= U
        if h:
            buf[p, :len(h)] = torch.tensor(h, dtype=torch.int64)
    n = torch.tensor([len(h) for h in hyps] if lens is None else lens, dtype=torch.int32)
    return buf.cuda()[:, :U], n.cuda()


def expand_route(logits, act, hyps, utt, U, blank):
    """what the loss gives for the same pairs: logits and labels gathered into a [P, T, V] / [P, U] batch -> costs f32 [P].  The copy has the
    pitch and the base phase of the original, so each of its rows has the 16-byte phase of the row it copies and the row walk splits it into
    the same head, vectors and tail: the log-sum-exp's order of additions, hence its last bit, depends on that split"""
    from ttmi import ops
    idx = torch.tensor(utt, dtype=torch.long, device="cuda")
    big = place_logits(logits[idx], logits.stride(1))
    lab = torch.zeros(len(hyps), U, dtype=torch.int32)
    for p, h in enumerate(hyps):
        if h:
            lab[p, :len(h)] = torch.tensor(h, dtype=torch.int32)
    tl = torch.tensor([act[b] for b in utt], dtype=torch.int32, device="cuda")
    ul = torch.tensor([len(h) for h in hyps], dtype=torch.int32, device="cuda")
    P, T, _ = big.shape
    ws = ops.ctc_workspace(P, T, U, "cuda")
    return ops.ctc_loss_fwd(big, lab.cuda(), tl, ul, blank, ws).cpu().numpy()


def run_hip(x, act, hyps, U, utt=None, blank=0, odd_pitch=False):
    """-> score f64 [P] (host).  Checks on the way: the guards behind workspace and score, a second run's bits and - unless the pitch is odd,
    see expand_route - the loss's bits"""
    import ctypes
    import ttmi
    from ttmi import ops
    B, T, V = x.shape
    P = len(hyps)
    logits = place_logits(np.asarray(x, dtype=np.float32), pitch_of(V, odd_pitch))
    tl = torch.tensor(act, dtype=torch.int32, device="cuda")
    hyp, hl = hyp_arrays(hyps, U)
    ut = None if utt is None else torch.tensor(utt, dtype=torch.int32, device="cuda")
    f = ttmi.lib().ttmi_ctc_score_ws_bytes
    f.restype = ctypes.c_size_t
    nw = f(B, T) // 4
    assert nw >= B * T
    ws = torch.full((nw + GUARD,), F_FILL, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        sc = torch.full((P + GUARD,), D_FILL, dtype=torch.float64, device="cuda")
        ttmi.check(ttmi.lib().ttmi_ctc_score_hyps(
            ctypes.c_void_p(logits.data_ptr()), ctypes.c_long(logits.stride(1)), ctypes.c_void_p(tl.data_ptr()), B, T, V, blank,
            ctypes.c_void_p(hyp.data_ptr()), ctypes.c_long(hyp.stride(0)), ctypes.c_void_p(hl.data_ptr()),
            ctypes.c_void_p(0 if ut is None else ut.data_ptr()), P, U, ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(sc.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ttmi_ctc_score_hyps")
        torch.cuda.synchronize()
        assert bool((ws[nw:] == F_FILL).all()), "guard behind the workspace"
        assert bool((sc[P:] == D_FILL).all()), "guard behind score"
        runs.append(sc[:P].cpu().numpy())
    assert np.array_equal(runs[0].view(np.int64), runs[1].view(np.int64)), "two runs, the same bits"
    got = runs[0]
    via_ops = ops.ctc_score_hyps(logits, tl, hyp, hl, ut, blank).cpu().numpy()
    assert np.array_equal(via_ops.view(np.int64), got.view(np.int64)), "ttmi.ops gives what the raw entry gave"
    if not odd_pitch:
        costs = expand_route(logits, act, hyps, [p // (P // B) for p in range(P)] if utt is None else [min(max(u, 0), B - 1) for u in utt], U, blank)
        mine = (-got).astype(np.float32)
        nan = np.isnan(costs)
        assert np.array_equal(nan, np.isnan(mine)), (costs, mine)
        assert np.array_equal(costs[~nan].view(np.int32), mine[~nan].view(np.int32)), (costs, mine)
    return got


def compare(got, want, planted=None):
    """feasible scores within TOL (relative); -inf exactly where the oracle has it, and as many as were planted"""
    assert got.shape == want.shape and got.dtype == np.float64
    dead = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), dead), (got, want)
    if planted is not None:
        assert int(np.isneginf(got).sum()) == int(sum(planted)) and dead.tolist() == [bool(v) for v in planted]
    live = ~dead
    assert np.isfinite(got[live]).all() and np.isfinite(want[live]).all()
    if live.any():
        err = np.abs(got[live] - want[live]) / np.abs(want[live])
        print("%d feasible pairs, %d infeasible: largest relative error %.3e" % (live.sum(), dead.sum(), err.max()))
        assert err.max() <= TOL, (err.max(), got, want)


# ----------------------------------------------------------------------------- the [B, N] layout at every corner
@pytest.mark.parametrize("U", [0, 1, 63, 64, 130])
@pytest.mark.parametrize("T", [1, 2, 8, 9, 10, 17])
def test_beam_layout(T, U):
    """T on both sides of the prefetch depth (8), U + 1 = one wave, the wave edge, three waves; V = the scalar route (5), vectors and a tail
    (37, 260).  Repeats, an empty hypothesis, a token equal to blank and a planted infeasible hypothesis in every utterance that has room"""
    n_dead = 0
    for V in (5, 37, 260):
        c = O.build_case(1000 + 7 * T + U + V, T, U, V)
        got = run_hip(c["x"], c["act_lens"], c["hyps"], U)
        compare(got, O.scores_ref(c["x"], c["act_lens"], c["hyps"]), c["planted"])
        n_dead += sum(c["planted"])
    assert n_dead > 0 or U < 2                                       # a hypothesis of two tokens can always be made infeasible on T_b = 1


# ----------------------------------------------------------------------------- live states across the wave boundary
@pytest.mark.parametrize("T,U,V", [(140, 64, 37), (275, 130, 5)])
def test_long_hypotheses_cross_the_wave_boundary(T, U, V):
    """hypotheses of U tokens: states on both sides of thread 63 | 64 (and 127 | 128) are alive, the boundary cell carries probability"""
    rng = np.random.default_rng(T)
    x = rng.standard_normal((2, T, V)).astype(np.float32)
    act = [T, T - 7]
    hyps = [[int(v) for v in rng.integers(1, V, U)] for _ in range(4)]
    r = min(64, U - 1)                                               # U = 130: label 64 is the first of the second wave
    hyps[1][r - 1], hyps[1][r] = 1, 1                                # a repeat there: no skip into it
    hyps[2][r - 2], hyps[2][r - 1], hyps[2][r] = 1, 2, 0             # a literal blank there
    hyps[3] = hyps[3][:U - 1]
    want = O.scores_ref(x, act, hyps)
    assert np.isfinite(want).all()
    compare(run_hip(x, act, hyps, U), want)


def test_minimal_feasible_and_one_frame_short():
    """[a, a, b] needs four frames: on T_b = 4 exactly one alignment, on T_b = 3 none - in one wave and across the boundary (U = 64)"""
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 5, 6)).astype(np.float32)
    got = run_hip(x, [4, 3], [[2, 2, 3], [2, 2, 3]], 3)
    lp = O.log_softmax(x[0])
    assert abs(got[0] - (lp[0, 2] + lp[1, 0] + lp[2, 2] + lp[3, 3])) <= TOL * abs(got[0]) and np.isneginf(got[1])
    T, U = 70, 64
    x = rng.standard_normal((2, T, 4)).astype(np.float32)
    h = [1 + (i % 3) for i in range(U)]                             # no adjacent repeat: needs U frames
    got = run_hip(x, [U, U - 1], [h, h], U)
    lp = O.log_softmax(x[0])
    assert abs(got[0] - sum(lp[t, h[t]] for t in range(U))) <= TOL * abs(got[0]) and np.isneginf(got[1])


# ----------------------------------------------------------------------------- an explicit utterance table
def test_explicit_utt_permuted():
    """B = 4, P = 9: utterance 1 five times, utterance 3 never, the pairs in no order; entries outside [0, B) are clamped; a token outside
    the vocabulary is clamped to V - 1 and a length above U to U"""
    c = O.build_case(5, 17, 6, 37)
    x, act = c["x"], c["act_lens"]
    rng = np.random.default_rng(6)
    utt = [1, 0, 1, 2, 1, -3, 1, 2, 1]
    hyps = [[int(v) for v in rng.integers(1, 37, int(rng.integers(0, 4)))] for _ in utt]
    hyps[2] = [5, 5, 9]
    want = np.array([O.score_ref(x[min(max(u, 0), 3)], h, act[min(max(u, 0), 3)]) for u, h in zip(utt, hyps)])
    got = run_hip(x, act, hyps, 6, utt=utt)
    compare(got, want)
    assert got[5] == run_hip(x, act, [hyps[5]] * 4, 6)[0]            # utt -3 is utterance 0
    # a pair's score does not depend on its neighbours: the same pairs in reverse order give the same bits
    rev = run_hip(x, act, hyps[::-1], 6, utt=utt[::-1])
    assert np.array_equal(rev[::-1].view(np.int64), got.view(np.int64))
    from ttmi import ops
    logits = place_logits(x, pitch_of(37))
    tl = torch.tensor(act, dtype=torch.int32, device="cuda")
    hyp, _ = hyp_arrays([[3, 99, 4, 36, 1, 2]] * 4, 6)
    a = ops.ctc_score_hyps(logits, tl, hyp, torch.tensor([4, 3, 6, 11], dtype=torch.int32, device="cuda")).cpu().numpy()
    full = [3, 36, 4, 36, 1, 2]
    want = np.array([O.score_ref(x[b], full[:n], act[b]) for b, n in enumerate((4, 3, 6, 6))])
    assert np.isneginf(want[3]) and np.isfinite(want[:3]).all()      # six tokens on utterance 3's five frames
    compare(a, want)


# ----------------------------------------------------------------------------- -inf and NaN logits
def test_neg_inf_column_and_nan_row():
    """utterance 1: column 3 is -inf on every frame - a hypothesis that needs it has no alignment, the others are exact; utterance 2: one NaN
    in frame 1 - its pairs are NaN; the pairs of utterances 0 and 3 have the bits they have without either"""
    rng = np.random.default_rng(12)
    B, T, V, U = 4, 12, 37, 4
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    act = [12, 11, 12, 9]
    hyps = [[4, 5], [6, 6, 1], [], [7]] * B
    hyps[4 + 1] = [6, 3, 1]                                          # needs column 3 of utterance 1
    clean = run_hip(x, act, hyps, U)
    y = x.copy()
    y[1, :, 3] = -np.inf
    y[2, 1, 20] = np.nan
    got = run_hip(y, act, hyps, U)
    want = O.scores_ref(y, act, hyps)
    assert np.isnan(got[8:12]).all() and np.isnan(want[8:12]).all()
    ok = [0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    compare(got[ok], want[ok], planted=[p == 5 for p in ok])
    same = [0, 1, 2, 3, 12, 13, 14, 15]
    assert np.array_equal(got[same].view(np.int64), clean[same].view(np.int64))


def test_another_blank():
    c = O.build_case(31, 10, 4, 5, blank=3)
    got = run_hip(c["x"], c["act_lens"], c["hyps"], 4, blank=3)
    odd = run_hip(c["x"], c["act_lens"], c["hyps"], 4, blank=3, odd_pitch=True)          # every row at another 16-byte phase
    compare(odd, O.scores_ref(c["x"], c["act_lens"], c["hyps"], blank=3), c["planted"])
    compare(got, O.scores_ref(c["x"], c["act_lens"], c["hyps"], blank=3), c["planted"])


# ----------------------------------------------------------------------------- public wrapper, graph capture
def test_public_wrapper_and_the_loss():
    """ttmi.ctc.ctc_score on nested lists (an utterance without hypotheses) = the oracle = -ctc_loss(reduction='none') of the same tokens"""
    from ttmi.ctc import ctc_loss, ctc_score
    rng = np.random.default_rng(14)
    x = rng.standard_normal((3, 20, 11)).astype(np.float32)
    nested = [[[1, 2, 2], []], [], [[4], [5, 6, 7, 8], [9, 9]]]
    act = [20, 20, 13]
    xs = torch.tensor(x, device="cuda")
    got = ctc_score(xs, nested, torch.tensor(act))
    assert got.dtype is torch.float64 and got.is_cuda and got.shape == (5,)
    flat = [(b, h) for b in range(3) for h in nested[b]]
    want = np.array([O.score_ref(x[b], h, act[b]) for b, h in flat])
    compare(got.cpu().numpy(), want)
    lab = torch.zeros(5, 4, dtype=torch.int32)
    for p, (_, h) in enumerate(flat):
        lab[p, :len(h)] = torch.tensor(h, dtype=torch.int32)
    idx = torch.tensor([b for b, _ in flat], device="cuda")
    costs = ctc_loss(xs[idx], lab, torch.tensor([act[b] for b, _ in flat]), torch.tensor([len(h) for _, h in flat]), reduction="none")
    assert torch.equal((-got).float(), costs)
    assert ctc_score(xs, [[], [], []]).shape == (0,)
    full = ctc_score(xs, nested)                                     # act_lens=None: every utterance has T frames
    assert torch.equal(full[:2], got[:2]) and not torch.equal(full[2:], got[2:])


def test_graph_capture():
    from ttmi import ops
    c = O.build_case(41, 17, 64, 37)
    rng = np.random.default_rng(42)
    xb = rng.standard_normal(c["x"].shape).astype(np.float32)
    static = place_logits(c["x"], pitch_of(37))
    tl = torch.tensor(c["act_lens"], dtype=torch.int32, device="cuda")
    hyp, hl = hyp_arrays(c["hyps"], 64)
    ws = ops.ctc_score_workspace(4, 17, "cuda")

    def run(x, w):
        return ops.ctc_score_hyps(x, tl, hyp, hl, None, 0, workspace=w)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static, ws)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static, ws)
    static.copy_(torch.tensor(xb, device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    eager = run(place_logits(xb, pitch_of(37)), ops.ctc_score_workspace(4, 17, "cuda"))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), eager.view(torch.int64))
    compare(out.cpu().numpy(), O.scores_ref(xb, c["act_lens"], c["hyps"]), c["planted"])
