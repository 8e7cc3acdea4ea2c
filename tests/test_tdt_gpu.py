"""The token-and-duration transducer kernels (csrc/tdt.hip) driven raw through ttmi.ops against the float64 reference of tests/tdt_oracle.py.

Tolerance: the project's 1e-4 (tests/test_mono_gpu.py) on costs, relative to the cost, and on gradients per utterance - conftest.rel_err of the
utterance's gradient, and for f32 logits also the largest deviation of any element relative to the utterance's largest gradient element.
bf16 logits: the oracle is evaluated on the bf16-rounded values widened to float64, and its gradient is rounded to bf16 before the comparison
(the kernel's last step); the bound stays 1e-4.  Utterances without a path are not compared with the oracle: cost +inf and all-zero rows are
asserted.  The shapes are the smallest at which each mechanism of the kernels can go wrong; every test prints its figures before it asserts."""
import itertools

import numpy as np
import pytest
import torch

import tdt_oracle as O
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64                     # elements behind the gradient buffer / floats behind the workspace that must keep their fill
FILL, WS_FILL = 7.0, 12345.0
GO, SCALE = np.array([0.5, -2.0, 3.0]), 0.25


def ws_floats_used(B, T, U1, D):
    """the bytes the documented layout occupies (alpha, beta [B, T+1, U1] f64, ll [B] f64, 4 + D tables [B, T, U1] f32), in floats"""
    return (8 * (2 * B * (T + 1) * U1 + B) + 4 * (4 + D) * B * T * U1) // 4


def run_hip(xt, labels, tl, ul, durations, blank=0, ld=None, go=None, scale=1.0, inplace=False, backward=True):
    """xt: torch f32 / bf16 [B, T, U1, V + D] on the host.  The logits live in a pitch-ld buffer whose pad columns start as garbage; in place the
    buffer is followed by guard elements.  The workspace is followed by guard floats.  -> (costs [B], full gradient buffer [B, T, U1, ld] f64)"""
    from ttmi import ops
    B, T, U1, W = xt.shape
    D = len(durations)
    ld = W if ld is None else ld
    n = B * T * U1 * ld
    flat = torch.full((n + GUARD,), FILL, dtype=xt.dtype, device="cuda")
    buf = flat[:n].view(B, T, U1, ld)
    buf[..., :W] = xt.cuda()
    logits = buf[..., :W]
    y = torch.tensor(np.asarray(labels).reshape(B, -1), dtype=torch.int32, device="cuda")
    tlg, ulg = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (tl, ul))
    nws = ops.tdt_workspace(B, T, U1, D, "cuda").numel()
    used = ws_floats_used(B, T, U1, D)
    assert used <= nws
    wsg = torch.full((nws + GUARD,), WS_FILL, dtype=torch.float32, device="cuda")
    ws = wsg[:nws]
    costs = ops.tdt_loss_fwd(logits, y, tlg, ulg, blank, durations, ws)
    if not backward:
        torch.cuda.synchronize()
        assert bool((wsg[used:] == WS_FILL).all()), "guard behind the workspace"
        return costs.cpu().numpy(), None
    g = torch.ones(B, device="cuda") if go is None else torch.tensor(np.asarray(go), dtype=torch.float32, device="cuda")
    grad = ops.tdt_loss_bwd(logits, y, tlg, ulg, blank, durations, ws, g, 1, scale, inplace=inplace)
    torch.cuda.synchronize()
    if inplace:
        assert grad.data_ptr() == logits.data_ptr()
        full = buf
    else:
        assert torch.equal(buf[..., :W].cpu(), xt)                                  # out of place: the logits are untouched
        full = torch.as_strided(grad, (B, T, U1, ld), (T * U1 * ld, U1 * ld, ld, 1))
    assert bool((flat[n:] == FILL).all()), "guard behind the gradient buffer"
    assert bool((wsg[used:] == WS_FILL).all()), "guard behind the workspace"
    return costs.cpu().numpy(), full.double().cpu().numpy()


def compare(costs, full, want_c, want_g, tl, ul, W, V, dtype, gmax, what):
    """the assertions every comparison with a reference shares -> the gradient [B, T, U1, W]"""
    B = len(costs)
    g = full[..., :W]
    dead = np.isposinf(want_c)
    cerr = np.abs(costs[~dead] - want_c[~dead]) / np.abs(want_c[~dead])
    gerr = [rel_err(g[b], want_g[b]) for b in range(B) if not dead[b]]
    eerr = [np.abs(g[b] - want_g[b]).max() / np.abs(want_g[b]).max() for b in range(B) if not dead[b]]
    sums = max(np.abs(g[..., :V].sum(-1)).max(), np.abs(g[..., V:].sum(-1)).max())
    print("%s: cost rel err %.2e, grad rel err %.2e, worst element / largest element %.2e, sub-row sums %.2e of %.2e"
          % (what, max(cerr, default=0.0), max(gerr, default=0.0), max(eerr, default=0.0), sums, gmax))
    assert np.all(np.isposinf(costs[dead])), costs                                  # no path: +inf ...
    for b in np.nonzero(dead)[0]:
        assert np.all(full[b] == 0), b                                              # ... and zero rows, never NaN
    assert np.all(cerr <= TOL), (costs, want_c)
    assert np.isfinite(g).all()
    assert all(e < TOL for e in gerr), gerr
    if dtype is torch.float32:
        assert all(e < TOL for e in eerr), eerr
        # a sub-row is g * (softmax * occ - patches): two sets of f32 terms that each add up to occ <= 1 (tests/test_mono_gpu.py)
        assert sums < 1e-5 * gmax
    for b in range(B):
        Tb, Ub = int(np.clip(tl[b], 1, full.shape[1])), int(np.clip(ul[b], 0, full.shape[2] - 1))
        assert np.all(full[b, Tb:] == 0) and np.all(full[b, :, Ub + 1:] == 0), b    # outside the lattice: exact zeros
    assert np.all(full[..., W:] == 0)                                               # pad columns
    return g


def check(x, labels, tl, ul, durations, blank=0, ld=None, dtype=torch.float32, inplace=False, go=None, scale=1.0):
    """one batch against the oracle -> (costs, gradient [B, T, U1, V + D])"""
    B, T, U1, W = x.shape
    V = W - len(durations)
    xt = torch.tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    want_c, want_g = O.tdt_loss(xt.double().numpy(), labels, tl, ul, durations, blank)
    gov = np.ones(B) if go is None else np.asarray(go, dtype=np.float64)
    want_g = want_g * (np.float32(scale) * gov.astype(np.float32)).astype(np.float64)[:, None, None, None]
    if dtype is torch.bfloat16:
        want_g = torch.tensor(want_g).to(torch.bfloat16).double().numpy()
    costs, full = run_hip(xt, labels, tl, ul, durations, blank, ld, go, scale, inplace)
    what = "B %d T %d U1 %d V %d durations %s ld %s %s blank %d inplace %d" % (B, T, U1, V, durations, ld, str(dtype)[6:], blank, inplace)
    g = compare(costs, full, want_c, want_g, tl, ul, W, V, dtype, np.abs(np.float32(scale) * gov).max(), what)
    return costs, g, want_c


def case(seed, B, T, U1, V, D, scale=1.5):
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((B, T, U1, V + D))).astype(np.float32)
    labels = rng.integers(0, V, (B, max(U1 - 1, 1))).astype(np.int32)               # the whole vocabulary: some labels equal `blank`
    return x, labels


# ----------------------------------------------------------------------------- the loss
def test_ragged_batch_every_option():
    """B 3, ragged lengths, T 12, U1 5, V 7, durations (1, 2, 4): dtype x pitch x blank x aliasing"""
    x, labels = case(1, 3, 12, 5, 7, 3)
    for dtype, pad, blank, inplace in itertools.product((torch.float32, torch.bfloat16), (0, 3), (0, 6), (False, True)):
        check(x, labels, [12, 10, 7], [4, 3, 0], (1, 2, 4), blank, 10 + pad, dtype, inplace, go=GO, scale=SCALE)


def test_no_labels_and_one_frame():
    x, labels = case(2, 3, 6, 1, 5, 2)
    check(x, labels, [6, 4, 1], [0, 0, 0], (1, 2), go=GO, scale=SCALE)                # U1 = 1: the label pointer is not read
    x, labels = case(3, 2, 1, 2, 5, 2)
    costs, _, want = check(x, labels, [1, 1], [1, 0], (1, 2))                         # T = 1: one decision of duration 1
    lt, ld = O.split_rows(x, 5, 2)
    assert abs(costs[0] + lt[0, 0, 0, labels[0, 0]] + ld[0, 0, 0, 0]) <= TOL * costs[0]
    assert abs(costs[1] + lt[1, 0, 0, 0] + ld[1, 0, 0, 0]) <= TOL * costs[1]


def test_duration_longer_than_the_utterance():
    x, labels = case(4, 3, 2, 3, 4, 2)
    check(x, labels, [2, 2, 1], [1, 2, 0], (1, 4), go=GO, scale=SCALE)


def test_one_long_duration():
    """durations (8,), T 16: T_b = 16 has the paths of two decisions, T_b = 8 of one, T_b = 12 none"""
    x, labels = case(5, 3, 16, 3, 5, 1)
    costs, _, _ = check(x, labels, [16, 8, 12], [2, 1, 0], (8,), go=GO, scale=SCALE)
    assert np.isposinf(costs[2])


def test_all_eight_durations():
    x, labels = case(6, 3, 19, 4, 6, 8)
    for dtype in (torch.float32, torch.bfloat16):
        check(x, labels, [19, 11, 8], [3, 2, 3], tuple(range(1, 9)), blank=5, ld=17, dtype=dtype, inplace=True, go=GO, scale=SCALE)


@pytest.mark.parametrize("U1", [64, 65, 66, 130])
def test_slot_seams(U1):
    """T 70, durations (1, 3): live cells cross labels 63 | 64 (lane 63 of slot 0 to lane 0 of slot 1).  The first utterance has as many
    labels as the frames allow (U_b = U1 - 1 up to U1 = 66, U_b = T at U1 = 130, whose live cells end at label 70); at U1 = 130 the
    second utterance has U_b = U1 - 1 = 129 on 69 frames: no path, cost +inf and zero rows between live neighbours.  The seam 127 | 128
    with live cells and gradients is test_second_slot_seam_with_gradients."""
    x, labels = case(U1, 3, 70, U1, 3, 2)
    top = min(U1 - 1, 70)
    second = U1 - 1 if U1 - 1 > 69 else min(U1 - 1, 66)
    costs, _, _ = check(x, labels, [70, 69, 67], [top, second, 0], (1, 3), blank=2, ld=8, inplace=True, go=GO, scale=SCALE)
    assert np.isposinf(costs[1]) == (U1 == 130)


def test_second_slot_seam_with_gradients():
    """U1 131, T 134, durations (1, 3): U_b = U1 - 1 = 130 and U_b = 129 - alpha, beta and the gradient with live cells on both sides of
    labels 127 | 128 (lane 63 of slot 1 to lane 0 of slot 2, three slots per lane in the four-slot instance); a third utterance without
    labels"""
    x, labels = case(131, 3, 134, 131, 3, 2)
    costs, g, _ = check(x, labels, [134, 133, 70], [130, 129, 0], (1, 3), blank=2, ld=8, inplace=True, go=GO, scale=SCALE)
    assert np.isfinite(costs).all() and np.abs(g[0, :, 126:130]).max() > 0 and np.abs(g[1, :, 126:130]).max() > 0


def test_longest_label_axis_cost_only():
    """U1 1024, T 1026, durations (1, 2): sixteen slots per lane and the whole 64 KB ring; the cost against the numpy alpha recursion
    vectorised over u (no Python loop over the cells)"""
    x, labels = case(7, 1, 1026, 1024, 2, 2)
    costs, _ = run_hip(torch.tensor(x), labels, [1026], [1023], (1, 2), blank=1, backward=False)
    want = O.tdt_cost_vectorised(x[0], labels[0], 1026, 1023, (1, 2), blank=1)
    print("U1 1024: cost %.6f, reference %.6f, rel err %.2e" % (costs[0], want, abs(costs[0] - want) / want))
    assert np.isfinite(want) and abs(costs[0] - want) <= TOL * want


@pytest.mark.parametrize("V,D", [(67, 3), (131, 2), (4334, 4)])
def test_row_walks(V, D):
    """V + D no multiple of the vector width, every pitch and dtype: the 16-byte walk's head, body and tail at each row alignment; V 4334 is
    the wide-row walk (B 1, T 4, U1 3)"""
    wide = V > 1000
    x, labels = case(V, 1 if wide else 2, 4, 3, V, D)
    tl, ul = ([4], [2]) if wide else ([4, 3], [2, 1])
    W = V + D
    for ld, dtype, inplace in itertools.product((W, W + 3, (W + 63) // 64 * 64), (torch.float32, torch.bfloat16), (False, True)):
        check(x, labels, tl, ul, tuple(range(1, D + 1)), V - 1, ld, dtype, inplace, go=GO[:len(tl)], scale=SCALE)


def test_no_path_between_live_neighbours():
    """U_b > T_b, and durations (2,) with an odd T_b: +inf, zero rows, no NaN; the neighbours within TOL (check compares them)"""
    x, labels = case(8, 3, 6, 5, 5, 2)
    costs, _, _ = check(x, labels, [6, 3, 5], [2, 4, 1], (1, 2), go=GO, scale=SCALE)
    assert np.isposinf(costs[1]) and np.isfinite(costs[[0, 2]]).all()
    x, labels = case(9, 3, 6, 3, 5, 1)
    for dtype in (torch.float32, torch.bfloat16):
        costs, _, _ = check(x, labels, [6, 5, 4], [2, 1, 0], (2,), dtype=dtype, inplace=True, go=GO, scale=SCALE)
        assert np.isposinf(costs[1]) and np.isfinite(costs[[0, 2]]).all()


def test_duration_one_is_the_monotonic_loss():
    """durations (1,): cost and token gradients against ttmi_mono_loss_fwd / _bwd on logits[..., :V]; the duration column is zero"""
    from ttmi import ops
    B, T, U1, V = 3, 9, 5, 11
    x, labels = case(10, B, T, U1, V, 1)
    tl, ul = [9, 7, 4], [4, 2, 0]
    costs, full = run_hip(torch.tensor(x), labels, tl, ul, (1,), go=GO, scale=SCALE)
    xm = torch.tensor(x[..., :V]).cuda().contiguous()
    y = torch.tensor(labels, device="cuda")
    tlg, ulg = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in (tl, ul))
    ws = ops.mono_workspace(B, T, U1, "cuda")
    mc = ops.mono_loss_fwd(xm, y, tlg, ulg, 0, ws).cpu().numpy()
    mg = ops.mono_loss_bwd(xm, y, tlg, ulg, 0, ws, torch.tensor(GO, dtype=torch.float32, device="cuda"), 1, SCALE).double().cpu().numpy()
    gmax = max(np.abs(mg[b]).max() for b in range(B))
    print("cost rel err %.2e, token grad %.2e, duration column %.2e of %.2e"
          % (np.abs(costs / mc - 1).max(), max(np.abs(full[b, ..., :V] - mg[b]).max() / np.abs(mg[b]).max() for b in range(B)),
             np.abs(full[..., V]).max(), gmax))
    assert np.all(np.abs(costs - mc) <= TOL * np.abs(mc))
    for b in range(B):
        assert np.abs(full[b, ..., :V] - mg[b]).max() <= TOL * np.abs(mg[b]).max()
    assert np.abs(full[..., V]).max() < 1e-5 * gmax


def test_lengths_and_labels_are_clamped():
    x, labels = case(11, 3, 4, 4, 5, 2)
    xt = torch.tensor(x)
    wild = labels.copy()
    wild[0, 0], wild[1, 1] = -3, 99
    a = run_hip(xt, wild, [9, 0, -2], [7, -1, 3], (1, 2))
    b = run_hip(xt, np.clip(wild, 0, 4), [4, 1, 1], [3, 0, 3], (1, 2))
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


# ----------------------------------------------------------------------------- reproducibility, graph capture
def test_two_runs_give_identical_bits():
    x, labels = case(12, 3, 40, 70, 19, 3)
    for dtype in (torch.float32, torch.bfloat16):
        xt = torch.tensor(x).to(dtype)
        runs = [run_hip(xt, labels, [40, 33, 30], [39, 33, 12], (1, 2, 5), go=GO, scale=SCALE) for _ in range(2)]
        assert np.array_equal(runs[0][0].view(np.int32), runs[1][0].view(np.int32))
        assert np.array_equal(runs[0][1], runs[1][1])


def test_graph_capture_forward_and_backward():
    from ttmi import ops
    rng = np.random.default_rng(14)
    B, T, U1, V, durations = 3, 11, 7, 37, (1, 2, 3)
    xa, xb = (rng.standard_normal((B, T, U1, V + 3)).astype(np.float32) for _ in range(2))
    yh = rng.integers(0, V, (B, U1 - 1)).astype(np.int32)
    y = torch.tensor(yh, device="cuda")
    tl, ul = torch.tensor([11, 9, 4], dtype=torch.int32, device="cuda"), torch.tensor([6, 4, 0], dtype=torch.int32, device="cuda")
    go = torch.tensor([1.0, 2.0, -1.0], device="cuda")

    def run(x, w):
        costs = ops.tdt_loss_fwd(x, y, tl, ul, 0, durations, w)
        return costs, ops.tdt_loss_bwd(x, y, tl, ul, 0, durations, w, go, 1, 0.5)

    static = torch.tensor(xa, device="cuda")
    ws = ops.tdt_workspace(B, T, U1, 3, "cuda")
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
    eager = run(torch.tensor(xb, device="cuda"), ops.tdt_workspace(B, T, U1, 3, "cuda"))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want_c, _ = O.tdt_loss(xb, yh, [11, 9, 4], [6, 4, 0], durations)
    assert rel_err(outs[0].cpu().numpy(), want_c) < TOL


# ----------------------------------------------------------------------------- greedy decoding: scan + advance against the oracle decoder
def _decode(table, T_len, durations, V, n, blank=0):
    """the lockstep of Transducer.decode_batch on synthetic rows: the joint row of utterance b at frame t with c tokens emitted is
    table[b, t, c % 8].  -> per utterance (tokens, frames, logprobs, durations, score), and the number of blocks scanned"""
    from ttmi import ops
    B, T = table.shape[0], table.shape[1]
    D = len(durations)
    dev = "cuda"
    tab = torch.tensor(table, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    hist = torch.zeros(B, T + 2, dtype=torch.long, device=dev)
    t, done, count, flags = i32(B), i32(B), i32(B), i32(2)
    need = torch.ones(B, dtype=torch.int32, device=dev)
    T_len = torch.tensor(T_len, dtype=torch.int32, device=dev)
    frames, tok_dur, tok_lp = i32(B, T + 1), i32(B, T + 1), torch.zeros(B, T + 1, device=dev)
    score = torch.zeros(B, dtype=torch.float64, device=dev)
    dec, lp = i32(B, n, 2), torch.zeros(B, n, 2, device=dev)
    rows = torch.arange(n, device=dev)[None, :]
    bidx = torch.arange(B, device=dev)[:, None]
    n_hist, blocks = 1, 0
    while True:
        torch.sub(1, done, out=need)
        while True:
            idx = (t.long()[:, None] + rows).clamp_(max=T - 1)
            logits = tab[bidx, idx, (count.long() % 8)[:, None]].contiguous()      # [B, n, V + D]
            ops.tdt_scan_batch(logits, D, t, T_len, need, dec, lp)
            ops.tdt_advance(dec, lp, durations, n_hist, hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, score, blank)
            blocks += 1
            pending, alive = flags.tolist()
            assert pending == int(need.sum()) and alive == int((done == 0).sum())
            if pending == 0:
                break
        if alive == 0:
            break
        n_hist += 1
    out = []
    for b in range(B):
        c = int(count[b])
        out.append((hist[b, 1:1 + c].tolist(), frames[b, :c].tolist(), tok_lp[b, :c].tolist(), tok_dur[b, :c].tolist(), float(score[b])))
    return out, blocks, t.cpu().tolist()


@pytest.mark.parametrize("n", [1, 4, 64])
def test_scan_and_advance_against_the_oracle_decoder(n):
    """B 4, T 37, V 6, durations (1, 2, 4, 7): jumps that cross the block edge (n 4 against durations up to 7) and that pass T_b; utterance 1
    emits nothing (its blank column is raised); utterance 2 has an exact tie across its whole duration sub-row (the lowest index wins)"""
    V, durations, T, blank = 6, (1, 2, 4, 7), 37, 2
    rng = np.random.default_rng(20)
    table = rng.standard_normal((4, T, 8, V + 4)).astype(np.float32)
    table[:, :, :, blank] += 1.0                        # about half of the decisions are blanks
    table[1, :, :, blank] += 50.0
    table[2, :, :, V:] = 0.25
    T_len = [37, 30, 37, 5]
    got, blocks, t_end = _decode(table, T_len, durations, V, n, blank)
    crossed = past = False
    for b in range(4):
        want = O.greedy_decode(lambda t, tokens: table[b, t, len(tokens) % 8], T_len[b], durations, V, blank)
        tokens, frames, lps, durs, score = got[b]
        print("n %d utt %d: %d tokens, score %.6f against %.6f, decisions %s" % (n, b, len(tokens), score, want[4], want[5]))
        assert (tokens, frames, durs) == (want[0], want[1], want[3])
        assert np.allclose(lps, want[2], rtol=1e-5, atol=1e-6)
        assert abs(score - want[4]) <= 1e-5 * abs(want[4])
        assert t_end[b] == sum(want[5])                                              # the carry-over: t is t0 + r exactly, overshoot included
        past |= sum(want[5]) > T_len[b]
        crossed |= any(d > n for d in want[5][:-1])                                  # a jump longer than the block leaves it wherever it starts
    assert got[1][0] == [] and got[2][0] and all(d == 1 for d in got[2][3]) and past
    assert crossed or n == 64


def test_rows_that_need_nothing_are_left_alone():
    from ttmi import ops
    V, D, n, dev = 5, 2, 3, "cuda"
    logits = torch.randn(2, n, V + D, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    t, T_len, need, done, count, flags = i32([1, 0]), i32([9, 9]), i32([0, 1]), i32([0, 0]), i32([2, 0]), i32([7, 7])
    dec = torch.full((2, n, 2), -5, dtype=torch.int32, device=dev)
    lp = torch.full((2, n, 2), 3.5, device=dev)
    hist = torch.full((2, 6), 9, dtype=torch.long, device=dev)
    frames, tok_dur = (torch.full((2, 4), -7, dtype=torch.int32, device=dev) for _ in range(2))
    tok_lp = torch.full((2, 4), 2.5, device=dev)
    score = torch.tensor([1.25, 0.0], dtype=torch.float64, device=dev)
    ops.tdt_scan_batch(logits, D, t, T_len, need, dec, lp)
    assert bool((dec[0] == -5).all()) and bool((lp[0] == 3.5).all()) and bool((dec[1, :, 0] >= 0).all())
    ops.tdt_advance(dec, lp, (1, 2), 1, hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, score)
    torch.cuda.synchronize()
    assert int(t[0]) == 1 and int(count[0]) == 2 and float(score[0]) == 1.25 and bool((hist[0] == 9).all())
    assert bool((frames[0] == -7).all()) and bool((tok_dur[0] == -7).all()) and bool((tok_lp[0] == 2.5).all())
    assert int(t[1]) >= 1 and flags.tolist() == [int(need.sum()), 2]
    # a bf16 block gives the decisions of its values widened to f32
    lb = logits.to(torch.bfloat16)
    dec2, lp2 = torch.zeros_like(dec), torch.zeros_like(lp)
    dec3, lp3 = torch.zeros_like(dec), torch.zeros_like(lp)
    one = i32([1, 1])
    ops.tdt_scan_batch(lb, D, i32([0, 0]), T_len, one, dec2, lp2)
    ops.tdt_scan_batch(lb.float(), D, i32([0, 0]), T_len, one, dec3, lp3)
    assert torch.equal(dec2, dec3) and torch.equal(lp2, lp3)
