"""CTC loss / greedy decode kernels (csrc/ctc.hip) and the Transducer's auxiliary CTC head against an independent oracle:
torch.nn.functional.ctc_loss on the CPU in float64 and its autograd.  Tolerance: the project's 1e-4 (tests/test_rnnt_gpu.py) on costs and,
through rel_err, on gradients.  The oracle's gradient of an infeasible utterance is not used: cost +inf and all-zero rows are asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4


def oracle(x, labels, tl, ul, blank=0):
    """-> (costs [B] f64, d costs[b] / d x [B, T, V] f64); rows of infeasible utterances (cost inf) are left zero"""
    xd = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    lp = xd.log_softmax(-1).transpose(0, 1)
    costs = F.ctc_loss(lp, torch.tensor(np.asarray(labels), dtype=torch.long), torch.tensor(np.asarray(tl), dtype=torch.long),
                       torch.tensor(np.asarray(ul), dtype=torch.long), blank=blank, reduction="none", zero_infinity=False)
    ok = torch.isfinite(costs)
    if ok.any():
        costs[ok].sum().backward()
        grad = xd.grad.numpy().copy()
        grad[~ok.numpy()] = 0.0
    else:
        grad = np.zeros(xd.shape)
    return costs.detach().numpy(), grad


def run_hip(x, labels, tl, ul, blank=0, ld=None, go=None, scale=1.0, inplace=False):
    """the raw kernels -> (costs [B], grad buffer [B, T, ld]) with grad_out = go (default ones, per utterance)"""
    from ttmi import ops
    x = np.asarray(x, dtype=np.float32)
    B, T, V = x.shape
    ld = V if ld is None else ld
    buf = torch.full((B, T, ld), 7.0, dtype=torch.float32, device="cuda")       # pad columns start as garbage
    buf[..., :V] = torch.tensor(x)
    logits = buf[..., :V]
    y = torch.tensor(np.asarray(labels).reshape(B, -1), dtype=torch.int32, device="cuda")
    tlg, ulg = (torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda") for v in (tl, ul))
    ws = ops.ctc_workspace(B, T, y.shape[1], "cuda")
    costs = ops.ctc_loss_fwd(logits, y, tlg, ulg, blank, ws)
    g = torch.ones(B, device="cuda") if go is None else torch.tensor(np.asarray(go), dtype=torch.float32, device="cuda")
    grad = ops.ctc_loss_bwd(logits, y, tlg, ulg, blank, ws, g, 1, scale, inplace=inplace)
    if inplace:
        assert grad.data_ptr() == logits.data_ptr()
        full = buf
    else:
        full = torch.as_strided(grad, (B, T, ld), (T * ld, ld, 1))
    torch.cuda.synchronize()
    return costs.cpu().numpy(), full.cpu().numpy()


def check(x, labels, tl, ul, blank=0, ld=None):
    V = np.asarray(x).shape[-1]
    want_c, want_g = oracle(x, labels, tl, ul, blank)
    costs, full = run_hip(x, labels, tl, ul, blank, ld)
    g = full[..., :V]
    fin = np.isfinite(want_c)
    print("costs", costs, "oracle", want_c, "grad rel err", rel_err(g, want_g))
    assert np.all(np.isposinf(costs[~fin])), costs
    assert np.all(np.abs(costs[fin] - want_c[fin]) <= TOL * np.abs(want_c[fin])), (costs, want_c)
    assert np.isfinite(g).all()
    assert rel_err(g, want_g) < TOL
    for b in range(len(tl)):
        assert np.all(full[b, tl[b]:] == 0), b                                  # frames past the utterance
        if not fin[b]:
            assert np.all(full[b] == 0), b                                      # no feasible alignment: zero rows, never NaN
    assert np.all(full[..., V:] == 0)                                           # pad columns
    # every row sums to zero: its entries are g * (softmax - occupancy), both sets of at most V f32 terms adding up to 1, so the sum's
    # rounding error is a few f32 ulps of 1 per addend pair at the worst - 1e-5 leaves room for V = 4334
    assert np.abs(g.sum(-1, dtype=np.float64)).max() < 1e-5
    return costs, g


# ----------------------------------------------------------------------------- smallest lattices
SMALL = [("T1_U0", 1, []), ("T1_U1", 1, [2]), ("T2_U1", 2, [3]), ("T5_U0", 5, []), ("aa_T3_min_feasible", 3, [2, 2]), ("aa_T2_infeasible", 2, [2, 2])]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_smallest_lattices(case):
    _, T, lab = case
    rng = np.random.default_rng(len(lab) * 10 + T)
    x = rng.standard_normal((1, T, 5)).astype(np.float32)
    costs, g = check(x, np.array(lab, dtype=np.int32).reshape(1, -1), [T], [len(lab)])
    if case[0] == "aa_T2_infeasible":
        assert np.isposinf(costs[0]) and np.all(g == 0)


def test_ragged_batch():
    """B 4, T 12, U 5, V 7, repeated labels, lengths that include U_b = 0 and T_b = 1, pitch 64"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 12, 7)).astype(np.float32)
    labels = np.array([[1, 1, 2, 2, 1], [3, 4, 3, 3, 6], [5, 5, 5, 1, 1], [2, 6, 6, 1, 3]], dtype=np.int32)
    check(x, labels, [12, 9, 1, 7], [5, 3, 0, 2], ld=64)
    check(x, labels, [12, 9, 1, 7], [5, 3, 1, 2], ld=64)


@pytest.mark.parametrize("U", [31, 32, 63, 64])
def test_lane_and_wave_boundaries(U):
    """S = 63, 65, 127, 129 states: the last lane of a wave, the first of the next, one wave and two; V = 37 rows are unaligned, so the head
    and tail of the 16-byte walk run"""
    rng = np.random.default_rng(U)
    T, V, B = U + 3, 37, 3
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = np.zeros((B, U), dtype=np.int32)
    labels[0] = 1 + (np.arange(U) % 3)                                          # three symbols, each about U / 3 times ...
    labels[0, 5], labels[0, U - 1] = labels[0, 4], labels[0, U - 2]             # ... and two adjacent repeats: feasible from T = U + 2 on
    labels[1] = 1 + (np.arange(U) % 2)                                          # no adjacent repeat: feasible at T = U exactly
    labels[2] = rng.integers(1, V, U)
    check(x, labels, [T, U, T - 1], [U, U, U - 2])


def test_long_labels_many_waves():
    rng = np.random.default_rng(7)
    B, T, U, V = 2, 450, 200, 11
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    check(x, labels, [T, 431], [U, 129])


def test_workload_vocabulary():
    rng = np.random.default_rng(8)
    B, T, U, V = 2, 20, 6, 4334
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    labels[1, 3] = labels[1, 2]
    check(x, labels, [T, 17], [U, 5], ld=4352)


def test_range_long_utterance():
    """B 1, T 2000, U 10, V 16, logits scaled until the cost is in the thousands: what the fp64 frontier is for"""
    rng = np.random.default_rng(9)
    x = (6.0 * rng.standard_normal((1, 2000, 16))).astype(np.float32)
    labels = rng.integers(1, 16, (1, 10)).astype(np.int32)
    want_c, _ = oracle(x, labels, [2000], [10])
    assert want_c[0] > 1000.0
    costs, _ = check(x, labels, [2000], [10])
    assert abs(costs[0] - want_c[0]) <= TOL * want_c[0]


# ----------------------------------------------------------------------------- options and aliasing
def test_in_place_gradient_and_grad_out():
    rng = np.random.default_rng(10)
    B, T, U, V = 3, 14, 4, 37
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, 6, (B, U)).astype(np.int32)
    tl, ul, go = [14, 10, 12], [4, 2, 3], np.array([0.5, -2.0, 3.0], dtype=np.float32)
    _, want_g = oracle(x, labels, tl, ul)
    want = want_g * go[:, None, None] * 0.25
    for ld in (V, 40, 64):
        c0, g0 = run_hip(x, labels, tl, ul, ld=ld, go=go, scale=0.25)
        c1, g1 = run_hip(x, labels, tl, ul, ld=ld, go=go, scale=0.25, inplace=True)
        assert np.array_equal(g0, g1) and np.array_equal(c0, c1), ld
        assert rel_err(g1[..., :V], want) < TOL and np.all(g1[..., V:] == 0), ld


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_reductions(reduction):
    from ttmi.ctc import CTCLoss
    rng = np.random.default_rng(11)
    B, T, U, V = 4, 10, 3, 9
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    tl, ul = [10, 8, 10, 5], [3, 1, 0, 2]
    want_c, want_g = oracle(x, labels, tl, ul)
    xg = torch.tensor(x, device="cuda", requires_grad=True)
    loss = CTCLoss(reduction=reduction)(xg, torch.tensor(labels), torch.tensor(tl), torch.tensor(ul))
    w = torch.tensor([1.0, -0.5, 2.0, 0.25], device="cuda")
    if reduction == "none":
        assert loss.shape == (B,) and rel_err(loss.detach().cpu().numpy(), want_c) < TOL
        (loss * w).sum().backward()                                              # a non-uniform upstream gradient
        want = want_g * w.cpu().numpy()[:, None, None]
    else:
        div = B if reduction == "mean" else 1                                    # 'mean' divides by the batch, not by target lengths
        assert loss.shape == (1,) and abs(float(loss) - want_c.sum() / div) <= TOL * want_c.sum() / div
        (3.0 * loss).sum().backward()
        want = 3.0 * want_g / div
    assert rel_err(xg.grad.cpu().numpy(), want) < TOL


def test_zero_infinity():
    from ttmi.ctc import ctc_loss
    rng = np.random.default_rng(12)
    x = rng.standard_normal((2, 3, 6)).astype(np.float32)
    labels = np.array([[2, 2], [1, 3]], dtype=np.int32)                          # [a, a] needs 3 frames
    tl, ul = torch.tensor([2, 3]), torch.tensor([2, 2])
    want_c, want_g = oracle(x, labels, [2, 3], [2, 2])
    for zi in (False, True):
        xg = torch.tensor(x, device="cuda", requires_grad=True)
        c = ctc_loss(xg, torch.tensor(labels), tl, ul, reduction="none", zero_infinity=zi)
        assert (float(c[0]) == 0.0) if zi else torch.isposinf(c[0])
        assert abs(float(c[1]) - want_c[1]) <= TOL * want_c[1]
        c[1].backward() if not zi else c.sum().backward()
        g = xg.grad.cpu().numpy()
        assert np.all(g[0] == 0) and rel_err(g[1], want_g[1]) < TOL
    xg = torch.tensor(x, device="cuda", requires_grad=True)
    m = ctc_loss(xg, torch.tensor(labels), tl, ul, reduction="mean", zero_infinity=True)
    assert abs(float(m) - want_c[1] / 2) <= TOL * want_c[1]
    m.backward()
    assert torch.isfinite(xg.grad).all()


def test_two_runs_give_identical_bits():
    """U 40 with labels drawn from two symbols only: every symbol's column sums twenty states"""
    rng = np.random.default_rng(13)
    B, T, U, V = 3, 70, 40, 19
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, 3, (B, U)).astype(np.int32)
    runs = [run_hip(x, labels, [70, 66, 70], [40, 33, 40]) for _ in range(2)]
    assert np.array_equal(runs[0][0].view(np.int32), runs[1][0].view(np.int32))
    assert np.array_equal(runs[0][1].view(np.int32), runs[1][1].view(np.int32))
    check(x, labels, [70, 66, 70], [40, 33, 40])


def test_graph_capture_forward_and_backward():
    from ttmi import ops
    rng = np.random.default_rng(14)
    B, T, U, V = 3, 25, 6, 37
    xa, xb = (rng.standard_normal((B, T, V)).astype(np.float32) for _ in range(2))
    y = torch.tensor(rng.integers(1, 5, (B, U)).astype(np.int32), device="cuda")
    tl, ul = torch.tensor([25, 20, 9], dtype=torch.int32, device="cuda"), torch.tensor([6, 4, 0], dtype=torch.int32, device="cuda")
    go = torch.tensor([1.0, 2.0, -1.0], device="cuda")

    def run(x, w):
        costs = ops.ctc_loss_fwd(x, y, tl, ul, 0, w)
        return costs, ops.ctc_loss_bwd(x, y, tl, ul, 0, w, go, 1, 0.5)

    static = torch.tensor(xa, device="cuda")
    ws = ops.ctc_workspace(B, T, U, "cuda")
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
    eager = run(torch.tensor(xb, device="cuda"), ops.ctc_workspace(B, T, U, "cuda"))
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want_c, _ = oracle(xb, y.cpu().numpy(), [25, 20, 9], [6, 4, 0])
    assert rel_err(outs[0].cpu().numpy(), want_c) < TOL


# ----------------------------------------------------------------------------- greedy decode
def collapse(x, lens, blank=0):
    out = []
    for b in range(x.shape[0]):
        am = np.argmax(x[b, :lens[b]], axis=-1)
        out.append([int(v) for i, v in enumerate(am) if v != blank and (i == 0 or v != am[i - 1])])
    return out


def test_ctc_greedy_against_numpy():
    from ttmi.ctc import ctc_greedy_decode
    rng = np.random.default_rng(15)
    V = 9
    x1 = rng.standard_normal((2, 1, V)).astype(np.float32)                       # T = 1
    assert ctc_greedy_decode(torch.tensor(x1, device="cuda")) == collapse(x1, [1, 1])
    xb = rng.standard_normal((2, 6, V)).astype(np.float32)
    xb[..., 0] += 50.0                                                           # all blank
    assert ctc_greedy_decode(torch.tensor(xb, device="cuda"), torch.tensor([6, 4])) == [[], []]
    xs = rng.standard_normal((1, 9, V)).astype(np.float32)
    xs[..., 4] += 50.0                                                           # one symbol throughout
    assert ctc_greedy_decode(torch.tensor(xs, device="cuda")) == [[4]]
    xr = rng.standard_normal((4, 130, V)).astype(np.float32)                     # ragged lengths, T = 130: three compaction chunks
    xr[0] = np.repeat(xr[0, ::3], 3, axis=0)[:130]                               # runs of three equal frames
    xr[1, :, 0] += 1.5                                                           # mostly blank
    lens = [130, 64, 65, 1]
    got = ctc_greedy_decode(torch.tensor(xr, device="cuda"), torch.tensor(lens))
    assert got == collapse(xr, lens)
    assert len(got[0]) > 10 and len(got[1]) < len(got[2]) + 40
    # non-zero blank, row-padded logits
    buf = torch.zeros(4, 130, 64, device="cuda")
    buf[..., :V] = torch.tensor(xr)
    assert ctc_greedy_decode(buf[..., :V], torch.tensor(lens), blank=3) == collapse(xr, lens, blank=3)


def test_ctc_greedy_raises_on_nan_row():
    from ttmi.ctc import ctc_greedy_decode
    rng = np.random.default_rng(16)
    x = rng.standard_normal((2, 7, 9)).astype(np.float32)
    x[1, 5, 3] = np.nan
    with pytest.raises(RuntimeError, match="frame 5 of utterance 1"):
        ctc_greedy_decode(torch.tensor(x, device="cuda"))
    assert ctc_greedy_decode(torch.tensor(x, device="cuda"), torch.tensor([7, 5])) == collapse(x, [7, 5])     # the NaN frame is past the utterance
    x[1, 5] = -np.inf
    with pytest.raises(RuntimeError):
        ctc_greedy_decode(torch.tensor(x, device="cuda"))


# ----------------------------------------------------------------------------- model level
def _tiny(ctc_weight):
    from tt.model import Transducer
    from tt.utils import AttrDict
    z, sd = load_golden("tiny_kshort")
    side = dict(n_layer=2, d_model=96, n_head=4, d_head=24, d_inner=160)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=sd["encoder.layers.0.r_emb"].shape[0]),
                        dec=dict(side, max_target_length=sd["decoder.layers.0.r_emb"].shape[0]),
                        joint=dict(input_size=192, inner_size=80), vocab_size=48, dropout=0.0, ctc_weight=ctc_weight))
    torch.manual_seed(5)
    model = Transducer(cfg).cuda().eval()
    res = model.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=False)
    assert sorted(res.missing_keys) == ["ctc_head.bias", "ctc_head.weight"] and not res.unexpected_keys
    return z, model


def _head_oracle(model, enc, targets, tl, ul):
    """the oracle's CTC ('mean' over the batch) on the module's own encoder output pushed through the head in float64, with autograd"""
    e = torch.tensor(enc.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
    w = torch.tensor(model.ctc_head.weight.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(model.ctc_head.bias.detach().cpu().numpy(), dtype=torch.float64, requires_grad=True)
    lp = (e @ w.t() + b).log_softmax(-1).transpose(0, 1)
    c = F.ctc_loss(lp, targets.cpu().long(), tl.cpu().long(), ul.cpu().long(), blank=0, reduction="none").sum() / e.shape[0]
    c.backward()
    return float(c), e.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def _batch(z):
    x = torch.tensor(z["inputs"], device="cuda")
    y = torch.tensor(z["targets"], device="cuda")
    tl = torch.tensor(z["full/act_lens"], device="cuda").int()
    ul = torch.tensor(z["full/label_lens"], device="cuda").int()
    tl = tl.clone()
    ul = ul.clone()
    if tl.numel() > 1:
        tl[-1] = max(int(tl[-1]) - 3, int(ul[-1]) * 2 + 1)                         # one ragged utterance
    return x, y, tl, ul


def test_model_loss_adds_weighted_ctc_fp32():
    z, model = _tiny(0.3)
    x, y, tl, ul = _batch(z)
    with torch.no_grad():
        enc = model.encoder(x, None)
    want, want_de, want_gw, want_gb = _head_oracle(model, enc, y, tl, ul)
    with torch.no_grad():
        both = float(model.loss(x, tl, y, ul, check_lengths=False, ctc_weight=0.3))
        plain = float(model.loss(x, tl, y, ul, check_lengths=False, ctc_weight=0))
        cfgw = float(model.loss(x, tl, y, ul, check_lengths=False))                  # None: the config's 0.3
    print("rnnt %.6f, rnnt + 0.3 ctc %.6f, oracle ctc %.6f" % (plain, both, want))
    assert cfgw == both
    assert abs((both - plain) - 0.3 * want) <= TOL * 0.3 * want
    # gradients of the CTC term alone: head weight, bias, and what reaches the encoder output
    e = enc.clone().requires_grad_(True)
    model.zero_grad()
    c = model._ctc_from_states(e, y, tl, ul, "mean")
    assert abs(float(c) - want) <= TOL * want
    c.backward()
    assert rel_err(model.ctc_head.weight.grad.cpu().numpy(), want_gw) < TOL
    assert rel_err(model.ctc_head.bias.grad.cpu().numpy(), want_gb) < TOL
    assert rel_err(e.grad.cpu().numpy(), want_de) < TOL
    # ... and through Transducer.ctc_loss (its own encoder pass), and recognize_ctc against the argmax of the same logits
    assert abs(float(model.ctc_loss(x, tl, y, ul)) - want) <= TOL * want
    logits = (enc @ model.ctc_head.weight.t() + model.ctc_head.bias).detach().cpu().numpy()
    assert model.recognize_ctc(x, tl) == collapse(logits, tl.cpu().tolist())


def test_model_bf16_mode_close(monkeypatch):
    """the tolerances tests/test_model_gpu.py::test_bf16_mode_close uses: loss 2e-3, gradients 6e-2"""
    z, model = _tiny(0.3)
    x, y, tl, ul = _batch(z)
    with torch.no_grad():
        enc = model.encoder(x, None)                                                 # fp32 encoder output: the head alone is under test
    want, want_de, want_gw, want_gb = _head_oracle(model, enc, y, tl, ul)
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    e = enc.clone().requires_grad_(True)
    model.zero_grad()
    c = model._ctc_from_states(e, y, tl, ul, "mean")
    c.backward()
    errs = (abs(float(c) - want) / want, rel_err(model.ctc_head.weight.grad.cpu().numpy(), want_gw),
            rel_err(model.ctc_head.bias.grad.cpu().numpy(), want_gb), rel_err(e.grad.cpu().numpy(), want_de))
    print("bf16 head: loss rel err %.2e, grad rel errs weight %.2e bias %.2e enc %.2e" % errs)
    assert errs[0] < 2e-3 and max(errs[1:]) < 6e-2
    full = model.loss(x, tl, y, ul, check_lengths=False, ctc_weight=0.3)             # the whole bf16 step runs and is finite
    full.backward()
    assert torch.isfinite(full).all() and all(torch.isfinite(p.grad).all() for p in model.parameters())


def test_flat_model_fused_optimizer_step_moves_the_head():
    from ttmi.train import FlatModel, FusedOptimizer
    z, model = _tiny(0.3)
    model.train()
    x, y, tl, ul = _batch(z)
    flat = FlatModel(model)
    opt = FusedOptimizer(flat, kind="sgd", lr=0.05, momentum=0.9, max_grad_norm=5.0)
    assert model.ctc_head.weight._ttmi_direct and model.ctc_head.weight.data_ptr() >= flat.flat.data_ptr()
    w0, b0 = model.ctc_head.weight.detach().clone(), model.ctc_head.bias.detach().clone()
    flat.zero_grad()
    loss = model.loss(x, tl, y, ul, check_lengths=False)
    loss.backward()
    assert float(model.ctc_head.weight.grad.abs().sum()) > 0 and float(model.ctc_head.bias.grad.abs().sum()) > 0
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(model.ctc_head.weight, w0) and not torch.equal(model.ctc_head.bias, b0)
    assert torch.isfinite(model.ctc_head.weight).all()


def test_two_call_form_reaches_the_audio_states():
    """train.py's form: logits = model(x, y); loss = criterion(logits, ...) with the criterion ttmi.dp_train wraps"""
    from warprnnt_pytorch import RNNTLoss
    from ttmi.dp_train import CTCAugmentedCriterion
    z, model = _tiny(0.3)
    x, y, tl, ul = _batch(z)
    with torch.no_grad():
        want = float(model.loss(x, tl, y, ul, check_lengths=False, ctc_weight=0.3))
        crit = CTCAugmentedCriterion(RNNTLoss(check_lengths=False), model, 0.3)
        got = float(crit(model(x, y), y.int(), tl, ul))
    assert abs(got - want) <= 1e-6 * abs(want)
    assert "_ctc_states" not in model.__dict__                                       # released after use
