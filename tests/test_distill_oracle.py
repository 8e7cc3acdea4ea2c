"""CPU-only: the float64 reference of the distillation on collapsed lattice posteriors (tests/distill_oracle.py) is held against torch
autograd, closed forms and the full-V KL; planted defects are shown to be visible at twice the bound the GPU tests use; and what the feature
offers without a GPU - argument validation of the entry points, the ValueErrors of the Python layers - is exercised."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distill_oracle as D
from conftest import PKG

TOL = 1e-4                     # the bound of tests/test_distill_gpu.py; a planted defect has to move something by twice that


def case(seed, B=3, T=5, U1=4, V=11, scale=2.0):
    rng = np.random.default_rng(seed)
    xs, xt = (scale * rng.standard_normal((B, T, U1, V)) for _ in range(2))
    labels = rng.integers(0, V, (B, U1 - 1)).astype(np.int32)           # the whole vocabulary: some labels equal `blank`
    return xs, xt, labels, [T, 1, T // 2 + 1], [U1 - 1, 0, 1]


# ----------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("blank", [0, 3])
def test_hand_gradient_equals_autograd(blank):
    import torch
    xs, xt, labels, tl, ul = case(1)
    labels[0, 0] = blank                                                # y == blank inside the lattice
    post = D.collapse(xt, labels, tl, ul, blank)
    costs, grad, _ = D.kd_loss(xs, post, labels, tl, ul, blank)
    x = torch.tensor(xs, requires_grad=True)
    c = D.kd_loss_torch(x, post, labels, tl, ul, blank)
    c.sum().backward()
    print("cost diff %.1e, gradient diff %.1e" % (np.abs(c.detach().numpy() - costs).max(), np.abs(x.grad.numpy() - grad).max()))
    assert np.abs(c.detach().numpy() - costs).max() < 1e-12
    assert np.abs(x.grad.numpy() - grad).max() < 1e-12
    assert np.abs(grad.sum(-1)).max() < 1e-12                           # every row sums to zero
    assert np.all(costs > 0)


def test_teacher_equal_to_student_costs_nothing():
    xs, _, labels, tl, ul = case(2)
    post = D.collapse(xs, labels, tl, ul)
    costs, grad, coef = D.kd_loss(xs, post, labels, tl, ul)
    assert np.abs(costs).max() < 1e-12 and np.abs(grad).max() < 1e-12
    Tb, Ub = D.lengths(tl, ul, 5, 4)
    for b in range(3):
        assert np.allclose(coef[b, :Tb[b], :Ub[b] + 1], 1.0, atol=1e-12)       # P^T_o / P^S_o = 1


def test_empty_label_class_has_two_classes():
    """u == U_b and y == blank: ly = NEG, the other class takes everything but blank, and the two probabilities add up to one"""
    xs, _, labels, tl, ul = case(3)
    labels[0, 1] = 0
    post = D.collapse(xs, labels, tl, ul)
    Tb, Ub = D.lengths(tl, ul, 5, 4)
    for b, u in [(b, Ub[b]) for b in range(3)] + [(0, 1)]:
        for t in range(Tb[b]):
            lb, ly, lo = post[b, t, u]
            assert ly == D.NEG
            assert abs(np.exp(lb) + np.exp(lo) - 1.0) < 1e-12
            assert abs(lo - (D.lse(np.delete(xs[b, t, u], 0)) - D.lse(xs[b, t, u]))) < 1e-12
    b, t, u = 0, 0, 0                                                   # a full node: three classes that add up to one
    assert labels[0, 0] != 0 and abs(np.exp(post[b, t, u]).sum() - 1.0) < 1e-12
    for b in range(3):                                                  # outside the ragged lattice: exact zeros
        assert np.all(post[b, Tb[b]:] == 0) and np.all(post[b, :, Ub[b] + 1:] == 0)
    # V = 2 with a label: no other column at all, and the other class holds NEG
    z2 = np.array([[[[0.3, -1.2], [0.1, 0.2]]]])
    p2 = D.collapse(z2, np.array([[1]]), [1], [1])
    assert p2[0, 0, 0, 2] == D.NEG and abs(np.exp(p2[0, 0, 0, :2]).sum() - 1.0) < 1e-12
    c, g, coef = D.kd_loss(z2, p2 * 1.0, np.array([[1]]), [1], [1])
    assert abs(c[0]) < 1e-12 and np.abs(g).max() < 1e-12
    assert coef[0, 0, 0] == 0 and abs(coef[0, 0, 1] - 1.0) < 1e-12         # empty on both sides: 0; at u == U_b column 1 is the other class


def test_collapsed_kl_is_never_above_the_full_kl():
    """collapsing classes is a deterministic map of the outcome: the KL cannot grow (data processing inequality)"""
    rng = np.random.default_rng(4)
    for i in range(200):
        V = int(rng.integers(2, 40))
        zt, zs = (3.0 * rng.standard_normal(V) for _ in range(2))
        blank = int(rng.integers(0, V))
        y = int(rng.integers(-1, V))
        y = -1 if y == blank else y
        tp = D.collapse_row(zt, y, blank)[1:]
        c, _, _ = D.kd_row(zs, tp, y, blank)
        full = D.full_kl_row(zt, zs)
        assert -1e-12 <= c <= full + 1e-12, (i, c, full)


# ----------------------------------------------------------------------------- planted defects
def test_planted_wrong_label_column_moves_the_cost():
    xs, xt, labels, tl, ul = case(5)
    labels[0] = [2, 5, 7]
    post = D.collapse(xt, labels, tl, ul)
    good, _, _ = D.kd_loss(xs, post, labels, tl, ul)
    bad, _, _ = D.kd_loss(xs, post, labels, tl, ul, defect="label_prev")
    print("labels[b][u-1] for labels[b][u]: cost %.6f -> %.6f" % (good[0], bad[0]))
    assert abs(bad[0] - good[0]) >= 2 * TOL * abs(good[0])


# blank margins of the teacher's and the student's row.  At 14 and 12 the subtraction form moves the coefficient by 1.4e-4 of itself, short of
# twice the bound; at 16 and 14 by 6.9e-5 (what is lost is one rounding of 1 - p, a matter of luck); at 18 and 16 by 3.4e-3
MARGIN_T, MARGIN_S = 18.0, 16.0


def test_planted_other_mass_by_f32_subtraction_moves_the_coefficient():
    """a confident row (V 37, blank ahead of every other column by MARGIN nats): 1 - p_b - p_y in float32 keeps a handful of bits of the other
    mass, and the gradient coefficient 1 - P^T_o / P^S_o of the other columns moves by more than twice the bound; the direct log-sum-exp,
    evaluated in float32 all the way, stays four orders of magnitude inside it"""
    rng = np.random.default_rng(6)
    V = 37
    zt, zs = rng.standard_normal(V), rng.standard_normal(V)
    zt[0], zs[0] = zt[1:].max() + MARGIN_T, zs[1:].max() + MARGIN_S
    y = 5
    tp = D.collapse_row(zt, y, 0)[1:]
    _, _, co = D.kd_row(zs, tp, y, 0)
    _, _, co_sub = D.kd_row(zs, tp, y, 0, defect="other_sub_f32")
    # the direct form in float32: an online-free log-sum-exp over the other columns with every operation rounded to float32
    z32 = zs.astype(np.float32)
    keep = np.ones(V, dtype=bool)
    keep[[0, y]] = False
    m = z32[keep].max()
    lo32 = m + np.log(np.exp(z32[keep] - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
    ma = z32.max()
    l32 = ma + np.log(np.exp(z32 - ma, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
    co_direct = float(np.exp(np.float32(tp[2]) - (lo32 - l32), dtype=np.float32))
    print("coefficient 1 - c_o: exact %.8f, f32 subtraction moves it by %.2e, f32 direct log-sum-exp by %.2e"
          % (1 - co, abs(co_sub - co), abs(co_direct - co)))
    assert abs(co_sub - co) >= 2 * TOL * abs(1 - co)
    assert abs(co_direct - co) < 0.1 * TOL * abs(1 - co)


def test_planted_extra_frame_moves_the_cost():
    xs, xt, labels, tl, ul = case(7)
    post = D.collapse(xt, labels, [5, 5, 5], ul)                        # a teacher that knows every frame
    good, _, _ = D.kd_loss(xs, post, labels, tl, ul)
    bad, _, _ = D.kd_loss(xs, post, labels, tl, ul, defect="count_t_Tb")
    print("row t == T_b counted: costs %s -> %s" % (good, bad))
    assert bad[0] == good[0]                                            # T_b == T: no such frame
    for b in (1, 2):
        assert abs(bad[b] - good[b]) >= 2 * TOL * abs(good[b])


def test_planted_label_class_at_the_last_row_moves_the_cost():
    xs, xt, labels, tl, ul = case(8)
    labels[:, :2] = [[3, 4], [5, 6], [7, 8]]
    post = D.collapse(xt, labels, tl, ul)
    good, _, _ = D.kd_loss(xs, post, labels, tl, ul)
    bad, _, _ = D.kd_loss(xs, post, labels, tl, ul, defect="label_at_Ub")
    print("a label class at u == U_b: costs %s -> %s" % (good, bad))
    assert bad[0] == good[0]                                            # U_b == U1 - 1: no label to read there
    for b in (1, 2):
        assert abs(bad[b] - good[b]) >= 2 * TOL * abs(good[b])


def test_planted_other_coefficient_on_the_blank_column_moves_the_gradient():
    xs, xt, labels, tl, ul = case(9)
    post = D.collapse(xt, labels, tl, ul)
    _, good, _ = D.kd_loss(xs, post, labels, tl, ul)
    _, bad, _ = D.kd_loss(xs, post, labels, tl, ul, defect="other_on_blank")
    moved = np.abs(bad - good).max(-1) / np.maximum(np.abs(good).max(-1), 1e-300)
    Tb, Ub = D.lengths(tl, ul, 5, 4)
    inside = np.concatenate([moved[b, :Tb[b], :Ub[b] + 1].ravel() for b in range(3)])
    print("other coefficient on the blank column: a gradient element moves by %.2e .. %.2e of its row's largest" % (inside.min(), inside.max()))
    assert inside.min() >= 2 * TOL
    assert np.array_equal(bad[..., 1:], good[..., 1:])                  # only the blank column


# ----------------------------------------------------------------------------- what the feature offers without a GPU
def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):              # (as tests/test_abi.py: a tree that was not built yet)
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    return ctypes.CDLL(so)


def test_entry_points_validate_without_gpu():
    lib = _lib()
    lib.ttmi_last_error.restype = ctypes.c_char_p
    L, F = ctypes.c_long, ctypes.c_float
    rc = lib.ttmi_kd_collapse(None, 0, L(5), None, None, None, 1, 1, 1, 5, 0, None, None)
    assert rc < 0 and b"kd_collapse: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_kd_loss_fwd(None, 0, L(5), None, None, None, 1, 1, 1, 5, 0, None, None, None, None)
    assert rc < 0 and b"kd_loss_fwd: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_kd_loss_bwd(None, 0, L(5), None, None, None, 1, 1, 1, 5, 0, None, None, 0, F(1.0), None, L(5), 0, None)
    assert rc < 0 and b"kd_loss_bwd: null pointer" in lib.ttmi_last_error()
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p, q = ctypes.c_void_p(base), ctypes.c_void_p(base + 1024)
    args = lambda **kw: [p, kw.get("dtype", 0), L(kw.get("ldv", 5)), p, p, p, 1, 1, 1, kw.get("V", 5), kw.get("blank", 0)]
    for kw, msg in (({"V": 1, "ldv": 1}, b"V=1 < 2"), ({"blank": 5}, b"blank 5 outside [0,5)"), ({"ldv": 4}, b"bad pitch/dtype"),
                    ({"dtype": 2}, b"bad pitch/dtype")):
        assert lib.ttmi_kd_collapse(*args(**kw), p, None) < 0 and msg in lib.ttmi_last_error(), kw
        assert lib.ttmi_kd_loss_fwd(*args(**kw), p, p, p, None) < 0 and msg in lib.ttmi_last_error(), kw
        assert lib.ttmi_kd_loss_bwd(*args(**kw), p, p, 0, F(1.0), q, L(5), 0, None) < 0 and msg in lib.ttmi_last_error(), kw
    odd = ctypes.c_void_p(base + 4)
    assert lib.ttmi_kd_loss_fwd(*args(), p, odd, p, None) < 0 and b"16-byte aligned" in lib.ttmi_last_error()
    assert lib.ttmi_kd_loss_bwd(*args(), odd, p, 0, F(1.0), q, L(5), 0, None) < 0 and b"16-byte aligned" in lib.ttmi_last_error()
    # the logits cannot be the gradient that is added to; written in place they need the same pitch
    assert lib.ttmi_kd_loss_bwd(*args(), p, p, 0, F(1.0), p, L(5), 1, None) < 0 and b"accumulate" in lib.ttmi_last_error()
    assert lib.ttmi_kd_loss_bwd(*args(), p, p, 0, F(1.0), p, L(8), 0, None) < 0 and b"in-place" in lib.ttmi_last_error()
    assert lib.ttmi_kd_loss_bwd(*args(), p, p, 0, F(1.0), q, L(5), 2, None) < 0 and b"accumulate" in lib.ttmi_last_error()
    assert lib.ttmi_kd_loss_bwd(*args(), p, p, 0, F(1.0), q, L(4), 0, None) < 0 and b"pitch" in lib.ttmi_last_error()


def test_workspace_bytes():
    lib = _lib()
    lib.ttmi_kd_workspace_bytes.restype = ctypes.c_size_t
    assert lib.ttmi_kd_workspace_bytes(2, 10, 4) == (16 + 4) * 2 * 10 * 4           # one 16-byte record and one f32 cost per row
    assert lib.ttmi_kd_workspace_bytes(0, 10, 4) == 0


def test_python_layers_refuse_without_device():
    import torch
    from ttmi import distill, ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    x, y = torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.kd_collapse(x, y, i32(2), i32(1))
    with pytest.raises(ValueError):
        ops.kd_loss_fwd(x, y, i32(2), i32(1), 0, torch.zeros(1, 2, 2, 3), torch.zeros(64))
    with pytest.raises(ValueError):
        ops.kd_loss_bwd(x, y, i32(2), i32(1), 0, torch.zeros(64), torch.ones(1), 0, 1.0)
    with pytest.raises(ValueError, match="GPU"):
        distill.lattice_posteriors(x, y, i32(2), i32(1))
    # the teacher's posteriors: shape, then dtype, then device
    with pytest.raises(ValueError, match=r"shape \[1, 2, 2, 3\]"):
        distill.lattice_kd_loss(x, torch.zeros(1, 2, 2, 4), y, i32(2), i32(1))
    with pytest.raises(ValueError, match=r"shape \[1, 2, 2, 3\]"):
        distill.lattice_kd_loss(x, torch.zeros(2, 2, 3), y, i32(2), i32(1))
    with pytest.raises(ValueError, match="float32"):
        distill.lattice_kd_loss(x, torch.zeros(1, 2, 2, 3, dtype=torch.float64), y, i32(2), i32(1))
    with pytest.raises(ValueError, match="GPU"):
        distill.lattice_kd_loss(x, torch.zeros(1, 2, 2, 3), y, i32(2), i32(1))
    with pytest.raises(ValueError, match="reduction"):
        distill.lattice_kd_loss(x, torch.zeros(1, 2, 2, 3), y, i32(2), i32(1), reduction="max")
    with pytest.raises(ValueError, match="reduction"):
        distill.LatticeKDLoss(reduction="max")
    assert distill.LatticeKDLoss(blank=2, reduction="sum").blank == 2


def test_transducer_loss_refuses_distill_with_exp_domain():
    """before anything runs on a device: the module is built on the host"""
    import torch
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    model = Transducer(cfg)
    x, y = torch.zeros(1, 4, 64), torch.ones(1, 2, dtype=torch.long)
    al, ll = torch.tensor([4], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    post = torch.zeros(1, 4, 3, 3)
    with pytest.raises(ValueError, match="distill"):
        model.loss(x, al, y, ll, exp_domain=True, distill=post, distill_weight=0.5)
    for bad in (-0.5, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="distill_weight"):
            model.loss(x, al, y, ll, distill=post, distill_weight=bad)
    # the pinned refusals stay what they were
    with pytest.raises(ValueError, match="fastemit"):
        model.loss(x, al, y, ll, topology="monotonic", fastemit_lambda=0.01, distill=post, distill_weight=0.5)
    with pytest.raises(ValueError, match="exp"):
        model.loss(x, al, y, ll, topology="monotonic", exp_domain=True)
    with pytest.raises(ValueError, match="GPU"):
        model.lattice_posteriors(x, al, y, ll)
