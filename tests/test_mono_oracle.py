"""CPU-only: the float64 reference of the monotonic RNN-T loss (tests/mono_oracle.py) checked against itself three ways, the defects it must be
able to see, and the parts of the feature that need no GPU (exported symbols, argument validation, the option's ValueErrors)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mono_oracle as M
from conftest import PKG, rel_err

TOL = 1e-4          # the bound tests/test_mono_gpu.py holds the kernels to


def _case(seed, B, T, U1, V, scale=1.0):
    rng = np.random.default_rng(seed)
    x = scale * rng.standard_normal((B, T, U1, V))
    labels = rng.integers(0, V, (B, max(U1 - 1, 1))).astype(np.int32)
    return rng, x, labels


# ----------------------------------------------------------------------------- the oracle against itself
def test_dp_equals_brute_force_for_all_small_lattices():
    """every T <= 6 and U <= T, blank 0 and blank V-1 (labels are drawn from the whole vocabulary: some equal `blank`)"""
    n = 0
    for T in range(1, 7):
        for U in range(0, T + 1):
            for blank in (0, 3):
                _, x, labels = _case(100 * T + 10 * U + blank, 1, T, U + 1, 4, scale=2.0)
                want = M.brute_force_cost(x[0], labels[0], T, U, blank)
                got, _ = M.mono_loss(x, labels, [T], [U], blank)
                assert abs(got[0] - want) <= 1e-12 * abs(want), (T, U, blank, got, want)
                n += 1
    assert n == 54


def test_analytic_gradient_equals_autograd():
    _, x, labels = _case(1, 4, 7, 5, 6)
    tl, ul = [7, 5, 4, 1], [4, 2, 4, 0]
    c0, g0 = M.mono_loss(x, labels, tl, ul, blank=2)
    c1, g1 = M.autograd_loss(x, labels, tl, ul, blank=2)
    assert np.allclose(c0, c1, rtol=1e-12, atol=0)
    assert rel_err(g0, g1) < 1e-12
    for b in range(4):
        assert np.all(g0[b, tl[b]:] == 0) and np.all(g0[b, :, ul[b] + 1:] == 0)      # outside the lattice


def test_rows_sum_to_zero_and_occupancy_is_conserved():
    _, x, labels = _case(2, 2, 9, 4, 5)
    _, g = M.mono_loss(x, labels, [9, 6], [3, 3])
    assert np.abs(g.sum(-1)).max() < 1e-14
    # every frame takes exactly one decision: the occupancies of a frame's cells add up to 1, i.e. minus the patched columns' sum is 1
    lp = M.log_softmax(x[0])
    lpb, lpl = M.emissions(lp, labels[0], 3, 0)
    alpha, beta, ll = M.lattice(lpb, lpl)
    occ = np.exp(alpha[:9] + beta[:9] - ll)
    assert np.allclose(occ.sum(-1), 1.0, rtol=0, atol=1e-12)


def test_closed_forms_at_the_corners():
    _, x, labels = _case(3, 1, 5, 6, 4)
    lp = M.log_softmax(x[0])
    c, _ = M.mono_loss(x, labels, [5], [0], blank=1)
    assert abs(c[0] + lp[:5, 0, 1].sum()) < 1e-12                                   # U_b = 0: every frame blank
    c, _ = M.mono_loss(x, labels, [5], [5], blank=1)
    assert abs(c[0] + sum(lp[t, t, labels[0, t]] for t in range(5))) < 1e-12        # U_b = T_b: every frame emits
    c, g = M.mono_loss(x, labels, [4], [5], blank=1)
    assert np.isposinf(c[0]) and np.all(g == 0)                                     # U_b > T_b: no path
    c, g = M.autograd_loss(x, labels, [4], [5], blank=1)
    assert np.isposinf(c[0]) and np.all(g == 0)


# ----------------------------------------------------------------------------- planted defects
def _defective(x, y, T, U, blank, defect):
    """a copy of the recursion for one utterance with ONE defect planted -> (cost, gradient [T, U+1, V]); defect None is the recursion itself"""
    lp = M.log_softmax(x[:T, :U + 1])
    NEG = -np.inf
    lae = np.logaddexp
    alpha = np.full((T + 1, U + 1), NEG)
    beta = np.full((T + 1, U + 1), NEG)
    alpha[0, 0], beta[T, U] = 0.0, 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            for u in range(U + 1):
                move = alpha[t, u - 1] + lp[t, u - 1, y[u - 1]] if u > 0 else NEG
                if defect == "seam64" and u == 64:
                    move = NEG                                                       # lane 0 of the second slot never hears from lane 63
                alpha[t + 1, u] = lae(alpha[t, u] + lp[t, u, blank], move)
        for t in range(T - 1, -1, -1):
            for u in range(U, -1, -1):
                nxt = beta[t, u + 1] if defect == "rnnt_label" and u < U else (beta[t + 1, u + 1] if u < U else NEG)      # the standard lattice keeps the frame
                move = lp[t, u, y[u]] + nxt if u < U else NEG
                if defect == "seam64" and u == 63:
                    move = NEG
                beta[t, u] = lae(lp[t, u, blank] + beta[t + 1, u], move)
        ll = alpha[T, U]
        if defect == "terminal_blank":
            ll = ll + lp[T - 1, U, blank]                                            # the standard lattice's closing blank
        g = np.zeros_like(lp)
        for t in range(T):
            for u in range(U + 1):
                occ = np.exp(alpha[t, u] + beta[t, u] - ll)
                g[t, u] = np.exp(lp[t, u]) * occ
                g[t, u, blank] -= np.exp(alpha[t, u] + lp[t, u, blank] + beta[t + 1, u] - ll)
                if u < U:
                    nxt = beta[t, u + 1] if defect == "rnnt_label" else beta[t + 1, u + 1]
                    g[t, u, y[u]] -= np.exp(alpha[t, u] + lp[t, u, y[u]] + nxt - ll)
    return -ll, np.nan_to_num(g, nan=0.0)


def _moved(x, y, T, U, blank, defect):
    """the largest relative move the defect causes: of the cost, or of one gradient row"""
    want_c, want_g = M.mono_loss(x[None], y[None], [T], [U], blank)
    c, g = _defective(x, y, T, U, blank, defect)
    dc = abs(c - want_c[0]) / abs(want_c[0]) if np.isfinite(c) else np.inf
    rows = [np.linalg.norm(g[t, u] - want_g[0, t, u]) / np.linalg.norm(want_g[0, t, u])
            for t in range(T) for u in range(U + 1) if np.linalg.norm(want_g[0, t, u]) > 1e-6]
    return max(dc, max(rows))


def test_the_copy_without_a_defect_is_the_recursion():
    _, x, labels = _case(4, 1, 6, 4, 5)
    assert _moved(x[0], labels[0], 6, 3, 0, None) < 1e-12


@pytest.mark.parametrize("defect", ["rnnt_label", "terminal_blank"])
def test_planted_defect_is_visible(defect):
    _, x, labels = _case(5, 1, 6, 4, 5)
    assert _moved(x[0], labels[0], 6, 3, 0, defect) >= 2 * TOL


def test_planted_seam_defect_is_visible():
    """a neighbour lost between label 63 and label 64 cuts every path of an utterance with more than 63 labels"""
    _, x, labels = _case(6, 1, 67, 66, 3)
    assert _moved(x[0], labels[0], 67, 65, 0, "seam64") >= 2 * TOL
    assert _moved(x[0], labels[0], 67, 65, 0, None) < 1e-12


# ----------------------------------------------------------------------------- what the feature offers without a GPU
def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):              # (as tests/test_abi.py: a tree that was not built yet)
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    return ctypes.CDLL(so)


def test_entry_points_validate_without_gpu():
    lib = _lib()
    lib.ttmi_last_error.restype = ctypes.c_char_p
    rc = lib.ttmi_mono_loss_fwd(None, 0, ctypes.c_long(5), None, None, None, 1, 1, 1, 5, 0, None, None, None)
    assert rc < 0 and b"mono_loss_fwd: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_mono_loss_bwd(None, 0, ctypes.c_long(5), None, None, None, 1, 1, 1, 5, 0, None, None, 0, ctypes.c_float(1.0), None,
                                ctypes.c_long(5), None)
    assert rc < 0 and b"mono_loss_bwd: null pointer" in lib.ttmi_last_error()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    args = lambda **kw: [p, kw.get("dtype", 0), ctypes.c_long(kw.get("ldv", 5)), p, p, p, 1, 1, kw.get("U1", 1), 5, kw.get("blank", 0)]
    for kw, msg in (({"blank": 5}, b"blank 5 outside [0,5)"), ({"U1": 1025}, b"> 1024 unsupported"), ({"ldv": 4}, b"bad pitch/dtype"),
                    ({"dtype": 2}, b"bad pitch/dtype")):
        assert lib.ttmi_mono_loss_fwd(*args(**kw), p, p, None) < 0 and msg in lib.ttmi_last_error(), kw
        assert lib.ttmi_mono_loss_bwd(*args(**kw), p, p, 0, ctypes.c_float(1.0), p, ctypes.c_long(5), None) < 0
        assert msg in lib.ttmi_last_error(), kw
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.ttmi_mono_loss_fwd(*args(), odd, p, None) < 0 and b"8-byte aligned" in lib.ttmi_last_error()


def test_workspace_bytes():
    lib = _lib()
    lib.ttmi_mono_workspace_bytes.restype = ctypes.c_size_t
    n = lib.ttmi_mono_workspace_bytes(2, 10, 4)
    assert n >= 8 * (2 * 2 * 11 * 4 + 2) + 4 * 3 * 2 * 10 * 4          # alpha, beta for t = 0 .. T, ll; lse and the two emission tables
    assert lib.ttmi_mono_workspace_bytes(0, 10, 4) == 0


def test_option_value_errors():
    import torch
    from warprnnt_pytorch import RNNTLoss, rnnt_loss
    with pytest.raises(ValueError, match="topology"):
        RNNTLoss(topology="x")
    with pytest.raises(ValueError, match="fastemit"):
        RNNTLoss(topology="monotonic", fastemit_lambda=0.01)
    assert RNNTLoss().topology == "rnnt" and RNNTLoss(topology="monotonic").topology == "monotonic"
    cpu = (torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        RNNTLoss(topology="monotonic")(*cpu)
    with pytest.raises(ValueError, match="topology"):
        rnnt_loss(*cpu, topology="ctc")


def test_topology_key_reaches_the_training_driver():
    src = open(os.path.join(PKG, "ttmi", "dp_train.py")).read()
    assert "config.training.get('loss_topology', 'rnnt')" in src and "topology=topology" in src


def test_ops_fail_loudly_without_device():
    import torch
    from ttmi import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.mono_loss_fwd(torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, dtype=torch.int32), i32(2), i32(1), 0, torch.zeros(64))
    with pytest.raises(ValueError):
        ops.mono_loss_bwd(torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, dtype=torch.int32), i32(2), i32(1), 0, torch.zeros(64), torch.ones(1), 0, 1.0)
    assert ops.check_topology("monotonic") == "monotonic"
