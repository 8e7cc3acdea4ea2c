"""FastEmit latency regularisation of the RNN-T loss (Yu et al., ICASSP 2021), CPU side: the public argument and its validation, the C ABI's
_fe entry points, and the float64 reference the GPU tests (tests/test_fastemit_gpu.py) measure against.

The contract (include/ttmi.h): the cost stays -log P(y|x); the gradient of the logits is the plain gradient w.r.t. the log-probs with its
label-emission entries scaled by (1 + lambda), chained through log_softmax:
    dz[k] = g * (softmax_k * (occ + lambda e_l) - [k == blank] e_b - [k == y_{u+1}] (1 + lambda) e_l)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, rel_err

FE_ENTRIES = ("ttmi_rnnt_loss_bwd_fe", "ttmi_rnnt_loss_bwd_split_fe", "ttmi_rnnt_loss_bwd_exp_fe")


# ----------------------------------------------------------------------------- float64 reference
def _lae(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def _lattice(lpb, lpl, Tb, Ub):
    """alpha, beta [Tb, Ub + 1] and ll from the blank / label log-probs of one utterance (lpl [Tb, Ub])"""
    alpha = np.full((Tb, Ub + 1), -np.inf)
    beta = np.full((Tb, Ub + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t or u:
                alpha[t, u] = _lae(alpha[t - 1, u] + lpb[t - 1, u] if t else -math.inf,
                                   alpha[t, u - 1] + lpl[t, u - 1] if u else -math.inf)
    beta[Tb - 1, Ub] = lpb[Tb - 1, Ub]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t < Tb - 1 or u < Ub:
                beta[t, u] = _lae(beta[t + 1, u] + lpb[t, u] if t < Tb - 1 else -math.inf,
                                  beta[t, u + 1] + lpl[t, u] if u < Ub else -math.inf)
    return alpha, beta, alpha[Tb - 1, Ub] + lpb[Tb - 1, Ub]


def fastemit_ref(logits, labels, act_lens, label_lens, blank=0, fastemit_lambda=0.0, grad_scale=None, delta=False):
    """-> (costs [B] = -log P(y|x), d sum_b(grad_scale[b] * cost_b) / d logits with FastEmit), all float64.
    grad_scale: per-utterance g (default 1).  delta=True: only the FastEmit part of the gradient, grad(lambda) - grad(0)
    = g lambda e_l (softmax - onehot(y_{u+1})) (what the bf16 exp-domain test compares)."""
    x = np.asarray(logits)
    B, T, U1, V = x.shape
    g_b = np.ones(B) if grad_scale is None else np.asarray(grad_scale, dtype=np.float64)
    lam = float(fastemit_lambda)
    costs = np.zeros(B)
    grad = np.zeros(x.shape, dtype=np.float64)
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        z = x[b, :Tb, :Ub + 1].astype(np.float64)
        m = z.max(-1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(-1, keepdims=True))
        sm = np.exp(z - lse)
        y = np.asarray(labels[b][:Ub], dtype=np.int64)
        lpb = z[:, :, blank] - lse[..., 0]
        lpl = (np.take_along_axis(z[:, :Ub, :], np.broadcast_to(y[None, :, None], (Tb, Ub, 1)), -1)[..., 0] - lse[:, :Ub, 0]) if Ub else \
            np.zeros((Tb, 0))
        alpha, beta, ll = _lattice(lpb, lpl, Tb, Ub)
        costs[b] = -ll
        occ = np.exp(alpha + beta - ll)
        eb = np.zeros((Tb, Ub + 1))
        eb[:Tb - 1] = np.exp(alpha[:Tb - 1] + lpb[:Tb - 1] + beta[1:] - ll)
        eb[Tb - 1, Ub] = np.exp(alpha[Tb - 1, Ub] + lpb[Tb - 1, Ub] - ll)
        el = np.zeros((Tb, Ub + 1))
        if Ub:
            el[:, :Ub] = np.exp(alpha[:, :Ub] + lpl + beta[:, 1:] - ll)
        if delta:
            gr = sm * (lam * el)[..., None]
        else:
            gr = sm * (occ + lam * el)[..., None]
            gr[:, :, blank] -= eb
        tt, uu = np.meshgrid(np.arange(Tb), np.arange(Ub), indexing="ij")
        if Ub:
            np.subtract.at(gr, (tt.ravel(), uu.ravel(), np.broadcast_to(y[None, :], (Tb, Ub)).ravel()),
                           ((lam if delta else 1.0 + lam) * el[:, :Ub]).ravel())
        grad[b, :Tb, :Ub + 1] = g_b[b] * gr
    return costs, grad


# ----------------------------------------------------------------------------- public argument
def test_rnnt_loss_accepts_and_validates_fastemit_lambda():
    from warprnnt_pytorch import RNNTLoss, rnnt_loss
    assert RNNTLoss(fastemit_lambda=0.01).fastemit_lambda == 0.01
    assert RNNTLoss().fastemit_lambda == 0.0
    assert RNNTLoss(blank=3, reduction="sum", fastemit_lambda=1).fastemit_lambda == 1.0
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), "fast", None):
        with pytest.raises(ValueError):
            RNNTLoss(fastemit_lambda=bad)
    with pytest.raises(ValueError):
        rnnt_loss(torch.zeros(1, 2, 2, 4), torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32),
                  torch.ones(1, dtype=torch.int32), fastemit_lambda=-0.5)
    with pytest.raises(TypeError):
        RNNTLoss(0, "mean", None, 0.01)                  # keyword-only: positional calls keep their meaning
    import inspect
    from tt.model import Transducer
    for fn in (Transducer.loss, rnnt_loss):
        p = inspect.signature(fn).parameters["fastemit_lambda"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0.0


def test_fastemit_key_reaches_the_training_driver():
    src = open(os.path.join(PKG, "ttmi", "dp_train.py")).read()
    assert re.search(r"RNNTLoss\(fastemit_lambda=config\.training\.get\('fastemit_lambda', 0\.0\)\)", src)


# ----------------------------------------------------------------------------- C ABI
def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_fe_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ttmi.h")).read()
    lib = _lib()
    for n in FE_ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % n, hdr)
        assert decl, n
        args = [a.strip() for a in decl.group(1).split(",")]
        assert args[-2] == "float fastemit_lambda" and args[-1] == "void* stream", (n, args[-2:])
        assert hasattr(lib, n), n


def _call(lib, name, null, lam):
    """the _fe entry with every pointer null (null=True) or pointing at a small host buffer (never dereferenced: validation fails first)"""
    buf = (ctypes.c_char * 64)()
    p = None if null else ctypes.cast(buf, ctypes.c_void_p)
    L, F, I = ctypes.c_long, ctypes.c_float, ctypes.c_int
    if name == "ttmi_rnnt_loss_bwd_fe":
        return lib.ttmi_rnnt_loss_bwd_fe(p, I(0), L(8), p, p, p, I(1), I(2), I(2), I(8), I(0), p, p, I(0), F(1.0), p, L(8), F(lam), None)
    if name == "ttmi_rnnt_loss_bwd_split_fe":
        return lib.ttmi_rnnt_loss_bwd_split_fe(p, L(64), p, p, p, I(1), I(2), I(2), I(8), I(0), p, p, I(0), F(1.0), F(lam), None)
    return lib.ttmi_rnnt_loss_bwd_exp_fe(p, L(64), p, p, p, I(1), I(2), I(2), I(8), I(0), p, p, I(0), F(1.0), p, p, F(lam), None)


@pytest.mark.parametrize("name", FE_ENTRIES)
def test_fe_entries_validate_without_gpu(name):
    lib = _lib()
    rc = _call(lib, name, True, 0.01)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    for bad in (-0.25, float("nan"), float("inf")):
        rc = _call(lib, name, False, bad)
        assert rc < 0 and b"fastemit_lambda" in lib.ttmi_last_error(), (name, bad)


# ----------------------------------------------------------------------------- the reference against autograd
def _autograd(x, labels, act_lens, label_lens, blank, lam, g_b):
    """torch float64: -ll by the alpha recursion over gathered blank / label log-probs; autograd gives d(-ll)/d lp_blank and d(-ll)/d lp_label,
    the label part is scaled by (1 + lambda) and chained through the gather and log_softmax"""
    z = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(z, -1)
    B = x.shape[0]
    total = torch.zeros((), dtype=torch.float64)
    pb_list, pl_list, costs = [], [], []
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        pb = lp[b, :Tb, :Ub + 1, blank]
        y = torch.tensor(np.asarray(labels[b][:Ub], dtype=np.int64))
        pl = lp[b, :Tb, :Ub].gather(-1, y.view(1, Ub, 1).expand(Tb, Ub, 1))[..., 0] if Ub else lp.new_zeros(Tb, 0)
        a = [[None] * (Ub + 1) for _ in range(Tb)]
        for t in range(Tb):
            for u in range(Ub + 1):
                if t == 0 and u == 0:
                    a[t][u] = torch.zeros((), dtype=torch.float64)
                    continue
                terms = []
                if t:
                    terms.append(a[t - 1][u] + pb[t - 1, u])
                if u:
                    terms.append(a[t][u - 1] + pl[t, u - 1])
                a[t][u] = torch.logsumexp(torch.stack(terms), 0)
        nll = -(a[Tb - 1][Ub] + pb[Tb - 1, Ub])
        costs.append(float(nll.detach()))
        total = total + g_b[b] * nll
        pb_list.append(pb)
        pl_list.append(pl)
    outs = [(t_, 1.0) for t_ in pb_list] + [(t_, 1.0 + lam) for t_ in pl_list if t_.requires_grad]
    gs = torch.autograd.grad(total, [t_ for t_, _ in outs], allow_unused=True)
    grads = [(gi if gi is not None else torch.zeros_like(t_)) * f for (t_, f), gi in zip(outs, gs)]
    outs = [t_ for t_, _ in outs]
    dz, = torch.autograd.grad(outs, z, grads, allow_unused=True)
    return np.array(costs), dz.numpy()


CASES = [  # B, T, U, V, blank, ragged
    (3, 5, 3, 6, 0, True),
    (2, 4, 4, 5, 3, True),
    (1, 3, 0, 4, 1, False),
]


@pytest.mark.parametrize("lam", [0.0, 1e-3, 0.5])
@pytest.mark.parametrize("B,T,U,V,blank,ragged", CASES)
def test_reference_matches_torch_autograd(B, T, U, V, blank, ragged, lam):
    rng = np.random.default_rng(100 * B + 10 * T + U)
    x = rng.normal(size=(B, T, U + 1, V)) * 1.5
    y = rng.integers(0, V, size=(B, U))
    tl, ul = np.full(B, T), np.full(B, U)
    if ragged:
        tl[-1], ul[-1] = T - 1, 0                         # one utterance with U_b = 0
        if B > 2:
            tl[1], ul[1] = T - 2, U - 1
    if U:
        y[0, 1 % U] = blank                               # one label equal to blank: both emission terms in one column
    g_b = 0.5 + rng.random(B)
    costs, grad = fastemit_ref(x, y, tl, ul, blank, lam, g_b)
    want_costs, want = _autograd(x, y, tl, ul, blank, lam, g_b)
    assert np.abs(costs - want_costs).max() < 1e-12 * np.abs(want_costs).max()
    assert rel_err(grad, want) < 1e-12
    assert np.abs(grad.sum(-1)).max() < 1e-13               # every row sums to zero
    d = fastemit_ref(x, y, tl, ul, blank, lam, g_b, delta=True)[1]
    assert rel_err(d, grad - fastemit_ref(x, y, tl, ul, blank, 0.0, g_b)[1]) < 1e-12
    if lam == 0.0:
        from oracle.rnnt_c import rnnt_loss_c
        _, c_costs, c_grad = rnnt_loss_c(x.astype(np.float32), y, tl, ul, blank=blank, reduction="sum")
        assert rel_err(c_costs, costs) < 1e-5
        assert rel_err(c_grad, grad / g_b[:, None, None, None]) < 1e-5
    elif ul.max() > 0:
        assert rel_err(grad, fastemit_ref(x, y, tl, ul, blank, 0.0, g_b)[1]) > 1e-4 * lam     # lambda changes the gradient
    else:
        assert np.array_equal(grad, fastemit_ref(x, y, tl, ul, blank, 0.0, g_b)[1])          # no label anywhere: nothing to favour
