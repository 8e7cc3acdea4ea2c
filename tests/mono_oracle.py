"""Float64 reference of the monotonic RNN-T loss (include/ttmi.h, "monotonic RNN-T loss"; Tripathi et al. 2019): every frame makes exactly one
decision, blank or one label, and the emitting frame is consumed.  Three independent statements of it:

    mono_loss         the alpha / beta recursion in numpy -> costs and the analytic gradient w.r.t. the logits
    brute_force_cost  the sum over the C(T, U) sets of emitting frames, path by path
    autograd_loss     the alpha recursion in torch float64; the gradient is torch autograd's

No GPU, no library code."""
import itertools

import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def emissions(lp, y, U, blank):
    """lp [T, >=U+1, V] -> lpb [T, U+1] = lp[t, u, blank], lpl [T, U] = lp[t, u, y[u]]"""
    lpb = lp[:, :U + 1, blank]
    lpl = lp[:, np.arange(U), y[:U]] if U > 0 else np.zeros((lp.shape[0], 0))
    return lpb, lpl


def lattice(lpb, lpl):
    """-> alpha, beta [T+1, U+1], ll.  alpha(t, u) = log-probability of having emitted u labels in the first t frames; beta(t, u) = of emitting the
    other U - u in the frames t .. T-1"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    alpha = np.full((T + 1, U + 1), -np.inf)
    beta = np.full((T + 1, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    beta[T, U] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            move = np.full(U + 1, -np.inf)
            move[1:] = alpha[t, :-1] + lpl[t]
            alpha[t + 1] = np.logaddexp(alpha[t] + lpb[t], move)
        for t in range(T - 1, -1, -1):
            move = np.full(U + 1, -np.inf)
            move[:-1] = lpl[t] + beta[t + 1, 1:]
            beta[t] = np.logaddexp(lpb[t] + beta[t + 1], move)
    return alpha, beta, alpha[T, U]


def mono_loss(x, labels, act_lens, label_lens, blank=0):
    """x [B, T, U1, V] -> (costs f64 [B], grad f64 [B, T, U1, V] = d costs[b] / d x[b]).  Lengths and labels are clamped as the library clamps
    them.  An utterance with U_b > T_b has no path: cost +inf, gradient rows zero."""
    x = np.asarray(x, dtype=np.float64)
    B, T, U1, V = x.shape
    labels = np.clip(np.asarray(labels).reshape(B, -1), 0, V - 1)
    costs, grad = np.zeros(B), np.zeros_like(x)
    for b in range(B):
        Tb, Ub = int(np.clip(act_lens[b], 1, T)), int(np.clip(label_lens[b], 0, U1 - 1))
        lp = log_softmax(x[b, :Tb, :Ub + 1])
        y = labels[b]
        lpb, lpl = emissions(lp, y, Ub, blank)
        alpha, beta, ll = lattice(lpb, lpl)
        costs[b] = -ll
        if not np.isfinite(ll):
            continue
        with np.errstate(invalid="ignore"):
            occ = np.exp(alpha[:Tb] + beta[:Tb] - ll)
            eb = np.exp(alpha[:Tb] + lpb + beta[1:] - ll)
            el = np.exp(alpha[:Tb, :Ub] + lpl + beta[1:, 1:] - ll)
        occ, eb, el = (np.nan_to_num(v, nan=0.0) for v in (occ, eb, el))          # (-inf) - (-inf) of two dead cells
        g = np.exp(lp) * occ[..., None]
        g[..., blank] -= eb
        for u in range(Ub):
            g[:, u, y[u]] -= el[:, u]
        grad[b, :Tb, :Ub + 1] = g
    return costs, grad


def brute_force_cost(x, y, T, U, blank=0):
    """one utterance, x [>=T, >=U+1, V]: -log of the sum over every set of U emitting frames of the path's probability"""
    lp = log_softmax(np.asarray(x, dtype=np.float64)[:T, :U + 1])
    total = -np.inf
    for emit in itertools.combinations(range(T), U):
        u, s = 0, 0.0
        for t in range(T):
            if u < U and emit[u] == t:
                s += lp[t, u, y[u]]
                u += 1
            else:
                s += lp[t, u, blank]
        total = np.logaddexp(total, s)
    return -total


def autograd_loss(x, labels, act_lens, label_lens, blank=0):
    """the alpha recursion cell by cell in torch float64 (unreachable cells are left out instead of carried as -inf) -> (costs [B], grad
    [B, T, U1, V] from torch.autograd); utterances without a path get cost +inf and zero rows"""
    import torch
    xd = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    B, T, U1, V = xd.shape
    labels = np.clip(np.asarray(labels).reshape(B, -1), 0, V - 1)
    costs = []
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        lp = torch.log_softmax(xd[b], -1)
        row = {0: torch.zeros((), dtype=torch.float64)}
        for t in range(Tb):
            new = {}
            for u in range(Ub + 1):
                terms = []
                if u in row:
                    terms.append(row[u] + lp[t, u, blank])
                if u > 0 and u - 1 in row:
                    terms.append(row[u - 1] + lp[t, u - 1, int(labels[b, u - 1])])
                if terms:
                    new[u] = torch.logsumexp(torch.stack(terms), 0)
            row = new
        costs.append(-row[Ub] if Ub in row else None)
    live = [c for c in costs if c is not None]
    if live:
        torch.stack(live).sum().backward()
    grad = xd.grad.numpy() if xd.grad is not None else np.zeros(xd.shape)
    return np.array([np.inf if c is None else float(c.detach()) for c in costs]), grad
