"""Float64 reference of the token-and-duration transducer (include/ttmi.h, "token-and-duration transducer"; Xu et al., ICML 2023): a row is V
token logits followed by D duration logits, each sub-row normalised by itself; a decision is a token (blank or the next label) together with
the number of frames it consumes, and a path lands exactly on frame T.  Three independent statements of the loss:

    tdt_loss          the alpha / beta recursion in numpy -> costs and the analytic gradient w.r.t. the logits
    brute_force_cost  the sum over every sequence of (token, duration) decisions, path by path
    autograd_loss     the alpha recursion in torch float64; the gradient is torch autograd's

and tdt_cost_vectorised (the alpha recursion alone, vectorised over u, for long lattices) and greedy_decode (the decoder's rule).  The
`defect` arguments plant one known mistake each: tests/test_tdt_oracle.py shows that the GPU tests' bounds would catch it.

No GPU, no library code."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def split_rows(x, V, D, defect=None):
    """x [..., >= V + D] -> (lt [..., V], ld [..., D]), each sub-row normalised by itself"""
    x = np.asarray(x, dtype=np.float64)
    if defect == "joint_norm":                   # planted: the duration sub-row normalised together with the tokens
        lp = log_softmax(x[..., :V + D])
        return lp[..., :V], lp[..., V:]
    return log_softmax(x[..., :V]), log_softmax(x[..., V:V + D])


def emissions(lt, y, U, blank):
    """lt [T, >= U+1, V] -> lpb [T, U+1] = lt[t, u, blank], lpl [T, U] = lt[t, u, y[u]]"""
    lpb = lt[:, :U + 1, blank]
    lpl = lt[:, np.arange(U), y[:U]] if U > 0 else np.zeros((lt.shape[0], 0))
    return lpb, lpl


def lattice(lpb, lpl, ld, durations, defect=None):
    """lpb [T, U+1], lpl [T, U], ld [T, U+1, D] -> alpha, beta [T+1, U+1], ll"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    alpha = np.full((T + 1, U + 1), -np.inf)
    beta = np.full((T + 1, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    beta[T, U] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(1, T + 1):
            acc = np.full(U + 1, -np.inf)
            for s in range(max(0, t - 8), t):
                for j, d in enumerate(durations):
                    hit = s + d == t
                    if defect == "clip" and t == T and s + d > T:      # planted: an overshooting move clipped to T_b instead of dropped
                        hit = True
                    if not hit:
                        continue
                    acc = np.logaddexp(acc, alpha[s] + lpb[s] + ld[s, :, j])
                    move = np.full(U + 1, -np.inf)
                    move[1:] = alpha[s, :-1] + lpl[s] + ld[s, :-1, j]
                    acc = np.logaddexp(acc, move)
            alpha[t] = acc
        for t in range(T - 1, -1, -1):
            acc = np.full(U + 1, -np.inf)
            for j, d in enumerate(durations):
                if t + d > T:
                    continue
                nxt = beta[t + 1] if defect == "beta_plus_1" else beta[t + d]      # planted: beta(t+1, .) in place of beta(t+d, .)
                acc = np.logaddexp(acc, lpb[t] + ld[t, :, j] + nxt)
                move = np.full(U + 1, -np.inf)
                move[:-1] = lpl[t] + ld[t, :-1, j] + nxt[1:]
                acc = np.logaddexp(acc, move)
            beta[t] = acc
    return alpha, beta, alpha[T, U]


def tdt_loss(x, labels, act_lens, label_lens, durations, blank=0, defect=None, return_lattice=False):
    """x [B, T, U1, >= V + D] with V = x.shape[-1] - D -> (costs f64 [B], grad f64 [B, T, U1, V + D] = d costs[b] / d x[b]).  Lengths and labels
    are clamped as the library clamps them.  An utterance without a path has cost +inf and zero gradient rows."""
    x = np.asarray(x, dtype=np.float64)
    B, T, U1, W = x.shape
    D = len(durations)
    V = W - D
    labels = np.clip(np.asarray(labels).reshape(B, -1), 0, V - 1)
    costs, grad = np.zeros(B), np.zeros_like(x)
    lats = []
    for b in range(B):
        Tb, Ub = int(np.clip(act_lens[b], 1, T)), int(np.clip(label_lens[b], 0, U1 - 1))
        lt, ld = split_rows(x[b, :Tb, :Ub + 1], V, D, defect)
        y = labels[b]
        lpb, lpl = emissions(lt, y, Ub, blank)
        alpha, beta, ll = lattice(lpb, lpl, ld, durations, defect)
        lats.append((alpha, beta))
        costs[b] = -ll
        if not np.isfinite(ll):
            continue
        # e_b,j / e_l,j of every move that exists; E_j = e_b,j + e_l,j; occ = sum_j E_j, which is exp(alpha + beta - ll) (the moves out of a
        # node carry its whole occupation: tests/test_tdt_oracle.py compares the two).  Formed this way the duration gradient of a lattice
        # with one duration, softmax_dur * occ - E_0 = 1 * E_0 - E_0, is an exact zero.
        eb, el = np.zeros((Tb, Ub + 1, D)), np.zeros((Tb, Ub + 1, D))
        with np.errstate(invalid="ignore"):
            for j, d in enumerate(durations):
                for t in range(Tb):
                    if t + d > Tb:
                        continue
                    eb[t, :, j] = np.nan_to_num(np.exp(alpha[t] + lpb[t] + ld[t, :, j] + beta[t + d] - ll), nan=0.0)
                    el[t, :Ub, j] = np.nan_to_num(np.exp(alpha[t, :Ub] + lpl[t] + ld[t, :Ub, j] + beta[t + d, 1:] - ll), nan=0.0)
            occ_ab = np.nan_to_num(np.exp(alpha[:Tb] + beta[:Tb] - ll), nan=0.0)
        Ej = eb + el
        occ = Ej.sum(-1)
        g = np.zeros((Tb, Ub + 1, W))
        g[..., :V] = np.exp(lt) * occ[..., None]
        g[..., blank] -= eb.sum(-1)
        for u in range(Ub):
            g[:, u, y[u]] -= el[:, u].sum(-1)
        g[..., V:] = np.exp(ld) * occ[..., None] - (eb if defect == "dur_no_label" else Ej)      # planted: the label share missing
        grad[b, :Tb, :Ub + 1] = g
        lats[-1] += (occ, occ_ab)
    if return_lattice:
        return costs, grad, lats
    return costs, grad


def tdt_cost_vectorised(x, y, T, U, durations, blank=0):
    """one utterance, x [>= T, >= U+1, V + D]: the cost by the alpha recursion alone, vectorised over u (for long lattices)"""
    D = len(durations)
    V = np.asarray(x).shape[-1] - D
    lt, ld = split_rows(np.asarray(x)[:T, :U + 1], V, D)
    lpb, lpl = emissions(lt, np.clip(np.asarray(y), 0, V - 1), U, blank)
    alpha = np.full((T + 1, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(1, T + 1):
            acc = np.full(U + 1, -np.inf)
            for j, d in enumerate(durations):
                s = t - d
                if s < 0:
                    continue
                acc = np.logaddexp(acc, alpha[s] + lpb[s] + ld[s, :, j])
                acc[1:] = np.logaddexp(acc[1:], alpha[s, :-1] + lpl[s] + ld[s, :-1, j])
            alpha[t] = acc
    return -alpha[T, U]


def brute_force_cost(x, y, T, U, durations, blank=0):
    """one utterance, x [>= T, >= U+1, V + D]: -log of the sum over every sequence of decisions that emits y[:U] and lands exactly on frame T"""
    D = len(durations)
    V = np.asarray(x).shape[-1] - D
    lt, ld = split_rows(np.asarray(x)[:T, :U + 1], V, D)
    total = [-np.inf]

    def walk(t, u, s):
        if t == T:
            if u == U:
                total[0] = np.logaddexp(total[0], s)
            return
        for j, d in enumerate(durations):
            if t + d > T:
                continue
            walk(t + d, u, s + lt[t, u, blank] + ld[t, u, j])
            if u < U:
                walk(t + d, u + 1, s + lt[t, u, y[u]] + ld[t, u, j])
    walk(0, 0, 0.0)
    return -total[0]


def autograd_loss(x, labels, act_lens, label_lens, durations, blank=0):
    """the alpha recursion cell by cell in torch float64 (unreachable cells are left out instead of carried as -inf) -> (costs [B], grad from
    torch.autograd); utterances without a path get cost +inf and zero rows"""
    import torch
    xd = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    B, T, U1, W = xd.shape
    D = len(durations)
    V = W - D
    labels = np.clip(np.asarray(labels).reshape(B, -1), 0, V - 1)
    costs = []
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        lt = torch.log_softmax(xd[b, :, :, :V], -1)
        ld = torch.log_softmax(xd[b, :, :, V:], -1)
        cells = {(0, 0): torch.zeros((), dtype=torch.float64)}
        for t in range(1, Tb + 1):
            for u in range(Ub + 1):
                terms = []
                for j, d in enumerate(durations):
                    s = t - d
                    if (s, u) in cells:
                        terms.append(cells[(s, u)] + lt[s, u, blank] + ld[s, u, j])
                    if u > 0 and (s, u - 1) in cells:
                        terms.append(cells[(s, u - 1)] + lt[s, u - 1, int(labels[b, u - 1])] + ld[s, u - 1, j])
                if terms:
                    cells[(t, u)] = torch.logsumexp(torch.stack(terms), 0)
        costs.append(-cells[(Tb, Ub)] if (Tb, Ub) in cells else None)
    live = [c for c in costs if c is not None]
    if live:
        torch.stack(live).sum().backward()
    grad = xd.grad.numpy() if xd.grad is not None else np.zeros(xd.shape)
    return np.array([np.inf if c is None else float(c.detach()) for c in costs]), grad


def greedy_decode(rows, T, durations, V, blank=0, defect=None):
    """The decoder's rule.  rows(t, tokens) -> the joint row (V + D values) of frame t against the label state of `tokens`.  At frame t:
    k* = argmax of the token sub-row, j* = argmax of the duration sub-row (the lowest index wins a tie), d = durations[j*]; the decision's
    log-probability is lt[k*] + ld[j*].  Blank: t += d.  Token: emitted on frame t, then t += d.  Ends when t >= T.
    -> (tokens, frames, logprobs (lt[k*] of every token), durations of the tokens, score, every decision's duration)"""
    D = len(durations)
    tokens, frames, lps, durs, taken = [], [], [], [], []
    t, score = 0, 0.0
    while t < T:
        z = np.asarray(rows(t, tokens), dtype=np.float64)
        lt, ld = log_softmax(z[:V]), log_softmax(z[V:V + D])
        k, j = int(np.argmax(z[:V])), int(np.argmax(z[V:V + D]))
        d = durations[j]
        score += lt[k] + ld[j]
        taken.append(d)
        if k != blank:
            tokens.append(k)
            frames.append(t)
            lps.append(float(lt[k]))
            durs.append(d)
            t += d
        else:
            t += 1 if defect == "blank_by_1" else d      # planted: a blank jump that advances by 1 instead of d
    return tokens, frames, lps, durs, score, taken
