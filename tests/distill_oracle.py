"""Float64 reference of the distillation on collapsed lattice posteriors (include/ttmi.h, csrc/distill.hip), in numpy, plus the same cost in
torch so that autograd can be held against the hand-written gradient.

A node (t, u) of utterance b, t < T_b, u <= U_b (lengths clamped as the kernels clamp them), with z = logits[b, t, u, :]:
    lb = z[blank] - lse(z),  ly = z[y] - lse(z) with y = labels[b][u],  lo = lse(z[k], k not in {blank, y}) - lse(z)
each clamped below at NEG; the label class is empty (ly = NEG, and nothing but `blank` is left out of lo) at u == U_b and for y == blank.
    kd = sum_c P^T_c (log P^T_c - log P^S_c) over the classes with P^T_c > 0
    d kd / d z[k] = s_k - P^T_b (k == blank),  s_k - P^T_y (k == y, label class not empty),  s_k (1 - c_o) otherwise,
    c_o = P^T_o / P^S_o, taken as 0 when the other class is empty on either side.

`defect` plants one mistake a kernel could make (tests/test_distill_oracle.py shows that each is visible at the bound the GPU tests use)."""
import numpy as np

NEG = float(np.float32(-1e30))
DEFECTS = ("label_prev", "other_sub_f32", "count_t_Tb", "label_at_Ub", "other_on_blank")


def lengths(tl, ul, T, U1):
    return np.clip(np.asarray(tl, dtype=np.int64), 1, T), np.clip(np.asarray(ul, dtype=np.int64), 0, U1 - 1)


def lse(v):
    if v.size == 0:
        return -np.inf
    m = v.max()
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.exp(v - m).sum()))


def _floor(x):
    return NEG if x < NEG else x


def label_of(labels, b, u, Ub, V, blank, defect=None):
    """-> the column of the label class at node (., u) of utterance b, or -1 when the class is empty"""
    lab = np.asarray(labels).reshape(len(Ub), -1)
    if defect == "label_at_Ub" and u == Ub[b] and u < lab.shape[1]:
        y = int(np.clip(lab[b, u], 0, V - 1))
        return -1 if y == blank else y
    if u >= Ub[b]:
        return -1
    y = int(np.clip(lab[b, max(u - 1, 0) if defect == "label_prev" else u], 0, V - 1))
    return -1 if y == blank else y


def collapse_row(z, y, blank, defect=None):
    """z f64 [V], y the label column or -1 -> (lse, lb, ly, lo)"""
    l = lse(z)
    keep = np.ones(z.shape[0], dtype=bool)
    keep[blank] = False
    if y >= 0:
        keep[y] = False
    lb = _floor(z[blank] - l)
    ly = _floor(z[y] - l) if y >= 0 else NEG
    if defect == "other_sub_f32":           # the other mass as 1 - p_b - p_y in float32
        po = np.float32(1.0) - np.float32(np.exp(lb)) - (np.float32(np.exp(ly)) if y >= 0 else np.float32(0.0))
        lo = _floor(float(np.log(np.float64(po)))) if po > 0 else NEG
    else:
        lo = _floor(lse(z[keep]) - l)
    return l, lb, ly, lo


def collapse(x, labels, tl, ul, blank=0, defect=None):
    """x f64 [B, T, U1, V] -> post f64 [B, T, U1, 3], zeros outside the ragged lattice"""
    x = np.asarray(x, dtype=np.float64)
    B, T, U1, V = x.shape
    Tb, Ub = lengths(tl, ul, T, U1)
    post = np.zeros((B, T, U1, 3))
    for b in range(B):
        for t in range(Tb[b]):
            for u in range(Ub[b] + 1):
                post[b, t, u] = collapse_row(x[b, t, u], label_of(labels, b, u, Ub, V, blank, defect), blank, defect)[1:]
    return post


def kd_row(z, tp, y, blank, defect=None):
    """one node: z f64 [V], tp the teacher's (lb, ly, lo) -> (cost, gradient [V], c_o)"""
    l, lb, ly, lo = collapse_row(z, y, blank, defect)
    s = np.exp(z - l)
    pb, po = np.exp(tp[0]), np.exp(tp[2])
    py = np.exp(tp[1]) if y >= 0 else 0.0
    cost = 0.0
    for p, a, c in ((pb, tp[0], lb), (py, tp[1], ly), (po, tp[2], lo)):
        if p != 0.0:
            cost += p * (a - c)
    co = 0.0 if (tp[2] <= NEG or lo <= NEG) else np.exp(tp[2] - lo)
    g = s * (1.0 - co)
    g[blank] = s[blank] * (1.0 - co) if defect == "other_on_blank" else s[blank] - pb
    if y >= 0:
        g[y] = s[y] - py
    return cost, g, co


def kd_loss(x, teacher, labels, tl, ul, blank=0, defect=None):
    """-> (costs f64 [B], d costs[b] / d x[b] f64 [B, T, U1, V] with zero rows outside the lattice, c_o f64 [B, T, U1])"""
    x = np.asarray(x, dtype=np.float64)
    teacher = np.asarray(teacher, dtype=np.float64)
    B, T, U1, V = x.shape
    Tb, Ub = lengths(tl, ul, T, U1)
    costs, grad, coef = np.zeros(B), np.zeros_like(x), np.zeros((B, T, U1))
    for b in range(B):
        frames = min(T, Tb[b] + 1) if defect == "count_t_Tb" else Tb[b]
        for t in range(frames):
            for u in range(Ub[b] + 1):
                c, g, co = kd_row(x[b, t, u], teacher[b, t, u], label_of(labels, b, u, Ub, V, blank, defect), blank, defect)
                costs[b] += c
                grad[b, t, u] = g
                coef[b, t, u] = co
    return costs, grad, coef


def kd_loss_torch(x, teacher, labels, tl, ul, blank=0):
    """the same cost written with torch ops on a float64 tensor x (which may require grad) -> costs [B]"""
    import torch
    B, T, U1, V = x.shape
    Tb, Ub = lengths(tl, ul, T, U1)
    teacher = torch.as_tensor(np.asarray(teacher), dtype=torch.float64)
    neg = torch.tensor(NEG, dtype=torch.float64)
    costs = []
    for b in range(B):
        c = torch.zeros((), dtype=torch.float64)
        for t in range(Tb[b]):
            for u in range(Ub[b] + 1):
                z = x[b, t, u]
                y = label_of(labels, b, u, Ub, V, blank)
                l = torch.logsumexp(z, 0)
                keep = torch.ones(V, dtype=torch.bool)
                keep[blank] = False
                if y >= 0:
                    keep[y] = False
                ls = [z[blank] - l, (z[y] - l) if y >= 0 else neg, (torch.logsumexp(z[keep], 0) - l) if bool(keep.any()) else neg]
                for k in range(3):
                    tp = teacher[b, t, u, k]
                    p = torch.exp(tp) if (k != 1 or y >= 0) else torch.zeros((), dtype=torch.float64)
                    if float(p) != 0.0:
                        c = c + p * (tp - torch.maximum(ls[k], neg))
        costs.append(c)
    return torch.stack(costs)


def full_kl_row(zt, zs):
    """KL(softmax(zt) || softmax(zs)) over all V outputs of one node"""
    lt, ls = zt - lse(zt), zs - lse(zs)
    return float((np.exp(lt) * (lt - ls)).sum())
