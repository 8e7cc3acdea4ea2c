"""Float64 reference of forced alignment and emission statistics on the CTC lattice (include/ttmi.h, ttmi_ctc_align / ttmi_ctc_emit_stats),
working from log_softmax of the logits:

    extended         l' of one utterance (S = 2 U + 1 states, built literally: a label equal to `blank` is one more blank symbol) and the
                     skip mask: the s-2 move is allowed only when l'_s != blank and l'_s != l'_{s-2}
    tables           one utterance's logits -> lp [T, S] = log_softmax(x[t])[l'_s]
    viterbi_ref      v(0,0) = lp(0,0), v(0,1) = lp(0,1), v(t,s) = lp(t,s) + max(v(t-1,s), v(t-1,s-1), v(t-1,s-2)); predecessors tried in the
                     order s, s-1, s-2, a later one replacing an earlier one only when STRICTLY greater; the path ends in S-1 unless
                     v(T-1, S-2) is strictly greater -> (path [T], score); no feasible alignment: all -1, -inf
    spans_of         (first, last) frame of every label state of a path
    valid_path       is a state sequence a CTC alignment of the labels
    path_score       its log-probability
    lattice          alpha, beta (beta includes the emission at t, as the library's), ll
    emit_stats_ref   expected onset frame, onset mass, expected duration of every label, and the blank states' total occupancy
    brute_force      all of the above from the enumeration of every alignment (small lattices only)
    runner_up        the best score among the alignments that differ from a given one
    planted_batch    logits whose planted symbol leads every frame by `boost`

The `defect` arguments plant one wrong rule each (tests/test_ctc_align_oracle.py shows that every one of them is visible).  No GPU, no library
code."""
import numpy as np

DEFECTS = ("skip_across_repeat", "tie_later", "final_tie_s2", "onset_no_t0", "duration_no_lp")
NINF = -np.inf


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def extended(y, U, blank=0, defect=None):
    """-> (ext int64 [S], skip bool [S])"""
    ext = np.full(2 * U + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(y, dtype=np.int64)[:U]
    skip = np.zeros(2 * U + 1, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    if defect == "skip_across_repeat":
        skip[2:] = ext[2:] != blank
    return ext, skip


def tables(x, y, T, U, blank=0):
    """one utterance, x [>=T, V] -> (lp float64 [T, S], ext, skip)"""
    ext, skip = extended(y, U, blank)
    return log_softmax(np.asarray(x, dtype=np.float64)[:T])[:, ext], ext, skip


def _shift(v, n):
    out = np.full_like(v, NINF)
    out[n:] = v[:len(v) - n] if n else v
    return out


def viterbi_ref(lp, skip, defect=None):
    """-> (path int64 [T], score)"""
    T, S = lp.shape
    v = np.full((T, S), NINF)
    v[0, :min(S, 2)] = lp[0, :min(S, 2)]
    dec = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        best = v[t - 1].copy()
        d = np.zeros(S, dtype=np.int64)
        for n in (1, 2):
            c = _shift(v[t - 1], n)
            if n == 2:
                c = np.where(skip, c, NINF)
            take = (c >= best) & (c > NINF) if defect == "tie_later" else c > best
            best, d = np.where(take, c, best), np.where(take, n, d)
        v[t], dec[t] = lp[t] + best, d
    s = S - 1
    if S > 1 and (v[T - 1, S - 2] >= v[T - 1, S - 1] if defect == "final_tie_s2" else v[T - 1, S - 2] > v[T - 1, S - 1]):
        s = S - 2
    if not v[T - 1, s] > NINF:
        return np.full(T, -1, dtype=np.int64), NINF
    score, path = float(v[T - 1, s]), np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= dec[t, s]
    assert path[0] in (0, 1)
    return path, score


def spans_of(path, U):
    """-> int64 [U, 2]: (first, last) frame of state 2u+1 on the path, (-1, -1) for a label the path does not visit"""
    sp = np.full((U, 2), -1, dtype=np.int64)
    for t, s in enumerate(path):
        if s >= 0 and s % 2 == 1:
            u = s // 2
            if sp[u, 0] < 0:
                sp[u, 0] = t
            sp[u, 1] = t
    return sp


def valid_path(path, skip):
    """a CTC alignment: starts in state 0 or 1, ends in S-1 or S-2, every step stays, moves one state up, or two under the skip rule"""
    S, p = len(skip), [int(s) for s in path]
    if not p or p[0] not in (0, 1)[:S] or p[-1] not in ((S - 1, S - 2) if S > 1 else (0,)):
        return False
    return all(b - a in (0, 1) or (b - a == 2 and skip[b]) for a, b in zip(p, p[1:])) and all(0 <= s < S for s in p)


def path_score(lp, path):
    return float(lp[np.arange(len(path)), np.asarray(path, dtype=np.int64)].sum())


def lattice(lp, skip):
    """-> (alpha [T, S], beta [T, S], ll)"""
    T, S = lp.shape
    alpha, beta = np.full((T, S), NINF), np.full((T, S), NINF)
    alpha[0, :min(S, 2)] = lp[0, :min(S, 2)]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = lp[t] + np.logaddexp(np.logaddexp(a, _shift(a, 1)), np.where(skip, _shift(a, 2), NINF))
    beta[T - 1, max(S - 2, 0):] = lp[T - 1, max(S - 2, 0):]
    skip_out = np.zeros(S, dtype=bool)            # the move s -> s+2 is the skip rule of s+2
    skip_out[:S - 2] = skip[2:]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        up1, up2 = np.full(S, NINF), np.full(S, NINF)
        up1[:S - 1], up2[:S - 2] = b[1:], b[2:]
        beta[t] = lp[t] + np.logaddexp(np.logaddexp(b, up1), np.where(skip_out, up2, NINF))
    ll = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, 0]
    return alpha, beta, float(ll)


def emit_stats_ref(lp, skip, defect=None):
    """-> (expected [U], mass [U], duration [U], blank occupancy); no feasible alignment: -1 / 0 / 0 / 0"""
    T, S = lp.shape
    U = S // 2
    alpha, beta, ll = lattice(lp, skip)
    if not np.isfinite(ll):
        return np.full(U, -1.0), np.zeros(U), np.zeros(U), 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.nan_to_num(np.exp(alpha + beta - (0.0 if defect == "duration_no_lp" else lp) - ll), nan=0.0)
        lab = np.arange(1, S, 2)
        e = np.zeros((T, U))
        a = alpha[:-1]
        into = np.logaddexp(a[:, lab - 1], np.where(skip[lab], np.concatenate([np.full((T - 1, 1), NINF), a[:, lab[:-1]]], axis=1), NINF)) \
            if U else np.zeros((T - 1, 0))
        e[1:] = np.nan_to_num(np.exp(into + beta[1:, lab] - ll), nan=0.0)
        if U and defect != "onset_no_t0":
            e[0, 0] = g[0, 1]
    return (np.arange(T)[:, None] * e).sum(0), e.sum(0), g[:, 1::2].sum(0), float(g[:, 0::2].sum())


def all_paths(T, skip):
    """every CTC alignment of a small lattice, as state tuples"""
    S = len(skip)
    out = []

    def walk(p):
        if len(p) == T:
            if p[-1] in ((S - 1, S - 2) if S > 1 else (0,)):
                out.append(tuple(p))
            return
        s = p[-1]
        for n in (0, 1, 2):
            if s + n < S and (n < 2 or skip[s + n]):
                walk(p + [s + n])

    for s0 in range(min(S, 2)):
        walk([s0])
    return out


def brute_force(lp, skip):
    """-> dict(best, paths_at_best, ll, expected [U], mass [U], duration [U], blank) from the enumeration; None when no alignment exists"""
    T, S = lp.shape
    U = S // 2
    paths = all_paths(T, skip)
    if not paths:
        return None
    scores = np.array([path_score(lp, p) for p in paths])
    best = scores.max()
    post = np.exp(scores - best)
    post /= post.sum()
    expected, mass, duration, blank = np.zeros(U), np.zeros(U), np.zeros(U), 0.0
    for p, w in zip(paths, post):
        sp = spans_of(p, U)
        for u in range(U):
            assert sp[u, 0] >= 0                   # every alignment enters every label state
            mass[u] += w
            expected[u] += w * sp[u, 0]
            duration[u] += w * (sp[u, 1] - sp[u, 0] + 1)
        blank += w * sum(1 for s in p if s % 2 == 0)
    return dict(best=float(best), paths_at_best=[p for p, s in zip(paths, scores) if s == best],
                ll=float(best + np.log(np.exp(scores - best).sum())), expected=expected, mass=mass, duration=duration, blank=blank)


def runner_up(lp, skip, path):
    """the best score among the alignments that differ from `path`: such an alignment passes through a cell (t, s != path[t]), and the best
    alignment through a cell is forward-Viterbi + backward-Viterbi - lp there"""
    T, S = lp.shape
    f, b = np.full((T, S), NINF), np.full((T, S), NINF)
    f[0, :min(S, 2)] = lp[0, :min(S, 2)]
    for t in range(1, T):
        a = f[t - 1]
        f[t] = lp[t] + np.maximum(np.maximum(a, _shift(a, 1)), np.where(skip, _shift(a, 2), NINF))
    b[T - 1, max(S - 2, 0):] = lp[T - 1, max(S - 2, 0):]
    skip_out = np.zeros(S, dtype=bool)
    skip_out[:S - 2] = skip[2:]
    for t in range(T - 2, -1, -1):
        n = b[t + 1]
        up1, up2 = np.full(S, NINF), np.full(S, NINF)
        up1[:S - 1], up2[:S - 2] = n[1:], n[2:]
        b[t] = lp[t] + np.maximum(np.maximum(n, up1), np.where(skip_out, up2, NINF))
    with np.errstate(invalid="ignore"):
        through = np.nan_to_num(f + b - lp, nan=NINF)
    through[np.arange(T), np.asarray(path, dtype=np.int64)] = NINF
    return float(through.max())


def random_path(rng, T, skip):
    """a uniformly drawn valid move at every frame, kept feasible: from state s at frame t the end (S-2 or S-1) must stay reachable"""
    S = len(skip)
    need = np.zeros(S + 1, dtype=np.int64)         # fewest further frames from state s to the end, moving as fast as the skip rule allows
    need[S - 1] = 0
    if S > 1:
        need[S - 2] = 0
    for s in range(S - 3, -1, -1):
        need[s] = 1 + min(need[s + 1], need[s + 2] if skip[s + 2] else 1 << 30)
    if min(need[0], need[1] if S > 1 else 1 << 30) > T - 1:
        return None
    starts = [s for s in range(min(S, 2)) if need[s] <= T - 1]
    p = [int(rng.choice(starts))]
    for t in range(1, T):
        s = p[-1]
        moves = [s + n for n in (0, 1, 2) if s + n < S and (n < 2 or skip[s + n]) and need[s + n] <= T - 1 - t]
        p.append(int(rng.choice(moves)))
    assert valid_path(p, skip)
    return np.array(p, dtype=np.int64)


def planted_batch(seed, T, U, act_lens, label_lens, V=8, boost=8.0, noise=0.1, blank=0, labels=None):
    """-> (logits f32 [B, T, V], labels i32 [B, U], act_lens i32 [B], label_lens i32 [B], paths i64 [B, T]).  Per utterance a random alignment
    is drawn and the symbol of its state gets +boost at every frame over `noise`-sized values: that symbol leads the frame by about `boost`,
    and leaving the alignment costs about `boost` at the first wrong frame.  The noise sits at -boost, so the boosted logits sit at 0 and a
    planted frame's log-probability, about -(V - 1) e^-boost, is not drowned by the f32 rounding of x - lse in the library's emission table
    (tests/mono_align_oracle.py, planted_batch).  Labels are drawn from [1, V) with adjacent repeats now and then; an utterance without a
    feasible alignment gets noise alone and a path of -1."""
    rng = np.random.default_rng(seed)
    B = len(act_lens)
    x = (noise * rng.standard_normal((B, T, V)) - boost).astype(np.float32)
    if labels is None:
        labels = rng.integers(1, V, (B, U)).astype(np.int32)
        for b in range(B):
            for u in range(1, U):
                if rng.random() < 0.2:
                    labels[b, u] = labels[b, u - 1]
    labels = np.asarray(labels, dtype=np.int32).reshape(B, U)
    paths = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        ext, skip = extended(labels[b], Ub, blank)
        p = random_path(rng, Tb, skip)
        if p is None:
            continue
        paths[b, :Tb] = p
        x[b, np.arange(Tb), ext[p]] += boost
    return x, labels, np.asarray(act_lens, dtype=np.int32), np.asarray(label_lens, dtype=np.int32), paths
