"""Float64 reference of forced alignment and emission statistics on the monotonic lattice (include/ttmi.h, ttmi_mono_align / _emit_stats), on
top of tests/mono_oracle.py's log_softmax / emissions / lattice:

    viterbi_ref      v(0,0) = 0, v(t+1,u) = max(v(t,u) + lpb(t,u), v(t,u-1) + lpl(t,u-1)); the label move only when STRICTLY greater (a tie
                     goes to blank); backtrace from (T, U) backwards in time -> (frames [U], score); no path (U > T): all -1, -inf
    path_score       the log-probability of the path that emits label u+1 at frames[u]
    brute_force      the same maximum over every C(T, U) set of emitting frames, and the emission posterior from the same enumeration
    emit_stats_ref   mass / expected emission frame of every label from the oracle's alpha / beta
    second_best      the best score among the paths that leave a given path somewhere (the gap a planted path keeps to its neighbours)
    planted_batch    logits with +8 on the blank or label logit of every decision of a chosen strictly increasing path

No GPU, no library code."""
import itertools

import numpy as np

import mono_oracle as M


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    r = (a + np.uint32(0x7FFF) + ((a >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def tables(x, y, T, U, blank=0):
    """one utterance, x [>=T, >=U+1, V] -> lpb [T, U+1], lpl [T, U] in float64"""
    lp = M.log_softmax(np.asarray(x, dtype=np.float64)[:T, :U + 1])
    return M.emissions(lp, np.asarray(y), U, blank)


def viterbi_ref(lpb, lpl):
    """-> (frames int64 [U], score).  frames[u] = the frame whose one decision is label u+1, strictly increasing"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    if U > T:
        return np.full(U, -1, dtype=np.int64), -np.inf
    v = np.full((T + 1, U + 1), -np.inf)
    v[0, 0] = 0.0
    lab = np.zeros((T, U + 1), dtype=bool)
    for t in range(T):
        tt = v[t] + lpb[t]
        tu = np.full(U + 1, -np.inf)
        tu[1:] = v[t, :-1] + lpl[t]
        lab[t] = tu > tt                    # strictly greater: a tie goes to blank
        v[t + 1] = np.where(lab[t], tu, tt)
    frames, u = np.full(U, -1, dtype=np.int64), U
    for t in range(T - 1, -1, -1):
        if u > 0 and lab[t, u]:
            frames[u - 1] = t
            u -= 1
    assert u == 0
    return frames, float(v[T, U])


def path_score(lpb, lpl, frames):
    """the sum of the T decisions of the path whose label u+1 is frame frames[u]'s decision (no terminal blank)"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    frames = [int(f) for f in frames[:U]]
    assert all(0 <= f < T for f in frames) and all(a < b for a, b in zip(frames, frames[1:])), frames
    u, s = 0, 0.0
    for t in range(T):
        if u < U and frames[u] == t:
            s += lpl[t, u]
            u += 1
        else:
            s += lpb[t, u]
    assert u == U
    return float(s)


def brute_force(lpb, lpl):
    """every set of U emitting frames -> (best score, its frames (the first maximum in lexicographic order of the sets), mass [U], expected [U])"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    best, arg, scores, sets = -np.inf, None, [], []
    for emit in itertools.combinations(range(T), U):
        s = path_score(lpb, lpl, emit)
        scores.append(s)
        sets.append(emit)
        if s > best:
            best, arg = s, emit
    scores = np.array(scores)
    post = np.exp(scores - scores.max())
    post /= post.sum()
    mass, expected = np.zeros(U), np.zeros(U)
    for p, emit in zip(post, sets):
        for u, t in enumerate(emit):
            mass[u] += p
            expected[u] += p * t
    return best, np.array(arg, dtype=np.int64), mass, expected


def emit_stats_ref(lpb, lpl):
    """-> (expected [U], mass [U]); an utterance without a path: -1 / 0"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    alpha, beta, ll = M.lattice(lpb, lpl)
    if not np.isfinite(ll):
        return np.full(U, -1.0), np.zeros(U)
    with np.errstate(invalid="ignore"):
        e = np.nan_to_num(np.exp(alpha[:T, :U] + lpl + beta[1:, 1:] - ll), nan=0.0)
    return (np.arange(T)[:, None] * e).sum(0), e.sum(0)


def second_best(lpb, lpl, frames):
    """the best score among the paths that differ from the path `frames`: such a path shares a prefix with it and then takes the OTHER move at one
    of its cells, after which it is free - prefix + other move + the best completion from where that lands"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    w = np.full((T + 1, U + 2), -np.inf)       # w(t, u) = best score from (t, u) to (T, U); column U+1 stays -inf
    w[T, U] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(U + 1):
            lab = lpl[t, u] + w[t + 1, u + 1] if u < U else -np.inf
            w[t, u] = max(lpb[t, u] + w[t + 1, u], lab)
    frames = [int(f) for f in frames[:U]]
    u, pre, best = 0, 0.0, -np.inf
    for t in range(T):
        if u < U and frames[u] == t:
            best = max(best, pre + lpb[t, u] + w[t + 1, u])
            pre += lpl[t, u]
            u += 1
        else:
            if u < U:
                best = max(best, pre + lpl[t, u] + w[t + 1, u + 1])
            pre += lpb[t, u]
    return float(best)


def planted_batch(seed, T, U, act_lens, label_lens, V=8, boost=8.0, noise=0.1, blank=0, no_path=()):
    """-> (logits f32 [B, T, U+1, V], labels i32 [B, max(U, 1)], act_lens i32 [B], label_lens i32 [B], frames i64 [B, U]).  Per utterance a random
    strictly increasing set of U_b frames out of T_b is drawn and every decision of that path gets +boost on its logit over `noise`-sized
    values: each decision then has probability about 1 - (V - 1) e^-boost and leaving the path costs about `boost` at the first wrong move.
    Utterances listed in no_path (U_b > T_b) get noise alone and frames -1.

    The noise sits at -boost, so the boosted logits sit at 0: a planted decision's log-probability is about -(V - 1) e^-boost = -0.0023, and the
    library's emission tables hold x - lse in f32, whose rounding error is an ulp of max(|x|, |lse|).  With the boosted logits at 8 that is
    5e-7 on a term of 0.0023 - twice the 1e-4 relative bound the GPU tests put on a planted path's score, from the table's number format
    alone, before any aligner has run; at 0 it is 4e-9.  (The softmax does not see the shift.)"""
    rng = np.random.default_rng(seed)
    B = len(act_lens)
    x = (noise * rng.standard_normal((B, T, U + 1, V)) - boost).astype(np.float32)
    labels = rng.integers(1, V, (B, max(U, 1))).astype(np.int32)
    frames = np.full((B, U), -1, dtype=np.int64)
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        if b in no_path or Ub > Tb:
            continue
        emit = np.sort(rng.choice(Tb, size=Ub, replace=False))
        frames[b, :Ub] = emit
        u = 0
        for t in range(Tb):
            if u < Ub and emit[u] == t:
                x[b, t, u, labels[b, u]] += boost
                u += 1
            else:
                x[b, t, u, blank] += boost
    return x, labels, np.asarray(act_lens, dtype=np.int32), np.asarray(label_lens, dtype=np.int32), frames
