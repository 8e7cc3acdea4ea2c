"""Float64 reference of the CTC hypothesis scorer (include/ttmi.h, ttmi_ctc_score_hyps), in numpy: the log-softmax in float64 of the f32 logits
the kernel sees, then the alpha recursion of ttmi_ctc_loss_fwd on the literally built extended sequence.  Beside it two enumerations for
lattices small enough to list (T <= 5, V <= 3): every symbol path whose collapse is the hypothesis (the definition of CTC, for hypotheses
without a blank token) and every admissible state path (which also covers a token equal to `blank`).  `defect` plants one wrong rule at a time,
for the test that shows the inputs of the GPU tests would see it."""
import itertools

import numpy as np

DEFECTS = ("skip_across_repeat", "last_state_only", "T_for_Tb", "utt_off_by_one")


def log_softmax(x):
    """f32 logits [T, V] -> float64 log-probabilities (a row with a NaN is all NaN, a -inf logit stays -inf)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(axis=-1, keepdims=True)
        return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def extended(hyp, blank=0):
    """l' = blank, y_0, blank, y_1, ..., blank and, per state, whether the s-2 move is allowed: l'_s != blank and l'_s != l'_{s-2}"""
    ext = [blank]
    for y in hyp:
        ext += [int(y), blank]
    skip = [s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(len(ext))]
    return ext, skip


def _lse(vals):
    vals = np.asarray(vals, dtype=np.float64)
    if np.isnan(vals).any():
        return np.nan
    m = vals.max()
    if m == -np.inf:
        return -np.inf
    return float(m + np.log(np.exp(vals - m).sum()))


def score_ref(x, hyp, Tb, blank=0, defect=None):
    """log P_ctc(hyp | x[:Tb]) in float64; -inf where no alignment exists"""
    x = np.asarray(x)
    T, V = x.shape
    Tb = T if defect == "T_for_Tb" else min(max(int(Tb), 1), T)
    hyp = [min(max(int(y), 0), V - 1) for y in hyp]
    lp = log_softmax(x[:Tb])
    ext, skip = extended(hyp, blank)
    if defect == "skip_across_repeat":
        skip = [s >= 2 and ext[s] != blank for s in range(len(ext))]
    S = len(ext)
    ext, skip = np.array(ext), np.array(skip)
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, ext[0]]
    if S > 1:
        alpha[1] = lp[0, ext[1]]
    dead = np.full(2, -np.inf)
    for t in range(1, Tb):                              # all states of a frame at once: logsumexp(alpha(s), alpha(s-1), alpha(s-2) if skip)
        a1 = np.concatenate([dead[:1], alpha])[:S]
        a2 = np.where(skip, np.concatenate([dead, alpha])[:S], -np.inf)
        terms = np.stack([alpha, a1, a2])
        with np.errstate(invalid="ignore", divide="ignore"):
            m = terms.max(axis=0)
            ms = np.where(np.isneginf(m), 0.0, m)
            alpha = lp[t, ext] + np.where(np.isneginf(m), -np.inf, ms + np.log(np.exp(terms - ms).sum(axis=0)))
    if S == 1 or defect == "last_state_only":
        return float(alpha[S - 1])
    return _lse([alpha[S - 1], alpha[S - 2]])


def scores_ref(x, act_lens, hyps, utt=None, blank=0, defect=None):
    """x [B, T, V]; hyps = P token lists; utt = P utterance indices, or None for the [B, N] layout (pair p on utterance p // (P // B))"""
    B, P = len(x), len(hyps)
    if utt is None:
        assert P % B == 0
        utt = [p // (P // B) for p in range(P)]
    out = []
    for p in range(P):
        b = min(max(int(utt[p]), 0), B - 1)
        if defect == "utt_off_by_one":
            b = (b + 1) % B
        out.append(score_ref(x[b], hyps[p], act_lens[b], blank, defect))
    return np.array(out, dtype=np.float64)


def frames_needed(hyp):
    """a hypothesis without a blank token has an alignment iff T_b >= its tokens plus its adjacent repeats"""
    return len(hyp) + sum(1 for a, b in zip(hyp, hyp[1:]) if a == b)


def build_case(seed, T, U, V, blank=0, N=4):
    """The batch the GPU tests score at (T, U, V), and the CPU tests plant defects on: B = 4 utterances with ragged lengths, N = 4 hypotheses
    each in the [B, N] layout: 0 = as long as T_b >= 2 U_h + 1 and U allow, with an adjacent repeat; 1 = empty; 2 = random length with one
    token equal to `blank`; 3 = one symbol min(U, T_b + 1) times, which no alignment fits when it needs more than T_b frames (`planted`).
    Every other hypothesis takes T_b >= 2 U_h + 1 and is feasible whatever it holds.
    -> dict(x f32 [B, T, V], act_lens, hyps (P lists), planted (P bools))"""
    rng = np.random.default_rng(seed)
    B = 4
    x = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    act = [T, max(1, T - 1), max(1, (T + 1) // 2), max(1, T // 3)]
    sym = [v for v in range(V) if v != blank]
    hyps, planted = [], []
    for b in range(B):
        cap = min(U, (act[b] - 1) // 2)
        h0 = [int(v) for v in rng.choice(sym, cap)]
        if cap >= 2:
            h0[1] = h0[0]
        h2 = [int(v) for v in rng.choice(sym, int(rng.integers(0, cap + 1)))]
        if h2:
            h2[int(rng.integers(0, len(h2)))] = blank
        h3 = [int(rng.choice(sym))] * min(U, act[b] + 1)
        for h, may_be_dead in ((h0, False), ([], False), (h2, False), (h3, True)):
            hyps.append(h)
            planted.append(may_be_dead and frames_needed(h) > act[b])
        assert len(hyps) == (b + 1) * N
    return dict(x=x, act_lens=act, hyps=hyps, planted=planted)


def collapse(path, blank=0):
    out, prev = [], None
    for v in path:
        if v != blank and v != prev:
            out.append(int(v))
        prev = v
    return out


def enumerate_symbol_paths(x, hyp, Tb, blank=0):
    """the definition: the summed probability of every length-T_b symbol sequence that collapses to hyp (hyp without a blank token)"""
    x = np.asarray(x)
    assert blank not in list(hyp)
    lp = log_softmax(x[:Tb])
    V = x.shape[1]
    terms = [sum(lp[t, v] for t, v in enumerate(path)) for path in itertools.product(range(V), repeat=Tb) if collapse(path, blank) == list(hyp)]
    return _lse(terms) if terms else -np.inf


def enumerate_state_paths(x, hyp, Tb, blank=0):
    """every path through the states of l': starts in 0 or 1, moves by 0, +1 or (where the skip rule allows) +2, ends in S-1 or S-2"""
    x = np.asarray(x)
    lp = log_softmax(x[:Tb])
    ext, skip = extended(hyp, blank)
    S = len(ext)
    terms = []
    for path in itertools.product(range(S), repeat=Tb):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        if all(b - a in (0, 1) or (b - a == 2 and skip[b]) for a, b in zip(path, path[1:])):
            terms.append(sum(lp[t, ext[s]] for t, s in enumerate(path)))
    return _lse(terms) if terms else -np.inf
