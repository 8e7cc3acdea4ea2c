"""Float64 numpy restatement of the frame-synchronous beam search rule (include/ttmi.h, ttmi_beam_step), for the tests of the kernel and of
Transducer.beam_decode_batch.  A helper, not a test module (like mask_cases.py).

The probability model is the greedy decoder's: each of an utterance's T frames takes one decision, blank or one symbol, against the label
state of the tokens emitted so far; the emitting frame is consumed.  `logits(b, t, tokens)` -> the V logits of frame t of utterance b given
the emitted symbols `tokens` (a tuple, the start symbol not included).

step()        one frame of one utterance: candidates, merge, total order, the W best
run()         a whole utterance -> the final beam (best first) and the run's margin
brute_force() the sum over all V^T decision sequences, grouped by token sequence
rng_logits()  the synthetic logits the kernel tests use"""
import collections
import math

import numpy as np

Hyp = collections.namedtuple("Hyp", ["tokens", "score", "frames", "logprobs"])

START = [Hyp((), 0.0, (), ())]


def log_softmax(x):
    """float64 log-probabilities of one row; a row without a finite log-sum-exp (NaN, +inf, nothing but -inf) gives NaN throughout"""
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x) if not np.isnan(x).any() else np.nan
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lse = m + np.log(np.sum(np.exp(x - m)))
        if not np.isfinite(lse):
            return np.full(x.shape, np.nan)
        return x - lse


def _key(s):
    return s if s > -math.inf else -math.inf          # NaN ranks as -inf


def step(beam, rows, t, W, blank=0):
    """beam: list of W entries, Hyp or None (an empty slot); rows[w]: the logits of frame t for slot w (ignored for empty slots).
    -> (new beam, parent, fresh, margin, merge_gap): parent / fresh as the kernel reports them (an empty new slot: its own index, 0); margin =
    the smallest gap between neighbouring scores among the best W + 1 candidates (inf with fewer than two); merge_gap = the smallest
    |a - b| of the two sides of any merge (which side the details come from hangs on its sign)."""
    live = [i for i, h in enumerate(beam) if h is not None and h.score > -math.inf]
    lp = {i: log_softmax(rows[i]) for i in live}
    where = {beam[i].tokens: i for i in live}
    assert len(where) == len(live), "live slots must hold distinct sequences"
    cands = []                                           # (score, parent, is_symbol, symbol, Hyp)
    merged_away = set()
    merge_gap = math.inf
    for i in live:
        h = beam[i]
        a = _key(h.score + lp[i][blank])
        new = Hyp(h.tokens, a, h.frames, h.logprobs)
        j = where.get(h.tokens[:-1]) if h.tokens else None
        if j is not None:
            k = h.tokens[-1]
            g = beam[j]
            b = _key(g.score + lp[j][k])
            merged_away.add((j, k))
            if b > -math.inf:
                if a > -math.inf:
                    merge_gap = min(merge_gap, abs(a - b))
                frames, lps = (g.frames + (t,), g.logprobs + (float(lp[j][k]),)) if b > a else (h.frames, h.logprobs)
                new = Hyp(h.tokens, float(np.logaddexp(a, b)), frames, lps)
        cands.append((new.score, i, 0, -1, new))
    for i in live:
        h = beam[i]
        for k in range(len(lp[i])):
            if k == blank or (i, k) in merged_away:
                continue
            s = _key(h.score + lp[i][k])
            if s > -math.inf:
                cands.append((s, i, 1, k, Hyp(h.tokens + (k,), s, h.frames + (t,), h.logprobs + (float(lp[i][k]),))))
    cands = [c for c in cands if c[0] > -math.inf]
    cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    top = [c[0] for c in cands[:W + 1]]
    margin = min([a - b for a, b in zip(top, top[1:])] or [math.inf])
    new_beam, parent, fresh = [None] * W, list(range(W)), [0] * W
    for r, c in enumerate(cands[:W]):
        new_beam[r], parent[r], fresh[r] = c[4], c[1], c[2]
    return new_beam, parent, fresh, margin, merge_gap


def run(logits, b, T, W, blank=0):
    """the whole utterance b of T frames -> (final beam: the live hypotheses, best first; margin; merge_gap)"""
    beam = START + [None] * (W - 1)
    margin = merge_gap = math.inf
    for t in range(T):
        rows = [logits(b, t, h.tokens) if h is not None else None for h in beam]
        beam, _, _, m, g = step(beam, rows, t, W, blank)
        margin, merge_gap = min(margin, m), min(merge_gap, g)
    return [h for h in beam if h is not None], margin, merge_gap


def brute_force(logits, b, T, blank=0):
    """{token sequence: log of the summed probability of every decision sequence of T frames that spells it}"""
    total = {}

    def walk(t, tokens, score):
        if t == T:
            total.setdefault(tokens, []).append(score)
            return
        lp = log_softmax(logits(b, t, tokens))
        for k in range(len(lp)):
            walk(t + 1, tokens if k == blank else tokens + (k,), score + lp[k])

    walk(0, (), 0.0)
    return {k: float(np.logaddexp.reduce(v)) for k, v in total.items()}


def rng_logits(seed, V):
    """the kernel tests' synthetic model: 3 * standard_normal(V), rounded to f32, seeded by (seed, t, the emitted symbols); the same for every
    utterance of a batch (they differ in their lengths)"""
    cache = {}

    def logits(b, t, tokens):
        key = (t, tokens)
        if key not in cache:
            rng = np.random.default_rng([seed, t, len(tokens), *tokens])
            cache[key] = (3.0 * rng.standard_normal(V)).astype(np.float32)
        return cache[key]

    return logits


def first_seed(make_logits, cases, W, blank=0, floor=1e-3, seeds=range(16)):
    """the seed rule: the first seed whose oracle margin over every (b, T) of `cases` is at least `floor` -> (seed, logits, {(b, T): run()});
    None if there is none (the caller fails, it does not skip)"""
    for seed in seeds:
        logits = make_logits(seed)
        runs = {c: run(logits, c[0], c[1], W, blank) for c in cases}
        if min(r[1] for r in runs.values()) >= floor:
            return seed, logits, runs
    return None
