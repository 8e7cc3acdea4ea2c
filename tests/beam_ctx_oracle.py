"""Float64 numpy restatement of the biased beam search rule (include/ttmi.h, ttmi_beam_step_ctx), of the hotword compiler's rule (restated
here, independently of ttmi/context.py) and the brute-force bias by substring counting.  A helper, not a test module (like beam_oracle.py,
whose probability model, log_softmax, _key and synthetic logits it takes over).

compile_tables()  phrases, boosts -> the automaton's tables (weights rounded to f32, as the device holds them)
fsa_step()        step(s, k) -> (s', delta) with delta summed in f64 in the contract's order, and what the walk met
brute_bias()      (running, final) bias of a token sequence by counting substring occurrences
step() / run()    one frame / one utterance of the biased search; hypotheses carry (tokens, score, frames, logprobs, state, bias)
final_order()     the live hypotheses by score + final bias
phrases_from()    the tests' phrase rule"""
import collections
import math

import numpy as np

import beam_oracle as BO
from beam_oracle import log_softmax, _key, rng_logits      # noqa: F401  (rng_logits: for the tests that import this module only)

Hyp = collections.namedtuple("Hyp", ["tokens", "score", "frames", "logprobs", "state", "bias"])
Tables = collections.namedtuple("Tables", ["arc_off", "arc_sym", "arc_next", "arc_w", "fail", "fail_w", "final_w"])

START = [Hyp((), 0.0, (), (), 0, 0.0)]
COUNTERS = ("arcs", "fail_hops", "merges", "differs")


# ------------------------------------------------------------------------------------------------------------ the compiler's rule
def compile_tables(phrases, boosts):
    """the rule of the issue, on prefixes as tuples: nodes = all prefixes, numbered breadth first with children by ascending symbol (= sorted
    by (length, tuple)); fail(n) = the longest proper suffix of n that is a node; out(n) = sum of boost * len over the phrases that are a
    suffix of n; pi(n) = depth * (largest boost of a phrase strictly extending n), 0 for a leaf"""
    phrases = [tuple(int(k) for k in p) for p in phrases]
    nodes = sorted({p[:i] for p in phrases for i in range(len(p) + 1)} | {()}, key=lambda n: (len(n), n))
    index = {n: i for i, n in enumerate(nodes)}

    def fail(n):
        return next(n[i:] for i in range(1, len(n) + 1) if n[i:] in index)

    def out(n):
        return sum(b * len(p) for p, b in zip(phrases, boosts) if len(p) <= len(n) and n[len(n) - len(p):] == p)

    def pi(n):
        ext = [b for p, b in zip(phrases, boosts) if len(p) > len(n) and p[:len(n)] == n]
        return max(ext) * len(n) if ext else 0.0
    arc_off, arc_sym, arc_next, arc_w = [0], [], [], []
    for n in nodes:
        for c in sorted(m for m in nodes if len(m) == len(n) + 1 and m[:-1] == n):
            arc_sym.append(c[-1])
            arc_next.append(index[c])
            arc_w.append(pi(c) - pi(n) + out(c))
        arc_off.append(len(arc_sym))
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)      # noqa: E731
    i32 = lambda v: np.asarray(v, dtype=np.int32)                            # noqa: E731
    return Tables(i32(arc_off), i32(arc_sym), i32(arc_next), f32(arc_w), i32([0] + [index[fail(n)] for n in nodes[1:]]),
                  f32([0.0] + [pi(fail(n)) - pi(n) for n in nodes[1:]]), f32([-pi(n) for n in nodes]))


def zero_weights(tb):
    """the same automaton with every weight 0"""
    return Tables(tb.arc_off, tb.arc_sym, tb.arc_next, np.zeros_like(tb.arc_w), tb.fail, np.zeros_like(tb.fail_w), np.zeros_like(tb.final_w))


def fsa_step(tb, s, k):
    """-> (s', delta, took an arc, failure hops with a non-zero weight)"""
    acc, hops = 0.0, 0
    while True:
        lo, hi = int(tb.arc_off[s]), int(tb.arc_off[s + 1])
        for a in range(lo, hi):
            if int(tb.arc_sym[a]) == k:
                return int(tb.arc_next[a]), acc + float(tb.arc_w[a]), True, hops
        if s == 0:
            return 0, acc + float(tb.fail_w[0]), False, hops
        hops += float(tb.fail_w[s]) != 0.0
        acc += float(tb.fail_w[s])
        s = int(tb.fail[s])


_ROWS, _ZERO = {}, {}


def fsa_row(tb, s, V):
    """fsa_step(tb, s, k) for every k in [0, V) as arrays (next state, delta, took an arc, hops); kept per (tables, state)"""
    if (id(tb), s, V) not in _ROWS:
        cols = list(zip(*(fsa_step(tb, s, k) for k in range(V))))
        _ROWS[(id(tb), s, V)] = (tb, np.asarray(cols[0]), np.asarray(cols[1], dtype=np.float64), np.asarray(cols[2]), np.asarray(cols[3]))
    return _ROWS[(id(tb), s, V)][1:]


def fsa_run(tb, y):
    """tokens y from the root -> (state, running bias, final bias)"""
    s, bias = 0, 0.0
    for k in y:
        s, d, _, _ = fsa_step(tb, s, int(k))
        bias += d
    return s, bias, bias + float(tb.final_w[s])


def brute_bias(phrases, boosts, y):
    """-> (running, final): final = sum over phrases of boost * len * occurrences in y (overlaps counted); running adds the advance on the
    longest suffix of y that is a prefix of a phrase: its length times the largest boost of a phrase strictly extending it"""
    y = tuple(y)
    phrases = [tuple(p) for p in phrases]
    final = sum(b * len(p) * sum(y[i:i + len(p)] == p for i in range(len(y) - len(p) + 1)) for p, b in zip(phrases, boosts))
    for i in range(len(y) + 1):                                # longest suffix first
        suf = y[i:]
        if any(p[:len(suf)] == suf for p in phrases):
            ext = [b for p, b in zip(phrases, boosts) if len(p) > len(suf) and p[:len(suf)] == suf]
            return final + (max(ext) * len(suf) if ext else 0.0), final
    raise AssertionError("the empty suffix is a prefix of every phrase")


def phrases_from(final_beam, V, blank=0, least=3):
    """the tests' phrase rule on an unbiased final beam (best first): h = the last hypothesis with at least three tokens -> h[:3], h[:2],
    [h[1], x], [h[1], h[2], x], x = 1 + h[2] % (V - 1) stepped on while it is h[2] (or the blank); least=2: with no such hypothesis the first
    two tokens of the last one with at least two.  None if there is none."""
    long = [h.tokens for h in final_beam if len(h.tokens) >= 3]
    if long:
        h = long[-1]
        x = 1 + h[2] % (V - 1)
        while x == h[2] or x == blank:
            x = 1 + x % (V - 1)
        return [list(h[:3]), list(h[:2]), [h[1], x], [h[1], h[2], x]]
    short = [h.tokens for h in final_beam if len(h.tokens) >= 2]
    return [list(short[-1][:2])] if least == 2 and short else None


# ------------------------------------------------------------------------------------------------------------ the beam rule
def step(beam, rows, t, W, tb, blank=0, compare=True):
    """beam: W entries, Hyp or None; rows[w]: the logits of frame t for slot w.  -> (new beam, parent, fresh, key margin, counters): the key
    margin = the smallest gap between neighbouring KEYS among the best W + 1 candidates; counters: arcs taken and failure hops with a non-zero
    weight over the selected candidates, merges with a finite symbol side (counted where the merged candidate is formed, before the
    selection: that is where the kernel takes its merge path), and whether the new beam's tokens differ from the unbiased rule's
    (this rule with every weight 0 on the same beam and rows: test_context.py shows that to be beam_oracle.step's beam exactly)"""
    live = [i for i, h in enumerate(beam) if h is not None and h.score > -math.inf]
    lp = {i: log_softmax(rows[i]) for i in live}
    where = {beam[i].tokens: i for i in live}
    assert len(where) == len(live), "live slots must hold distinct sequences"
    cands = []                                           # (key, parent, is_symbol, symbol, Hyp, (arc, hops))
    merged_away = set()
    merges = 0
    for i in live:
        h = beam[i]
        a = _key(h.score + lp[i][blank])
        new = Hyp(h.tokens, a, h.frames, h.logprobs, h.state, h.bias)
        j = where.get(h.tokens[:-1]) if h.tokens else None
        if j is not None:
            k = h.tokens[-1]
            g = beam[j]
            b = _key(g.score + lp[j][k])
            merged_away.add((j, k))
            if b > -math.inf:
                s2, d, _, _ = fsa_step(tb, g.state, k)
                assert s2 == h.state and g.bias + d == h.bias, "the two sides of a merge carry the same state and bias"
                merges += 1
                frames, lps = (g.frames + (t,), g.logprobs + (float(lp[j][k]),)) if b > a else (h.frames, h.logprobs)
                new = Hyp(h.tokens, float(np.logaddexp(a, b)), frames, lps, h.state, h.bias)
        cands.append((_key(new.score + new.bias), i, 0, -1, new, (0, 0)))
    for i in live:
        h = beam[i]
        _, delta, _, _ = fsa_row(tb, h.state, len(lp[i]))
        with np.errstate(invalid="ignore"):
            score = h.score + lp[i]
            score = np.where(score > -math.inf, score, -math.inf)        # NaN ranks as -inf
            key = score + (h.bias + delta)
            key = np.where(key > -math.inf, key, -math.inf)
        key[blank] = -math.inf
        for j, k in merged_away:
            if j == i:
                key[k] = -math.inf
        # the W + 1 best of this parent under (key descending, symbol ascending) hold every one of its candidates among the W + 1 best of all
        for k in np.lexsort((np.arange(len(key)), -key))[:W + 1].tolist():
            if key[k] > -math.inf and score[k] > -math.inf:
                s2, d, arc, hops = fsa_step(tb, h.state, k)
                cands.append((float(key[k]), i, 1, k, Hyp(h.tokens + (k,), float(score[k]), h.frames + (t,), h.logprobs + (float(lp[i][k]),),
                                                       s2, h.bias + d), (int(arc), hops)))
    cands = [c for c in cands if c[0] > -math.inf and c[4].score > -math.inf]
    cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    top = [c[0] for c in cands[:W + 1]]
    margin = min([a - b for a, b in zip(top, top[1:])] or [math.inf])
    new_beam, parent, fresh = [None] * W, list(range(W)), [0] * W
    counters = dict.fromkeys(COUNTERS, 0)
    counters["merges"] = merges
    for r, c in enumerate(cands[:W]):
        new_beam[r], parent[r], fresh[r] = c[4], c[1], c[2]
        for name, v in zip(COUNTERS, c[5]):
            counters[name] += v
    if compare:
        if id(tb) not in _ZERO:
            _ZERO[id(tb)] = (tb, zero_weights(tb))
        plain = step([h and h._replace(bias=0.0) for h in beam], rows, t, W, _ZERO[id(tb)][1], blank, compare=False)[0]
        counters["differs"] = int([h and h.tokens for h in plain] != [h and h.tokens for h in new_beam])
    return new_beam, parent, fresh, margin, counters


def final_order(beam, tb):
    """the live hypotheses of a final beam -> [(Hyp, final bias)] by score + final bias descending, the slot ascending on ties, and the
    smallest gap between neighbouring final keys"""
    live = [(h, h.bias + float(tb.final_w[h.state])) for h in beam if h is not None]
    live.sort(key=lambda e: -(e[0].score + e[1]))                        # (stable: the slot order on ties)
    keys = [h.score + fb for h, fb in live]
    return live, min([a - b for a, b in zip(keys, keys[1:])] or [math.inf])


def run(logits, b, T, W, tb, blank=0):
    """utterance b of T frames -> (final beam in slot order, None for an empty slot; the smallest key margin of any step; counters summed over
    the steps; the smallest gap of the final order)"""
    beam = START + [None] * (W - 1)
    margin, total = math.inf, dict.fromkeys(COUNTERS, 0)
    for t in range(T):
        rows = [logits(b, t, h.tokens) if h is not None else None for h in beam]
        beam, _, _, m, c = step(beam, rows, t, W, tb, blank)
        margin = min(margin, m)
        for name in COUNTERS:
            total[name] += c[name]
    return beam, margin, total, final_order(beam, tb)[1]
