"""Float64 numpy restatement of the fused beam search rule (include/ttmi.h, ttmi_beam_step_fuse) on top of beam_ctx_oracle.py: the biased
search with up to two dense external sources (a language model's rows, the internal LM's rows) and a bonus per symbol.  A helper, not a test
module.  Hypotheses carry `fuse` beside `state` / `bias`.

Fuse              (bonus, ((weight, norm) or None, (weight, norm) or None)): what ttmi_beam_step_fuse takes beside the rows
ext_logp()        a source row -> its lpx under norm 0 / 1 / 2
e_row()           e(w, k) of every symbol k of one slot
step() / run()    one frame / one utterance; `defect` plants one of DEFECTS
final_order()     the live hypotheses by score + final bias + fuse
rng_source()      the tests' synthetic sources: functions of the tokens alone
token_sum()       the fuse of a token sequence, token by token"""
import collections
import math

import numpy as np

import beam_ctx_oracle as CO
from beam_ctx_oracle import log_softmax, _key, fsa_step, fsa_row

Hyp = collections.namedtuple("Hyp", ["tokens", "score", "frames", "logprobs", "state", "bias", "fuse"])
Fuse = collections.namedtuple("Fuse", ["bonus", "sources"])

START = [Hyp((), 0.0, (), (), 0, 0.0, 0.0)]
NONE = Fuse(0.0, (None, None))
TRIVIAL = CO.Tables(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(1, np.int32),
                    np.zeros(1, np.float32), np.zeros(1, np.float32))      # S = 1, A = 0, fail_w[0] = 0: a search without hotwords
DEFECTS = ("lm_on_blank", "norm2_keeps_blank", "merge_takes_j", "only_source0", "row_mixup", "bonus_per_frame")


def ext_logp(x, norm, blank=0):
    """lpx of one source row in f64: norm 0 -> the row itself; 1 -> minus its log-sum-exp; 2 -> minus the log-sum-exp of all entries but the
    blank; a row without a finite log-sum-exp gives NaN throughout"""
    x = np.asarray(x, dtype=np.float64)
    if norm == 0:
        return x.copy()
    sel = x if norm == 1 else np.delete(x, blank)
    m = np.max(sel) if not np.isnan(sel).any() else np.nan
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lse = m + np.log(np.sum(np.exp(sel - m)))
        if not np.isfinite(lse):
            return np.full(x.shape, np.nan)
        return x - lse


def e_row(ext, cfg, V, blank=0, defect=None, bonus=True):
    """e(w, k) for every k: bonus + w_0 * lpx_0 + w_1 * lpx_1 in that order, absent sources skipped; ext = (row or None, row or None)"""
    e = np.full(V, cfg.bonus if bonus else 0.0, dtype=np.float64)
    for j, src in enumerate(cfg.sources):
        if src is None or ext[j] is None or (defect == "only_source0" and j == 1):
            continue
        norm = 1 if (defect == "norm2_keeps_blank" and src[1] == 2) else src[1]
        with np.errstate(invalid="ignore"):
            e = e + src[0] * ext_logp(ext[j], norm, blank)
    return e


def step(beam, rows, ext, t, W, tb, cfg, blank=0, defect=None):
    """beam: W entries, Hyp or None; rows[w]: the logits of frame t for slot w; ext[w] = (source 0's row, source 1's row) of slot w, None
    where absent.  -> (new beam, parent, fresh, key margin, merges): CO.step's rule with fuse' = fuse_i + e(i, k) on a symbol extension, fuse_i
    on the blank one, key = score + (bias' + fuse'); a symbol whose e is not finite takes no slot; a merged candidate keeps i's fuse"""
    live = [i for i, h in enumerate(beam) if h is not None and h.score > -math.inf]
    lp = {i: log_softmax(rows[i]) for i in live}
    es = {i: e_row(ext[i], cfg, len(lp[i]), blank, defect) for i in live}
    where = {beam[i].tokens: i for i in live}
    assert len(where) == len(live), "live slots must hold distinct sequences"
    cands = []                                           # (key, parent, is_symbol, symbol, Hyp)
    merged_away = set()
    merges = 0
    for i in live:
        h = beam[i]
        a = _key(h.score + lp[i][blank])
        fuse = h.fuse
        if defect == "lm_on_blank":
            fuse = fuse + e_row(ext[i], cfg, len(lp[i]), blank, defect, bonus=False)[blank]
        if defect == "bonus_per_frame":
            fuse = fuse + cfg.bonus
        new = Hyp(h.tokens, a, h.frames, h.logprobs, h.state, h.bias, fuse)
        j = where.get(h.tokens[:-1]) if h.tokens else None
        if j is not None:
            k = h.tokens[-1]
            g = beam[j]
            b = _key(g.score + lp[j][k])
            merged_away.add((j, k))
            if b > -math.inf:
                merges += 1
                frames, lps = (g.frames + (t,), g.logprobs + (float(lp[j][k]),)) if b > a else (h.frames, h.logprobs)
                new = Hyp(h.tokens, float(np.logaddexp(a, b)), frames, lps, h.state, h.bias, g.fuse if defect == "merge_takes_j" else fuse)
        cands.append((_key(new.score + (new.bias + new.fuse)), i, 0, -1, new))
    for i in live:
        h = beam[i]
        _, delta, _, _ = fsa_row(tb, h.state, len(lp[i]))
        with np.errstate(invalid="ignore"):
            score = h.score + lp[i]
            score = np.where(score > -math.inf, score, -math.inf)        # NaN ranks as -inf
            key = score + ((h.bias + delta) + (h.fuse + es[i]))
            key = np.where((key > -math.inf) & np.isfinite(es[i]), key, -math.inf)
        key[blank] = -math.inf
        for j, k in merged_away:
            if j == i:
                key[k] = -math.inf
        for k in np.lexsort((np.arange(len(key)), -key))[:W + 1].tolist():
            if key[k] > -math.inf and score[k] > -math.inf:
                s2, d, _, _ = fsa_step(tb, h.state, k)
                cands.append((float(key[k]), i, 1, k, Hyp(h.tokens + (k,), float(score[k]), h.frames + (t,), h.logprobs + (float(lp[i][k]),),
                                                       s2, h.bias + d, h.fuse + float(es[i][k]))))
    cands = [c for c in cands if c[0] > -math.inf and c[4].score > -math.inf]
    cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    top = [c[0] for c in cands[:W + 1]]
    margin = min([a - b for a, b in zip(top, top[1:])] or [math.inf])
    new_beam, parent, fresh = [None] * W, list(range(W)), [0] * W
    for r, c in enumerate(cands[:W]):
        new_beam[r], parent[r], fresh[r] = c[4], c[1], c[2]
    return new_beam, parent, fresh, margin, merges


def final_order(beam, tb, eos=None):
    """the live hypotheses of a final beam -> [(Hyp, final bias, lm_total)] by score + final bias + lm_total descending, the slot ascending on
    ties, and the smallest gap between neighbouring final keys; eos(tokens) -> the closing term added to fuse (None: nothing)"""
    live = [(h, h.bias + float(tb.final_w[h.state]), h.fuse + (eos(h.tokens) if eos is not None else 0.0)) for h in beam if h is not None]
    live.sort(key=lambda e: -(e[0].score + e[1] + e[2]))                 # (stable: the slot order on ties)
    keys = [h.score + fb + lt for h, fb, lt in live]
    return live, min([a - b for a, b in zip(keys, keys[1:])] or [math.inf])


def run(logits, sources, b, T, W, tb, cfg, blank=0, defect=None):
    """utterance b of T frames; sources(j, tokens) -> source j's row for a hypothesis (called for present sources only) -> (final beam in slot
    order, None for an empty slot; the smallest key margin of any step; merges summed over the steps)"""
    beam = START + [None] * (W - 1)
    parent = list(range(W))
    margin, merges = math.inf, 0
    for t in range(T):
        rows = [logits(b, t, h.tokens) if h is not None else None for h in beam]
        owner = beam
        if defect == "row_mixup":                       # the row tables indexed by the parent's slot once more after the reorder
            owner = [beam[parent[w]] if beam[parent[w]] is not None else beam[w] for w in range(W)]
        ext = [tuple(sources(j, o.tokens) if cfg.sources[j] is not None else None for j in range(2)) if h is not None else None
               for h, o in zip(beam, owner)]
        beam, parent, _, m, g = step(beam, rows, ext, t, W, tb, cfg, blank, defect)
        margin, merges = min(margin, m), merges + g
    return beam, margin, merges


def rng_source(base_seed, V, scale=2.0, bf16=False):
    """tokens -> scale * standard_normal(V) as f32 from default_rng([base_seed, len(tokens), *tokens]); bf16: rounded to bf16 (to nearest even)
    and widened again, the values a bf16 source holds"""
    cache = {}

    def row(tokens):
        if tokens not in cache:
            x = (scale * np.random.default_rng([base_seed, len(tokens), *tokens]).standard_normal(V)).astype(np.float32)
            if bf16:
                u = x.view(np.uint32).astype(np.uint64)
                x = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
            cache[tokens] = x
        return cache[tokens]
    return row


def token_sum(tokens, sources, cfg, V, blank=0):
    """the fuse of a token sequence from the start: e(tokens[:n], tokens[n]) summed token by token"""
    total = 0.0
    for n, k in enumerate(tokens):
        ext = tuple(sources(j, tuple(tokens[:n])) if cfg.sources[j] is not None else None for j in range(2))
        total += float(e_row(ext, cfg, V, blank)[k])
    return total


def to_ctx(h):
    return None if h is None else CO.Hyp(*h[:6])


# ------------------------------------------------------------------------------------------------------------ the tests' seeded cases
LM_WEIGHT, ILM_WEIGHT, BONUS, BOOST = 0.6, -0.3, 0.25, 2.0
NEED_MERGE = {(130, 8, 12), (5, 8, 10), (3, 32, 4)}


def case_sources(V, seed, lm_bf16=False, lm_norm=1, scale=2.0):
    """-> (cfg, sources, (lm, ilm)): the LM's row 2 * standard_normal(V) from 1000 + seed at weight 0.6, the internal LM's from 2000 + seed at
    weight -0.3 and norm 2, a bonus of 0.25 per symbol"""
    lm, ilm = rng_source(1000 + seed, V, scale, bf16=lm_bf16), rng_source(2000 + seed, V, scale)
    cfg = Fuse(BONUS, ((LM_WEIGHT, lm_norm), (ILM_WEIGHT, 2)))
    return cfg, (lambda j, tokens: (lm, ilm)[j](tokens)), (lm, ilm)


def seed_case(make_logits, V, W, T, lens, blank=0, lm_bf16=False, lm_norm=1, scale=2.0, floor=1e-3):
    """the seed rule: the first seed in 0 .. 15 whose key margin is at least `floor` in both configurations (the trivial automaton; the
    four-phrase hotword automaton of test_context_gpu.py at boost 2.0) over the utterances of `lens`, with a final beam that differs from the
    same search without the sources and, for the shapes of NEED_MERGE, a merge.  -> dict(seed, logits, cfg, sources, tables: {name: tb},
    runs: {name: {b: run()}}, phrases); AssertionError if no seed qualifies"""
    import beam_oracle as BO
    for seed in range(16):
        logits = make_logits(seed)
        phrases = CO.phrases_from(BO.run(logits, 0, lens[0], W, blank)[0], V, blank)
        if phrases is None:
            continue
        cfg, sources, _ = case_sources(V, seed, lm_bf16, lm_norm, scale)
        tables = {"trivial": TRIVIAL, "hotword": CO.compile_tables(phrases, [BOOST] * len(phrases))}
        runs = {name: {} for name in tables}
        ok = True
        for name, tb in tables.items():
            for b in range(len(lens)):
                runs[name][b] = run(logits, sources, b, lens[b], W, tb, cfg, blank)
                ok = ok and runs[name][b][1] >= floor
                if not ok:
                    break
            if not ok:
                break
        if not ok:
            continue
        apart = any([h and h.tokens for h in runs[name][b][0]] != [h and h.tokens for h in CO.run(logits, b, lens[b], W, tb, blank)[0]]
                    for name, tb in tables.items() for b in range(len(lens)))
        merges = sum(r[2] for rs in runs.values() for r in rs.values())
        if apart and (merges >= 1 or (V, W, T) not in NEED_MERGE):
            return dict(seed=seed, logits=logits, cfg=cfg, sources=sources, tables=tables, runs=runs, phrases=phrases)
    raise AssertionError("no seed in 0..15 meets the seed rule for V=%d W=%d T=%d" % (V, W, T))


def fuse_bound(n_tokens, cfg, xmax):
    """the kernel tests' bound on |fuse - oracle|: per emitted token and source, |w_j| times the project's bound of an f32 log-probability"""
    return n_tokens * sum(abs(src[0]) * (1e-5 + 4 * 2.0 ** -23 * xmax[j]) for j, src in enumerate(cfg.sources) if src is not None)
