"""Language-model fusion on the device: ttmi_beam_step_fuse driven through ops.beam_step_fuse beside the float64 oracle of its rule
(tests/beam_fuse_oracle.py), frame by frame.  The method is tests/test_context_gpu.py's: the same synthetic logits, batches of three with
lengths (T, 1, T // 2 + 1); the pad, the rows of empty slots and the rows of finished utterances are poisoned in all three row tensors (the
logits, the LM's rows, the internal LM's rows).

The sources are functions of the tokens alone: the LM's row is 2 * standard_normal(V) as f32 from default_rng([1000 + seed, len(tokens),
*tokens]) at weight 0.6 and norm 1, the internal LM's the same from 2000 + seed at weight -0.3 and norm 2; the bonus per symbol is 0.25.  One
case holds the LM's rows in bf16, one passes them with norm 0.  Both run under the trivial automaton (S = 1, A = 0) and under the four-phrase
hotword automaton of test_context_gpu.py at boost 2.0.  Each case takes the first seed in 0 .. 15 whose oracle KEY margin is at least 1e-3 in
both configurations over the three utterances, with a final beam that differs from the same search without the sources and - for (130, 8, 12),
(5, 8, 10), (3, 32, 4) - a merge; no seed qualifying is a failure.

Tokens, lengths, parents, fresh flags, frames, states and the bias (as f64 bits) are compared exactly; scores within (f + 1) times the bound of
test_beam_gpu.py, 1e-5 + 4 * 2^-23 * max|x|; fuse within n_tokens * sum_j |w_j| * (1e-5 + 4 * 2^-23 * max|x_j|): that bound per f32
log-probability, per emitted token, times the weights.

Seeds, margins and the largest errors measured on an MI355X (printed by every test): see DESIGN.md section 4s."""
import math

import numpy as np
import pytest
import torch

import beam_ctx_oracle as CO
import beam_fuse_oracle as FO
from test_beam_gpu import POISON_ROW, _lens, _make_logits
from test_context_gpu import _buffers, _graph, _rows, _start
from test_greedy_kernels_gpu import _padded

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 12), (37, 4, 12), (130, 8, 12), (5, 8, 10), (4334, 4, 9), (3, 32, 4)]      # (V, W, T)


@pytest.fixture(scope="module")
def seeded():
    cache = {}

    def get(V, W, T, dtype, lm_bf16=False, lm_norm=1, blank=0):
        key = (V, W, T, dtype, lm_bf16, lm_norm, blank)
        if key not in cache:
            cache[key] = FO.seed_case(_make_logits(V, dtype), V, W, T, _lens(T), blank=blank, lm_bf16=lm_bf16, lm_norm=lm_norm)
        return cache[key]
    return get


def _ext_rows(source, beams, lens, f, V, blank):
    """one source's [B, W, V] rows for the frame: poison everywhere the kernel must not read -> (rows, max |x| of the real rows)"""
    B, W = len(beams), len(beams[0])
    rows = torch.full((B, W, V), POISON_ROW)
    rows[:, :, (blank + 1) % V] = float("nan")
    xmax = 0.0
    for b in range(B):
        if f >= lens[b]:
            continue
        for w, tokens in enumerate(beams[b]):
            if tokens is not None:
                x = source(tokens)
                rows[b, w] = torch.from_numpy(x)
                xmax = max(xmax, float(np.abs(x).max()))
    return rows, xmax


def _fuse_start(B, W, fill):
    fuse = torch.full((B, W), float(fill), dtype=torch.float64).cuda()
    fuse[:, 0] = 0.0
    return fuse


def _drive(case, name, V, W, lens, dtype, lm_dtype=torch.float32, blank=0, cfg=None, check=True):
    """the kernel over frames 0 .. max(lens) - 1 beside the oracle under the automaton `name` of the case -> (every step's outputs as CPU
    tensors, final oracle beams, worst score error, worst fuse error and its bound, key margin)"""
    from ttmi import ops
    logits, sources, tb = case["logits"], case["sources"], case["tables"][name]
    cfg = case["cfg"] if cfg is None else cfg
    graph = _graph(tb)
    B, T = len(lens), max(lens)
    ld_hist, ld_det = T + 2, T + 1
    (cur, cur_ctx), (nxt, nxt_ctx) = _start(B, W, ld_hist, ld_det, -7), _buffers(B, W, ld_hist, ld_det, -9)
    cur_fuse, nxt_fuse = _fuse_start(B, W, -7), torch.full((B, W), -9.0, dtype=torch.float64).cuda()
    ws = ops.beam_fuse_workspace(B, W, V, "cuda")
    ws.fill_(0xff)
    t = torch.zeros(B, dtype=torch.int32).cuda()
    T_len = torch.tensor(lens, dtype=torch.int32).cuda()
    beams = [FO.START + [None] * (W - 1) for _ in range(B)]
    outputs, worst_score, worst_fuse, worst_bound, xmax, smax, margin = [], 0.0, 0.0, 0.0, 0.0, [0.0, 0.0], math.inf
    for f in range(T):
        toks = [[h.tokens if h is not None else None for h in bm] for bm in beams]
        rows, m = _rows(logits, toks, lens, f, V, blank)
        xmax = max(xmax, m)
        ext, dev_ext = [], []
        for j in range(2):
            if cfg.sources[j] is None:
                ext.append(None)
                dev_ext.append(None)
                continue
            e, m = _ext_rows(lambda tokens, j=j: sources(j, tokens), toks, lens, f, V, blank)
            smax[j] = max(smax[j], m)
            ext.append(e)
            dev_ext.append((_padded(e, lm_dtype if j == 0 else torch.float32, pad=5 + j), cfg.sources[j][0], cfg.sources[j][1]))
        want = [FO.step(beams[b], [rows[b, w].numpy() if h is not None else None for w, h in enumerate(beams[b])],
                        [tuple(e[b, w].numpy() if e is not None else None for e in ext) if h is not None else None
                         for w, h in enumerate(beams[b])], f, W, tb, cfg, blank) if f < lens[b] else None for b in range(B)]
        parent = torch.full((B, W), -3, dtype=torch.int32).cuda()
        fresh = torch.full((B, W), -3, dtype=torch.int32).cuda()
        before = [x.cpu() for x in cur + cur_ctx] + [cur_fuse.cpu()]
        ops.beam_step_fuse(_padded(rows, dtype), t, T_len, cur, nxt, parent, fresh, graph.tables, cur_ctx, nxt_ctx, ws, cur_fuse, nxt_fuse,
                           sources=dev_ext, sym_bonus=cfg.bonus, blank=blank)
        t += 1
        got = [x.cpu() for x in nxt] + [parent.cpu(), fresh.cpu()] + [x.cpu() for x in nxt_ctx] + [nxt_fuse.cpu()]
        outputs.append(got)
        score, n_tok, hist, frames, tok_lp, par, fr, state, bias, fuse = got
        bound = 1e-5 + 4 * 2.0 ** -23 * xmax
        for b in range(B):
            what = "%s frame %d utterance %d" % (name, f, b)
            if not check:
                if want[b] is not None:
                    beams[b] = want[b][0]
                continue
            if want[b] is None:                               # finished: the beam passes through untouched, state, bias and fuse with it
                assert par[b].tolist() == list(range(W)) and fr[b].tolist() == [0] * W, what
                assert torch.equal(score[b], before[0][b]) and torch.equal(n_tok[b], before[1][b]), what
                assert torch.equal(state[b], before[5][b]) and torch.equal(bias[b].view(torch.int64), before[6][b].view(torch.int64)), what
                assert torch.equal(fuse[b].view(torch.int64), before[7][b].view(torch.int64)), what
                continue
            beams[b], w_parent, w_fresh, m, _ = want[b]
            margin = min(margin, m)
            assert par[b].tolist() == w_parent and fr[b].tolist() == w_fresh, (what, par[b].tolist(), w_parent, fr[b].tolist(), w_fresh)
            for w, h in enumerate(beams[b]):
                if h is None:                                 # an empty new slot: state 0, bias 0, fuse 0
                    assert float(score[b, w]) == -math.inf and int(n_tok[b, w]) == 0, (what, w)
                    assert int(state[b, w]) == 0 and bias[b, w:w + 1].view(torch.int64).item() == 0, (what, w)
                    assert fuse[b, w:w + 1].view(torch.int64).item() == 0, (what, w)
                    continue
                n = len(h.tokens)
                assert int(n_tok[b, w]) == n and hist[b, w, :n + 1].tolist() == [0] + list(h.tokens), (what, w, hist[b, w].tolist(), h.tokens)
                assert frames[b, w, :n].tolist() == list(h.frames), (what, w, frames[b, w].tolist(), h.frames)
                assert int(state[b, w]) == h.state, (what, w, int(state[b, w]), h.state)
                assert bias[b, w:w + 1].view(torch.int64).item() == np.float64(h.bias).view(np.int64), (what, w, float(bias[b, w]), h.bias)
                e = abs(float(score[b, w]) - h.score)
                assert e <= (f + 1) * bound, (what, w, float(score[b, w]), h.score, (f + 1) * bound)
                worst_score = max(worst_score, e)
                fb = FO.fuse_bound(n, cfg, smax)
                e = abs(float(fuse[b, w]) - h.fuse)
                assert e <= fb, (what, w, float(fuse[b, w]), h.fuse, fb)
                if e > worst_fuse:
                    worst_fuse, worst_bound = e, fb
        cur, nxt, cur_ctx, nxt_ctx, cur_fuse, nxt_fuse = nxt, cur, nxt_ctx, cur_ctx, nxt_fuse, cur_fuse
    return outputs, beams, worst_score, (worst_fuse, worst_bound), margin, (T * (1e-5 + 4 * 2.0 ** -23 * xmax), smax)


def _follow(case, V, W, T, dtype, what, **kw):
    lens = _lens(T)
    for name in ("trivial", "hotword"):
        _, beams, worst_score, (worst_fuse, fuse_bound), margin, (score_bound, smax) = _drive(case, name, V, W, lens, dtype, **kw)
        for b in range(3):                                    # the frame-by-frame drive ends where the oracle's own run ends
            assert beams[b] == case["runs"][name][b][0]
        both = score_bound + FO.fuse_bound(T, case["cfg"], smax)
        assert both < 1e-3, "score and fuse bounds together (%.3e) do not stay below the margin floor" % both
        print("%s V=%d W=%d T=%d %s seed %d %s: key margin %.3e, merges %d, max |score - oracle| = %.3e (bound %.3e), max |fuse - oracle| = %.3e "
              "(its bound %.3e), both bounds %.3e" % (what, V, W, T, str(dtype)[6:], case["seed"], name,
                                                      min(r[1] for r in case["runs"][name].values()),
                                                      sum(r[2] for r in case["runs"][name].values()), worst_score, score_bound, worst_fuse,
                                                      fuse_bound, both))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,W,T", SHAPES)
def test_beam_step_fuse_follows_the_oracle(V, W, T, dtype, seeded):
    _follow(seeded(V, W, T, dtype), V, W, T, dtype, "f32 sources")


def test_beam_step_fuse_with_a_bf16_source(seeded):
    V, W, T = 130, 8, 12
    _follow(seeded(V, W, T, torch.float32, lm_bf16=True), V, W, T, torch.float32, "bf16 LM rows", lm_dtype=torch.bfloat16)


def test_beam_step_fuse_with_log_probability_rows(seeded):
    """norm 0: the LM's rows are taken as they are and no pass is made over them"""
    V, W, T = 37, 4, 12
    _follow(seeded(V, W, T, torch.float32, lm_norm=0), V, W, T, torch.float32, "norm 0 LM rows")


def test_beam_step_fuse_with_another_blank(seeded):
    """blank = 3 of V = 5: the internal LM's norm 2 leaves entry 3 out of its sum"""
    V, W, T, blank = 5, 8, 10, 3
    case = seeded(V, W, T, torch.float32, blank=blank)
    assert all(blank not in p for p in case["phrases"])
    for name in ("trivial", "hotword"):
        beams = _drive(case, name, V, W, _lens(T), torch.float32, blank=blank)[1]
        assert [beams[b] == case["runs"][name][b][0] for b in range(3)] == [True] * 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_step_fuse_gives_the_same_bits_twice(dtype, seeded):
    V, W, T = 130, 8, 12
    case = seeded(V, W, T, dtype)
    first = _drive(case, "hotword", V, W, _lens(T), dtype, check=False)[0]
    second = _drive(case, "hotword", V, W, _lens(T), dtype, check=False)[0]
    assert len(first) == len(second) == T
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,W,T", [(130, 8, 12), (4334, 4, 9)])
def test_without_sources_and_bonus_it_is_beam_step_ctx_bit_for_bit(V, W, T, dtype, seeded):
    """no source, no bonus: on the same inputs every output ops.beam_step_ctx also has is ops.beam_step_ctx's, as raw bytes, over all frames,
    under the hotword automaton; fuse_out is all zero.  The drive takes the next frame's hypotheses from the kernel's own histories."""
    from ttmi import ops
    case = seeded(V, W, T, dtype)
    graph = _graph(case["tables"]["hotword"])
    lens = _lens(T)
    B = len(lens)
    ld_hist, ld_det = T + 2, T + 1
    (cur, cur_ctx), (nxt, nxt_ctx) = _start(B, W, ld_hist, ld_det, -7), _buffers(B, W, ld_hist, ld_det, -9)
    cur_ctx[1].zero_()
    ref, ref_ctx = _buffers(B, W, ld_hist, ld_det, -9)
    cur_fuse, nxt_fuse = torch.zeros(B, W, dtype=torch.float64).cuda(), torch.full((B, W), -9.0, dtype=torch.float64).cuda()
    ws, ws_ref = ops.beam_fuse_workspace(B, W, V, "cuda"), ops.beam_ctx_workspace(B, W, V, "cuda")
    t = torch.zeros(B, dtype=torch.int32).cuda()
    T_len = torch.tensor(lens, dtype=torch.int32).cuda()
    beams = [[()] + [None] * (W - 1) for _ in range(B)]
    biased = False
    for f in range(T):
        rows, _ = _rows(case["logits"], beams, lens, f, V, 0)
        dev = _padded(rows, dtype)
        par, fr, par0, fr0 = (torch.full((B, W), -3, dtype=torch.int32).cuda() for _ in range(4))
        for dst, src in zip(list(ref) + list(ref_ctx), list(nxt) + list(nxt_ctx)):      # the same bytes in both sets of output buffers
            dst.copy_(src)
        ops.beam_step_fuse(dev, t, T_len, cur, nxt, par, fr, graph.tables, cur_ctx, nxt_ctx, ws, cur_fuse, nxt_fuse)
        ops.beam_step_ctx(dev, t, T_len, cur, ref, par0, fr0, graph.tables, cur_ctx, ref_ctx, ws_ref)
        t += 1
        for x, y in zip(list(nxt) + list(nxt_ctx) + [par, fr], list(ref) + list(ref_ctx) + [par0, fr0]):
            assert x.dtype == y.dtype and torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8)), "frame %d" % f
        assert nxt_fuse.cpu().view(torch.int64).eq(0).all(), "frame %d" % f
        biased = biased or bool(nxt_ctx[1].ne(0).any())
        score, n_tok, hist = nxt[0].cpu(), nxt[1].cpu(), nxt[2].cpu()
        for b in range(B):
            if f < lens[b]:
                beams[b] = [tuple(hist[b, w, 1:int(n_tok[b, w]) + 1].tolist()) if float(score[b, w]) > -math.inf else None for w in range(W)]
        cur, nxt, cur_ctx, nxt_ctx, cur_fuse, nxt_fuse = nxt, cur, nxt_ctx, cur_ctx, nxt_fuse, cur_fuse
    assert biased


def test_non_finite_sources_on_the_device():
    """one frame at V = 5, W = 4 from the start: a source row of all -inf, a NaN row and a single -inf entry under a negative weight"""
    from ttmi import ops
    V, W = 5, 4
    logits = CO.rng_logits(1, V)
    x = np.array([0.5, -1.0, 2.0, 0.0, 1.0], dtype=np.float32)
    y = x.copy()
    y[2] = -np.inf
    graph = _graph(FO.TRIVIAL)
    for row, cfg in ((np.full(V, -np.inf, dtype=np.float32), FO.Fuse(0.0, ((0.6, 1), None))),
                     (np.full(V, np.nan, dtype=np.float32), FO.Fuse(0.25, ((0.6, 0), None))), (y, FO.Fuse(0.0, ((-0.3, 1), None)))):
        (cur, cur_ctx), (nxt, nxt_ctx) = _start(1, W, 3, 2, -7), _buffers(1, W, 3, 2, -9)
        cur_fuse, nxt_fuse = _fuse_start(1, W, -7), torch.full((1, W), -9.0, dtype=torch.float64).cuda()
        rows = torch.full((1, W, V), POISON_ROW)
        rows[0, 0] = torch.from_numpy(logits(0, 0, ()))
        ext = torch.full((1, W, V), float("nan"))
        ext[0, 0] = torch.from_numpy(row)
        want = FO.step(FO.START + [None] * (W - 1), [rows[0, 0].numpy()] + [None] * (W - 1), [(row, None)] + [None] * (W - 1), 0, W, FO.TRIVIAL,
                       cfg)
        par, fr = (torch.full((1, W), -3, dtype=torch.int32).cuda() for _ in range(2))
        ops.beam_step_fuse(_padded(rows, torch.float32), torch.zeros(1, dtype=torch.int32).cuda(), torch.ones(1, dtype=torch.int32).cuda(), cur,
                           nxt, par, fr, graph.tables, cur_ctx, nxt_ctx, ops.beam_fuse_workspace(1, W, V, "cuda"), cur_fuse, nxt_fuse,
                           sources=[(_padded(ext, torch.float32), cfg.sources[0][0], cfg.sources[0][1])], sym_bonus=cfg.bonus)
        n_tok, hist, score, fuse = nxt[1].cpu(), nxt[2].cpu(), nxt[0].cpu(), nxt_fuse.cpu()
        assert par.cpu()[0].tolist() == want[1] and fr.cpu()[0].tolist() == want[2]
        for w, h in enumerate(want[0]):
            if h is None:
                assert float(score[0, w]) == -math.inf and float(fuse[0, w]) == 0.0
            else:
                assert hist[0, w, 1:int(n_tok[0, w]) + 1].tolist() == list(h.tokens) and abs(float(fuse[0, w]) - h.fuse) <= 1e-5


def _call(**change):
    """a well-formed one-frame call at B = 1, W = 2, V = 5 with two sources, then `change` applied -> the call's keyword arguments"""
    from ttmi import ops
    B, W, V = 1, 2, 5
    (cur, cur_ctx), (nxt, nxt_ctx) = _start(B, W, 3, 2, -7), _buffers(B, W, 3, 2, -9)
    kw = dict(logits=torch.zeros(B, W, V).cuda(), t=torch.zeros(B, dtype=torch.int32).cuda(), T_len=torch.ones(B, dtype=torch.int32).cuda(),
              beam_in=cur, beam_out=nxt, parent=torch.zeros(B, W, dtype=torch.int32).cuda(), fresh=torch.zeros(B, W, dtype=torch.int32).cuda(),
              tables=_graph(FO.TRIVIAL).tables, ctx_in=cur_ctx, ctx_out=nxt_ctx, ws=ops.beam_fuse_workspace(B, W, V, "cuda"),
              fuse_in=_fuse_start(B, W, 0), fuse_out=torch.zeros(B, W, dtype=torch.float64).cuda(),
              sources=[(torch.zeros(B, W, V).cuda(), 0.6, 1), (torch.zeros(B, W, V).cuda(), -0.3, 2)], sym_bonus=0.25)
    for k, v in change.items():
        kw[k] = v(kw) if callable(v) else v
    return kw


def test_beam_step_fuse_refuses_bad_arguments():
    from ttmi import ops
    ops.beam_step_fuse(**_call())                             # the well-formed call passes
    src = lambda kw, j, **c: [tuple(c.get(n, s[i]) for i, n in enumerate(("rows", "weight", "norm"))) if q == j else s      # noqa: E731
                              for q, s in enumerate(kw["sources"])]
    bad = dict(
        norm_3=dict(sources=lambda kw: src(kw, 0, norm=3)), norm_negative=dict(sources=lambda kw: src(kw, 1, norm=-1)),
        weight_nan=dict(sources=lambda kw: src(kw, 0, weight=float("nan"))), weight_inf=dict(sources=lambda kw: src(kw, 1, weight=math.inf)),
        bonus_inf=dict(sym_bonus=math.inf), bonus_nan=dict(sym_bonus=float("nan")),
        pitch_below_V=dict(sources=lambda kw: src(kw, 0, rows=torch.zeros(16).cuda().as_strided((1, 2, 5), (8, 4, 1)))),
        fuse_out_is_fuse_in=dict(fuse_out=lambda kw: kw["fuse_in"]),
        source_is_the_workspace=dict(sources=lambda kw: src(kw, 1, rows=kw["ws"].view(torch.float32)[:10].view(1, 2, 5))),
        source_is_score_out=dict(), source_overlaps_fuse_out=dict(),      # (built below: the source and the output share one buffer)
        state_out_is_state_in=dict(ctx_out=lambda kw: (kw["ctx_in"][0], kw["ctx_out"][1])),      # (one of what beam_step_ctx refuses)
        score_out_is_score_in=dict(beam_out=lambda kw: (kw["beam_in"][0],) + tuple(kw["beam_out"][1:])),
    )
    for name, change in bad.items():
        kw = _call()
        for k in ("fuse_out", "beam_out", "ctx_out", "sym_bonus", "sources"):       # (in this order: a source may be built on a changed buffer)
            if k in change:
                kw[k] = change[k](kw) if callable(change[k]) else change[k]
        if name == "source_is_score_out":
            rows = torch.zeros(16, dtype=torch.float32).cuda()
            kw["sources"] = [(rows[:10].view(1, 2, 5), 0.6, 1), kw["sources"][1]]
            kw["beam_out"] = (rows[4:8].view(torch.float64).view(1, 2),) + tuple(kw["beam_out"][1:])
        if name == "source_overlaps_fuse_out":                # fuse_out = bytes 0 .. 15 of a buffer, the source's rows bytes 8 .. 47
            big = torch.zeros(8, dtype=torch.float64).cuda()
            kw["fuse_out"] = big[:2].view(1, 2)
            kw["sources"] = [kw["sources"][0], (big.view(torch.float32)[2:12].view(1, 2, 5), -0.3, 2)]
        with pytest.raises(ValueError, match="beam_step_fuse"):
            ops.beam_step_fuse(**kw)
    with pytest.raises(ValueError):                           # a CPU tensor never reaches the library
        ops.beam_step_fuse(**_call(fuse_in=torch.zeros(1, 2, dtype=torch.float64)))
    with pytest.raises(ValueError):
        ops.beam_step_fuse(**_call(sources=lambda kw: [(torch.zeros(1, 2, 5), 0.6, 1)]))
