"""The frame-synchronous beam search on the device: ttmi_beam_step driven directly through ops.beam_step beside the float64 oracle of its rule
(tests/beam_oracle.py), frame by frame, and Transducer.recognize_nbest / beam_decode_batch on the tiny model of test_decode_details_gpu.py.

Kernel tests.  Logits of (t, tokens) are 3 * standard_normal(V) in f32 from default_rng([seed, t, len(tokens), *tokens]); the utterances of a
batch of three share that model and differ in their lengths (T, 1, T // 2 + 1), so one has a single frame and two sit finished in the batch
while the longest goes on.  Rows the kernel must not read (empty slots, finished utterances) and the pad of every row are poisoned.  Each case
takes the first seed in 0 .. 15 whose oracle margin (smallest gap between neighbouring scores among the best W + 1 candidates of any step) is
at least 1e-3: the f32 error of a score is orders below that, so tokens, lengths, parents, fresh flags and frames are compared exactly; no seed
qualifying is a failure.  Scores are compared within T times, token log-probabilities within once, the bound
test_greedy_details_gpu.py applies to one row's log-probabilities: 1e-5 + 4 * 2^-23 * max|x|.

Largest errors measured on an MI355X (printed by every test): see DESIGN.md section 4n."""
import math

import numpy as np
import pytest
import torch

import beam_oracle as BO
from test_greedy_kernels_gpu import _padded

pytestmark = pytest.mark.gpu

SHAPES = [(37, 1, 12), (37, 2, 12), (37, 4, 12), (130, 8, 12), (5, 8, 10), (4334, 4, 9), (3, 32, 4)]      # (V, W, T)
POISON_ROW = 1000.0


def _lens(T):
    return [T, 1, T // 2 + 1]


def _make_logits(V, dtype, nan_at=None):
    """seed -> the oracle's callable: the synthetic model, rounded to bf16 and widened again for the bf16 cases (the oracle is fed the values the
    kernel reads); nan_at = (b, t): every row of utterance b at frame t holds one NaN"""
    def make(seed):
        base = BO.rng_logits(seed, V)

        def logits(b, t, tokens):
            x = base(b, t, tokens)
            if dtype is torch.bfloat16:
                x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
            if nan_at == (b, t):
                x = x.copy()
                x[V // 2] = np.nan
            return x
        return logits
    return make


def _seeded(V, W, T, dtype, blank=0, nan_at=None):
    lens = _lens(T)
    found = BO.first_seed(_make_logits(V, dtype, nan_at), [(b, lens[b]) for b in range(3)], W, blank)
    assert found is not None, "no seed in 0..15 with an oracle margin of 1e-3 for V=%d W=%d T=%d" % (V, W, T)
    return found


def _buffers(B, W, ld_hist, ld_det, fill):
    """one beam's arrays, pre-filled so that what the kernel leaves alone is visible"""
    return (torch.full((B, W), -math.inf, dtype=torch.float64).cuda(), torch.full((B, W), fill, dtype=torch.int32).cuda(),
            torch.full((B, W, ld_hist), fill, dtype=torch.long).cuda(), torch.full((B, W, ld_det), fill, dtype=torch.int32).cuda(),
            torch.full((B, W, ld_det), float(fill), dtype=torch.float32).cuda())


def _drive(logits, V, W, lens, dtype, blank=0):
    """the kernel over frames 0 .. max(lens) - 1 beside the oracle -> (every step's outputs as CPU tensors, final oracle beams, worst score
    error, worst tok_lp error, bound per row)"""
    from ttmi import ops
    B, T = len(lens), max(lens)
    ld_hist, ld_det = T + 2, T + 1
    cur, nxt = _buffers(B, W, ld_hist, ld_det, -7), _buffers(B, W, ld_hist, ld_det, -9)
    cur[0][:, 0] = 0.0
    cur[1].zero_()
    cur[2][:, :, 0] = 0                                       # the start symbol; a blank other than 0 changes nothing about column 0
    t = torch.zeros(B, dtype=torch.int32).cuda()
    T_len = torch.tensor(lens, dtype=torch.int32).cuda()
    beams = [list(BO.START) + [None] * (W - 1) for _ in range(B)]
    outputs, worst_score, worst_lp, xmax = [], 0.0, 0.0, 0.0
    for f in range(T):
        rows = torch.full((B, W, V), POISON_ROW)
        rows[:, :, (blank + 1) % V] = 2 * POISON_ROW
        want = []
        for b in range(B):
            if f >= lens[b]:
                want.append(None)
                continue
            r = [logits(b, f, h.tokens) if h is not None else None for h in beams[b]]
            for w, x in enumerate(r):
                if x is not None:
                    rows[b, w] = torch.from_numpy(x)
                    xmax = max(xmax, float(np.nanmax(np.abs(x))))
            want.append(BO.step(beams[b], r, f, W, blank))
        dev_logits = _padded(rows, dtype)
        parent = torch.full((B, W), -3, dtype=torch.int32).cuda()
        fresh = torch.full((B, W), -3, dtype=torch.int32).cuda()
        before = [x.cpu() for x in cur]
        ops.beam_step(dev_logits, t, T_len, cur, nxt, parent, fresh, blank=blank)
        t += 1
        got = [x.cpu() for x in nxt] + [parent.cpu(), fresh.cpu()]
        outputs.append(got)
        score, n_tok, hist, frames, tok_lp, par, fr = got
        bound = 1e-5 + 4 * 2.0 ** -23 * xmax
        for b in range(B):
            what = "frame %d utterance %d" % (f, b)
            if want[b] is None:                               # finished: the beam passes through untouched
                assert par[b].tolist() == list(range(W)) and fr[b].tolist() == [0] * W, what
                assert torch.equal(score[b], before[0][b]) and torch.equal(n_tok[b], before[1][b]), what
                for w in range(W):
                    n = int(n_tok[b, w])
                    assert torch.equal(hist[b, w, :n + 1], before[2][b, w, :n + 1]), what
                    assert torch.equal(frames[b, w, :n], before[3][b, w, :n]) and torch.equal(tok_lp[b, w, :n], before[4][b, w, :n]), what
                continue
            beams[b], w_parent, w_fresh, _, _ = want[b]
            assert par[b].tolist() == w_parent and fr[b].tolist() == w_fresh, (what, par[b].tolist(), w_parent, fr[b].tolist(), w_fresh)
            for w, h in enumerate(beams[b]):
                if h is None:
                    assert float(score[b, w]) == -math.inf and int(n_tok[b, w]) == 0, (what, w)
                    continue
                n = len(h.tokens)
                assert int(n_tok[b, w]) == n and hist[b, w, :n + 1].tolist() == [0] + list(h.tokens), (what, w, hist[b, w].tolist(), h.tokens)
                assert frames[b, w, :n].tolist() == list(h.frames), (what, w, frames[b, w].tolist(), h.frames)
                e = abs(float(score[b, w]) - h.score)
                assert e <= (f + 1) * bound, (what, w, float(score[b, w]), h.score, (f + 1) * bound)
                worst_score = max(worst_score, e)
                for g, l in zip(tok_lp[b, w, :n].tolist(), h.logprobs):
                    assert abs(g - l) <= bound, (what, w, g, l, bound)
                    worst_lp = max(worst_lp, abs(g - l))
        cur, nxt = nxt, cur
    return outputs, beams, worst_score, worst_lp, 1e-5 + 4 * 2.0 ** -23 * xmax


@pytest.fixture(scope="module")
def seeded():
    """(V, W, T, dtype) -> (seed, logits, oracle runs): the seed search of a case is done once"""
    cache = {}

    def get(V, W, T, dtype):
        key = (V, W, T, dtype)
        if key not in cache:
            cache[key] = _seeded(V, W, T, dtype)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,W,T", SHAPES)
def test_beam_step_follows_the_oracle(V, W, T, dtype, seeded):
    seed, logits, runs = seeded(V, W, T, dtype)
    lens = _lens(T)
    outputs, beams, worst_score, worst_lp, bound = _drive(logits, V, W, lens, dtype)
    for b in range(3):                                        # the frame-by-frame drive ends where the oracle's own run ends
        final, margin, gap = runs[(b, lens[b])]
        assert [h for h in beams[b] if h is not None] == final
    print("V=%d W=%d T=%d %s seed %d: margin %.3e, merge gap %.3e, max |score - oracle| = %.3e (bound %.3e), max |tok_lp - oracle| = %.3e (bound %.3e)"
          % (V, W, T, str(dtype)[6:], seed, min(r[1] for r in runs.values()), min(r[2] for r in runs.values()), worst_score, T * bound,
             worst_lp, bound))
    if (V, W, T) == (3, 32, 4):                               # nothing is pruned: the scores are the sums over all decision sequences
        for b in range(3):
            want = BO.brute_force(logits, b, lens[b])
            live = [h for h in beams[b] if h is not None]
            assert {h.tokens for h in live} == set(want)
            step = outputs[lens[b] - 1]                       # the utterance's last own step (later ones pass it through)
            score, n_tok, hist = step[0][b], step[1][b], step[2][b]
            for w, h in enumerate(live):
                assert tuple(hist[w, 1:int(n_tok[w]) + 1].tolist()) == h.tokens
                assert abs(float(score[w]) - want[h.tokens]) <= lens[b] * bound, (b, w, float(score[w]), want[h.tokens])
            assert abs(sum(math.exp(float(s)) for s in score[:len(live)]) - 1.0) <= lens[b] * bound


@pytest.mark.parametrize("blank", [0, 3])
def test_beam_step_with_another_blank(blank):
    V, W, T = 5, 8, 10
    lens = _lens(T)
    found = BO.first_seed(_make_logits(V, torch.float32), [(b, lens[b]) for b in range(3)], W, blank)
    assert found is not None
    _drive(found[1], V, W, lens, torch.float32, blank=blank)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_step_gives_the_same_bits_twice(dtype, seeded):
    V, W, T = 130, 8, 12
    _, logits, _ = seeded(V, W, T, dtype)
    first = _drive(logits, V, W, _lens(T), dtype)[0]
    second = _drive(logits, V, W, _lens(T), dtype)[0]
    assert len(first) == len(second) == T
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))      # bits: NaN or -inf would compare too


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W,frame", [(1, 2), (4, 0)])
def test_beam_step_row_with_nan(W, frame, dtype):
    """one row holding a NaN - the only live row of utterance 0 at that frame (a beam of one at frame 2; the start of a beam of four) - leaves
    that utterance's beam without a finite score from there on; the other utterances follow the oracle as if nothing had happened"""
    V, T = 37, 12
    lens = _lens(T)
    seed, logits, runs = _seeded(V, W, T, dtype, nan_at=(0, frame))
    assert runs[(0, lens[0])][0] == [] and all(runs[(b, lens[b])][0] for b in (1, 2))
    outputs, beams, _, _, _ = _drive(logits, V, W, lens, dtype)
    assert all(h is None for h in beams[0]) and all(beams[b][0] is not None for b in (1, 2))
    for f in range(frame, T):
        assert not torch.isfinite(outputs[f][0][0]).any() and (outputs[f][0][0] == -math.inf).all()
        assert outputs[f][1][0].tolist() == [0] * W and outputs[f][6][0].tolist() == [0] * W


# ---------------------------------------------------------------------------------------------------------------- through the model
E2E_LENS = [12, 9, 1]


@pytest.fixture(scope="module")
def ctx():
    """the tiny model of test_decode_details_gpu.py in the fp32 mode; the input seed is the first of 0 .. 15 whose oracle margin at beam width
    4 is at least 1e-3 (the oracle's logits: the model's own label encoder and joint, one hypothesis at a time)"""
    import os
    from test_decode_details_gpu import _model
    prev = os.environ.pop("TTMI_PRECISION", None)
    try:
        model = _model()
        state = {}

        def make(seed):
            x = torch.randn(3, max(E2E_LENS), 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + seed))
            with torch.no_grad():
                enc = model.encoder(x)
            dstates, rows = {}, {}

            def logits(b, t, tokens):
                if (b, t, tokens) not in rows:
                    with torch.no_grad():
                        if tokens not in dstates:
                            dstates[tokens] = model.decoder(torch.tensor([[0] + list(tokens)], device="cuda"))[:, -1, :]
                        rows[(b, t, tokens)] = model.joint(enc[b, t].view(-1), dstates[tokens].view(-1)).float().cpu().numpy()
                return rows[(b, t, tokens)]
            state[seed] = (x, enc, rows)
            return logits
        found = BO.first_seed(make, [(b, E2E_LENS[b]) for b in range(3)], 4)
        assert found is not None, "no input seed in 0..15 with an oracle margin of 1e-3"
        seed, logits, runs = found
        x, enc, rows = state[seed]
        xmax = max(float(np.abs(r).max()) for r in rows.values())
        print("input seed %d, margin %.3e, max |logit| %.3f" % (seed, min(r[1] for r in runs.values()), xmax))
        yield dict(model=model, x=x, enc=enc, logits=logits, runs=runs, bound=1e-5 + 4 * 2.0 ** -23 * xmax)
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def _well_formed(results, T):
    from tt.model import DecodeResult
    assert all(isinstance(r, DecodeResult) for r in results) and len(results) >= 1
    assert all(a.score >= b.score for a, b in zip(results, results[1:]))
    assert len({tuple(r.tokens) for r in results}) == len(results)
    for r in results:
        assert math.isfinite(r.score) and isinstance(r.score, float) and len(r.frames) == len(r.logprobs) == len(r.tokens)
        assert all(a < b for a, b in zip(r.frames, r.frames[1:])) and all(0 <= f < T for f in r.frames)
        assert all(isinstance(v, int) for v in r.tokens + r.frames) and all(isinstance(v, float) and v <= 0.0 for v in r.logprobs)


def test_beam_of_one_is_greedy_decoding(ctx):
    """on test_decode_details_gpu.py's own input (40 frames, lengths 40 / 37 / 29: the model's blank bias leaves 12 frames without a symbol);
    max|x| of the bound is taken over the lattice of the greedy tokens, which holds every row either decoder scores"""
    model = ctx["model"]
    LENS = [40, 37, 29]
    x = torch.randn(3, 40, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    lens = torch.tensor(LENS)
    greedy = model.recognize(x, lens, details=True)
    beam = model.recognize_nbest(x, lens, beam_width=1)
    assert all(g.tokens for g in greedy)
    targets = torch.zeros(3, max(len(g.tokens) for g in greedy), dtype=torch.long)
    for b, g in enumerate(greedy):
        targets[b, :len(g.tokens)] = torch.tensor(g.tokens)
    with torch.no_grad():
        bound = 1e-5 + 4 * 2.0 ** -23 * float(model(x, targets.cuda()).float().abs().max())
    for b, (g, res) in enumerate(zip(greedy, beam)):
        assert len(res) == 1
        _well_formed(res, LENS[b])
        r = res[0]
        assert r.tokens == g.tokens and r.frames == g.frames, (b, r, g)
        worst = max([abs(a - c) for a, c in zip(r.logprobs, g.logprobs)] or [0.0])
        print("utterance %d: |score - greedy| = %.3e (bound %.3e), max |logprob - greedy| = %.3e (bound %.3e)"
              % (b, abs(r.score - g.score), LENS[b] * bound, worst, bound))
        assert worst <= bound and abs(r.score - g.score) <= LENS[b] * bound


def test_beam_of_four_matches_the_oracle(ctx):
    model, x, enc, runs, bound = ctx["model"], ctx["x"], ctx["enc"], ctx["runs"], ctx["bound"]
    res = model.recognize_nbest(x, torch.tensor(E2E_LENS), beam_width=4)
    again = model.beam_decode_batch(enc, E2E_LENS, beam_width=4)
    assert again == model.beam_decode_batch(enc, E2E_LENS, beam_width=4)         # the same encoder states: the same bits
    assert [[(r.tokens, r.frames) for r in u] for u in res] == [[(r.tokens, r.frames) for r in u] for u in again]
    for b in range(3):
        want = runs[(b, E2E_LENS[b])][0]
        _well_formed(res[b], E2E_LENS[b])
        assert [tuple(r.tokens) for r in res[b]] == [h.tokens for h in want], (b, res[b], want)
        assert [tuple(r.frames) for r in res[b]] == [h.frames for h in want], (b, res[b], want)
        worst_s = max(abs(r.score - h.score) for r, h in zip(res[b], want))
        worst_l = max([abs(a - c) for r, h in zip(res[b], want) for a, c in zip(r.logprobs, h.logprobs)] or [0.0])
        print("utterance %d: %d hypotheses, max |score - oracle| = %.3e (bound %.3e), max |logprob - oracle| = %.3e (bound %.3e)"
              % (b, len(want), worst_s, E2E_LENS[b] * bound, worst_l, bound))
        assert worst_s <= E2E_LENS[b] * bound and worst_l <= bound
    assert len(res[0]) == 4 and len(res[2]) >= 2                                 # the single-frame utterance has blank and symbols in its beam


def test_nbest_is_a_prefix_of_the_full_list(ctx):
    model, enc = ctx["model"], ctx["enc"]
    full = model.beam_decode_batch(enc, E2E_LENS, beam_width=4)
    two = model.beam_decode_batch(enc, E2E_LENS, beam_width=4, nbest=2)
    assert two == [r[:2] for r in full] and all(len(r) == 2 for r in two)
    wide = model.beam_decode_batch(enc, E2E_LENS, beam_width=8, nbest=3)
    for b in range(3):
        _well_formed(wide[b], E2E_LENS[b])
        assert len(wide[b]) == 3


def test_no_finite_score_is_an_error(ctx):
    model, enc = ctx["model"], ctx["enc"]
    bad = enc.clone()
    bad[1, 0, 5] = float("nan")
    with pytest.raises(RuntimeError, match="no hypothesis with a finite score"):
        model.beam_decode_batch(bad, E2E_LENS, beam_width=4)
    with pytest.raises(ValueError):
        model.beam_decode_batch(enc, E2E_LENS, beam_width=33)
