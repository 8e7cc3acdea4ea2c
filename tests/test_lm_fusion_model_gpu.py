"""Language-model fusion through the model: Transducer.recognize_nbest / beam_decode_batch with lm=, lm_weight, ilm_weight on the tiny model
of test_decode_details_gpu.py in the fp32 mode, lengths 12 / 9 / 1, and a seeded two-layer ttmi.lm.TransformerLM of random weights, against
the float64 oracle of the fused rule (tests/beam_fuse_oracle.py) fed the model's own rows - the joint's, the internal LM's (the joint without
an encoder) and the LM's, one hypothesis at a time - as test_context_gpu.py feeds its oracle the joint's.

The input seed is the first of 0 .. 63 at which the oracle's key margins at beam widths 4 and 1 and the gaps of their final orders (by
score + lm_total) are all at least 1e-3, so tokens and frames are compared exactly; scores within T * (1e-5 + 4 * 2^-23 * max|x|), lm_total
within (n_tokens + 1) * sum_j |w_j| * (1e-5 + 4 * 2^-23 * max|x_j|): the kernel tests' bound per token, once more for the closing term."""
import math
import os

import numpy as np
import pytest
import torch

import beam_fuse_oracle as FO
import beam_oracle as BO

pytestmark = pytest.mark.gpu

E2E_LENS = [12, 9, 1]
LM_WEIGHT, ILM_WEIGHT = 0.6, 0.3
CFG = FO.Fuse(0.0, ((LM_WEIGHT, 1), (-ILM_WEIGHT, 2)))
LM_CONFIG = dict(vocab_size=29, n_layer=2, d_model=64, n_head=2, d_head=32, d_inner=96, max_target_length=16, dropout=0.0)


def _lm(seed=11):
    from ttmi.lm import TransformerLM
    torch.manual_seed(seed)
    return TransformerLM(LM_CONFIG).cuda().eval()


@pytest.fixture(scope="module")
def ctx():
    from test_decode_details_gpu import _model
    prev = os.environ.pop("TTMI_PRECISION", None)
    try:
        model, lm = _model(), _lm()
        for seed in range(64):
            x = torch.randn(3, max(E2E_LENS), 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + seed))
            with torch.no_grad():
                enc = model.encoder(x)
            dstates, rows, ext = {}, {}, {}

            def dstate(tokens):
                if tokens not in dstates:
                    with torch.no_grad():
                        dstates[tokens] = model.decoder(torch.tensor([[0] + list(tokens)], device="cuda"))[:, -1, :]
                return dstates[tokens]

            def logits(b, t, tokens):
                if (b, t, tokens) not in rows:
                    with torch.no_grad():
                        rows[(b, t, tokens)] = model.joint(enc[b, t].view(-1), dstate(tokens).view(-1)).float().cpu().numpy()
                return rows[(b, t, tokens)]

            def sources(j, tokens):
                if (j, tokens) not in ext:
                    with torch.no_grad():
                        if j == 0:
                            r = lm.next_logits(torch.tensor([[0] + list(tokens)], device="cuda"))[0]
                        else:
                            r = model.joint(torch.zeros_like(enc[0, 0]).view(-1), dstate(tokens).view(-1))
                    ext[(j, tokens)] = r.float().cpu().numpy()
                return ext[(j, tokens)]

            def eos(tokens):
                return LM_WEIGHT * float(FO.ext_logp(sources(0, tokens), 1)[0])
            four = {b: FO.run(logits, sources, b, E2E_LENS[b], 4, FO.TRIVIAL, CFG) for b in range(3)}
            one = {b: FO.run(logits, sources, b, E2E_LENS[b], 1, FO.TRIVIAL, CFG) for b in range(3)}
            runs = list(four.values()) + list(one.values())
            margin = min(min(r[1], FO.final_order(r[0], FO.TRIVIAL, eos)[1]) for r in runs)
            plain = {b: BO.run(logits, b, E2E_LENS[b], 4) for b in range(3)}
            if margin >= 1e-3 and min(r[1] for r in plain.values()) >= 1e-3:
                break
        else:
            raise AssertionError("no input seed in 0..63 meets the seed rule")
        xmax = max(float(np.abs(r).max()) for r in rows.values())
        smax = [max(float(np.abs(r).max()) for (j, _), r in ext.items() if j == q) for q in range(2)]
        apart = any([h.tokens for h in four[b][0] if h is not None] != [h.tokens for h in plain[b][0]] for b in range(3))
        print("input seed %d, key margin %.3e, plain margin %.3e, max |logit| %.3f, max |LM row| %.3f, max |ILM row| %.3f, the fused beams differ "
              "from the plain ones: %s" % (seed, margin, min(r[1] for r in plain.values()), xmax, smax[0], smax[1], apart))
        yield dict(model=model, lm=lm, x=x, enc=enc, four=four, one=one, plain=plain, eos=eos, smax=smax, bound=1e-5 + 4 * 2.0 ** -23 * xmax)
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def _matches(res, lms, run, ctx, T, what):
    want = FO.final_order(run[0], FO.TRIVIAL, ctx["eos"])[0]
    assert [tuple(r.tokens) for r in res] == [h.tokens for h, _, _ in want], (what, res, want)
    assert [tuple(r.frames) for r in res] == [h.frames for h, _, _ in want], (what, res, want)
    worst_s = max(abs(r.score - h.score) for r, (h, _, _) in zip(res, want))
    assert worst_s <= T * ctx["bound"], (what, worst_s, T * ctx["bound"])
    worst = (0.0, 0.0)
    for got, (h, _, lt) in zip(lms, want):
        bound = FO.fuse_bound(len(h.tokens), CFG, ctx["smax"]) + LM_WEIGHT * (1e-5 + 4 * 2.0 ** -23 * ctx["smax"][0])
        assert isinstance(got, float) and abs(got - lt) <= bound, (what, got, lt, bound)
        worst = max(worst, (abs(got - lt), bound))
    assert all(a.score + la >= b.score + lb for a, la, b, lb in zip(res, lms, res[1:], lms[1:]))
    return worst_s, worst


def test_fused_beam_of_four_matches_the_oracle(ctx):
    model, x = ctx["model"], ctx["x"]
    kw = dict(lm=ctx["lm"], lm_weight=LM_WEIGHT, ilm_weight=ILM_WEIGHT)
    res, lms = model.recognize_nbest(x, torch.tensor(E2E_LENS), beam_width=4, return_lm=True, **kw)
    again = model.beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, return_lm=True, **kw)
    assert again == model.beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, return_lm=True, **kw)
    assert [[(r.tokens, r.frames) for r in u] for u in res] == [[(r.tokens, r.frames) for r in u] for u in again[0]]
    assert model.beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, **kw) == again[0]
    both = model.beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, return_bias=True, return_lm=True, **kw)
    assert both[0] == again[0] and both[2] == again[1] and both[1] == [[0.0] * len(u) for u in again[0]]
    for b in range(3):
        worst_s, (worst_l, bound_l) = _matches(res[b], lms[b], ctx["four"][b], ctx, E2E_LENS[b], b)
        print("utterance %d: %d hypotheses, lm_total %s, max |score - oracle| = %.3e (bound %.3e), max |lm_total - oracle| = %.3e (its bound %.3e)"
              % (b, len(res[b]), ["%.4f" % v for v in lms[b]], worst_s, E2E_LENS[b] * ctx["bound"], worst_l, bound_l))


def test_fused_beam_of_one_follows_the_oracle(ctx):
    res, lms = ctx["model"].beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=1, lm=ctx["lm"], lm_weight=LM_WEIGHT, ilm_weight=ILM_WEIGHT,
                                              return_lm=True)
    for b in range(3):
        assert len(res[b]) == 1
        _matches(res[b], lms[b], ctx["one"][b], ctx, E2E_LENS[b], b)


def test_without_a_language_model_nothing_changes(ctx):
    model, x = ctx["model"], ctx["x"]
    res = model.recognize_nbest(x, torch.tensor(E2E_LENS), beam_width=4)
    assert model.recognize_nbest(x, torch.tensor(E2E_LENS), beam_width=4, lm=None, lm_weight=0.6) == res
    with_zero, zeros = model.recognize_nbest(x, torch.tensor(E2E_LENS), beam_width=4, return_lm=True)
    assert with_zero == res and zeros == [[0.0] * len(u) for u in res]
    for b in range(3):
        want = ctx["plain"][b][0]
        assert [tuple(r.tokens) for r in res[b]] == [h.tokens for h in want] and [tuple(r.frames) for r in res[b]] == [h.frames for h in want]
        assert max(abs(r.score - h.score) for r, h in zip(res[b], want)) <= E2E_LENS[b] * ctx["bound"]


def test_length_bonus_alone_runs_the_fused_step(ctx):
    """a bonus per symbol and nothing else: lm_total = bonus * tokens, exactly (0.25 sums without rounding)"""
    res, lms = ctx["model"].beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, length_bonus=0.25, return_lm=True)
    assert lms == [[0.25 * len(r.tokens) for r in u] for u in res]
    assert all(a.score + la >= b.score + lb for u, l in zip(res, lms) for a, la, b, lb in zip(u, l, u[1:], l[1:]))


def test_bad_fusion_arguments_are_refused(ctx):
    from ttmi.lm import TransformerLM
    model, enc = ctx["model"], ctx["enc"]
    for kw in (dict(lm=ctx["lm"], lm_weight=-0.1), dict(lm=ctx["lm"], lm_weight=float("nan")), dict(ilm_weight=-1.0), dict(ilm_weight=math.inf),
               dict(length_bonus=float("nan")), dict(lm=TransformerLM(LM_CONFIG), lm_weight=0.5)):
        with pytest.raises(ValueError):
            model.beam_decode_batch(enc, E2E_LENS, beam_width=4, **kw)
    with pytest.raises(ValueError):
        model.beam_decode_batch(enc.cpu(), E2E_LENS, beam_width=4, lm=ctx["lm"], lm_weight=0.5)


def test_next_logits_is_the_last_position_of_forward():
    """both run the stack under the causal mask (without one the earlier positions of a two-layer stack look ahead, and the last position of
    the second layer attends to them), so they differ by no more than the rounding of two f32 layers: 1e-4 of the largest logit"""
    prev = os.environ.pop("TTMI_PRECISION", None)
    try:
        lm = _lm()
        h = torch.randint(1, 29, (5, 7), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        h[:, 0] = 0
        with torch.no_grad():
            full, last = lm(h), lm.next_logits(h)
        assert tuple(full.shape) == (5, 7, 29) and tuple(last.shape) == (5, 29) and last.dtype is torch.float32 and last.stride(-1) == 1
        err, scale = float((full[:, -1] - last).abs().max()), float(full.abs().max())
        print("max |forward[:, -1] - next_logits| = %.3e at max |logit| = %.3f" % (err, scale))
        assert err <= 1e-4 * scale
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def test_twenty_adam_steps_lower_the_loss():
    prev = os.environ.pop("TTMI_PRECISION", None)
    try:
        lm = _lm(12).train()
        g = torch.Generator().manual_seed(5)
        tokens = torch.randint(1, 29, (2, 6), generator=g).repeat(4, 1).cuda()       # eight sequences, two distinct
        lengths = torch.tensor([6, 4] * 4).cuda()
        opt = torch.optim.Adam(lm.parameters(), lr=3e-3)
        first = float(lm.loss(tokens, lengths))
        for _ in range(20):
            opt.zero_grad()
            loss = lm.loss(tokens, lengths)
            loss.backward()
            opt.step()
        last = float(lm.loss(tokens, lengths))
        print("loss %.4f -> %.4f" % (first, last))
        assert math.isfinite(first) and last < first
    finally:
        if prev is not None:
            os.environ["TTMI_PRECISION"] = prev


def test_an_ngram_context_starts_in_its_start_state(ctx):
    """NGramLM.from_arpa as context=: slot 0 starts in the <s> context, so every returned bias is the walk of the result's tokens from
    graph.start plus the final weight - the same f32 weights summed in f64 in the same order, hence the same bits - and not the walk from
    the root, which misses <s>'s back-off weight"""
    import beam_ctx_oracle as CO
    from test_ngram_lm import ARPA, SYMBOLS
    from ttmi.lm import NGramLM
    g = NGramLM.from_arpa(ARPA, SYMBOLS, weight=0.5)
    tb = CO.Tables(*(x.numpy() for x in g.cpu_tables()))
    res, biases = ctx["model"].beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4, context=g, return_bias=True)
    from_root = 0
    for u, bs in zip(res, biases):
        for r, got in zip(u, bs):
            s, bias = g.start, 0.0
            for k in r.tokens:
                s, d, _, _ = CO.fsa_step(tb, s, int(k))
                bias += d
            assert got == bias + float(tb.final_w[s]), (r.tokens, got, bias + float(tb.final_w[s]))
            from_root += got != CO.fsa_run(tb, r.tokens)[2]
    assert from_root > 0
