"""Rescoring of the beam's N-best with the CTC head (Transducer.beam_decode_batch / recognize_nbest with ctc_weight, Transducer.ctc_score) on a
tiny Transducer built with ctc_weight > 0 in its config, in the fp32 mode.  The scorer itself is tested raw in tests/test_ctc_score_gpu.py.
Unless a test sets another width the runs use beam_width = nbest = 4."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
W = 4
LENS = [12, 9, 6]


def _tiny(ctc_weight=0.3):
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=2, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0, ctc_weight=ctc_weight))
    torch.manual_seed(9)
    model = Transducer(cfg).cuda().eval()
    with torch.no_grad():
        model.joint.project_layer.bias[0] += 0.9             # some blank frames between the emissions
    return model


@pytest.fixture(scope="module")
def ctx():
    prev = os.environ.get("TTMI_PRECISION")
    os.environ["TTMI_PRECISION"] = "fp32"
    try:
        model = _tiny()
        x = torch.randn(3, max(LENS), 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(103))
        with torch.no_grad():
            enc = model.encoder(x)
        plain = model.beam_decode_batch(enc, LENS, beam_width=W)                 # without a context or fusion: the slots in their order
        assert all(len(r) >= 3 for r in plain[:2])
        yield dict(model=model, x=x, enc=enc, plain=plain)
    finally:
        if prev is None:
            os.environ.pop("TTMI_PRECISION", None)
        else:
            os.environ["TTMI_PRECISION"] = prev


def _tokens(results):
    return [[r.tokens for r in u] for u in results]


def _key_order(results, ctcs, lam, biases=None, lms=None):
    """the documented order of one utterance's slots: score + final_bias + lm_total + lam * ctc in that order, descending, the slot ascending on
    ties; a hypothesis the head cannot align (or a NaN) after all others, by the key without the head's term"""
    n = len(results)
    biases, lms = biases or [0.0] * n, lms or [0.0] * n

    def key(i):
        base = results[i].score + biases[i] + lms[i]
        return (0, -(base + lam * ctcs[i]), i) if math.isfinite(ctcs[i]) else (1, -base, i)
    return sorted(range(n), key=key)


def test_ctc_score_is_minus_the_ctc_loss_of_the_heads_logits(ctx):
    from ttmi.ctc import ctc_loss
    model, x, enc, plain = ctx["model"], ctx["x"], ctx["enc"], ctx["plain"]
    nested = _tokens(plain)
    nested[1] = nested[1] + [[5, 5, 7], []]
    got = model.ctc_score(x, torch.tensor(LENS), nested)
    assert [len(u) for u in got] == [len(u) for u in nested] and all(isinstance(v, float) for u in got for v in u)
    logits = model._ctc_head_logits(enc)
    flat = [(b, h) for b in range(3) for h in nested[b]]
    U = max(len(h) for _, h in flat)
    lab = torch.zeros(len(flat), U, dtype=torch.int32)
    for p, (_, h) in enumerate(flat):
        if h:
            lab[p, :len(h)] = torch.tensor(h, dtype=torch.int32)
    idx = torch.tensor([b for b, _ in flat], device="cuda")
    costs = ctc_loss(logits[idx].contiguous(), lab, torch.tensor([LENS[b] for b, _ in flat]), torch.tensor([len(h) for _, h in flat]),
                     reduction="none").cpu().tolist()
    mine = [v for u in got for v in u]
    assert all(math.isfinite(v) for v in mine)
    worst = max(abs(a + c) / abs(c) for a, c in zip(mine, costs))
    print("Transducer.ctc_score against -ctc_loss on %d hypotheses: largest relative difference %.3e" % (len(mine), worst))
    assert worst <= TOL


def test_weight_zero_changes_nothing(ctx):
    model, x, enc, plain = ctx["model"], ctx["x"], ctx["enc"], ctx["plain"]
    assert model.beam_decode_batch(enc, LENS, beam_width=W, ctc_weight=0.0, return_ctc=False) == plain
    assert model.beam_decode_batch(enc, LENS, beam_width=W, nbest=2, ctc_weight=0) == [u[:2] for u in plain]
    a = model.recognize_nbest(x, torch.tensor(LENS), beam_width=W)
    assert model.recognize_nbest(x, torch.tensor(LENS), beam_width=W, ctc_weight=0.0) == a
    # the values alone, asked for without a weight: the plain lists in the plain order, and the head's score of each
    res, ctcs = model.beam_decode_batch(enc, LENS, beam_width=W, return_ctc=True)
    assert res == plain and ctcs == model.ctc_score(x, torch.tensor(LENS), _tokens(plain))


@pytest.mark.parametrize("lam", [0.3, 5.0])
def test_weighted_order_is_the_documented_key(ctx, lam):
    model, x, enc, plain = ctx["model"], ctx["x"], ctx["enc"], ctx["plain"]
    res, ctcs = model.beam_decode_batch(enc, LENS, beam_width=W, ctc_weight=lam, return_ctc=True)
    again = model.recognize_nbest(x, torch.tensor(LENS), beam_width=W, ctc_weight=lam, return_ctc=True)
    assert _tokens(again[0]) == _tokens(res) and again[1] == ctcs
    head = model.ctc_score(x, torch.tensor(LENS), _tokens(plain))
    moved = 0
    for b in range(3):
        # the same hypotheses with the same scores, frames and log-probabilities - only their order may differ
        assert sorted(res[b], key=lambda r: r.tokens) == sorted(plain[b], key=lambda r: r.tokens)
        assert ctcs[b] == model.ctc_score(x, torch.tensor(LENS), [_tokens(res)[i] if i == b else [] for i in range(3)])[b]
        order = _key_order(plain[b], head[b], lam)
        assert [r.tokens for r in res[b]] == [plain[b][i].tokens for i in order], (b, lam, res[b], plain[b], head[b])
        assert ctcs[b] == [head[b][i] for i in order]
        moved += order != list(range(len(order)))
    print("ctc_weight %.1f: %d of 3 lists reordered" % (lam, moved))


def _prefer(model, hyp):
    """the head made to prefer `hyp` whatever the audio: weight zero, the bias high on the hypothesis's tokens, low on blank, lowest elsewhere"""
    with torch.no_grad():
        model.ctc_head.weight.zero_()
        model.ctc_head.bias.fill_(-30.0)
        model.ctc_head.bias[0] = -6.0
        for v in hyp:
            model.ctc_head.bias[v] = 0.0


def test_the_head_promotes_the_last_hypothesis_into_the_cut(ctx):
    """nbest = 2 of a beam of 4: the plain cut holds slots 0 and 1.  With a head that prefers the last-ranked hypothesis (constructed per
    utterance; it qualifies when the head then scores that hypothesis strictly above the utterance's others) and a weight large enough for the
    key, that hypothesis leads the cut list: promoted from outside the cut, and the 1-best has changed"""
    model, x, enc, plain = ctx["model"], ctx["x"], ctx["enc"], ctx["plain"]
    saved = (model.ctc_head.weight.detach().clone(), model.ctc_head.bias.detach().clone())
    lens = torch.tensor(LENS)
    promoted = 0
    try:
        for b in range(3):
            if len(plain[b]) < 3 or not plain[b][-1].tokens:
                continue
            last = plain[b][-1]
            _prefer(model, last.tokens)
            head = model.ctc_score(x, lens, _tokens(plain))[b]
            gaps = [head[-1] - v for v in head[:-1]]
            print("utterance %d: last-ranked %s, head's score %.3f, margin over the others %.3f" % (b, last.tokens, head[-1], min(gaps)))
            if not (math.isfinite(head[-1]) and min(gaps) > 0.0):
                continue
            lam = 1.0 + 2.0 * max((r.score - last.score) / g for r, g in zip(plain[b][:-1], gaps))
            cut, ctcs = model.beam_decode_batch(enc, LENS, beam_width=W, nbest=2, ctc_weight=lam, return_ctc=True)
            assert all(len(u) <= 2 for u in cut) and len(cut[b]) == 2
            assert last.tokens not in [r.tokens for r in plain[b][:2]]          # outside the plain cut ...
            assert cut[b][0] == last and ctcs[b][0] == head[-1]                  # ... and now its head, with the model's own score
            assert cut[b][0].tokens != plain[b][0].tokens                        # this utterance's 1-best has changed
            promoted += 1
    finally:
        with torch.no_grad():
            model.ctc_head.weight.copy_(saved[0])
            model.ctc_head.bias.copy_(saved[1])
    assert promoted >= 1, "no utterance qualified: the case is vacuous"


def test_return_ctc_composes_with_bias_and_lm(ctx):
    model, x, enc = ctx["model"], ctx["x"], ctx["enc"]
    ret = model.beam_decode_batch(enc, LENS, beam_width=W, length_bonus=0.25, ctc_weight=0.7, return_bias=True, return_lm=True, return_ctc=True)
    assert isinstance(ret, tuple) and len(ret) == 4
    res, biases, lms, ctcs = ret
    fused = model.beam_decode_batch(enc, LENS, beam_width=W, length_bonus=0.25, return_lm=True)
    head = model.ctc_score(x, torch.tensor(LENS), _tokens(res))
    for b in range(3):
        n = len(res[b])
        assert len(biases[b]) == len(lms[b]) == len(ctcs[b]) == n and biases[b] == [0.0] * n
        assert all(abs(v - 0.25 * len(r.tokens)) < 1e-9 for v, r in zip(lms[b], res[b]))                  # lm_total = the length bonus
        assert ctcs[b] == head[b]
        assert sorted(res[b], key=lambda r: r.tokens) == sorted(fused[0][b], key=lambda r: r.tokens)
        keys = [r.score + biases[b][i] + lms[b][i] + 0.7 * ctcs[b][i] for i, r in enumerate(res[b])]
        assert all(math.isfinite(k) for k in keys) and all(a >= c for a, c in zip(keys, keys[1:])), (b, keys)
    two = model.beam_decode_batch(enc, LENS, beam_width=W, ctc_weight=0.7, return_ctc=True, return_bias=True)
    assert len(two) == 3 and two[1] == [[0.0] * len(u) for u in two[0]] and all(isinstance(v, float) for u in two[2] for v in u)


def test_arguments_are_checked(ctx):
    model, enc = ctx["model"], ctx["enc"]
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ctc_weight must be finite and >= 0"):
            model.beam_decode_batch(enc, LENS, beam_width=W, ctc_weight=bad)
    with pytest.raises(ValueError, match="GPU"):
        model.ctc_score(ctx["x"].cpu(), torch.tensor(LENS), [[[1]], [], []])


def test_a_model_without_the_head_raises():
    model = _tiny(0.0)
    assert getattr(model, "ctc_head", None) is None
    x = torch.randn(2, 6, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        enc = model.encoder(x)
    msg = "no CTC head: build it with config.ctc_weight > 0"
    with pytest.raises(ValueError, match=msg):
        model.beam_decode_batch(enc, [6, 5], beam_width=2, ctc_weight=0.5)
    with pytest.raises(ValueError, match=msg):
        model.beam_decode_batch(enc, [6, 5], beam_width=2, return_ctc=True)
    with pytest.raises(ValueError, match=msg):
        model.recognize_nbest(x, torch.tensor([6, 5]), beam_width=2, ctc_weight=0.5)
    with pytest.raises(ValueError, match=msg):
        model.ctc_score(x, torch.tensor([6, 5]), [[[1]], [[2]]])
    assert len(model.beam_decode_batch(enc, [6, 5], beam_width=2, ctc_weight=0.0)) == 2


def test_a_hypothesis_the_head_cannot_align_comes_last(monkeypatch):
    """a joint that emits symbol 7 on every frame: on the utterance of two frames the best hypothesis is [7, 7], which CTC needs three frames
    for.  With a weight it is returned last, its transducer score untouched, and its ctc is -inf"""
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _tiny()
    with torch.no_grad():
        model.joint.project_layer.bias[7] += 25.0
    x = torch.randn(2, 8, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    lens = [8, 2]
    with torch.no_grad():
        enc = model.encoder(x)
    plain = model.beam_decode_batch(enc, lens, beam_width=W)
    assert plain[1][0].tokens == [7, 7] and len(plain[1]) >= 2
    res, ctcs = model.beam_decode_batch(enc, lens, beam_width=W, ctc_weight=0.5, return_ctc=True)
    assert res[1][-1] == plain[1][0] and ctcs[1][-1] == -math.inf
    assert all(math.isfinite(v) for v in ctcs[1][:-1]) and sorted(res[1], key=lambda r: r.tokens) == sorted(plain[1], key=lambda r: r.tokens)
    assert [r.tokens for r in res[1]] == [plain[1][i].tokens for i in _key_order(plain[1], model.ctc_score(x, torch.tensor(lens), _tokens(plain))[1], 0.5)]
    # the utterance of eight frames holds [7] * 8 as well: every hypothesis with two sevens in a row there needs more frames than it has
    assert all(math.isfinite(c) == (len(r.tokens) + sum(a == b for a, b in zip(r.tokens, r.tokens[1:])) <= 8) for r, c in zip(res[0], ctcs[0]))
