"""The resumable beam search (Transducer.beam_search_state -> ttmi.beam.BeamSearch) on the tiny model and inputs of test_beam_gpu.py's `ctx`
fixture (3 utterances, lengths 12 / 9 / 1, fp32 mode).

history = "full": however the 12 frames are split into blocks, finish() returns what beam_decode_batch returns AS PYTHON OBJECTS - the same
tokens, frames and float bits.  That is a condition, not a tolerance: the same kernels see the same operands in the same order.  capacity = 4
makes the history buffers grow on the way.  The same with a ContextGraph (biases compared) and with a language model, internal-LM
subtraction and a length bonus (lm_totals compared).

history = "stream" (max_history = 3): against beam_oracle.run fed the model's own label encoder and joint under the stream rule, the input
seed chosen by beam_oracle.first_seed (margin at least 1e-3): tokens and frames equal, scores and log-probabilities within test_beam_gpu.py's
bound.  stable() after every block equals the count of the oracle's driver (tests/beam_stream_oracle.py)."""
import numpy as np
import pytest
import torch

import beam_oracle as BO
import beam_stream_oracle as SO
from test_beam_gpu import E2E_LENS, _well_formed, ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SPLITS = [(12,), (1,) * 12, (5, 7), (3, 3, 3, 3), (0, 12)]


def _advance(search, enc, split, lens=E2E_LENS, after=None):
    a = 0
    for n in split:
        search.advance(enc[:, a:a + n], [min(max(v - a, 0), n) for v in lens])
        a += n
        if after is not None:
            after(a)
    assert a == enc.shape[1]
    return search


@pytest.fixture(scope="module")
def one_shot(ctx):
    return ctx["model"].beam_decode_batch(ctx["enc"], E2E_LENS, beam_width=4)


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_any_split_gives_the_one_shot_bits(ctx, one_shot, split):
    model, enc = ctx["model"], ctx["enc"]
    full = {b: SO.drive(lambda u, t, ids: ctx["logits"](u, t, ids[1:]), b, E2E_LENS[b], 4)[1] for b in range(3)}
    search = model.beam_search_state(3, 4, history="full", capacity=4)
    seen = []

    def after(a):
        got = search.stable()
        seen.append(got)
        if a:
            assert got == [full[b][min(a, E2E_LENS[b]) - 1] for b in range(3)], (a, got)
        part = search.partial()
        for b in range(3):
            assert part[b].tokens[:got[b]] == one_shot[b][0].tokens[:got[b]] and len(part[b].frames) == len(part[b].tokens)
    _advance(search, enc, split, after=after)
    assert search.cap >= 13 and all(x <= y for p, q in zip(seen, seen[1:]) for x, y in zip(p, q))
    if split == (3, 3, 3, 3):
        assert search.cap == 16                                       # 4 -> 8 -> 16: two growths on the way
    assert search.finish() == one_shot
    with pytest.raises(RuntimeError):
        search.advance(enc[:, :1])
    again = _advance(model.beam_search_state(3, 4, capacity=4), enc, split)
    assert again.finish(nbest=2) == [r[:2] for r in one_shot]


def test_default_capacity_and_a_later_stop(ctx):
    """without growth the bits are the same; a search stopped after 5 frames is the one-shot search of 5 frames"""
    model, enc = ctx["model"], ctx["enc"]
    search = _advance(model.beam_search_state(3, 4), enc, (5, 7))
    assert search.cap == 64 and search.finish() == model.beam_decode_batch(enc, E2E_LENS, beam_width=4)
    short = [min(v, 5) for v in E2E_LENS]
    search = model.beam_search_state(3, 4, capacity=4)
    search.advance(enc[:, :2], [min(v, 2) for v in E2E_LENS])
    search.advance(enc[:, 2:5], [min(max(v - 2, 0), 3) for v in E2E_LENS])
    assert search.finish() == model.beam_decode_batch(enc[:, :5].contiguous(), short, beam_width=4)


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_with_a_context_graph(ctx, one_shot, split):
    from ttmi.context import ContextGraph
    model, enc = ctx["model"], ctx["enc"]
    second = one_shot[0][1].tokens
    graph = ContextGraph([p for p in (second[-2:], one_shot[1][0].tokens[:3]) if p], boost=1.5)
    want = model.beam_decode_batch(enc, E2E_LENS, beam_width=4, context=graph, return_bias=True)
    assert any(v != 0.0 for u in want[1] for v in u)                  # the automaton acted
    search = _advance(model.beam_search_state(3, 4, context=graph, capacity=4), enc, split)
    assert search.finish(return_bias=True) == want


@pytest.fixture(scope="module")
def lm():
    from test_lm_fusion_model_gpu import _lm
    return _lm()


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_with_a_language_model(ctx, lm, split):
    model, enc = ctx["model"], ctx["enc"]
    kw = dict(lm=lm, lm_weight=0.6, ilm_weight=0.3, length_bonus=0.25)
    want = model.beam_decode_batch(enc, E2E_LENS, beam_width=4, return_bias=True, return_lm=True, **kw)
    assert all(v != 0.0 for u in want[2] for v in u)
    search = _advance(model.beam_search_state(3, 4, capacity=4, **kw), enc, split)
    assert search.finish(return_bias=True, return_lm=True) == want


def test_language_model_without_a_closing_term(ctx, lm):
    """eos = None: no LM row is needed after an utterance's last frame, and none is computed"""
    model, enc = ctx["model"], ctx["enc"]

    class NoEos:
        norm, eos = lm.norm, None

        def __init__(self):
            self.calls = 0

        def next_logits(self, hist):
            self.calls += 1
            return lm.next_logits(hist)
    a, b = NoEos(), NoEos()
    want = model.beam_decode_batch(enc, E2E_LENS, beam_width=4, lm=a, lm_weight=0.6, return_lm=True)
    search = _advance(model.beam_search_state(3, 4, lm=b, lm_weight=0.6, capacity=4), enc, (5, 7))
    assert search.finish(return_lm=True) == want and a.calls == b.calls


@pytest.fixture(scope="module")
def stream(ctx):
    """the ctx fixture's recipe under the stream rule (max_history = 3): the label state of a hypothesis is decoder(its last 3 tokens), of the
    empty one decoder([[0]])"""
    model = ctx["model"]
    state = {}

    def make(seed):
        x = torch.randn(3, max(E2E_LENS), 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + seed))
        with torch.no_grad():
            enc = model.encoder(x)
        dstates, rows = {}, {}

        def by_ids(b, t, ids):
            if (b, t, ids) not in rows:
                with torch.no_grad():
                    if ids not in dstates:
                        dstates[ids] = model.decoder(torch.tensor([list(ids)], device="cuda"))[:, -1, :]
                    rows[(b, t, ids)] = model.joint(enc[b, t].view(-1), dstates[ids].view(-1)).float().cpu().numpy()
            return rows[(b, t, ids)]
        state[seed] = (enc, rows, by_ids)
        return lambda b, t, tokens: by_ids(b, t, SO.fed_ids(tokens, "stream", 3))
    found = BO.first_seed(make, [(b, E2E_LENS[b]) for b in range(3)], 4)
    assert found is not None, "no input seed in 0..15 with an oracle margin of 1e-3 under the stream rule"
    seed, logits, runs = found
    enc, rows, by_ids = state[seed]
    xmax = max(float(np.abs(r).max()) for r in rows.values())
    print("stream rule: input seed %d, margin %.3e, max |logit| %.3f" % (seed, min(r[1] for r in runs.values()), xmax))
    return dict(enc=enc, runs=runs, by_ids=by_ids, bound=1e-5 + 4 * 2.0 ** -23 * xmax)


@pytest.mark.parametrize("split", [(1,) * 12, (5, 7)], ids=lambda s: "-".join(map(str, s)))
def test_stream_history_follows_the_oracle(ctx, stream, split):
    model, enc, bound = ctx["model"], stream["enc"], stream["bound"]
    counts = {b: SO.drive(stream["by_ids"], b, E2E_LENS[b], 4, history="stream", max_history=3)[1] for b in range(3)}
    search = model.beam_search_state(3, 4, history="stream", max_history=3, capacity=4)

    def after(a):
        assert search.stable() == [counts[b][min(a, E2E_LENS[b]) - 1] for b in range(3)], a
    _advance(search, enc, split, after=after)
    res = search.finish()
    assert any(len(r.tokens) > 3 for u in res for r in u)             # histories longer than max_history were fed clamped
    for b in range(3):
        want = stream["runs"][(b, E2E_LENS[b])][0]
        _well_formed(res[b], E2E_LENS[b])
        assert [tuple(r.tokens) for r in res[b]] == [h.tokens for h in want], (b, res[b], want)
        assert [tuple(r.frames) for r in res[b]] == [h.frames for h in want], (b, res[b], want)
        worst_s = max(abs(r.score - h.score) for r, h in zip(res[b], want))
        worst_l = max([abs(x - y) for r, h in zip(res[b], want) for x, y in zip(r.logprobs, h.logprobs)] or [0.0])
        print("utterance %d: max |score - oracle| = %.3e (bound %.3e), max |logprob - oracle| = %.3e (bound %.3e)"
              % (b, worst_s, E2E_LENS[b] * bound, worst_l, bound))
        assert worst_s <= E2E_LENS[b] * bound and worst_l <= bound
