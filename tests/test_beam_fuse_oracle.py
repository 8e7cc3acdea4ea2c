"""The float64 restatement of the fused beam search rule (tests/beam_fuse_oracle.py; the rule: include/ttmi.h, ttmi_beam_step_fuse) checked
against what it is built on, without a GPU: with nothing to fuse it is beam_ctx_oracle.step; on an exhaustive beam its scores are the brute
force's and its fuse the token-by-token sum of e; six planted defects each move the result of the kernel tests' seeded cases by more than the
kernel tests could miss; non-finite source entries take their candidates out and nothing else."""
import math

import numpy as np
import pytest

import beam_ctx_oracle as CO
import beam_fuse_oracle as FO
import beam_oracle as BO

SHAPES = [(37, 1, 12), (37, 4, 12), (130, 8, 12), (5, 8, 10), (4334, 4, 9), (3, 32, 4)]      # (V, W, T): the kernel tests' shapes


def _lens(T):
    return [T, 1, T // 2 + 1]


def _f32_logits(V):
    return lambda seed: BO.rng_logits(seed, V)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(V, W, T):
        if (V, W, T) not in cache:
            cache[(V, W, T)] = FO.seed_case(_f32_logits(V), V, W, T, _lens(T))
        return cache[(V, W, T)]
    return get


@pytest.mark.parametrize("V,W,T", [(37, 4, 12), (5, 8, 10)])
def test_without_sources_and_bonus_it_is_the_biased_rule(V, W, T):
    logits = BO.rng_logits(3, V)
    phrases = CO.phrases_from(BO.run(logits, 0, T, W)[0], V) or [[1, 2]]
    for tb in (FO.TRIVIAL, CO.compile_tables(phrases, [2.0] * len(phrases))):
        beam, ref = FO.START + [None] * (W - 1), CO.START + [None] * (W - 1)
        for t in range(T):
            rows = [logits(0, t, h.tokens) if h is not None else None for h in ref]
            got = FO.step(beam, rows, [(None, None)] * W, t, W, tb, FO.NONE)
            want = CO.step(ref, rows, t, W, tb)
            assert [FO.to_ctx(h) for h in got[0]] == want[0] and got[1:4] == want[1:4] and got[4] == want[4]["merges"]
            assert all(h is None or h.fuse == 0.0 for h in got[0])
            beam, ref = got[0], want[0]


def test_exhaustive_beam_is_the_brute_force_with_the_token_sum():
    V, W, T = 3, 32, 4
    logits = BO.rng_logits(0, V)
    cfg, sources, _ = FO.case_sources(V, 0)
    brute = BO.brute_force(logits, 0, T)
    assert len(brute) == 31
    for tb in (FO.TRIVIAL, CO.compile_tables([[1, 2], [2]], [2.0, 2.0])):
        beam = FO.run(logits, sources, 0, T, W, tb, cfg)[0]
        live = [h for h in beam if h is not None]
        assert sorted(h.tokens for h in live) == sorted(brute)
        for h in live:
            assert abs(h.score - brute[h.tokens]) <= 1e-12
            assert abs(h.fuse - FO.token_sum(h.tokens, sources, cfg, V)) <= 1e-12
            assert h.bias == CO.fsa_run(tb, h.tokens)[1]


def _moved(clean, broken, cfg, xmax):
    """does a final beam's token list differ, or a fuse by at least twice the kernel tests' bound (and by more than nothing)"""
    for a, b in zip(clean, broken):
        if [h and h.tokens for h in a] != [h and h.tokens for h in b]:
            return True
        for h, g in zip(a, b):
            if h is not None and abs(h.fuse - g.fuse) > 0.0 and abs(h.fuse - g.fuse) >= 2 * FO.fuse_bound(len(h.tokens), cfg, xmax):
                return True
    return False


def test_planted_defects_show_on_the_seeded_cases(cases):
    """every defect shows on every seeded case where it can act.  Where it cannot: at W = 1 there is one slot, so no merge and one row to
    take; at V = 4334 the synthetic logits let no blank extension into a final beam (every hypothesis there holds one symbol per frame:
    checked below), so what a defect does to the blank extension is not seen; a merge shows only where a merged candidate survives to the
    final beam, which the shapes that must show a merge are there for: at least one of them has to show it."""
    caught = {d: [] for d in FO.DEFECTS}
    for V, W, T in SHAPES:
        case = cases(V, W, T)
        lens = _lens(T)
        xmax = [2 * 6.0, 2 * 6.0]                          # |standard_normal| stays below 6 at these counts: the bound is not understated
        for defect in FO.DEFECTS:
            hit = False
            for name, tb in case["tables"].items():
                clean = [case["runs"][name][b][0] for b in range(3)]
                broken = [FO.run(case["logits"], case["sources"], b, lens[b], W, tb, case["cfg"], defect=defect)[0] for b in range(3)]
                hit = hit or _moved(clean, broken, case["cfg"], xmax)
            caught[defect].append(((V, W, T), hit))
    print(caught)
    for defect, hits in caught.items():
        for shape, hit in hits:
            if defect == "merge_takes_j" or (defect == "row_mixup" and shape[1] == 1):
                continue
            if defect in ("lm_on_blank", "bonus_per_frame") and shape[0] == 4334 and not hit:
                assert all(len(h.tokens) == n for rs in cases(*shape)["runs"].values() for r, n in zip(rs.values(), _lens(shape[2]))
                           for h in r[0] if h is not None), "a blank extension in a final beam at V = 4334: the defect can act"
                continue
            assert hit, (defect, shape)
    assert any(hit for shape, hit in caught["merge_takes_j"] if shape in FO.NEED_MERGE)


def test_seeds_of_the_f32_cases(cases):
    for V, W, T in SHAPES:
        case = cases(V, W, T)
        print("V=%d W=%d T=%d: seed %d, key margin %.3e, merges %d" % (
            V, W, T, case["seed"], min(r[1] for rs in case["runs"].values() for r in rs.values()),
            sum(r[2] for rs in case["runs"].values() for r in rs.values())))


def _one_step(ext0, cfg, V=5, W=4):
    logits = BO.rng_logits(1, V)
    beam = FO.START + [None] * (W - 1)
    rows = [logits(0, 0, ())] + [None] * (W - 1)
    return FO.step(beam, rows, [(ext0, None)] + [None] * (W - 1), 0, W, FO.TRIVIAL, cfg), BO.log_softmax(rows[0])


def test_non_finite_source_entries():
    V = 5
    x = np.array([0.5, -1.0, 2.0, 0.0, 1.0], dtype=np.float32)
    # a source row of all -inf under norm 1: no finite log-sum-exp, every symbol is out, the blank extension stays as it was
    (beam, parent, fresh, _, _), lp = _one_step(np.full(V, -np.inf, dtype=np.float32), FO.Fuse(0.0, ((0.6, 1), None)))
    assert [h and h.tokens for h in beam] == [(), None, None, None] and beam[0].score == lp[0] and beam[0].fuse == 0.0 and fresh == [0] * 4
    # a NaN row under norm 0
    (beam, _, _, _, _), lp = _one_step(np.full(V, np.nan, dtype=np.float32), FO.Fuse(0.25, ((0.6, 0), None)))
    assert [h and h.tokens for h in beam] == [(), None, None, None] and beam[0].fuse == 0.0
    # one -inf entry under a negative weight: e = +inf, that symbol alone takes no slot
    y = x.copy()
    y[2] = -np.inf
    (beam, _, _, _, _), lp = _one_step(y, FO.Fuse(0.0, ((-0.3, 1), None)))
    tokens = sorted(h.tokens for h in beam if h is not None)
    assert tokens == [(), (1,), (3,), (4,)] and all(math.isfinite(h.fuse) for h in beam if h is not None)
    # ... and under a positive one: e = -inf, the same
    (beam, _, _, _, _), lp = _one_step(y, FO.Fuse(0.0, ((0.6, 1), None)))
    assert sorted(h.tokens for h in beam if h is not None) == [(), (1,), (3,), (4,)]
    # a NaN row under norm 1 poisons the symbols of its slot only through e: the scores are the model's
    (beam, _, _, _, _), lp = _one_step(np.where(np.arange(V) == 1, np.nan, x).astype(np.float32), FO.Fuse(0.0, ((0.6, 1), None)))
    assert [h and h.tokens for h in beam] == [(), None, None, None] and beam[0].score == lp[0]
