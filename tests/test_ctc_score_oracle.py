"""The float64 restatement of the CTC hypothesis scorer (tests/ctc_score_oracle.py; the rule: include/ttmi.h, ttmi_ctc_score_hyps) checked
without a GPU: against the enumeration of every alignment on lattices small enough to list, against torch's CTC loss in float64, and for the
power of the GPU tests' inputs - each planted defect must move a score of tests/test_ctc_score_gpu.py's batches by at least twice their
tolerance."""
import itertools

import numpy as np
import pytest
import torch

import ctc_score_oracle as O

TOL = 1e-4                      # the GPU tests' relative tolerance (tests/test_ctc_score_gpu.py)


def _same(a, b):
    if np.isneginf(a) or np.isneginf(b):
        return np.isneginf(a) and np.isneginf(b)
    return abs(a - b) <= 1e-12 * max(1.0, abs(a))


@pytest.mark.parametrize("T,V", [(1, 2), (2, 3), (3, 3), (4, 3), (5, 3), (5, 2)])
def test_oracle_equals_enumeration(T, V):
    """every hypothesis of length <= 3 over the V symbols, blank included as a token: repeats, the empty one, and those no alignment fits"""
    rng = np.random.default_rng(10 * T + V)
    x = rng.standard_normal((T, V)).astype(np.float32)
    seen_dead = seen_repeat = seen_blank = 0
    for Tb in sorted({T, max(1, T - 2)}):
        for n in range(4):
            for hyp in itertools.product(range(V), repeat=n):
                got = O.score_ref(x, hyp, Tb)
                want = O.enumerate_state_paths(x, hyp, Tb)
                assert _same(got, want), (Tb, hyp, got, want)
                if 0 not in hyp:
                    by_def = O.enumerate_symbol_paths(x, hyp, Tb)
                    assert _same(got, by_def), (Tb, hyp, got, by_def)
                    assert np.isneginf(got) == (O.frames_needed(list(hyp)) > Tb), (Tb, hyp)
                seen_dead += bool(np.isneginf(got))
                seen_repeat += any(a == b for a, b in zip(hyp, hyp[1:]))
                seen_blank += 0 in hyp
    assert seen_repeat and seen_blank and seen_dead
    assert _same(O.score_ref(x, [], T), float(O.log_softmax(x)[:, 0].sum()))        # the empty hypothesis: blank on every frame


def test_oracle_equals_enumeration_with_another_blank():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 3)).astype(np.float32)
    for n in range(4):
        for hyp in itertools.product(range(3), repeat=n):
            assert _same(O.score_ref(x, hyp, 4, blank=2), O.enumerate_state_paths(x, hyp, 4, blank=2)), hyp
            if 2 not in hyp:
                assert _same(O.score_ref(x, hyp, 4, blank=2), O.enumerate_symbol_paths(x, hyp, 4, blank=2)), hyp


def test_oracle_equals_torch_ctc_loss_in_float64():
    rng = np.random.default_rng(5)
    B, T, V, U = 6, 23, 11, 7
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    act = [23, 20, 15, 15, 9, 6]
    hyps = [[int(v) for v in rng.integers(1, V, n)] for n in (7, 5, 7, 0, 4, 4)]
    hyps[2][3] = hyps[2][2]
    hyps[4] = [3, 3, 3, 3]                                                          # needs 7 of its 9 frames
    hyps[5] = [3, 3, 3, 3]                                                          # ... and has 6: torch gives +inf
    lp = torch.log_softmax(torch.tensor(x, dtype=torch.float64), dim=-1).transpose(0, 1)
    tgt = torch.zeros(B, U, dtype=torch.long)
    for b, h in enumerate(hyps):
        tgt[b, :len(h)] = torch.tensor(h, dtype=torch.long)
    want = -torch.nn.functional.ctc_loss(lp, tgt, torch.tensor(act), torch.tensor([len(h) for h in hyps]), blank=0, reduction="none")
    got = O.scores_ref(x, act, hyps, utt=list(range(B)))
    assert np.isneginf(got[5]) and float(want[5]) == -np.inf
    for b in range(B - 1):
        assert abs(got[b] - float(want[b])) <= 1e-10 * abs(got[b]), (b, got[b], float(want[b]))


def test_infeasible_matches_torch_inf():
    x = np.random.default_rng(6).standard_normal((1, 3, 4)).astype(np.float32)
    assert np.isneginf(O.score_ref(x[0], [1, 1], 2)) and np.isfinite(O.score_ref(x[0], [1, 1], 3))
    assert np.isneginf(O.score_ref(x[0], [1, 2, 3, 1], 3))


# the (T, U, V) corners of tests/test_ctc_score_gpu.py at which a defect of each kind has something to act on
POWER_CASES = [(8, 64, 37), (9, 1, 5), (10, 130, 260), (17, 63, 37), (17, 130, 5), (2, 64, 5)]


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_planted_defects_move_a_score(defect):
    """on the GPU tests' own batches each wrong rule moves at least one feasible score by 2 TOL (relative), feasible before and after"""
    moved = 0.0
    for T, U, V in POWER_CASES:
        c = O.build_case(1000 + 7 * T + U + V, T, U, V)
        good = O.scores_ref(c["x"], c["act_lens"], c["hyps"])
        bad = O.scores_ref(c["x"], c["act_lens"], c["hyps"], defect=defect)
        assert [bool(np.isneginf(v)) for v in good] == c["planted"]
        for g, w in zip(good, bad):
            if np.isfinite(g) and np.isfinite(w):
                moved = max(moved, abs(g - w) / abs(g))
    print("defect %s: largest relative move %.3e" % (defect, moved))
    assert moved >= 2 * TOL, (defect, moved)


def test_utt_mapping_with_an_explicit_table():
    c = O.build_case(77, 9, 3, 5)
    utt = [2, 0, 0, 3, 0, 2, 0, 0]
    hyps = c["hyps"][:8]
    got = O.scores_ref(c["x"], c["act_lens"], hyps, utt=utt)
    for p in range(8):
        assert got[p] == O.score_ref(c["x"][utt[p]], hyps[p], c["act_lens"][utt[p]])
    assert O.scores_ref(c["x"], c["act_lens"], hyps, utt=[-5, 9] + utt[2:])[0] == O.score_ref(c["x"][0], hyps[0], c["act_lens"][0])      # clamped
