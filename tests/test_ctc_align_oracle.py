"""CPU-only: the float64 reference of tests/ctc_align_oracle.py against the enumeration of every CTC alignment on small lattices
(T <= 6, U <= 3, V = 4), and the visibility of five planted defects: each one changes a path, or moves a statistic by at least 2e-4 relative -
twice the 1e-4 the GPU tests allow - on the inputs chosen here."""
import zlib

import numpy as np
import pytest

import ctc_align_oracle as A

V = 4
# (name, T, labels, blank): a repeated label, a label equal to `blank`, U = 0, the shortest feasible lengths, a non-zero blank
CASES = [("T1_U0", 1, [], 0), ("T5_U0", 5, [], 0), ("T1_U1", 1, [2], 0), ("T2_U1", 2, [3], 0), ("T4_ab", 4, [1, 2], 0),
         ("T3_aa_min", 3, [2, 2], 0), ("T6_aab", 6, [1, 1, 3], 0), ("T6_aba", 6, [1, 2, 1], 0), ("T6_abc", 6, [1, 2, 3], 0),
         ("T5_label_is_blank", 5, [1, 0], 0), ("T6_blank_first", 6, [0, 2, 2], 0), ("T5_blank2", 5, [2, 1], 2), ("T6_blank3_rep", 6, [0, 0, 1], 3)]


def _case(case, seed=0, scale=1.5):
    name, T, lab, blank = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + seed)
    x = scale * rng.standard_normal((T, V))
    lp, ext, skip = A.tables(x, lab, T, len(lab), blank)
    return lp, ext, skip


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_against_enumeration(case):
    lp, ext, skip = _case(case)
    T, S = lp.shape
    U = S // 2
    bf = A.brute_force(lp, skip)
    # random float64 logits: no tie - unless a label IS the blank, whose states then emit the same symbol and tie by construction
    assert bf is not None and (len(bf["paths_at_best"]) == 1 or case[3] in case[2])
    path, score = A.viterbi_ref(lp, skip)
    assert tuple(path) in bf["paths_at_best"] and A.valid_path(path, skip)
    assert abs(score - bf["best"]) <= 1e-12 * max(1.0, abs(bf["best"])) and abs(A.path_score(lp, path) - score) <= 1e-12 * max(1.0, abs(score))
    _, _, ll = A.lattice(lp, skip)
    assert abs(ll - bf["ll"]) <= 1e-12 * max(1.0, abs(ll))
    expected, mass, duration, blank_occ = A.emit_stats_ref(lp, skip)
    assert expected.shape == mass.shape == duration.shape == (U,)
    assert np.abs(mass - 1.0).max(initial=0.0) <= 1e-12
    assert np.abs(expected - bf["expected"]).max(initial=0.0) <= 1e-12 and np.abs(duration - bf["duration"]).max(initial=0.0) <= 1e-12
    assert abs(blank_occ - bf["blank"]) <= 1e-12
    assert abs(duration.sum() + blank_occ - T) <= 1e-12 * T
    sp = A.spans_of(path, U)
    assert all(sp[u, 0] <= sp[u, 1] for u in range(U)) and all(sp[u, 1] < sp[u + 1, 0] for u in range(U - 1))


def test_repeat_needs_its_blank():
    """[a, a] on two frames has no alignment: all -1, -inf, statistics -1 / 0 / 0; on three frames exactly one"""
    x = np.random.default_rng(3).standard_normal((3, V))
    lp, _, skip = A.tables(x, [2, 2], 2, 2)
    assert A.brute_force(lp, skip) is None
    path, score = A.viterbi_ref(lp, skip)
    assert (path == -1).all() and score == -np.inf
    e, m, d, bo = A.emit_stats_ref(lp, skip)
    assert (e == -1).all() and (m == 0).all() and (d == 0).all() and bo == 0
    lp, _, skip = A.tables(x, [2, 2], 3, 2)
    assert A.all_paths(3, skip) == [(1, 2, 3)]
    assert tuple(A.viterbi_ref(lp, skip)[0]) == (1, 2, 3)


def test_tie_rule_on_all_equal_logits():
    """every alignment scores the same: the path stays in the later state as long as it can.  Worked by hand for [1, 2] on five frames:
    the end is S-1 = 4 (S-2 is not strictly greater); state 4 exists from frame 2 on (s <= 2 t + 1), so frames 4, 3, 2 stay; frame 2 came
    from s-1 = 3 (its own state is dead at frame 1); state 3 at frame 1 came from s-2 = 1 (s and s-1 are dead at frame 0)."""
    lp, _, skip = A.tables(np.zeros((5, V)), [1, 2], 5, 2)
    path, score = A.viterbi_ref(lp, skip)
    assert tuple(path) == (1, 3, 4, 4, 4) and abs(score + 5 * np.log(V)) < 1e-12
    assert np.array_equal(A.spans_of(path, 2), [[0, 0], [1, 1]])
    # with a repeat the skip is closed: [1, 1] walks 1, 2, 3, then rests in 4
    lp, _, skip = A.tables(np.zeros((5, V)), [1, 1], 5, 2)
    assert tuple(A.viterbi_ref(lp, skip)[0]) == (1, 2, 3, 4, 4)
    lp, _, skip = A.tables(np.zeros((4, V)), [], 4, 0)
    assert tuple(A.viterbi_ref(lp, skip)[0]) == (0, 0, 0, 0)


def test_runner_up_and_planted_batch():
    x, labels, al, ll, paths = A.planted_batch(5, 12, 4, [12, 9, 3, 1], [4, 2, 4, 0])
    assert (paths[2] == -1).all()                                             # four labels on three frames
    for b in (0, 1, 3):
        lp, ext, skip = A.tables(x[b], labels[b], al[b], ll[b])
        path, score = A.viterbi_ref(lp, skip)
        assert np.array_equal(path, paths[b, :al[b]]) and (paths[b, al[b]:] == -1).all()
        ru = A.runner_up(lp, skip, path)
        others = [A.path_score(lp, p) for p in A.all_paths(int(al[b]), skip) if p != tuple(path)] if al[b] <= 9 else None
        if others is not None:
            want = max(others) if others else -np.inf
            assert ru == want or abs(ru - want) <= 1e-12 * abs(want)
        assert score - ru > 1.0


# ----------------------------------------------------------------------------- planted defects
REL = 2e-4          # twice the project tolerance


def _moved(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) >= REL * np.maximum(np.abs(a), 1e-300)).any())


def test_defect_skip_across_a_repeat():
    """[1, 1] with the label leading frames 0 and 1 and the blank nowhere near: the right lattice has to spend a frame in the blank between
    the two, the defective one jumps 1 -> 3"""
    x = np.full((4, V), -6.0)
    x[:, 1] = 0.0
    lp, ext, _ = A.tables(x, [1, 1], 4, 2)
    good, bad = A.extended([1, 1], 2)[1], A.extended([1, 1], 2, defect="skip_across_repeat")[1]
    pg, sg = A.viterbi_ref(lp, good)
    pb, sb = A.viterbi_ref(lp, bad)
    assert A.valid_path(pg, good) and not A.valid_path(pb, good) and not np.array_equal(pg, pb)
    assert _moved(sg, sb)
    assert _moved(A.emit_stats_ref(lp, good)[2], A.emit_stats_ref(lp, bad)[2])          # and the durations move with it


def test_defect_tie_taken_by_the_later_predecessor():
    lp, _, skip = A.tables(np.zeros((5, V)), [1, 2], 5, 2)
    good, bad = A.viterbi_ref(lp, skip)[0], A.viterbi_ref(lp, skip, defect="tie_later")[0]
    assert tuple(good) == (1, 3, 4, 4, 4) and A.valid_path(bad, skip) and not np.array_equal(good, bad)


def test_defect_final_tie_ends_in_s_minus_2():
    lp, _, skip = A.tables(np.zeros((5, V)), [1, 2], 5, 2)
    good, bad = A.viterbi_ref(lp, skip)[0], A.viterbi_ref(lp, skip, defect="final_tie_s2")[0]
    assert good[-1] == 4 and bad[-1] == 3 and A.valid_path(bad, skip)


def test_defect_onset_without_its_frame_0_term():
    """the first label leads frame 0: nearly all of its onset mass is the t = 0 term"""
    x, labels, al, ll, paths = A.planted_batch(11, 8, 3, [8], [3])
    x[0, 0] = -8.0
    x[0, 0, labels[0, 0]] = 0.0
    lp, _, skip = A.tables(x[0], labels[0], 8, 3)
    eg, mg, dg, _ = A.emit_stats_ref(lp, skip)
    eb, mb, db, _ = A.emit_stats_ref(lp, skip, defect="onset_no_t0")
    assert abs(mg[0] - 1.0) < 1e-12 and mb[0] < 0.01 and _moved(mg, mb)
    assert np.array_equal(dg, db)


def test_defect_duration_without_minus_lp():
    lp, _, skip = _case(CASES[8])
    dg = A.emit_stats_ref(lp, skip)[2]
    db = A.emit_stats_ref(lp, skip, defect="duration_no_lp")[2]
    assert _moved(dg, db) and (db < dg).all()                                   # lp < 0 counted twice
