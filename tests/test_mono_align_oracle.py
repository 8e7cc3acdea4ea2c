"""CPU-only: the float64 reference of forced alignment and emission statistics on the monotonic lattice (tests/mono_align_oracle.py) against
a brute force over every set of emitting frames and against closed forms; the planted batches the GPU tests use, checked here after bf16
rounding; planted defects (what a wrong kernel would compute) against the bounds the GPU tests use; and the parts of the new entry points
that answer without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import mono_align_oracle as A
import mono_oracle as M
from conftest import PKG

TOL = 1e-4          # the bound of tests/test_mono_align_gpu.py: relative on scores, absolute on mass, times T_b on expected frames


def random_tables(seed, T, U, V=6, scale=1.5):
    rng = np.random.default_rng(seed)
    x = scale * rng.standard_normal((T, U + 1, V))
    y = rng.integers(1, V, max(U, 1))
    return A.tables(x, y, T, U)


# ----------------------------------------------------------------------------- the recursion against the enumeration
@pytest.mark.parametrize("T,U", [(1, 0), (1, 1), (4, 2), (6, 3), (7, 7), (8, 1)])
def test_viterbi_and_stats_equal_the_brute_force(T, U):
    for seed in range(5):
        lpb, lpl = random_tables(100 * T + 10 * U + seed, T, U)
        frames, score = A.viterbi_ref(lpb, lpl)
        best, arg, mass, expected = A.brute_force(lpb, lpl)
        assert abs(score - best) <= 1e-12 * max(1.0, abs(best))
        assert np.array_equal(frames, arg)
        assert abs(A.path_score(lpb, lpl, frames) - score) <= 1e-12 * max(1.0, abs(score))
        e_ref, m_ref = A.emit_stats_ref(lpb, lpl)
        assert np.allclose(m_ref, mass, rtol=0, atol=1e-12) and np.allclose(e_ref, expected, rtol=0, atol=1e-11)
        assert np.allclose(m_ref, 1.0, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- closed forms
def test_as_many_labels_as_frames():
    T = U = 9
    lpb, lpl = random_tables(1, T, U)
    frames, score = A.viterbi_ref(lpb, lpl)
    _, _, ll = M.lattice(lpb, lpl)
    expected, mass = A.emit_stats_ref(lpb, lpl)
    assert np.array_equal(frames, np.arange(T))
    assert abs(score - ll) < 1e-12 and abs(score - lpl[np.arange(T), np.arange(T)].sum()) < 1e-12      # the one path: score = -cost
    assert np.allclose(expected, np.arange(T), rtol=0, atol=1e-12) and np.allclose(mass, 1.0, rtol=0, atol=1e-12)


def test_no_labels():
    lpb, lpl = random_tables(2, 11, 0)
    frames, score = A.viterbi_ref(lpb, lpl)
    _, _, ll = M.lattice(lpb, lpl)
    assert frames.shape == (0,) and abs(score - ll) < 1e-12 and abs(score - lpb[:, 0].sum()) < 1e-12


@pytest.mark.parametrize("T,U", [(9, 4), (70, 65), (5, 5), (17, 0), (130, 129)])
def test_all_equal_logits_tie_rule(T, U):
    """every reachable cell's two candidates are the same sum of the same numbers: exactly equal, the tie goes to blank, and the backtrace from
    (T, U) takes a label only where the blank's source is unreachable (u = t + 1) -> frames 0 .. U-1"""
    lpb, lpl = A.tables(np.zeros((T, U + 1, 8)), np.ones(max(U, 1), dtype=np.int64), T, U)
    frames, score = A.viterbi_ref(lpb, lpl)
    assert np.array_equal(frames, np.arange(U))
    assert abs(score + T * np.log(8.0)) < 1e-9


def test_more_labels_than_frames_has_no_path():
    lpb, lpl = random_tables(3, 3, 5)
    frames, score = A.viterbi_ref(lpb, lpl)
    expected, mass = A.emit_stats_ref(lpb, lpl)
    assert np.array_equal(frames, np.full(5, -1)) and score == -np.inf
    assert np.array_equal(expected, np.full(5, -1.0)) and np.array_equal(mass, np.zeros(5))


def greedy_frames(lpb, lpl):
    """frame by frame the better of the two decisions, a label being forced once as many labels as frames are left and barred once none is"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    u, frames = 0, []
    for t in range(T):
        if u < U and (U - u == T - t or lpl[t, u] > lpb[t, u]):
            frames.append(t)
            u += 1
    return frames


@pytest.mark.parametrize("T,U", [(12, 5), (40, 17), (9, 9), (6, 0)])
def test_greedy_walk_never_scores_above_viterbi(T, U):
    for seed in range(10):
        lpb, lpl = random_tables(7000 + seed, T, U)
        _, score = A.viterbi_ref(lpb, lpl)
        assert A.path_score(lpb, lpl, greedy_frames(lpb, lpl)) <= score + 1e-12


# ----------------------------------------------------------------------------- the planted batches of the GPU tests
@pytest.mark.parametrize("T,U", [(9, 4), (70, 65), (130, 129), (17, 0), (5, 5)])
@pytest.mark.parametrize("bf16", [False, True])
def test_planted_path_is_the_viterbi_path_with_a_gap(T, U, bf16):
    x, labels, al, ll, planted = A.planted_batch(10 * T + U, T, U, [T], [U])
    xs = A.bf16_round(x) if bf16 else x
    lpb, lpl = A.tables(xs[0], labels[0], T, U)
    frames, score = A.viterbi_ref(lpb, lpl)
    assert np.array_equal(frames, planted[0])
    assert abs(score - A.path_score(lpb, lpl, planted[0])) < 1e-9
    if 0 < U < T:                           # (U = 0 and U = T leave one path only)
        gap = score - A.second_best(lpb, lpl, planted[0])
        assert gap >= 7.7, gap


# ----------------------------------------------------------------------------- planted defects: what a wrong kernel would return
def viterbi_variant(lpb, lpl, tie_to_label=False, lost_neighbour=None, terminal_blank=False):
    """viterbi_ref with one rule broken"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    v = np.full((T + 1, U + 1), -np.inf)
    v[0, 0] = 0.0
    lab = np.zeros((T, U + 1), dtype=bool)
    for t in range(T):
        tt = v[t] + lpb[t]
        tu = np.full(U + 1, -np.inf)
        tu[1:] = v[t, :-1] + lpl[t]
        if lost_neighbour is not None and lost_neighbour <= U:
            tu[lost_neighbour] = -np.inf
        lab[t] = (tu >= tt) & np.isfinite(tu) if tie_to_label else tu > tt
        v[t + 1] = np.where(lab[t], tu, tt)
    frames, u = np.full(U, -1, dtype=np.int64), U
    for t in range(T - 1, -1, -1):
        if u > 0 and lab[t, u]:
            frames[u - 1] = t
            u -= 1
    return frames, float(v[T, U] + (lpb[T - 1, U] if terminal_blank else 0.0))


def standard_lattice(lpb, lpl):
    """the standard RNN-T lattice on the same tables (a label keeps its frame; terminal blank) -> (viterbi score, emission mass [U])"""
    T, U = lpb.shape[0], lpb.shape[1] - 1
    v = np.full((T, U + 1), -np.inf)
    al = np.full((T, U + 1), -np.inf)
    be = np.full((T, U + 1), -np.inf)
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                v[t, u] = al[t, u] = 0.0
                continue
            a = (v[t - 1, u] + lpb[t - 1, u], al[t - 1, u] + lpb[t - 1, u]) if t > 0 else (-np.inf, -np.inf)
            b = (v[t, u - 1] + lpl[t, u - 1], al[t, u - 1] + lpl[t, u - 1]) if u > 0 else (-np.inf, -np.inf)
            v[t, u], al[t, u] = max(a[0], b[0]), np.logaddexp(a[1], b[1])
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            if t == T - 1 and u == U:
                be[t, u] = lpb[t, u]
                continue
            a = be[t + 1, u] + lpb[t, u] if t + 1 < T else -np.inf
            b = be[t, u + 1] + lpl[t, u] if u < U else -np.inf
            be[t, u] = np.logaddexp(a, b)
    return float(v[T - 1, U] + lpb[T - 1, U]), al, be


def test_defect_standard_lattice_label_term():
    T, U = 12, 5
    lpb, lpl = random_tables(41, T, U)
    _, score = A.viterbi_ref(lpb, lpl)
    std, al, be = standard_lattice(lpb, lpl)
    assert abs(std - score) > 2 * TOL * abs(score)
    # the statistics with the standard lattice's beta term, beta(t, u+1) in place of beta(t+1, u+1), on the monotonic alpha / beta / ll
    alpha, beta, ll = M.lattice(lpb, lpl)
    wrong = np.exp(alpha[:T, :U] + lpl + beta[:T, 1:] - ll).sum(0)
    assert np.abs(wrong - 1.0).max() > 2 * TOL


def test_defect_tie_going_to_the_label():
    T, U = 9, 4
    lpb, lpl = A.tables(np.zeros((T, U + 1, 8)), np.ones(U, dtype=np.int64), T, U)
    frames, _ = viterbi_variant(lpb, lpl, tie_to_label=True)
    assert np.array_equal(frames, np.arange(T - U, T)) and not np.array_equal(frames, np.arange(U))      # frames are compared exactly


def test_defect_terminal_blank():
    T, U = 12, 5
    lpb, lpl = random_tables(42, T, U)
    _, score = A.viterbi_ref(lpb, lpl)
    _, wrong = viterbi_variant(lpb, lpl, terminal_blank=True)
    assert abs(wrong - score) > 2 * TOL * abs(score)


def test_defect_neighbour_lost_at_the_slot_seam():
    T, U = 70, 65
    x, labels, _, _, planted = A.planted_batch(10 * T + U, T, U, [T], [U])
    lpb, lpl = A.tables(x[0], labels[0], T, U)
    frames, score = viterbi_variant(lpb, lpl, lost_neighbour=64)
    assert score == -np.inf and not np.array_equal(frames, planted[0])      # label 64 is never reached: no score, labels 64 and up without a frame


# ----------------------------------------------------------------------------- the entry points, without a GPU
def _lib():
    import ttmi
    lib = ttmi.lib()
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_null_pointers_are_refused_before_any_launch():
    lib = _lib()
    rc = lib.ttmi_mono_align(None, None, None, 1, 4, 3, None, None, None, None)
    assert rc < 0 and b"mono_align: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_mono_emit_stats(None, None, None, 1, 4, 3, None, None, None)
    assert rc < 0 and b"mono_emit_stats: null pointer" in lib.ttmi_last_error()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.ttmi_mono_align(p, p, p, 1, 4, 1025, p, p, p, None)
    assert rc < 0 and b"1024" in lib.ttmi_last_error()
    rc = lib.ttmi_mono_emit_stats(p, p, p, 0, 4, 3, p, p, None)
    assert rc < 0 and b"bad shape" in lib.ttmi_last_error()


def test_align_workspace_bytes():
    lib = _lib()
    f = lib.ttmi_mono_align_workspace_bytes
    f.restype = ctypes.c_size_t
    assert f(1, 1, 1) == 8 and f(8, 2000, 201) == 8 * 2000 * 4 * 8 and f(2, 10, 65) == 2 * 10 * 2 * 8
    assert f(0, 4, 3) == 0


def test_ops_raise_on_cpu_tensors():
    import torch
    from ttmi import ops
    ws = torch.zeros(64)
    lens = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.mono_align(ws, lens, lens, 1, 2, 2)
    with pytest.raises(ValueError):
        ops.mono_emit_stats(ws, lens, lens, 1, 2, 2)


def test_topology_value_errors():
    import torch
    from tt.model import Transducer
    from tt.utils import AttrDict
    from warprnnt_pytorch import rnnt_align
    acts = torch.zeros(1, 2, 2, 4)
    y, tl, ul = torch.zeros(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    with pytest.raises(ValueError, match="topology"):
        rnnt_align(acts, y, tl, ul, topology="x")
    with pytest.raises(ValueError):
        rnnt_align(acts, y, tl, ul, topology="monotonic")              # no CPU path on this topology either
    side = dict(n_layer=1, d_model=16, n_head=2, d_head=8, d_inner=16)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=8), dec=dict(side, max_target_length=4),
                        joint=dict(input_size=32, inner_size=16), vocab_size=5, dropout=0.0))
    model = Transducer(cfg)
    x = torch.zeros(1, 4, 16)
    # the model-level entry is Transducer.align_monotonic: `align` keeps its pinned parameter list (tests/test_align.py), so the lattice is
    # a method and not a keyword there, and the method has no exp_domain to refuse; the rule "monotonic + exp-domain is a ValueError whose
    # text contains exp" lives where the two can still meet, in the chunk loop both methods and the handle call
    import inspect
    import tt.model as TM
    sig = inspect.signature(Transducer.align_monotonic)
    assert list(sig.parameters)[1:] == ["inputs", "inputs_length", "targets", "targets_length", "chunk", "check_lengths", "stats"]
    assert sig.parameters["stats"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "topology" in inspect.signature(TM.DeferredLogits.rnnt_align).parameters
    yl, n = torch.ones(1, 2, dtype=torch.long), torch.tensor([2])
    with pytest.raises(ValueError, match="GPU"):
        model.align_monotonic(x, torch.tensor([4]), yl, n)
    with pytest.raises(ValueError, match="exp"):
        TM._joint_align(model.joint, x, x, yl.int(), torch.tensor([4]).int(), n.int(), 0, 1, 0, object(), False, "monotonic")
    with pytest.raises(ValueError, match="topology"):
        TM._joint_align(model.joint, x, x, yl.int(), torch.tensor([4]).int(), n.int(), 0, 1, 0, None, False, "x")


def test_header_states_the_contract():
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "ttmi.h")).read()
    for word in ("ttmi_mono_align_workspace_bytes", "ttmi_mono_align", "ttmi_mono_emit_stats", "STRICTLY increasing", "a tie goes to blank"):
        assert word in hdr, word
