"""CPU-only: the float64 reference of the token-and-duration transducer (tests/tdt_oracle.py) agrees with itself in its three statements, reduces
to the monotonic oracle for durations = (1,), and would catch each planted defect at the GPU tests' bound; check_durations, the TDT entry
points' refusals and the C ABI's argument checks work without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mono_oracle as M
import tdt_oracle as O
from conftest import PKG

GPU_TOL = 1e-4                 # the bound of tests/test_tdt_gpu.py: a planted defect must move a figure by at least twice this
# (durations, T, U, V) of the CPU check the feature was specified with
CASES = [((1, 2, 3), 6, 3, 5), ((1,), 5, 2, 4), ((2,), 5, 1, 4), ((2,), 6, 2, 4), ((1, 4), 3, 1, 3), ((2, 3), 7, 3, 4), ((1, 2, 4, 8), 9, 0, 3)]
IDS = ["d%s_T%d_U%d_V%d" % ("".join(map(str, c[0])), c[1], c[2], c[3]) for c in CASES]


def _case(durations, T, U, V, seed=0):
    rng = np.random.default_rng(100 + seed)
    x = 1.5 * rng.standard_normal((1, T, U + 1, V + len(durations)))
    y = rng.integers(0, V, (1, max(U, 1)))
    return x, y


def _has_path(durations, T, U):
    """T reachable by a sum of at least U durations"""
    reach = {(0, 0)}
    for _ in range(T):
        reach |= {(t + d, min(n + 1, U)) for t, n in reach for d in durations if t + d <= T}
    return (T, U) in reach


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recursion_enumeration_and_autograd_agree(case):
    durations, T, U, V = case
    x, y = _case(*case)
    cost, grad, lats = O.tdt_loss(x, y, [T], [U], durations, return_lattice=True)
    brute = O.brute_force_cost(x[0], y[0], T, U, durations)
    acost, agrad = O.autograd_loss(x, y, [T], [U], durations)
    vec = O.tdt_cost_vectorised(x[0], y[0], T, U, durations)
    if not _has_path(durations, T, U):
        assert np.isposinf(cost[0]) and np.isposinf(brute) and np.isposinf(acost[0]) and np.isposinf(vec)
        assert np.all(grad == 0) and np.all(agrad == 0)
        return
    assert abs(cost[0] - brute) < 1e-12 * abs(brute) and abs(cost[0] - acost[0]) < 1e-12 * abs(brute) and abs(cost[0] - vec) < 1e-12 * abs(brute)
    assert np.abs(grad - agrad).max() < 1e-12
    alpha, beta, occ, occ_ab = lats[0]
    assert abs(-beta[0, 0] - cost[0]) < 1e-12 * abs(cost[0])                        # the backward pass tells the same likelihood
    assert np.abs(occ - occ_ab).max() < 1e-12                                       # sum_j E_j = exp(alpha + beta - ll)
    D = len(durations)
    assert np.abs(grad[..., :V].sum(-1)).max() < 1e-12 and np.abs(grad[..., V:V + D].sum(-1)).max() < 1e-12      # both sub-rows sum to zero
    assert np.abs(grad).max() > 1e-3


def test_only_one_case_of_the_list_has_no_path():
    assert [c for c in CASES if not _has_path(c[0], c[1], c[2])] == [((2,), 5, 1, 4)]


def test_duration_one_is_the_monotonic_lattice():
    rng = np.random.default_rng(5)
    B, T, U1, V = 3, 5, 3, 4
    x = 1.5 * rng.standard_normal((B, T, U1, V + 1))
    y = rng.integers(0, V, (B, U1 - 1))
    tl, ul = [5, 4, 2], [2, 1, 2]
    for blank in (0, V - 1):
        cost, grad = O.tdt_loss(x, y, tl, ul, (1,), blank)
        mcost, mgrad = M.mono_loss(x[..., :V], y, tl, ul, blank)
        assert np.abs(cost - mcost).max() < 1e-12 and np.abs(grad[..., :V] - mgrad).max() < 1e-12
        assert np.all(grad[..., V] == 0)                                            # softmax of one column is 1: occ - E_0 = 0 exactly


def test_no_path_utterances_between_live_neighbours():
    """U_b > T_b, and durations = (2,) with an odd T_b: +inf and zero rows; the neighbours are what they are alone"""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 6, 4, 5 + 2))
    y = rng.integers(0, 5, (3, 3))
    cost, grad = O.tdt_loss(x, y, [6, 2, 5], [2, 3, 1], (1, 2))
    assert np.isfinite(cost[[0, 2]]).all() and np.isposinf(cost[1]) and np.all(grad[1] == 0)
    x2 = rng.standard_normal((3, 6, 3, 4 + 1))
    cost, grad = O.tdt_loss(x2, y[:, :2], [6, 5, 4], [2, 1, 0], (2,))
    assert np.isfinite(cost[[0, 2]]).all() and np.isposinf(cost[1]) and np.all(grad[1] == 0) and np.isfinite(grad).all()
    alone, galone = O.tdt_loss(x2[2:], y[2:, :2], [4], [0], (2,))
    assert alone[0] == cost[2] and np.array_equal(galone[0], grad[2])


def test_lengths_and_labels_are_clamped():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 4, 3, 4 + 2))
    a = O.tdt_loss(x, [[-3, 99], [1, 2]], [9, 0], [7, -1], (1, 2))
    b = O.tdt_loss(x, [[0, 3], [1, 2]], [4, 1], [2, 0], (1, 2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ----------------------------------------------------------------------------- planted defects: each would be caught at the GPU bound
def _moved(good, bad):
    """the largest figure a defect moved, in the GPU tests' measures: costs relative to the cost, gradients relative to the utterance's largest
    gradient element"""
    (gc, gg), (bc, bg) = good, bad
    return max(np.abs(bc - gc).max() / np.abs(gc).max(), np.abs(bg - gg).max() / np.abs(gg).max())


@pytest.mark.parametrize("defect", ["clip", "beta_plus_1", "dur_no_label", "joint_norm"])
def test_planted_loss_defects_move_a_figure_beyond_the_gpu_bound(defect):
    """overshooting moves clipped to T_b instead of dropped; beta(t+1, .) in place of beta(t+d, .); the label share missing from the duration
    gradient; the duration sub-row normalised together with the tokens - on the GPU tests' first shape"""
    rng = np.random.default_rng(8)
    B, T, U1, V, durations = 3, 12, 5, 7, (1, 2, 4)
    x = 1.5 * rng.standard_normal((B, T, U1, V + 3))
    y = rng.integers(0, V, (B, U1 - 1))
    tl, ul = [12, 10, 7], [4, 3, 0]
    good = O.tdt_loss(x, y, tl, ul, durations)
    bad = O.tdt_loss(x, y, tl, ul, durations, defect=defect)
    print(defect, "moves", _moved(good, bad))
    assert _moved(good, bad) >= 2 * GPU_TOL


def _rows(seed, T, V, D):
    table = np.random.default_rng(seed).standard_normal((T, 8, V + D))
    return lambda t, tokens: table[t, len(tokens) % 8]


def test_decoder_rule_and_its_planted_defect():
    """a blank jump that advances by 1 instead of d changes the decisions the GPU test compares exactly"""
    V, durations, T = 6, (1, 2, 4), 40
    rows = _rows(9, T, V, 3)
    good = O.greedy_decode(rows, T, durations, V)
    bad = O.greedy_decode(rows, T, durations, V, defect="blank_by_1")
    tokens, frames, lps, durs, score, taken = good
    assert len(tokens) == len(frames) == len(lps) == len(durs) and tokens and all(b > a for a, b in zip(frames, frames[1:]))
    assert all(f2 - f1 >= d for f1, f2, d in zip(frames, frames[1:], durs))          # the next token is at least the token's jump away
    assert sum(taken) >= T and sum(taken[:-1]) < T                                   # the decisions tile the utterance; only the last may overshoot
    assert (bad[0], bad[1], bad[3]) != (tokens, frames, durs) or abs(bad[4] - score) > 2e-5 * abs(score)
    # the lowest index wins a tie, in both sub-rows
    tie = np.zeros(V + 3)
    t2 = O.greedy_decode(lambda t, tokens: tie, 3, durations, V, blank=1)
    assert t2[0] == [0, 0, 0] and t2[3] == [1, 1, 1]


# ----------------------------------------------------------------------------- refusals without a device
def test_check_durations():
    from ttmi.tdt import check_durations
    assert check_durations([1, 2, 4]) == (1, 2, 4) and check_durations((8,)) == (8,) and check_durations(range(1, 9)) == tuple(range(1, 9))
    for bad, text in (([0, 1], "duration 0"), ([], "between 1 and 8"), (list(range(1, 10)), "between 1 and 8"), ([1, 9], "outside"),
                      ([-1, 2], "outside"), ([2, 1], "strictly increasing"), ([1, 1], "strictly increasing"), ([1.0, 2], "integers"),
                      ([True, 2], "integers"), (["1"], "integers"), (3, "sequence")):
        with pytest.raises(ValueError, match=text):
            check_durations(bad)


def test_python_entry_points_fail_loudly_without_device():
    import torch
    from ttmi import ops
    from ttmi.tdt import TDTLoss, tdt_loss
    x = torch.zeros(1, 2, 2, 4 + 2)
    y, n = torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.tdt_loss_fwd(x, y, n, n, 0, (1, 2), torch.zeros(64))
    with pytest.raises(ValueError):
        ops.tdt_loss_bwd(x, y, n, n, 0, (1, 2), torch.zeros(64), torch.ones(1), 1, 1.0)
    with pytest.raises(ValueError, match="GPU"):
        TDTLoss((1, 2))(x, y, torch.tensor([2], dtype=torch.int32), n)
    with pytest.raises(ValueError, match="GPU"):
        tdt_loss(x, y, torch.tensor([2], dtype=torch.int32), n, (1, 2))
    with pytest.raises(ValueError, match="duration 0"):
        TDTLoss((0, 1))
    with pytest.raises(ValueError):
        TDTLoss((1, 2), reduction="max")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.tdt_scan_batch(torch.zeros(1, 2, 6), 2, i32(1), i32(1), i32(1), i32(1, 2, 2), torch.zeros(1, 2, 2))
    with pytest.raises(ValueError):
        ops.tdt_advance(i32(1, 2, 2), torch.zeros(1, 2, 2), (1, 2), 1, torch.zeros(1, 4, dtype=torch.long), i32(1), i32(1), i32(1), i32(1),
                        i32(1), i32(2), i32(1, 3), torch.zeros(1, 3), i32(1, 3), torch.zeros(1, dtype=torch.float64))
    lat = ops.TDTLattice([1, 2, 3])
    assert (lat.has_exp_forms, lat.takes_fastemit, lat.label_takes_frame, lat.durations) == (False, False, True, (1, 2, 3))
    assert lat.fastemit_kw(0.5) == {}
    for entry in (lat.align, lat.emit_stats):
        with pytest.raises(ValueError, match="TDT"):
            entry()
    assert set(ops.LATTICES) == {"rnnt", "monotonic"}                                # TDT is no topology of the same logits


def _tiny(**extra):
    import torch
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0, **extra))
    torch.manual_seed(1)
    return Transducer(cfg)


def test_model_config_key():
    """absent / None / empty: today's module and state_dict; a list: D more rows of the projection, behind the token rows"""
    import torch
    plain = _tiny()
    for v in (None, [], ()):
        m = _tiny(tdt_durations=v)
        assert m.tdt_durations is None and m.joint.project_layer.out_features == 29
        assert list(m.state_dict()) == list(plain.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), plain.state_dict().values()))
    m = _tiny(tdt_durations=[1, 2, 3])
    assert m.tdt_durations == (1, 2, 3) and m.joint.project_layer.out_features == 32
    assert list(m.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="duration 0"):
        _tiny(tdt_durations=[0, 1])


def test_every_entry_point_that_is_not_built_raises_for_a_tdt_model():
    import torch
    from ttmi.beam import BeamSearch
    from ttmi.streaming import StreamingRecognizer
    m = _tiny(tdt_durations=[1, 2, 3]).eval()
    x, y = torch.zeros(2, 6, 64), torch.ones(2, 3, dtype=torch.long)
    al, ll = torch.tensor([6, 5], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    enc = torch.zeros(2, 6, 64)
    calls = [lambda: m.loss(x, al, y, ll, topology="monotonic"), lambda: m.loss(x, al, y, ll, exp_domain=True),
             lambda: m.loss(x, al, y, ll, fastemit_lambda=0.01), lambda: m.loss(x, al, y, ll, distill=torch.zeros(2, 6, 4, 3), distill_weight=0.5),
             lambda: m.lattice_posteriors(x, al, y, ll), lambda: m.mwer_loss(x, al, y, ll), lambda: m.align(x, al, y, ll),
             lambda: m.align_monotonic(x, al, y, ll), lambda: m.beam_decode_batch(enc, [6, 5]), lambda: m.recognize_nbest(x, al),
             lambda: m.recognize_nbest(x, al, ctc_weight=0.3), lambda: m.beam_search_state(2), lambda: m.beam_search(enc[0], 6),
             lambda: m.beam_search(enc[0], 6, block=0), lambda: m.recognize_beam_search(x, al), lambda: BeamSearch(m, 2),
             lambda: StreamingRecognizer(m), lambda: StreamingRecognizer(m, beam_width=4)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="TDT.*not built"):
            call()
    # greedy decoding is built, on the device only
    with pytest.raises(ValueError, match="GPU"):
        m.recognize(x, al)
    with pytest.raises(ValueError, match="GPU"):
        m.decode_batch(enc, [6, 5], details=True)


def test_training_driver_picks_the_criterion():
    from ttmi.dp_train import make_criterion
    from ttmi.tdt import TDTLoss
    from warprnnt_pytorch import RNNTLoss
    from tt.utils import AttrDict

    def cfg(model, training):
        return AttrDict(dict(model=model, training=training))
    crit = make_criterion(cfg(dict(tdt_durations=[1, 2, 4]), dict()))
    assert isinstance(crit, TDTLoss) and crit.durations == (1, 2, 4)
    assert isinstance(make_criterion(cfg(dict(), dict())), RNNTLoss) and isinstance(make_criterion(cfg(dict(tdt_durations=None), dict())), RNNTLoss)
    assert make_criterion(cfg(dict(), dict(loss_topology="monotonic"))).topology == "monotonic"
    assert make_criterion(cfg(dict(), dict(fastemit_lambda=0.01))).fastemit_lambda == 0.01
    with pytest.raises(ValueError, match="TDT.*not built"):
        make_criterion(cfg(dict(tdt_durations=[1, 2]), dict(loss_topology="monotonic")))
    with pytest.raises(ValueError, match="TDT.*not built"):
        make_criterion(cfg(dict(tdt_durations=[1, 2]), dict(fastemit_lambda=0.01)))


# ----------------------------------------------------------------------------- the C ABI without a device
I, L, F = ctypes.c_int, ctypes.c_long, ctypes.c_float
SYMBOLS = ("ttmi_tdt_workspace_bytes", "ttmi_tdt_loss_fwd", "ttmi_tdt_loss_bwd", "ttmi_tdt_scan_batch", "ttmi_tdt_advance")


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_symbols_are_declared_and_exported_and_the_workspace_is_sized():
    from conftest import ROOT
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "ttmi.h")).read()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n + "(" in hdr, n
    f = lib.ttmi_tdt_workspace_bytes
    f.restype = ctypes.c_size_t
    # alpha, beta f64 [B, T+1, U1], ll f64 [B], (4 + D) f32 tables [B, T, U1], and the 64 bytes of slack ttmi_mono_workspace_bytes has
    assert f(2, 3, 4, 3) == 8 * (2 * 2 * 4 * 4 + 2) + 4 * 7 * 2 * 3 * 4 + 64
    assert f(0, 3, 4, 3) == 0 and f(2, 3, 4, 0) == 0 and f(2, 3, 4, 9) == 0


def _good():
    fl, ints, ws = (ctypes.c_float * 256)(), (ctypes.c_int * 64)(), (ctypes.c_double * 256)()
    return dict(logits=fl, dtype=0, ldv=8, labels=ints, act_lens=ints, label_lens=ints, B=1, T=2, U1=2, V=5, blank=0, dur=(1, 2, 3), ws=ws,
                costs=(ctypes.c_float * 4)(), go=(ctypes.c_float * 4)(), grad=(ctypes.c_float * 256)(), ldg=8)


def _fwd(lib, a):
    d = a["dur"]
    dur = None if d is None else (ctypes.c_int * max(len(d), 1))(*d)
    return lib.ttmi_tdt_loss_fwd(a["logits"], I(a["dtype"]), L(a["ldv"]), a["labels"], a["act_lens"], a["label_lens"], I(a["B"]), I(a["T"]), I(a["U1"]),
                                 I(a["V"]), I(a["blank"]), dur, I(a.get("D", 0 if d is None else len(d))), a["ws"], a["costs"], None)


def _bwd(lib, a):
    d = a["dur"]
    dur = None if d is None else (ctypes.c_int * max(len(d), 1))(*d)
    return lib.ttmi_tdt_loss_bwd(a["logits"], I(a["dtype"]), L(a["ldv"]), a["labels"], a["act_lens"], a["label_lens"], I(a["B"]), I(a["T"]), I(a["U1"]),
                                 I(a["V"]), I(a["blank"]), dur, I(a.get("D", 0 if d is None else len(d))), a["ws"], a["go"], I(1), F(1.0),
                                 a["grad"], L(a["ldg"]), None)


BAD = [("null_logits", dict(logits=None), b"null pointer"), ("null_act_lens", dict(act_lens=None), b"null pointer"),
       ("null_workspace", dict(ws=None), b"null pointer"), ("null_durations", dict(dur=None, D=2), b"null pointer"),
       ("null_labels", dict(labels=None), b"null pointer"),
       ("B0", dict(B=0), b"bad shape"), ("T0", dict(T=0), b"bad shape"), ("V0", dict(V=0), b"bad shape"), ("U1_1025", dict(U1=1025), b"> 1024"),
       ("D0", dict(dur=(), D=0), b"D=0 outside [1,8]"), ("D9", dict(dur=tuple(range(1, 10)), ldv=16, ldg=16), b"D=9 outside [1,8]"),
       ("duration_0", dict(dur=(0, 1)), b"duration 0 outside [1,8]"), ("duration_9", dict(dur=(1, 9)), b"duration 9 outside [1,8]"),
       ("not_increasing", dict(dur=(2, 1)), b"strictly increasing"), ("repeated", dict(dur=(1, 1)), b"strictly increasing"),
       ("ldv_below_V_plus_D", dict(ldv=7, ldg=7), b"bad pitch"), ("dtype", dict(dtype=2), b"bad pitch/dtype"),
       ("blank", dict(blank=5), b"blank 5 outside [0,5)")]


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_loss_entries_refuse_before_any_launch(case):
    lib = _lib()
    for call, who in ((_fwd, b"tdt_loss_fwd"), (_bwd, b"tdt_loss_bwd")):
        a = _good()
        a.update(case[1])
        rc = call(lib, a)
        msg = lib.ttmi_last_error()
        assert rc < 0 and msg.startswith(who) and case[2] in msg, (rc, msg)


def test_backward_only_refusals_and_the_decode_pair():
    lib = _lib()
    a = _good()
    a.update(ldg=7)
    assert _bwd(lib, a) < 0 and b"bad pitch" in lib.ttmi_last_error()
    a = _good()
    a.update(grad=a["logits"], ldg=9, ldv=8)
    assert _bwd(lib, a) < 0 and b"in-place needs ldg == ldv" in lib.ttmi_last_error()
    a = _good()
    a["ws"] = ctypes.c_void_p(ctypes.addressof(a["ws"]) + 4)
    assert _fwd(lib, a) < 0 and b"8-byte aligned" in lib.ttmi_last_error()
    fl, ints = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    rc = lib.ttmi_tdt_scan_batch(None, I(0), L(8), I(1), I(2), I(5), I(3), ints, ints, ints, ints, fl, None)
    assert rc < 0 and b"tdt_scan_batch: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_tdt_scan_batch(fl, I(0), L(7), I(1), I(2), I(5), I(3), ints, ints, ints, ints, fl, None)
    assert rc < 0 and b"bad pitch" in lib.ttmi_last_error()
    rc = lib.ttmi_tdt_scan_batch(fl, I(0), L(16), I(1), I(2), I(5), I(9), ints, ints, ints, ints, fl, None)
    assert rc < 0 and b"D=9 outside [1,8]" in lib.ttmi_last_error()
    longs, sc = (ctypes.c_longlong * 64)(), (ctypes.c_double * 8)()

    def advance(dur, **kw):
        k = dict(dec=ints, n=2, n_hist=1, ld_hist=4)
        k.update(kw)
        d = (ctypes.c_int * len(dur))(*dur)
        return lib.ttmi_tdt_advance(k["dec"], fl, I(1), I(k["n"]), I(0), d, I(len(dur)), I(k["n_hist"]), longs, L(k["ld_hist"]), ints, ints, ints,
                                    ints, ints, ints, ints, fl, ints, L(3), sc, None)
    assert advance((1, 2), dec=None) < 0 and b"tdt_advance: null pointer" in lib.ttmi_last_error()
    assert advance((2, 1)) < 0 and b"strictly increasing" in lib.ttmi_last_error()
    assert advance((1, 2), n=0) < 0 and b"bad arguments" in lib.ttmi_last_error()
    assert advance((1, 2), n_hist=4) < 0 and b"bad arguments" in lib.ttmi_last_error()
