"""Forced alignment and emission-time statistics from the RNN-T lattice, CPU side: the float64 reference the GPU tests compare with
(`viterbi_ref`, `emit_stats_ref`; pinned here against brute-force enumeration of every alignment), the planted-path generator the GPU
tests use, the C ABI's argument validation and the public Python surface.

Recurrence and tie rule (include/ttmi.h, ttmi_rnnt_align): v(0,0) = 0, v(t,u) = max(v(t-1,u) + lpb(t-1,u), v(t,u-1) + lpl(t,u-1)); the
label move is taken only when it is STRICTLY greater, a tie goes to blank.  frames[u] = the frame at which label u+1 is emitted."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT


# ----------------------------------------------------------------------------- float64 reference
def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def emissions(logits, labels, Tb, Ub, blank=0):
    """one utterance: logits [T, U+1, V] -> (lpb [Tb, Ub+1], lpl [Tb, Ub+1]; lpl[:, Ub] = -inf) in float64"""
    lp = log_softmax64(np.asarray(logits)[:Tb, :Ub + 1])
    lpb = lp[:, :, blank].copy()
    lpl = np.full((Tb, Ub + 1), -np.inf)
    for u in range(Ub):
        lpl[:, u] = lp[:, u, int(labels[u])]
    return lpb, lpl


def _diagonals(Tb, U1):
    """the cells of each anti-diagonal d = t + u >= 1 as index arrays (ts, us): a diagonal depends on the one before it only"""
    for d in range(1, Tb + U1 - 1):
        us = np.arange(max(0, d - Tb + 1), min(d, U1 - 1) + 1)
        yield d - us, us


def _viterbi(lpb, lpl):
    """-> (v [Tb, Ub+1] best prefix scores, lab [Tb, Ub+1] decision bits, score); numpy over one anti-diagonal at a time"""
    Tb, U1 = lpb.shape
    v = np.full((Tb, U1), -np.inf)
    lab = np.zeros((Tb, U1), dtype=bool)
    v[0, 0] = 0.0
    for ts, us in _diagonals(Tb, U1):
        # (index -1 wraps to a cell that exists; the term it forms is replaced by -inf)
        tt = np.where(ts > 0, v[ts - 1, us] + lpb[ts - 1, us], -np.inf)
        tu = np.where(us > 0, v[ts, us - 1] + lpl[ts, us - 1], -np.inf)
        take = tu > tt                          # strictly greater: a tie goes to blank
        v[ts, us] = np.where(take, tu, tt)
        lab[ts, us] = take
    return v, lab, float(v[Tb - 1, U1 - 1] + lpb[Tb - 1, U1 - 1])


def viterbi_ref(logits, labels, Tb, Ub, blank=0):
    """one utterance -> (frames int [Ub], score float): the best path under the recurrence and tie rule of the module docstring"""
    lpb, lpl = emissions(logits, labels, Tb, Ub, blank)
    _, lab, score = _viterbi(lpb, lpl)
    frames = np.full(Ub, -1, dtype=np.int64)
    t, u = Tb - 1, Ub
    while t > 0 or u > 0:
        if lab[t, u]:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return frames, score


def path_score(logits, labels, Tb, Ub, frames, blank=0):
    """float64 log-probability of the alignment that emits label u+1 at frames[u]"""
    lpb, lpl = emissions(logits, labels, Tb, Ub, blank)
    s, u = 0.0, 0
    for t in range(Tb):
        while u < Ub and frames[u] == t:
            s += lpl[t, u]
            u += 1
        s += lpb[t, u]
    assert u == Ub, "not an alignment: %s" % (frames,)
    return s


def _alpha_beta(lpb, lpl):
    Tb, U1 = lpb.shape
    al = np.full((Tb, U1), -np.inf)
    be = np.full((Tb, U1), -np.inf)
    al[0, 0] = 0.0
    for ts, us in _diagonals(Tb, U1):
        tt = np.where(ts > 0, al[ts - 1, us] + lpb[ts - 1, us], -np.inf)
        tu = np.where(us > 0, al[ts, us - 1] + lpl[ts, us - 1], -np.inf)
        al[ts, us] = np.logaddexp(tt, tu)
    be[Tb - 1, U1 - 1] = lpb[Tb - 1, U1 - 1]
    for d in range(Tb + U1 - 3, -1, -1):
        us = np.arange(max(0, d - Tb + 1), min(d, U1 - 1) + 1)
        ts = d - us
        tn, un = np.minimum(ts + 1, Tb - 1), np.minimum(us + 1, U1 - 1)      # clamped: the term is replaced by -inf where there is no such cell
        tt = np.where(ts < Tb - 1, be[tn, us] + lpb[ts, us], -np.inf)
        tu = np.where(us < U1 - 1, be[ts, un] + lpl[ts, us], -np.inf)
        be[ts, us] = np.logaddexp(tt, tu)
    return al, be, float(al[Tb - 1, U1 - 1] + lpb[Tb - 1, U1 - 1])


def emit_stats_ref(logits, labels, Tb, Ub, blank=0):
    """one utterance -> (expected [Ub], mass [Ub], ll): e(t,u) = exp(alpha(t,u) + lpl(t,u) + beta(t,u+1) - ll)"""
    lpb, lpl = emissions(logits, labels, Tb, Ub, blank)
    al, be, ll = _alpha_beta(lpb, lpl)
    if Ub == 0:
        return np.zeros(0), np.zeros(0), ll
    e = np.exp(al[:, :Ub] + lpl[:, :Ub] + be[:, 1:] - ll)
    return (np.arange(Tb)[:, None] * e).sum(axis=0), e.sum(axis=0), ll


def enumerate_alignments(logits, labels, Tb, Ub, blank=0):
    """every alignment (non-decreasing frames in [0, Tb)) with its float64 score"""
    out = []
    for fr in itertools.combinations_with_replacement(range(Tb), Ub):
        out.append((fr, path_score(logits, labels, Tb, Ub, fr, blank)))
    return out


# ----------------------------------------------------------------------------- planted paths (shared with tests/test_align_gpu.py)
V_PLANT = 32


def planted_utterance(rng, T, U, Tb, Ub, V=V_PLANT):
    """standard-normal logits [T, U+1, V], labels in 1..V-1, a sorted random frame per label; +8 on the label logit of each emission
    cell and +8 on the blank logit of every other cell of the path"""
    logits = rng.standard_normal((T, U + 1, V)).astype(np.float32)
    labels = rng.integers(1, V, size=U).astype(np.int32)
    frames = np.sort(rng.integers(0, Tb, size=Ub)).astype(np.int64)
    u = 0
    for t in range(Tb):
        while u < Ub and frames[u] == t:
            logits[t, u, labels[u]] += 8.0
            u += 1
        logits[t, u, 0] += 8.0
    return logits, labels, frames


def planted_batch(seed, B, T, U, V=V_PLANT):
    """ragged batch: utterance 0 has the full lengths, utterance 1 (if any) U_b = 0, utterance 2 (if any) T_b = 1, the rest random.
    -> logits f32 [B,T,U+1,V], labels i32 [B,U], act_lens i32 [B], label_lens i32 [B], frames i64 [B,U] (-1 padded)"""
    rng = np.random.default_rng(seed)
    logits = np.zeros((B, T, U + 1, V), dtype=np.float32)
    labels = np.zeros((B, U), dtype=np.int32)
    frames = np.full((B, U), -1, dtype=np.int64)
    al, ll = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        Tb, Ub = int(rng.integers(1, T + 1)), int(rng.integers(0, U + 1))
        if b == 0:
            Tb, Ub = T, U
        elif b == 1:
            Ub = 0
        elif b == 2:
            Tb = 1
        logits[b], labels[b], fr = planted_utterance(rng, T, U, Tb, Ub, V)
        frames[b, :Ub] = fr
        al[b], ll[b] = Tb, Ub
    return logits, labels, al, ll, frames


def planted_gap(logits, labels, Tb, Ub, frames, blank=0):
    """best path score minus the score of the best path that moves any ONE label off its planted frame (inf without labels): with v the
    best prefix and w the best suffix scores, the best path emitting label u+1 at frame t is v(t,u) + lpl(t,u) + w(t,u+1)"""
    if Ub == 0:
        return float("inf")
    lpb, lpl = emissions(logits, labels, Tb, Ub, blank)
    v, _, best = _viterbi(lpb, lpl)
    # suffix scores: the same recurrence on the reversed lattice
    U1 = Ub + 1
    w = np.full((Tb, U1), -np.inf)
    w[Tb - 1, Ub] = lpb[Tb - 1, Ub]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                continue
            tt = w[t + 1, u] + lpb[t, u] if t < Tb - 1 else -np.inf
            tu = w[t, u + 1] + lpl[t, u] if u < Ub else -np.inf
            w[t, u] = max(tt, tu)
    gap = float("inf")
    for u in range(Ub):
        through = v[:, u] + lpl[:, u] + w[:, u + 1]
        assert abs(through[frames[u]] - best) < 1e-9 * max(1.0, abs(best)), "the planted path is not the best path"
        other = np.delete(through, frames[u])
        if other.size:
            gap = min(gap, best - other.max())
    return gap


# (name, seed, B, T, U): U+1 in {1, 2, 51, 64, 65, 201} and the slot counts of the kernel's dispatch (129 = 3 slots -> R 4, 257 -> R 8, 513 and
# 961 -> R 16, 1024 = the largest supported), T in {1, 7, 500}; every batch of three or more has a U_b = 0 and a T_b = 1 utterance
GPU_PLANTED_CASES = [
    ("u1_1", 11, 3, 7, 0), ("u1_2", 12, 4, 7, 1), ("t1", 13, 3, 1, 5), ("u1_51", 14, 4, 500, 50), ("u1_64", 15, 4, 7, 63),
    ("u1_64_long", 16, 3, 500, 63), ("u1_65", 17, 4, 7, 64), ("u1_65_long", 18, 3, 500, 64), ("u1_129", 19, 3, 7, 128),
    ("u1_201", 20, 3, 500, 200), ("u1_257", 21, 3, 7, 256), ("u1_513", 22, 3, 7, 512), ("u1_961", 23, 3, 7, 960), ("u1_1024", 24, 3, 7, 1023),
]


# ----------------------------------------------------------------------------- 1. the reference, pinned
@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("U", [0, 1, 2, 3])
def test_reference_against_enumeration(T, U):
    rng = np.random.default_rng(100 * T + U)
    for V in (2, 3, 5):
        for _ in range(4):
            logits = rng.standard_normal((T, U + 1, V)) * 2.0
            labels = rng.integers(0, V, size=U)          # labels equal to the blank symbol included
            allp = enumerate_alignments(logits, labels, T, U)
            best = max(s for _, s in allp)
            frames, score = viterbi_ref(logits, labels, T, U)
            assert abs(score - best) <= 1e-12 * max(1.0, abs(best))
            assert abs(path_score(logits, labels, T, U, frames) - best) <= 1e-12 * max(1.0, abs(best))      # the returned path is a maximiser
            assert all(0 <= frames[i] < T for i in range(U)) and all(frames[i] <= frames[i + 1] for i in range(U - 1))
            scores = np.array([s for _, s in allp])
            ll = np.log(np.exp(scores - best).sum()) + best
            post = np.exp(scores - ll)
            expected, mass, ll_ref = emit_stats_ref(logits, labels, T, U)
            assert abs(ll_ref - ll) <= 1e-12 * max(1.0, abs(ll))
            for u in range(U):
                assert abs(mass[u] - 1.0) <= 1e-12
                mean = sum(p * fr[u] for (fr, _), p in zip(allp, post))
                assert abs(expected[u] - mean) <= 1e-12 * max(1.0, T)


def test_tie_goes_to_blank():
    """all logits equal: every path has the same score; a cell with a choice is entered by the blank move, so the backtrace from
    (T-1, U) runs down the last column to frame 0 and every label is emitted there"""
    T, U = 4, 3
    frames, _ = viterbi_ref(np.zeros((T, U + 1, 5)), np.array([1, 2, 3]), T, U)
    assert list(frames) == [0] * U


# ----------------------------------------------------------------------------- 2. planted paths
def test_planted_paths_small_seeds():
    worst = float("inf")
    for seed in range(60):
        rng = np.random.default_rng(1000 + seed)
        T, U = int(rng.integers(1, 40)), int(rng.integers(0, 12))
        Tb, Ub = int(rng.integers(1, T + 1)), int(rng.integers(0, U + 1))
        logits, labels, planted = planted_utterance(rng, T, U, Tb, Ub)
        frames, score = viterbi_ref(logits, labels, Tb, Ub)
        assert list(frames) == list(planted), seed
        assert abs(score - path_score(logits, labels, Tb, Ub, planted)) < 1e-9
        worst = min(worst, planted_gap(logits, labels, Tb, Ub, planted))
    assert worst > 1.0, worst


@pytest.mark.parametrize("case", GPU_PLANTED_CASES, ids=[c[0] for c in GPU_PLANTED_CASES])
def test_planted_paths_of_the_gpu_cases(case):
    """the batches tests/test_align_gpu.py feeds the kernel: the reference returns the planted frames and no utterance leans on a near-tie
    (moving any one label off its frame costs more than 1 nat; measured minimum over these batches: see the assertion message)"""
    _, seed, B, T, U = case
    logits, labels, al, ll, planted = planted_batch(seed, B, T, U)
    assert al[0] == T and ll[0] == U and (B < 2 or ll[1] == 0) and (B < 3 or al[2] == 1)
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        frames, _ = viterbi_ref(logits[b], labels[b], Tb, Ub)
        assert list(frames) == list(planted[b, :Ub]) and (planted[b, Ub:] == -1).all()
        gap = planted_gap(logits[b], labels[b], Tb, Ub, planted[b])
        assert gap > 1.0, (b, gap)


# ----------------------------------------------------------------------------- 3. ABI
NAMES = ("ttmi_rnnt_align_workspace_bytes", "ttmi_rnnt_align", "ttmi_rnnt_emit_stats")


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_abi_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ttmi.h")).read()
    declared = set(re.findall(r"\b(ttmi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib()
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert "strictly greater" in hdr and "tie goes to blank" in hdr          # the tie rule is part of the published contract
    assert lib.ttmi_version() >= 101


def test_abi_argument_validation_without_gpu():
    lib = _lib()
    lib.ttmi_rnnt_align_workspace_bytes.restype = ctypes.c_size_t
    wsb = lib.ttmi_rnnt_align_workspace_bytes
    assert 0 < wsb(2, 100, 51) < wsb(2, 200, 51) < wsb(2, 200, 65)          # grows with T and with the 64-label groups
    assert wsb(2, 500, 51) >= 2 * (500 + 50) * 8
    assert wsb(0, 10, 4) == 0 and wsb(2, -1, 4) == 0
    buf = (ctypes.c_double * 64)()
    ok = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    # null pointers
    rc = lib.ttmi_rnnt_align(None, None, None, 1, 4, 3, None, None, None, None)
    assert rc < 0 and b"rnnt_align: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_align(ok, ok, ok, 1, 4, 3, None, ok, ok, None)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_emit_stats(None, None, None, 1, 4, 3, None, None, None)
    assert rc < 0 and b"rnnt_emit_stats: null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_emit_stats(ok, ok, ok, 1, 4, 3, ok, None, None)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    # shapes
    for B, T, U1 in ((0, 4, 3), (1, 0, 3), (1, 4, 0), (-1, 4, 3)):
        rc = lib.ttmi_rnnt_align(ok, ok, ok, B, T, U1, ok, ok, ok, None)
        assert rc < 0 and b"bad shape" in lib.ttmi_last_error(), (B, T, U1)
        rc = lib.ttmi_rnnt_emit_stats(ok, ok, ok, B, T, U1, ok, ok, None)
        assert rc < 0 and b"bad shape" in lib.ttmi_last_error(), (B, T, U1)
    rc = lib.ttmi_rnnt_align(ok, ok, ok, 1, 4, 1025, ok, ok, ok, None)
    assert rc < 0 and b"1024" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_emit_stats(ok, ok, ok, 1, 4, 1025, ok, ok, None)
    assert rc < 0 and b"1024" in lib.ttmi_last_error()
    # misaligned workspaces
    rc = lib.ttmi_rnnt_align(odd, ok, ok, 1, 4, 3, ok, ok, ok, None)
    assert rc < 0 and b"aligned" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_align(ok, ok, ok, 1, 4, 3, odd, ok, ok, None)
    assert rc < 0 and b"aligned" in lib.ttmi_last_error()
    rc = lib.ttmi_rnnt_emit_stats(odd, ok, ok, 1, 4, 3, ok, ok, None)
    assert rc < 0 and b"aligned" in lib.ttmi_last_error()


# ----------------------------------------------------------------------------- 4. public surface
def test_public_surface_rnnt_align():
    import torch
    import warprnnt_pytorch as W
    assert "rnnt_align" in W.__all__ and callable(W.rnnt_align)
    acts = torch.zeros(2, 4, 3, 5)
    labels = torch.ones(2, 2, dtype=torch.int32)
    al, ll = torch.tensor([4, 3], dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        W.rnnt_align(acts, labels, al, ll)                                   # CPU tensors: no CPU path, as for the loss
    with pytest.raises(ValueError, match="GPU"):
        W.rnnt_align(acts, labels, al, ll, stats=True)
    with pytest.raises(TypeError):
        W.rnnt_align(acts, labels.long(), al, ll)                            # int32 labels / lengths, as for the loss
    with pytest.raises(TypeError):
        W.rnnt_align(acts.double(), labels, al, ll)
    with pytest.raises(ValueError):
        W.rnnt_align(acts, labels[:, :1], al, ll)                            # labels must be [B, U]
    with pytest.raises(ValueError):
        W.rnnt_align(acts, labels, al - 1, ll)                               # max(act_lens) != T
    with pytest.raises(ValueError):
        W.rnnt_align(acts, labels, al[:1], ll)
    r = W.AlignResult(1, 2, 3)
    assert r._fields == ("frames", "score", "cost", "expected_frames", "mass") and r.expected_frames is None and r.mass is None


def test_public_surface_ops_and_model():
    import inspect
    import torch
    from tt.model import DeferredLogits, Transducer
    from tt.utils import AttrDict
    from ttmi import ops
    ws = torch.zeros(64)
    one = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.rnnt_align(ws, one, one, 1, 1, 1)
    with pytest.raises(ValueError):
        ops.rnnt_emit_stats(ws, one, one, 1, 1, 1)
    sig = inspect.signature(Transducer.align)
    assert list(sig.parameters)[1:] == ["inputs", "inputs_length", "targets", "targets_length", "chunk", "check_lengths", "exp_domain", "stats"]
    assert sig.parameters["stats"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["exp_domain"].default is False
    assert callable(DeferredLogits.rnnt_align)
    side = dict(n_layer=1, d_model=16, n_head=2, d_head=8, d_inner=16)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=32, inner_size=16), vocab_size=7, dropout=0.0))
    model = Transducer(cfg)
    x, y = torch.zeros(2, 6, 16), torch.ones(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="GPU"):
        model.align(x, torch.tensor([6, 5]), y, torch.tensor([3, 2]))
    with pytest.raises(ValueError):
        model.align(x, torch.tensor([6]), y, torch.tensor([3, 2]))           # a length per utterance, checked before anything runs
