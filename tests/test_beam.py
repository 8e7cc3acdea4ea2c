"""CPU-only side of the frame-synchronous beam search: the float64 oracle of the rule (tests/beam_oracle.py) against a brute-force sum over
every decision sequence, ttmi_beam_step's argument validation without a GPU, and beam decoding on CPU tensors being an error (this build has
no CPU path).

With V = 3 and T = 4 there are 1 + 2 + 4 + 8 + 16 = 31 token sequences, so a beam of 32 prunes nothing: the oracle's merged scores must then be
the brute force's sums over all 3^4 decision sequences grouped by token sequence, and the total mass 1."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import beam_oracle as BO
from conftest import PKG


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_without_pruning_is_the_brute_force_sum(seed, blank):
    V, T, W = 3, 4, 32
    logits = BO.rng_logits(seed, V)
    beam, margin, _ = BO.run(logits, 0, T, W, blank)
    want = BO.brute_force(logits, 0, T, blank)
    assert len(want) == 31 and len(beam) == 31
    assert {h.tokens for h in beam} == set(want)
    worst = max(abs(h.score - want[h.tokens]) for h in beam)
    mass = sum(math.exp(h.score) for h in beam)
    print("seed %d blank %d: max |oracle - brute force| = %.3e, mass = %.15f, margin %.3e" % (seed, blank, worst, mass, margin))
    assert worst <= 1e-12
    assert abs(mass - 1.0) <= 1e-12
    assert all(a.score >= b.score for a, b in zip(beam, beam[1:]))
    for h in beam:                                           # the details are one path's: a frame and a log-probability per token, in frame order
        assert len(h.frames) == len(h.logprobs) == len(h.tokens)
        assert all(a < b for a, b in zip(h.frames, h.frames[1:])) and all(0 <= f < T for f in h.frames)
        path = 0.0                                           # that path's own score: never above the merged one
        toks = ()
        for t in range(T):
            lp = BO.log_softmax(logits(0, t, toks))
            if t in h.frames:
                k = h.tokens[h.frames.index(t)]
                assert abs(lp[k] - h.logprobs[h.frames.index(t)]) <= 1e-15
                path, toks = path + lp[k], toks + (k,)
            else:
                path += lp[blank]
        assert toks == h.tokens and path <= h.score + 1e-12


def test_oracle_beam_of_one_is_the_greedy_path():
    V, T = 37, 12
    logits = BO.rng_logits(3, V)
    beam, _, _ = BO.run(logits, 0, T, 1)
    toks, score, frames = (), 0.0, ()
    for t in range(T):
        lp = BO.log_softmax(logits(0, t, toks))
        k = int(np.argmax(lp))
        score += lp[k]
        if k != 0:
            toks, frames = toks + (k,), frames + (t,)
    assert len(beam) == 1 and beam[0].tokens == toks and beam[0].frames == frames and abs(beam[0].score - score) <= 1e-12


def test_oracle_pruned_beam_is_distinct_sorted_and_below_the_full_sums():
    V, T, W = 5, 6, 4
    logits = BO.rng_logits(1, V)
    beam, _, _ = BO.run(logits, 0, T, W)
    full = BO.brute_force(logits, 0, T)
    assert len(beam) == W and len({h.tokens for h in beam}) == W
    assert all(a.score >= b.score for a, b in zip(beam, beam[1:]))
    assert all(h.score <= full[h.tokens] + 1e-12 for h in beam)          # pruning only ever drops mass


def test_oracle_row_with_nan_empties_the_beam():
    logits = BO.rng_logits(0, 5)

    def bad(b, t, tokens):
        x = logits(b, t, tokens).copy()
        if t == 1:
            x[2] = np.nan
        return x
    beam, _, _ = BO.run(bad, 0, 3, 1)
    assert beam == []


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_beam_step_validates_its_arguments_without_gpu():
    lib = _lib()
    L = ctypes.c_long
    buf = (ctypes.c_double * 8)()
    bufs = [(ctypes.c_double * 8)() for _ in range(5)]
    p = ctypes.cast(buf, ctypes.c_void_p)
    o = [ctypes.cast(x, ctypes.c_void_p) for x in bufs]      # the _out arrays: buffers of their own

    def call(logits=p, ld=5, B=1, W=4, V=5, blank=0, ins=(p, p, p, p, p), outs=None, ld_hist=8, ld_det=8, parent=p, dtype=0):
        outs = o if outs is None else outs
        return lib.ttmi_beam_step(logits, dtype, L(ld), B, W, V, blank, p, p, *ins, *outs, L(ld_hist), L(ld_det), parent, p, None)

    assert call(logits=None) < 0 and b"beam_step" in lib.ttmi_last_error() and b"null pointer" in lib.ttmi_last_error()
    assert call(parent=None) < 0 and b"null pointer" in lib.ttmi_last_error()
    for W in (0, 33, -1):
        assert call(W=W) < 0 and b"beam width" in lib.ttmi_last_error()
    assert call(V=1, ld=1) < 0 and b"bad arguments" in lib.ttmi_last_error()
    assert call(ld=4) < 0                                    # pitch below V
    assert call(blank=5) < 0 and call(blank=-1) < 0
    assert call(ld_hist=1) < 0 and call(ld_det=0) < 0 and call(B=0) < 0
    assert call(dtype=2) < 0
    assert call(ins=(p, p, p, None, p)) < 0 and b"all four" in lib.ttmi_last_error()
    assert call(outs=[p] + o[1:]) < 0 and b"buffers of its own" in lib.ttmi_last_error()


def test_beam_decoding_on_cpu_tensors_is_an_error():
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    torch.manual_seed(0)
    model = Transducer(cfg).eval()
    with pytest.raises(ValueError, match="must live on the GPU"):
        model.beam_decode_batch(torch.zeros(2, 6, 64), [6, 4])
    with pytest.raises(ValueError, match="must live on the GPU"):
        model.recognize_nbest(torch.zeros(2, 6, 64), torch.tensor([6, 4]))
