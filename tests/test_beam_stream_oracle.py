"""The numpy restatement of the stable prefix (tests/beam_stream_oracle.py; the rule: include/ttmi.h, ttmi_beam_stable_prefix) checked without
a GPU against what it claims: on the kernel tests' synthetic model the prefix reported after a frame is a prefix of every live hypothesis
after every later frame and the count never decreases; a beam of one has nothing tentative; three planted defects each change the answer
on a stated input.  Then what the new entry points refuse before they touch a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import beam_oracle as BO
import beam_stream_oracle as SO
from conftest import PKG, ROOT


@pytest.mark.parametrize("history", ["full", "stream"])
@pytest.mark.parametrize("W", [1, 2, 4])
def test_stable_prefix_is_permanent(W, history):
    V, T = 7, 10
    for seed in range(4):
        logits = BO.rng_logits(seed, V)
        _, counts, beams = SO.drive(logits, 0, T, W, history=history, max_history=3)
        assert all(a <= b for a, b in zip(counts, counts[1:])), counts
        for t in range(T):
            live = [h for h in beams[t] if h is not None]
            assert live and all(len(h.tokens) >= counts[t] for h in live)
            prefix = live[0].tokens[:counts[t]]
            for later in beams[t:]:
                assert all(h.tokens[:counts[t]] == prefix for h in later if h is not None), (seed, t, prefix, later)
        if W == 1:
            assert counts == [len(b[0].tokens) for b in beams]
    if W == 2 and history == "full":                                  # the case is not vacuous: something is stable before the end, not all of it
        _, counts, beams = SO.drive(BO.rng_logits(2, V), 0, T, W)
        assert 0 < counts[3] < counts[-1] < min(len(h.tokens) for h in beams[-1] if h is not None), counts


def test_stable_prefix_rule_on_stated_inputs():
    inf = math.inf
    hist = np.array([[[0, 5, 6, 7, 9], [0, 5, 6, 8, 9], [0, 5, 6, 7, 9], [0, 1, 1, 1, 1]]])
    assert SO.stable_prefix([[0.0, -1.0, -2.0, -inf]], [[4, 4, 3, 4]], hist).tolist() == [2]
    assert SO.stable_prefix([[0.0, -inf, -2.0, -inf]], [[4, 4, 3, 4]], hist).tolist() == [3]        # the shorter slot bounds it
    assert SO.stable_prefix([[-inf, -1.0, -inf, -inf]], [[4, 4, 3, 4]], hist).tolist() == [4]       # slot 0 empty: w0 = 1
    assert SO.stable_prefix([[0.0, math.nan, -2.0, -inf]], [[4, 4, 3, 4]], hist).tolist() == [3]    # NaN is empty
    assert SO.stable_prefix([[-inf] * 4], [[4, 4, 3, 4]], hist).tolist() == [0]
    assert SO.stable_prefix([[0.0, -1.0, -2.0, -3.0]], [[0, 0, 0, 0]], hist).tolist() == [0]
    assert SO.stable_prefix([[0.0, -inf, 0.0, -inf]], [[99, 4, 99, 4]], hist).tolist() == [4]       # len clamped to ld_hist - 1
    assert SO.stable_prefix([[0.0, -inf, 0.0, -inf]], [[-3, 4, 99, 4]], hist).tolist() == [0]


def test_planted_defects_change_the_answer():
    inf = math.inf
    # empty slots counted as live: slot 3 is empty and spells something else
    hist = np.array([[[0, 5, 6, 7], [0, 5, 6, 7], [0, 5, 6, 8], [0, 1, 1, 1]]])
    args = ([[0.0, -1.0, -2.0, -inf]], [[3, 3, 3, 3]], hist)
    assert SO.stable_prefix(*args).tolist() == [2] and SO.stable_prefix(*args, defect="empty_live").tolist() == [0]
    # the comparison starting at column 0: the start symbol, which every slot shares, is counted as a token
    args = ([[0.0, -1.0, -inf, -inf]], [[3, 3, 0, 0]], hist)
    assert SO.stable_prefix(*args).tolist() == [3]
    hist2 = np.array([[[0, 5, 6, 7], [0, 9, 6, 7], [0, 0, 0, 0], [0, 0, 0, 0]]])
    args = ([[0.0, -1.0, -inf, -inf]], [[3, 3, 0, 0]], hist2)
    assert SO.stable_prefix(*args).tolist() == [0] and SO.stable_prefix(*args, defect="column_0").tolist() == [1]
    # len of the first slot used for all: slot 1 holds one token and stale words behind it that happen to agree
    args = ([[0.0, -1.0, -inf, -inf]], [[3, 1, 0, 0]], hist)
    assert SO.stable_prefix(*args).tolist() == [1] and SO.stable_prefix(*args, defect="first_len").tolist() == [3]
    # ... and on the driver's beams of the synthetic model the column defect shows wherever a tentative tail exists (the other two need an
    # empty slot or stale words that agree, which these full beams do not have: the stated inputs above are their cases)
    V, W, T = 7, 2, 10
    _, counts, beams = SO.drive(BO.rng_logits(2, V), 0, T, W)
    for beam, want in zip(beams, counts):
        arrays = SO.to_arrays(beam, W, T + 2)
        tail = want < min(len(h.tokens) for h in beam if h is not None)
        assert SO.stable_prefix(*arrays, defect="column_0").tolist() == [want + 1 if tail else want]


def _tiny_cpu_model():
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    torch.manual_seed(0)
    return Transducer(cfg).eval()


def test_streaming_arguments_are_checked_without_a_device():
    from ttmi.context import ContextGraph
    from ttmi.streaming import StreamingRecognizer
    model = _tiny_cpu_model()
    kw = dict(left_context=2, right_context=1)
    with pytest.raises(ValueError, match="GPU"):
        StreamingRecognizer(model, beam_width=4, **kw)
    with pytest.raises(ValueError, match="beam_width"):
        StreamingRecognizer(model, context=ContextGraph([[3, 4]], boost=2.0), **kw)
    with pytest.raises(ValueError, match="beam_width"):
        StreamingRecognizer(model, lm_weight=0.3, **kw)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="beam_width"):
            StreamingRecognizer(model, beam_width=bad, **kw)
    with pytest.raises(ValueError, match="GPU"):
        model.beam_search_state(1, 4)


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_stable_prefix_entry_point_refuses_before_any_launch():
    """declared in the header, exported by the library, and every refusal comes with rc < 0 and a message on a machine without a device"""
    header = open(os.path.join(ROOT, "include", "ttmi.h")).read()
    decl = re.search(r"int ttmi_beam_stable_prefix\(([^;]*)\);", header)
    assert decl and re.sub(r"\s+", " ", decl.group(1)) == ("const double* score, const int* len, const long* hist, long ld_hist, int B, int W, "
                                                          "int* stable, void* stream")
    lib = _lib()
    fn = lib.ttmi_beam_stable_prefix
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    buf = (ctypes.c_long * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(score=p, len=p, hist=p, ld_hist=5, B=2, W=4, stable=p)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["score"], a["len"], a["hist"], a["ld_hist"], a["B"], a["W"], a["stable"], None)
    for name in ("score", "len", "hist", "stable"):
        assert call(**{name: None}) < 0 and b"null pointer" in lib.ttmi_last_error(), name
    for W in (0, 33):
        assert call(W=W) < 0 and b"beam width %d" % W in lib.ttmi_last_error()
    assert call(ld_hist=0) < 0 and b"ld_hist = 0" in lib.ttmi_last_error()
    assert call(B=-1) < 0 and b"B = -1" in lib.ttmi_last_error()
    assert call(B=0) == 0                                    # nothing to do: no launch, no device needed
