"""CPU-only: the CTC hypothesis scorer's entries (include/ttmi.h: ttmi_ctc_score_ws_bytes, ttmi_ctc_score_hyps) are exported, and every refusal
the header lists returns rc < 0 with a ttmi_last_error text before any launch - no GPU is touched."""
import ctypes
import os
import subprocess

import pytest

from conftest import PKG

I, L = ctypes.c_int, ctypes.c_long


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_symbols_are_exported_and_the_workspace_is_sized():
    lib = _lib()
    for n in ("ttmi_ctc_score_ws_bytes", "ttmi_ctc_score_hyps"):
        assert hasattr(lib, n), n
    f = lib.ttmi_ctc_score_ws_bytes
    f.restype = ctypes.c_size_t
    # one f32 log-sum-exp per (utterance, frame), rounded up to 16 bytes - whatever the number of hypotheses
    assert f(1, 1) == 16 and f(1, 4) == 16 and f(1, 5) == 32 and f(32, 500) == 64000 and f(3, 7) == 96
    assert f(0, 5) == 0 and f(1, 0) == 0 and f(-1, 5) == 0 and f(5, -3) == 0


# host memory stands in for the device pointers: a refused call reads none of it
def _bufs():
    fl = (ctypes.c_float * 64)()
    ints = (ctypes.c_int * 64)()
    longs = (ctypes.c_longlong * 64)()
    ws = (ctypes.c_double * 64)()
    sc = (ctypes.c_double * 64)()
    assert ctypes.addressof(ws) % 16 == 0 and ctypes.addressof(sc) % 8 == 0
    return fl, ints, longs, ws, sc


KEYS = ("logits", "ldv", "act_lens", "B", "T", "V", "blank", "hyp", "ld_hyp", "hyp_len", "utt", "P", "U", "ws", "score")


def _good():
    fl, ints, longs, ws, sc = _bufs()
    return dict(logits=fl, ldv=5, act_lens=ints, B=2, T=4, V=5, blank=0, hyp=longs, ld_hyp=3, hyp_len=ints, utt=ints, P=4, U=3, ws=ws, score=sc)


def _call(lib, a):
    return lib.ttmi_ctc_score_hyps(a["logits"], L(a["ldv"]), a["act_lens"], I(a["B"]), I(a["T"]), I(a["V"]), I(a["blank"]), a["hyp"],
                                   L(a["ld_hyp"]), a["hyp_len"], a["utt"], I(a["P"]), I(a["U"]), a["ws"], a["score"], None)


def _refused(lib, rc, text):
    assert rc < 0, rc
    msg = lib.ttmi_last_error()
    assert msg and text in msg, (text, msg)


def test_null_pointers():
    lib = _lib()
    for k in ("logits", "act_lens", "hyp", "hyp_len", "ws", "score"):
        a = _good()
        a[k] = None
        _refused(lib, _call(lib, a), b"ctc_score_hyps: null pointer")
    # hyp may be null when U = 0 and utt may always be null: those calls get past the pointer check and are refused by a later one
    a = _good()
    a.update(hyp=None, U=0, blank=7)
    _refused(lib, _call(lib, a), b"blank 7 outside [0,5)")
    a = _good()
    a.update(utt=None, blank=7)
    _refused(lib, _call(lib, a), b"blank 7 outside [0,5)")


BAD = [("B0", dict(B=0), b"bad shape"), ("T0", dict(T=0), b"bad shape"), ("P0", dict(P=0), b"bad shape"), ("P_negative", dict(P=-4), b"bad shape"),
       ("V1", dict(V=1, ldv=5), b"bad shape"), ("V0", dict(V=0), b"bad shape"),
       ("blank_negative", dict(blank=-1), b"blank -1 outside [0,5)"), ("blank_V", dict(blank=5), b"blank 5 outside [0,5)"),
       ("U_negative", dict(U=-1), b"bad shape U=-1"), ("U1024", dict(U=1024, ld_hyp=2048), b"U=1024 > 1023"),
       ("U_above_pitch", dict(U=4), b"U=4 above the hypothesis pitch 3"), ("ldv_below_V", dict(ldv=4), b"bad pitch"),
       ("P_no_multiple_of_B", dict(utt=None, P=3), b"P=3 must be a multiple of B=2")]


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_arguments_outside_the_limits(case):
    lib = _lib()
    a = _good()
    a.update(case[1])
    _refused(lib, _call(lib, a), case[2])


def test_an_explicit_utt_lifts_the_multiple_rule():
    """P = 3 on B = 2 is refused only without utt: with it the call passes that check (and is stopped here by the next one)"""
    lib = _lib()
    a = _good()
    a.update(P=3)
    a["ws"] = ctypes.c_void_p(ctypes.addressof(a["ws"]) + 8)
    _refused(lib, _call(lib, a), b"workspace must be 16-byte aligned")


def test_misaligned_workspace_and_score():
    lib = _lib()
    a = _good()
    a["ws"] = ctypes.c_void_p(ctypes.addressof(a["ws"]) + 8)
    _refused(lib, _call(lib, a), b"workspace must be 16-byte aligned")
    a = _good()
    a["score"] = ctypes.c_void_p(ctypes.addressof(a["score"]) + 4)
    _refused(lib, _call(lib, a), b"score must be 8-byte aligned")


def test_python_wrappers_fail_loudly_without_device():
    import torch
    from ttmi import ops
    from ttmi.ctc import ctc_score
    x = torch.zeros(2, 4, 5)
    n = torch.ones(2, dtype=torch.int32)
    hyp, hl = torch.zeros(4, 3, dtype=torch.int64), torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.ctc_score_hyps(x, n, hyp, hl)
    with pytest.raises(ValueError):
        ops.ctc_score_hyps(x, n, hyp, hl, utt=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        ctc_score(x, [[[1]], [[2, 3]]])
    with pytest.raises(ValueError, match="GPU"):
        ctc_score(x, [[[1]], []], act_lens=n)


def test_model_entry_points_take_the_rescoring_arguments():
    """both searches take ctc_weight / return_ctc with defaults that change nothing, and Transducer.ctc_score has the documented signature"""
    import inspect
    from tt.model import Transducer
    for fn in (Transducer.beam_decode_batch, Transducer.recognize_nbest):
        p = inspect.signature(fn).parameters
        assert p["ctc_weight"].default == 0.0 and p["return_ctc"].default is False
    assert list(inspect.signature(Transducer.ctc_score).parameters)[1:] == ["inputs", "inputs_length", "hypotheses", "audio_mask"]
