"""CPU-only: the CTC alignment entries (include/ttmi.h: ttmi_ctc_align_workspace_bytes, ttmi_ctc_align, ttmi_ctc_emit_stats) are exported, and
every refusal the header lists returns rc < 0 with a ttmi_last_error text before any launch - no GPU is touched."""
import ctypes
import os
import subprocess

import pytest

from conftest import PKG

I = ctypes.c_int


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_symbols_are_exported_and_the_workspace_is_sized():
    lib = _lib()
    for n in ("ttmi_ctc_align_workspace_bytes", "ttmi_ctc_align", "ttmi_ctc_emit_stats"):
        assert hasattr(lib, n), n
    f = lib.ttmi_ctc_align_workspace_bytes
    f.restype = ctypes.c_size_t
    # three 8-byte decision words per frame and 64 label positions (U + 1 pairs of states)
    assert f(1, 1, 0) == 24 and f(2, 10, 63) == 2 * 10 * 24 and f(2, 10, 64) == 2 * 10 * 2 * 24 and f(1, 1030, 1023) == 1030 * 16 * 24
    assert f(1, 1030, 1023) > 128 * 1024 >= f(1, 500, 50)                       # the first lives in global memory by its shape
    assert f(0, 5, 5) == 0 and f(1, 0, 5) == 0 and f(1, 5, -1) == 0 and f(1, 5, 1024) == 0


# host memory stands in for the device pointers: a refused call reads none of it
def _bufs():
    ws = (ctypes.c_double * 64)()
    ints = (ctypes.c_int * 64)()
    aws = (ctypes.c_longlong * 64)()
    fl = (ctypes.c_float * 64)()
    assert ctypes.addressof(ws) % 16 == 0 and ctypes.addressof(aws) % 8 == 0
    return ws, ints, aws, fl


def _align(lib, ws, labels, al, ll, B, T, U, V, blank, aws, path, spans, score):
    return lib.ttmi_ctc_align(ws, labels, al, ll, I(B), I(T), I(U), I(V), I(blank), aws, path, spans, score, None)


def _stats(lib, ws, labels, al, ll, B, T, U, V, blank, e, m, d):
    return lib.ttmi_ctc_emit_stats(ws, labels, al, ll, I(B), I(T), I(U), I(V), I(blank), e, m, d, None)


def _refused(lib, rc, text):
    assert rc < 0, rc
    msg = lib.ttmi_last_error()
    assert msg and text in msg, (text, msg)


def test_align_null_pointers():
    lib = _lib()
    ws, ints, aws, fl = _bufs()
    good = [ws, ints, ints, ints, 1, 4, 2, 5, 0, aws, ints, ints, fl]
    for i in (0, 1, 2, 3, 9, 10, 11, 12):
        args = list(good)
        args[i] = None
        _refused(lib, _align(lib, *args), b"ctc_align: null pointer")


def test_emit_stats_null_pointers():
    lib = _lib()
    ws, ints, aws, fl = _bufs()
    good = [ws, ints, ints, ints, 1, 4, 2, 5, 0, fl, fl, fl]
    for i in (0, 1, 2, 3, 9, 10, 11):
        args = list(good)
        args[i] = None
        _refused(lib, _stats(lib, *args), b"ctc_emit_stats: null pointer")


BAD_SHAPES = [("B0", dict(B=0), b"bad shape"), ("T0", dict(T=0), b"bad shape"), ("U_negative", dict(U=-1), b"bad shape"),
              ("U1024", dict(U=1024), b"U=1024 > 1023"), ("V1", dict(V=1), b"bad shape"), ("V0", dict(V=0), b"bad shape"),
              ("blank_negative", dict(blank=-1), b"blank -1 outside [0,5)"), ("blank_V", dict(blank=5), b"blank 5 outside [0,5)")]


@pytest.mark.parametrize("case", BAD_SHAPES, ids=[c[0] for c in BAD_SHAPES])
def test_shapes_outside_the_limits(case):
    lib = _lib()
    ws, ints, aws, fl = _bufs()
    dims = dict(B=1, T=4, U=2, V=5, blank=0)
    dims.update(case[1])
    d = [dims[k] for k in ("B", "T", "U", "V", "blank")]
    _refused(lib, _align(lib, ws, ints, ints, ints, *d, aws, ints, ints, fl), case[2])
    _refused(lib, _stats(lib, ws, ints, ints, ints, *d, fl, fl, fl), case[2])


def test_misaligned_workspaces():
    lib = _lib()
    ws, ints, aws, fl = _bufs()
    off = ctypes.c_void_p(ctypes.addressof(aws) + 4)
    _refused(lib, _align(lib, ws, ints, ints, ints, 1, 4, 2, 5, 0, off, ints, ints, fl), b"align_workspace must be 8-byte aligned")
    off = ctypes.c_void_p(ctypes.addressof(ws) + 8)
    _refused(lib, _align(lib, off, ints, ints, ints, 1, 4, 2, 5, 0, aws, ints, ints, fl), b"workspace must be 16-byte aligned")
    _refused(lib, _stats(lib, off, ints, ints, ints, 1, 4, 2, 5, 0, fl, fl, fl), b"workspace must be 16-byte aligned")


def test_python_wrappers_fail_loudly_without_device():
    import torch
    from ttmi import ops
    from ttmi.ctc import CTCAlignment, ctc_align
    assert CTCAlignment._fields == ("path", "spans", "score", "expected", "mass", "duration")
    y, n = torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.ctc_align(torch.zeros(64), y, n, n, 1, 4, 5)
    with pytest.raises(ValueError):
        ops.ctc_emit_stats(torch.zeros(64), y, n, n, 1, 4, 5)
    with pytest.raises(ValueError, match="GPU"):
        ctc_align(torch.zeros(1, 4, 5), y, n, n)
