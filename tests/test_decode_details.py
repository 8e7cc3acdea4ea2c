"""CPU-only side of decode details (DecodeResult, ttmi_greedy_scan_batch_lp, ttmi_greedy_advance_lp): the two entry points validate their
arguments without a GPU, the result type is importable, and details=True on CPU tensors is an error (this build has no CPU path)."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import PKG


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_lp_entry_points_reject_null_pointers_without_gpu():
    lib = _lib()
    L = ctypes.c_long
    rc = lib.ttmi_greedy_scan_batch_lp(None, 0, L(5), 1, 1, 5, 0, None, None, None, None, None, None)
    assert rc < 0 and b"greedy_scan_batch_lp" in lib.ttmi_last_error() and b"null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_greedy_advance_lp(None, 1, 1, 1, None, L(4), None, None, None, None, None, None, None, None, None, L(4), None, None)
    assert rc < 0 and b"greedy_advance_lp" in lib.ttmi_last_error() and b"null pointer" in lib.ttmi_last_error()
    # sizes are checked too: all pointers set (never dereferenced: the call fails before any launch), n = 0 / ld < V / ld_det = 0
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ttmi_greedy_scan_batch_lp(p, 0, L(5), 1, 0, 5, 0, p, p, p, p, p, None) < 0
    assert lib.ttmi_greedy_scan_batch_lp(p, 0, L(4), 1, 1, 5, 0, p, p, p, p, p, None) < 0
    assert b"bad arguments" in lib.ttmi_last_error()
    assert lib.ttmi_greedy_advance_lp(p, 1, 1, 1, p, L(4), p, p, p, p, p, p, p, p, p, L(0), p, None) < 0
    assert lib.ttmi_greedy_advance_lp(p, 1, 1, 4, p, L(4), p, p, p, p, p, p, p, p, p, L(4), p, None) < 0      # n_hist == ld_hist


def test_decode_result_type():
    from tt.model import DecodeResult
    r = DecodeResult([3, 4], [0, 7], [-0.5, -0.25], -9.0)
    assert r.tokens == [3, 4] and r.frames == [0, 7] and r.logprobs == [-0.5, -0.25] and r.score == -9.0
    assert DecodeResult._fields == ("tokens", "frames", "logprobs", "score")
    assert "lattice" in DecodeResult.__doc__               # the score's meaning is documented on the type


def _tiny_cpu_model():
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    torch.manual_seed(0)
    return Transducer(cfg).eval()


def test_details_on_cpu_tensors_is_an_error():
    from ttmi.streaming import StreamingRecognizer
    model = _tiny_cpu_model()
    enc = torch.zeros(2, 6, 64)
    with pytest.raises(ValueError):
        model.decode_batch(enc, [6, 4], details=True)
    with pytest.raises(ValueError):
        model.decode(enc[0], 6, details=True)
    with pytest.raises(ValueError):
        model.recognize(torch.zeros(2, 6, 64), torch.tensor([6, 4]), details=True)
    with pytest.raises(ValueError):
        StreamingRecognizer(model, left_context=2, right_context=1, details=True)
