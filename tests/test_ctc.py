"""CPU-only: the CTC entry points validate their arguments without a GPU, a config without `ctc_weight` builds the module it always built,
and the Python layer refuses CPU tensors (there is no CPU path)."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import PKG

c_long, c_float = ctypes.c_long, ctypes.c_float


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    lib.ttmi_ctc_workspace_bytes.restype = ctypes.c_size_t
    return lib


def test_argument_validation_without_gpu():
    lib = _lib()
    rc = lib.ttmi_ctc_loss_fwd(None, c_long(5), None, None, None, 1, 1, 1, 5, 0, None, None, None)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_loss_bwd(None, c_long(5), None, None, None, 1, 1, 1, 5, 0, None, None, 0, c_float(1.0), None, c_long(5), None)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_greedy(None, c_long(5), None, 1, 1, 5, 0, None, None, None)
    assert rc < 0 and b"null pointer" in lib.ttmi_last_error()
    # shape checks come after the pointer checks: hand over non-null (never dereferenced) addresses
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.ttmi_ctc_loss_fwd(p, c_long(5), p, p, p, 1, 1, 1024, 5, 0, p, p, None)
    assert rc < 0 and b"1023" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_loss_bwd(p, c_long(5), p, p, p, 1, 1, 1024, 5, 0, p, p, 0, c_float(1.0), p, c_long(5), None)
    assert rc < 0 and b"1023" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_loss_fwd(p, c_long(4), p, p, p, 1, 1, 1, 5, 0, p, p, None)          # pitch < V
    assert rc < 0 and b"pitch" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_loss_fwd(p, c_long(5), p, p, p, 1, 1, 1, 5, 5, p, p, None)          # blank outside [0, V)
    assert rc < 0 and b"blank" in lib.ttmi_last_error()
    rc = lib.ttmi_ctc_greedy(p, c_long(4), p, 1, 1, 5, 0, p, p, None)
    assert rc < 0


def test_workspace_size_holds_what_the_header_lists():
    lib = _lib()
    B, T, U = 3, 17, 5
    S = 2 * U + 1
    n = lib.ttmi_ctc_workspace_bytes(B, T, U)
    # emission table (f32) + alpha + beta (f64) per state, ll (f64) per utterance, log-sum-exp (f32) per frame
    assert n >= B * T * S * (4 + 8 + 8) + B * 8 + B * T * 4
    assert lib.ttmi_ctc_workspace_bytes(B, T, 0) > 0
    assert lib.ttmi_ctc_workspace_bytes(2 * B, T, U) > n


def _cfg(**extra):
    from tt.utils import AttrDict
    side = dict(n_layer=1, d_model=32, n_head=2, d_head=16, d_inner=48)
    return AttrDict(dict(enc=dict(side, max_input_length=8), dec=dict(side, max_target_length=4),
                         joint=dict(input_size=64, inner_size=24), vocab_size=11, dropout=0.0, **extra))


def test_config_without_ctc_weight_builds_the_same_module():
    from tt.model import Transducer
    keys = {}
    for name, extra in (("absent", {}), ("none", dict(ctc_weight=None)), ("zero", dict(ctc_weight=0)), ("on", dict(ctc_weight=0.3))):
        torch.manual_seed(0)
        keys[name] = list(Transducer(_cfg(**extra)).state_dict().keys())
    # today's list: the two encoders and the joint, nothing else
    assert all(k.split(".")[0] in ("encoder", "decoder", "joint") for k in keys["absent"])
    assert keys["absent"][-4:] == ["joint.forward_layer.weight", "joint.forward_layer.bias", "joint.project_layer.weight", "joint.project_layer.bias"]
    assert keys["none"] == keys["absent"] and keys["zero"] == keys["absent"]
    assert keys["on"] == keys["absent"] + ["ctc_head.weight", "ctc_head.bias"]
    m = Transducer(_cfg(ctc_weight=0.3))
    assert m.ctc_head.weight.shape == (11, 32) and not hasattr(Transducer(_cfg()), "ctc_head")
    with pytest.raises(ValueError):
        Transducer(_cfg(ctc_weight=-0.1))


def test_positive_weight_without_a_head_raises():
    from tt.model import Transducer
    m = Transducer(_cfg())
    x, y = torch.zeros(1, 6, 32), torch.ones(1, 2, dtype=torch.long)
    tl, ul = torch.tensor([6], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError, match="CTC head"):
        m.loss(x, tl, y, ul, ctc_weight=0.3)
    with pytest.raises(ValueError, match="CTC head"):
        m.ctc_loss(x, tl, y, ul)
    with pytest.raises(ValueError, match="CTC head"):
        m.recognize_ctc(x, tl)


def test_cpu_tensors_raise():
    from ttmi import ops
    from ttmi.ctc import CTCLoss, ctc_greedy_decode, ctc_loss
    from tt.model import Transducer
    x = torch.zeros(1, 4, 5)
    y = torch.ones(1, 2, dtype=torch.int32)
    tl, ul = torch.tensor([4], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.ctc_loss_fwd(x, y, tl, ul, 0, torch.zeros(64))
    with pytest.raises(ValueError):
        ops.ctc_loss_bwd(x, y, tl, ul, 0, torch.zeros(64), torch.ones(1), 1, 1.0)
    with pytest.raises(ValueError):
        ops.ctc_greedy(x, tl)
    with pytest.raises(ValueError):
        ctc_loss(x, y, tl, ul)
    with pytest.raises(ValueError):
        CTCLoss()(x, y, tl, ul)
    with pytest.raises(ValueError):
        ctc_greedy_decode(x, tl)
    with pytest.raises(ValueError):
        ctc_loss(x, y, tl, ul, reduction="batchmean")
    m = Transducer(_cfg(ctc_weight=0.3))
    with pytest.raises(ValueError):
        m.ctc_loss(torch.zeros(1, 6, 32), torch.tensor([6]), torch.ones(1, 2, dtype=torch.long), torch.tensor([2]))
    with pytest.raises(ValueError):
        m.recognize_ctc(torch.zeros(1, 6, 32))
