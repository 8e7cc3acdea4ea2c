"""CPU-only: the table of transducer lattices in ttmi.ops (ops.LATTICES, ops.lattice) and the helpers every lattice loss shares - the
size-valued library entries and the gradient-buffer rule - against the built library, without a GPU."""
import ctypes

import pytest
import torch

import ttmi
from ttmi import ops

ENTRIES = {"workspace", "loss_fwd", "loss_bwd", "align_workspace", "align", "emit_stats"}


def test_every_entry_is_an_exported_symbol_and_the_lattices_share_none():
    lib = ttmi.lib()
    assert set(ops.LATTICES) == set(ops.TOPOLOGIES) == {"rnnt", "monotonic"}
    for name, lat in ops.LATTICES.items():
        assert lat.name == name and set(lat.symbols) == ENTRIES
        for sym in lat.symbols.values():
            assert sym.startswith("ttmi_") and hasattr(lib, sym), sym
        assert len(set(lat.symbols.values())) == len(ENTRIES)
    r, m = ops.LATTICES["rnnt"], ops.LATTICES["monotonic"]
    assert not set(r.symbols.values()) & set(m.symbols.values())
    assert (r.takes_fastemit, r.has_exp_forms, r.label_takes_frame) == (True, True, False)
    assert (m.takes_fastemit, m.has_exp_forms, m.label_takes_frame) == (False, False, True)
    # the gradient entries the wrappers called before the table: the FastEmit form on the standard lattice, the plain one on the other
    assert r.symbols["loss_bwd"] == "ttmi_rnnt_loss_bwd_fe" and m.symbols["loss_bwd"] == "ttmi_mono_loss_bwd"


def test_a_records_entries_are_the_per_lattice_functions_of_the_module(monkeypatch):
    for prefix, lat in (("rnnt", ops.LATTICES["rnnt"]), ("mono", ops.LATTICES["monotonic"])):
        assert lat.prefix == prefix
        for entry in ("workspace", "loss_fwd", "loss_bwd", "align", "emit_stats"):
            assert getattr(lat, entry) is getattr(ops, "%s_%s" % (prefix, entry))
        with pytest.raises(AttributeError):
            lat.no_such_entry
    # looked up at call time: a wrapped ops.mono_align is what the record hands out
    marker = object()
    monkeypatch.setattr(ops, "mono_align", marker)
    assert ops.LATTICES["monotonic"].align is marker and ops.LATTICES["rnnt"].align is ops.rnnt_align
    assert ops.LATTICES["rnnt"].fastemit_kw(0.01) == {"fastemit_lambda": 0.01} and ops.LATTICES["monotonic"].fastemit_kw(0.0) == {}


def test_lattice_checks_what_check_topology_checks():
    assert ops.lattice("rnnt") is ops.LATTICES["rnnt"] and ops.lattice("rnnt", 0.01) is ops.LATTICES["rnnt"]
    assert ops.lattice("monotonic") is ops.LATTICES["monotonic"] and ops.lattice("monotonic", 0.0) is ops.LATTICES["monotonic"]
    with pytest.raises(ValueError) as e:
        ops.lattice("x")
    assert str(e.value) == "topology must be 'rnnt' or 'monotonic', got 'x'"
    with pytest.raises(ValueError) as e:
        ops.lattice("monotonic", 0.01)
    assert str(e.value) == "topology='monotonic' does not take fastemit_lambda > 0 (FastEmit is defined on the standard lattice here)"
    for args in (("x",), ("monotonic", 0.01)):
        with pytest.raises(ValueError) as e2:
            ops.check_topology(*args)
        with pytest.raises(ValueError) as e3:
            ops.lattice(*args)
        assert str(e2.value) == str(e3.value)


def test_size_helper_returns_the_pinned_workspace_sizes():
    """the values tests/test_mono_align_oracle.py::test_align_workspace_bytes pins on the raw entry"""
    def f(B, T, U1):
        return ops._sized("ttmi_mono_align_workspace_bytes", ctypes.c_int(B), ctypes.c_int(T), ctypes.c_int(U1))
    assert f(1, 1, 1) == 8 and f(8, 2000, 201) == 8 * 2000 * 4 * 8 and f(2, 10, 65) == 2 * 10 * 2 * 8
    assert f(0, 4, 3) == 0
    assert ttmi.lib().ttmi_mono_align_workspace_bytes.restype is ctypes.c_size_t
    # a lattice workspace past 2^31 bytes comes back whole (an int restype would wrap it)
    n = ops._sized("ttmi_rnnt_workspace_bytes", ctypes.c_int(64), ctypes.c_int(20000), ctypes.c_int(401))
    assert n >= 2 * 4 * 64 * 20000 * 401 > 2 ** 31


@pytest.mark.parametrize("shape", [(2, 3, 4, 5), (2, 3, 5)])
def test_gradient_buffer_rule(shape):
    V = shape[-1]
    dense = torch.zeros(shape)
    g, ld = ops.grad_buffer(dense)
    assert g.shape == dense.shape and g.dtype == dense.dtype and g.is_contiguous() and ld == V
    assert g.data_ptr() != dense.data_ptr() and not hasattr(g, "_ttmi_zero_pad")

    buf = torch.zeros(*shape[:-1], 8, dtype=torch.bfloat16)
    view = buf[..., :V]
    g, ld = ops.grad_buffer(view)
    assert g.shape == view.shape and g.dtype == view.dtype and ld == 8 and ops.row_pitch(g) == 8 and g.stride() == view.stride()
    assert g.data_ptr() != view.data_ptr() and g._ttmi_zero_pad == 8
    g, ld = ops.grad_buffer(view, zero_pad=False)                  # the CTC gradient: same buffer rule, no mark
    assert ops.row_pitch(g) == ld == 8 and not hasattr(g, "_ttmi_zero_pad")

    g, ld = ops.grad_buffer(view, inplace=True)
    assert g is view and ld == 8 and view._ttmi_zero_pad == 8
    g, ld = ops.grad_buffer(dense, inplace=True)
    assert g is dense and ld == V and not hasattr(dense, "_ttmi_zero_pad")
    view2 = buf[..., :V]
    g, ld = ops.grad_buffer(view2, inplace=True, zero_pad=False)
    assert g is view2 and not hasattr(view2, "_ttmi_zero_pad")
