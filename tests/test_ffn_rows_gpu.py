"""ttmi_ffn_fwd / ttmi_ffn_bwd row by row against the reference of tests/ffn_oracle.py fed the exact dropout masks the kernels drew, at
every width route of the LayerNorm launchers (csrc/rowops.hip: one-chunk and two-chunk row kernels with full and partly filled chunks,
the general three-pass / two-launch kernels at d > 512 and d % 4 != 0), over more rows than one pass of the grid-stride backward kernels
covers, and with their grid cut to 3 blocks (option 12).  Every row of z and dy and every row / element of the six gradients is held
to the bound of its precision: one wrong row among 1541 fails here and moves a whole-tensor norm by 2.5e-2.

Worst row or element measured over the cases (bound): prec 0 6.9e-6 (1e-4), prec 2 2.4e-5 (1e-4), prec 1 on the bf16 pipeline 1.7e-3
(TOL_MAX 8.4e-3; worst 90 % quantile 3.0e-4 against TOL_Q90 1.0e-3), prec 1 off it ("operands") 3.0e-4 (TOL_MAX)."""
import ctypes
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

import ffn_oracle as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
LN_BWD_GRID = 384           # csrc/rowops.hip LN_BWD_GRID, the default of option 12


def _p(t):
    return c_void_p(t.data_ptr())


def _ffn(case, c, seed):
    """forward + backward through the C ABI -> (dict of OUTPUTS as float64 numpy, sentinel rows of z and dy)"""
    from ttmi import check, lib
    L_ = lib()
    L_.ttmi_ffn_ctx_floats.restype = ctypes.c_size_t
    L_.ttmi_ffn_ws_floats.restype = ctypes.c_size_t
    rows, d, Di = c.rows, c.d, c.Di
    dev = torch.device("cuda")
    t = {k: case[k].to(torch.float32).to(dev).contiguous() for k in ("y", "dz", "w1", "b1", "w2", "b2", "ln_g", "ln_b")}
    dims = (c_long(rows), c_int(d), c_int(Di), c_int(c.prec))
    ctx = torch.empty(int(L_.ttmi_ffn_ctx_floats(*dims)), dtype=torch.float32, device=dev)
    ws = torch.empty(int(L_.ttmi_ffn_ws_floats(*dims)), dtype=torch.float32, device=dev)
    z = torch.full((rows + 1, d), SENTINEL, dtype=torch.float32, device=dev)
    dy = torch.full((rows + 1, d), SENTINEL, dtype=torch.float32, device=dev)
    g = {k: torch.ones_like(t[k]) for k in ("w1", "b1", "w2", "b2", "ln_g", "ln_b")}  # the ABI accumulates into the gradient buffers
    drop = (c_float(c.p), c_float(c.p), ctypes.c_uint(seed))
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    check(L_.ttmi_ffn_fwd(_p(t["y"]), _p(t["w1"]), _p(t["b1"]), _p(t["w2"]), _p(t["b2"]), _p(t["ln_g"]), _p(t["ln_b"]), *dims, *drop,
                          _p(ctx), _p(ws), _p(z), stream), "ttmi_ffn_fwd")
    check(L_.ttmi_ffn_bwd(_p(t["dz"]), _p(t["y"]), _p(t["w1"]), _p(t["w2"]), _p(t["ln_g"]), *dims, *drop, _p(ctx), _p(ws), _p(dy),
                          _p(g["w1"]), _p(g["b1"]), _p(g["w2"]), _p(g["b2"]), _p(g["ln_g"]), _p(g["ln_b"]), stream), "ttmi_ffn_bwd")
    torch.cuda.synchronize()
    out = dict(z=z[:rows], dy=dy[:rows])
    out.update({"g_" + k: v - 1.0 for k, v in g.items()})
    return {k: v.double().cpu().numpy() for k, v in out.items()}, (z[rows].cpu().numpy(), dy[rows].cpu().numpy())


def _masks(c, seed):
    from ttmi import ops
    if c.p <= 0:
        return None
    return tuple(ops.dropout_multipliers(n, c.p, seed ^ salt, "cuda").double().cpu()
                 for n, salt in ((c.rows * c.Di, 0xB2), (c.rows * c.d, 0xC3), (c.rows * c.d, 0xD4)))


_refs = {}


def _reference(c, seed):
    """one float64 reference per (shape, rounding form): prec 0 and prec 2 share the exact one"""
    key = (c.rows, c.d, c.Di, c.p, R.rounding_of(c))
    if key not in _refs:
        _refs.clear()                                            # cases of a shape are adjacent: keep one
        case = R.cached_case(c.rows, c.d, c.Di, c.p)
        _refs[key] = {k: v.numpy() for k, v in R.ffn_ref(case, _masks(c, seed), R.rounding_of(c)).items()}
    return _refs[key]


@pytest.mark.parametrize("c", sorted(R.CASES, key=lambda c: (c.rows, c.d, c.Di, c.p, R.rounding_of(c) or "")), ids=R.case_id)
def test_ffn_rows(c):
    from ttmi import ops
    seed = R.case_seed(c)
    case = R.cached_case(c.rows, c.d, c.Di, c.p)
    try:
        if c.grid is not None:
            ops.set_option(12, c.grid)
        got, (z_end, dy_end) = _ffn(case, c, seed)
    finally:
        ops.set_option(12, LN_BWD_GRID)
    want = _reference(c, seed)
    tol_max, tol_q90 = R.tolerances(c)
    e = R.errors(got, want)
    print("%s (%s): " % (R.case_id(c), R.rounding_of(c)) + "  ".join("%s %.1e/%.1e" % (k, *e[k]) for k in R.OUTPUTS))
    assert (z_end == SENTINEL).all() and (dy_end == SENTINEL).all(), "a row past the last one was written"
    for k in R.OUTPUTS:
        assert e[k][0] < tol_max, (k, "worst row", e[k][0], tol_max)
        if tol_q90 is not None:
            assert e[k][1] < tol_q90, (k, "90 % quantile", e[k][1], tol_q90)
