"""ttmi_attn_fwd / ttmi_attn_bwd ROW BY ROW against the reference of tests/attn_oracle.py, the sub-layer alone through the C ABI: every
row of y and dx, every row of the two weight gradients, every row of the table gradient and every element of the four vectors is held to the
bound of its precision - not a whole-tensor norm, under which one wrong query row in 500 moves 4.5e-2.  Lengths at every tail of the 64-key
and 128-query tiles, across the 192 .. 512 window of the resident forward kernel and both column-group counts of attn_dqde_kernel, with
L % 8 != 0; every mask form of the ABI (causal, band, bytes, interval tables, per-utterance); both table branches (L <= K, L > K, L - K >=
256); head widths 64 and 32, the unfused bf16 chain and the f32 data flow of prec 1; the measurement switches one at a time; dropout.  y and
dx carry a sentinel row past the end, the gradient buffers arrive filled with 1.0 (the ABI accumulates), and the table rows no effective
position maps to must come back exactly 1.0.

Worst row or element measured over the cases (bound): prec 0 y 1.4e-6, dx 3.7e-6, weight rows 2.2e-6, table / bias elements 2.5e-5 (1e-4); prec 2
y 1.5e-5, dx 3.9e-5, weight rows 1.8e-5, table / bias elements 4.3e-5 (1e-4); prec 1 on the flash kernels ("fused"), `mixed`: y 4.2e-3 (1.5e-2),
dx 1.6e-2 (5.6e-2), weight rows 8.2e-3 (8.2e-2), tables 1.0e-1 (6.6e-1), 90 % quantiles 2.4e-3 / 5.1e-3 / 5.4e-3 / 1.1e-2 (1.0e-2 / 2.7e-2 / 3.9e-2 / 2.2e-1);
`planted`: y 4.5e-3 (1.5e-2), dx 3.0e-2 (1.3e-1), weight rows 1.9e-2 (8.2e-2), tables 1.2e-1 (1.1), 90 % quantiles 2.9e-3 / 1.4e-2 / 9.9e-3 / 5.2e-2
(1.1e-2 / 5.4e-2 / 4.9e-2 / 3.0e-1); "fast-unfused" y 1.4e-3, dx 4.4e-3, weight rows 2.5e-3, tables 6.9e-3; "operands" y 2.7e-3, dx 4.0e-3, weight rows
1.8e-3, tables 3.3e-3 (the bounds of `mixed`).  From 1536 rows on (B 3, L 513) the bf16x3 mode's errors are ten times those of the shorter stacks
(y 1.5e-5 against 1.1e-6): the three-term form of its dense products; DESIGN.md section 6."""
import ctypes
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import attn_oracle as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GRADS = ("qkv_w", "o_w", "ln_g", "ln_b", "r_emb", "r_w_bias", "r_bias")


def _p(t):
    return c_void_p(t.data_ptr())


def _mask_spec(spec):
    from ttmi.ops import MaskSpec
    kind, left, right, arr = spec
    if kind in (3, 4):
        return MaskSpec(kind, left=left, right=right, tensor=torch.from_numpy(arr).cuda().contiguous())
    return MaskSpec(kind, left=left, right=right)


def _attn(case, c, spec, seed):
    """forward + backward through the C ABI -> (dict of OUTPUTS as float64 numpy, gradients with the 1.0 they arrived with taken off; the
    sentinel rows of y and dx; the raw r_emb / r_bias gradient buffers)"""
    from ttmi import check, lib
    L_ = lib()
    L_.ttmi_attn_ctx_floats.restype = ctypes.c_size_t
    L_.ttmi_attn_ws_floats.restype = ctypes.c_size_t
    B, H, Dh, L, K = c.B, c.H, c.Dh, c.L, c.K
    d = H * Dh
    dev = torch.device("cuda")
    t = {k: case[k].to(torch.float32).to(dev).contiguous() for k in ("x", "dy") + GRADS}
    dims = (c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh))
    ctx = torch.empty(int(L_.ttmi_attn_ctx_floats(*dims, c_int(c.prec))), dtype=torch.float32, device=dev)
    ws = torch.empty(int(L_.ttmi_attn_ws_floats(*dims, c_int(c.prec))), dtype=torch.float32, device=dev)
    y = torch.full((B * L + 1, d), SENTINEL, dtype=torch.float32, device=dev)
    dx = torch.full((B * L + 1, d), SENTINEL, dtype=torch.float32, device=dev)
    g = {k: torch.ones_like(t[k]) for k in GRADS}                      # the ABI accumulates into the gradient buffers
    mask = _mask_spec(spec)
    tail = (c_int(c.prec), c_float(c.p), ctypes.c_uint(seed))
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    check(L_.ttmi_attn_fwd(_p(t["x"]), _p(t["qkv_w"]), _p(t["o_w"]), _p(t["ln_g"]), _p(t["ln_b"]), _p(t["r_emb"]), _p(t["r_w_bias"]), _p(t["r_bias"]),
                           *dims, c_int(K), *mask.args(), *tail, _p(ctx), _p(ws), _p(y), stream), "ttmi_attn_fwd")
    check(L_.ttmi_attn_bwd(_p(t["dy"]), _p(t["x"]), _p(t["qkv_w"]), _p(t["o_w"]), _p(t["ln_g"]), _p(t["r_emb"]), _p(t["r_w_bias"]), _p(t["r_bias"]),
                           *dims, c_int(K), *mask.args(), *tail, _p(ctx), _p(ws), _p(dx), _p(g["qkv_w"]), _p(g["o_w"]), _p(g["ln_g"]), _p(g["ln_b"]),
                           _p(g["r_emb"]), _p(g["r_w_bias"]), _p(g["r_bias"]), stream), "ttmi_attn_bwd")
    torch.cuda.synchronize()
    out = dict(y=y[:B * L], dx=dx[:B * L])
    out.update({"g_" + k: v - 1.0 for k, v in g.items()})
    out = {k: v.double().cpu().numpy() for k, v in out.items()}
    out["g_r_emb"] = out["g_r_emb"].reshape(K * H, Dh)
    out["g_r_w_bias"], out["g_r_bias"] = out["g_r_w_bias"].reshape(-1), out["g_r_bias"].reshape(-1)
    return out, (y[B * L].cpu().numpy(), dx[B * L].cpu().numpy()), (g["r_emb"].cpu().numpy(), g["r_bias"].cpu().numpy())


def _drop(c, seed):
    from ttmi import ops
    if c.p <= 0:
        return None
    return ops.dropout_multipliers(c.B * c.L * c.H * c.Dh, c.p, seed ^ 0xA1, "cuda").double().cpu()


_refs = {}


def _reference(c, case, m, seed):
    """one float64 reference per (inputs, mask, rounding form, dropout): prec 0 and prec 2 share the exact one, the switches' cases their form's"""
    key = (R.input_key(c), R.rounding_of(c), c.p)
    if key not in _refs:
        if len(_refs) >= 4:
            _refs.clear()                                            # cases of one key are adjacent
        _refs[key] = {k: v.numpy() for k, v in R.attn_ref(case, m, _drop(c, seed), R.rounding_of(c)).items()}
    return _refs[key]


@pytest.mark.parametrize("c", sorted(R.CASES, key=lambda c: (R.input_key(c), c.p, R.rounding_of(c) or "", c.prec, c.opt or ())), ids=R.case_id)
def test_attn_rows(c):
    from ttmi import ops
    seed = R.case_seed(c)
    case, m, spec = R.cached_case(*R.input_key(c))
    try:
        if c.opt is not None:
            ops.set_option(c.opt[0], c.opt[1])                       # (option 8 changes the ctx layout: set around a complete forward + backward)
        got, (y_end, dx_end), (raw_emb, raw_bias) = _attn(case, c, spec, seed)
    finally:
        if c.opt is not None:
            ops.set_option(c.opt[0], c.opt[2])
    want = _reference(c, case, m, seed)
    tol_max, tol_q90 = R.tolerances(c)
    e = R.errors(got, want)
    print("%s (%s): " % (R.case_id(c), R.rounding_of(c)) + "  ".join("%s %.1e/%.1e" % (k, *e[k]) for k in R.OUTPUTS))
    assert (y_end == SENTINEL).all() and (dx_end == SENTINEL).all(), "a row past the last one was written"
    n = R.unused_table_rows(c.L, c.K)
    assert (raw_emb[:n] == 1.0).all() and (raw_bias[:n] == 1.0).all(), "a table row that no effective position maps to was written"
    for k in R.OUTPUTS:
        cl = R.CLASS_OF[k]
        assert e[k][0] < tol_max[cl], (k, "worst row", e[k][0], tol_max[cl])
        if tol_q90 is not None:
            assert e[k][1] < tol_q90[cl], (k, "90 % quantile", e[k][1], tol_q90[cl])
