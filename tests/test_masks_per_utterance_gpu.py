"""Attention masks that differ per utterance (mask_sb != 0): byte masks [B, L, L] (kind 3), per-utterance interval tables [B, L, 2]
(kind 4) and the reference's 2-D (klen, bsz) key mask (kind 3 with mask_si = 0), through one encoder layer against the float64 oracle,
against the same utterances run one at a time with their mask as a shared table (mask_sb = 0, the path every other test pins), kind 4
against kind 3, under the measurement switches, and with the attention backward cut into batch slices (ttmi_set_option(10, n)).  The
masks come from tests/mask_cases.py, which tests/test_oracle_masks.py pins on the CPU together with the oracle's handling of them."""
import numpy as np
import pytest
import torch

import mask_cases as MC
from conftest import rel_err
from oracle import tt_oracle as O

pytestmark = pytest.mark.gpu

NAMES = {v: k for k, v in O._LAYER_KEYS.items()}
_oracle_cache = {}


def _run(layer, x, cot, mask):
    layer.zero_grad()
    xg = x.clone().requires_grad_(True)
    y = layer.forward_bm(xg, mask)
    (y * cot).sum().backward()
    return y.detach(), xg.grad.clone(), {n: p.grad.clone() for n, p in layer.named_parameters()}


def _case(Dh, H, L, K, B, family, Di=64):
    """layer, x, cot (device), the mask in the reference's form (numpy, None for the parametric kinds) and the float64 oracle's
    (y, dx, gradients), computed once per case and shared by every test and precision that uses it"""
    from tt.encoder import BaseEncoder
    d = H * Dh
    torch.manual_seed(L + Dh)
    layer = BaseEncoder(k_len=K, n_head=H, d_model=d, d_head=Dh, d_inner=Di, dropout=0.0).cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, d, generator=g)
    cot = torch.randn(B, L, d, generator=g)
    if family == "none":
        m = None
    elif family == "band":
        m = O.context_mask(L, 20, 3)[:, :, None]
    else:
        m, _ = MC.build(family, L, B)
        assert MC.every_row_keeps_a_key(m, B, L)
    key = (Dh, H, L, K, B, family, Di)
    if key not in _oracle_cache:
        sd = {"encoder.layers.0." + k: v.detach().cpu().numpy().astype(np.float64) for k, v in layer.state_dict().items()}
        prm = O.layer_params(sd, "encoder.", 0)
        want, cache = O.layer_fwd(x.numpy().astype(np.float64), prm, m)
        dxo, go = O.layer_bwd(cot.numpy().astype(np.float64), cache, prm)
        assert np.isfinite(want).all() and np.isfinite(dxo).all()
        _oracle_cache[key] = (want, dxo, {n: go[NAMES[n]] for n, _ in layer.named_parameters()})
    return layer, x.cuda(), cot.cuda(), m, _oracle_cache[key]


def _spec(m, B, L):
    from tt.transformer import as_mask_spec
    return as_mask_spec(torch.tensor(m).cuda(), B, L)


def _sb_si(spec):
    a = spec.args()
    return a[4].value, a[5].value


def _errors(y, dx, g, ref):
    """relative errors against the oracle: {'y', 'dx', every parameter name}"""
    want, dxo, go = ref
    e = {"y": rel_err(y.cpu().numpy(), want), "dx": rel_err(dx.cpu().numpy(), dxo)}
    e.update({n: rel_err(g[n].cpu().numpy(), go[n]) for n in g})
    return e


def _check_spec(spec, family, m, B, L):
    """what as_mask_spec makes of each family: the per-utterance forms of the sub-layer ABI"""
    sb, si = _sb_si(spec)
    if family == "keypad":
        assert spec.kind == 3 and spec.tensor.shape == (B, 1, L) and si == 0 and sb != 0
    elif family == "holes":
        assert spec.kind == 3 and spec.tensor.shape == (B, L, L) and sb == L * L and si == L
    else:
        lo, hi, interval = MC.row_intervals(m, B, L)
        assert interval and spec.kind == 4 and spec.tensor.shape == (B, L, 2) and sb == 2 * L
        assert (spec.left, spec.right) == MC.reach(lo, hi)
        assert np.array_equal(spec.tensor.cpu().numpy(), np.stack([lo, hi], -1))
        assert not torch.equal(spec.tensor[0], spec.tensor[1])                     # a table per utterance
        if family == "causal_pad":
            assert (spec.left, spec.right) == (L - 1, 0)


SMALL = [(32, 4, 33, 64, 2), (64, 2, 129, 16, 3), (64, 2, 500, 410, 3), (32, 2, 500, 512, 2)]        # Dh, H, L, K, B: L <= K and L > K
LARGE = [(64, 1, 600, 64, 2), (64, 2, 1100, 410, 3)]                  # L > 512: the column-group form of attn_dqde_kernel
CASES = [s + (f, p) for p in ("bf16", "fp32", "bf16x3") for s in (SMALL if p == "bf16" else SMALL[:3]) for f in MC.FAMILIES] + \
        [s + (f, "bf16") for s in LARGE for f in MC.FAMILIES]
# the floor under the "no worse than one utterance at a time" comparison: bf16 from test_one_pass_position_gradients_vs_the_gemm_launches;
# the f32-flow modes: see the docstring below
FLOOR = {"bf16": 5e-3, "fp32": 2e-6, "bf16x3": 1e-5}


@pytest.mark.parametrize("Dh,H,L,K,B,family,prec", CASES)
def test_per_utterance_masks_vs_oracle_and_vs_one_utterance_at_a_time(Dh, H, L, K, B, family, prec, monkeypatch):
    """1. against the float64 oracle: output, dx and every parameter gradient, padded rows included, with the bounds the project uses for
    these quantities (bf16: 3e-2 / 8e-2 of test_flash_gpu.py; fp32 and bf16x3: 1e-4, TOL of test_rnnt_gpu.py / test_configs_gpu.py).
    2. against every utterance run alone (B = 1) with its own mask as a shared table: y_b and dx_b of the batched run against the single
    run, the batched parameter gradients against the sum over the single runs - two runs of one pipeline whose GEMMs (chosen by B * L)
    sum in another order, so bf16: the bounds test_position_term_inside_the_kernels_vs_the_slab_design uses for such a pair (5e-3 / 2e-2 /
    4e-2), f32 flow: 1e-4 - and the batched run's error against the oracle is at most max(1.3 x the single runs' error, floor).  Floor:
    bf16 5e-3 (test_one_pass_position_gradients_vs_the_gemm_launches); fp32 2e-6 and bf16x3 1e-5: the largest error of the SINGLE runs
    against the oracle over all cases of this test, rounded up (measured on an MI355X, this file's first run: fp32 y 8.6e-8, dx 1.3e-7,
    gradients 1.0e-6; bf16x3 y 8.6e-8, dx 9.7e-7, gradients 6.1e-6; the batched runs: fp32 1.2e-6, bf16x3 6.1e-6.  In bf16 the batched y
    and dx came out bit-identical to the single runs, gradients within 8.9e-7).  A kernel that reads utterance 0's mask for utterance 1 is
    off by O(1): the lengths differ by more than a tile."""
    monkeypatch.setenv("TTMI_PRECISION", prec)
    layer, x, cot, m, ref = _case(Dh, H, L, K, B, family)
    spec = _spec(m, B, L)
    _check_spec(spec, family, m, B, L)
    y, dx, g = _run(layer, x, cot, spec)
    e_b = _errors(y, dx, g, ref)
    ys, dxs, gs = [], [], None
    for b in range(B):
        sb = _spec(MC.single(m, b), 1, L)
        assert _sb_si(sb)[0] == 0 and sb.tensor.shape[0] == 1
        y1, dx1, g1 = _run(layer, x[b:b + 1].contiguous(), cot[b:b + 1].contiguous(), sb)
        ys.append(y1); dxs.append(dx1)
        gs = g1 if gs is None else {n: gs[n] + g1[n] for n in g1}
    ys, dxs = torch.cat(ys), torch.cat(dxs)
    e_s = _errors(ys, dxs, gs, ref)
    e_d = {"y": max(rel_err(y[b].cpu().numpy(), ys[b].cpu().numpy()) for b in range(B)),
           "dx": max(rel_err(dx[b].cpu().numpy(), dxs[b].cpu().numpy()) for b in range(B))}
    e_d.update({n: rel_err(g[n].cpu().numpy(), gs[n].cpu().numpy()) for n in g})
    worst = max((n for n in e_b if n not in ("y", "dx")), key=lambda n: e_b[n])
    print("%s %s L=%d B=%d | batched vs oracle: y %.2e dx %.2e grads %.2e (%s) | single: y %.2e dx %.2e grads %.2e | batched vs single: y %.2e dx %.2e grads %.2e"
          % (prec, family, L, B, e_b["y"], e_b["dx"], e_b[worst], worst, e_s["y"], e_s["dx"], max(v for n, v in e_s.items() if n not in ("y", "dx")),
             e_d["y"], e_d["dx"], max(v for n, v in e_d.items() if n not in ("y", "dx"))))
    bf = prec == "bf16"
    for n in e_b:
        bound = (3e-2 if n == "y" else 8e-2) if bf else 1e-4
        direct = (5e-3 if n == "y" else 2e-2 if n == "dx" else 4e-2) if bf else 1e-4
        assert e_b[n] < bound, ("oracle", n, e_b[n])
        assert e_d[n] < direct, ("batched vs single", n, e_d[n])
        assert e_b[n] <= max(1.3 * e_s[n], FLOOR[prec]), ("worse than one utterance at a time", n, e_b[n], e_s[n])


@pytest.mark.parametrize("family", MC.INTERVAL_FAMILIES)
@pytest.mark.parametrize("L", [500, 1100])
def test_interval_tables_per_utterance_equal_byte_masks_bit_for_bit(L, family, monkeypatch):
    """the contract of test_masked_tile_skipping_changes_nothing with tables that differ per utterance: tile skipping in the forward and
    the backward's skip window are decided from other rows for every b, skipped tiles contribute exact zeros, so y and dx under the
    per-utterance interval table (kind 4) equal those under the same mask as [B, L, L] bytes (kind 3, nothing skipped) bit for bit;
    parameter gradients are f32 atomic sums: 1e-5"""
    from ttmi.ops import MaskSpec
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    Dh, H, K, B = 64, 2, 64, 3
    layer, x, cot, m, ref = _case(Dh, H, L, K, B, family)
    spec = _spec(m, B, L)
    _check_spec(spec, family, m, B, L)
    y, dx, g = _run(layer, x, cot, spec)
    bytes3 = MaskSpec(3, tensor=torch.tensor(MC.per_row(m, B, L).astype(np.uint8)).cuda().contiguous())
    assert _sb_si(bytes3) == (L * L, L)
    y3, dx3, g3 = _run(layer, x, cot, bytes3)
    assert torch.equal(y, y3) and torch.equal(dx, dx3)
    for n in g:
        assert rel_err(g[n].cpu().numpy(), g3[n].cpu().numpy()) < 1e-5, n
    e = _errors(y, dx, g, ref)
    assert e["y"] < 3e-2 and max(v for n, v in e.items() if n != "y") < 8e-2


SWITCH_SHAPES = [(64, 2, 500, 410, 3, "chunk_pad"), (64, 2, 129, 16, 3, "keypad"), (64, 2, 300, 64, 2, "holes")]
SWITCH_CASES = [(sw,) + s for sw in ("tiled_forward", "unfused", "slab", "gemm_position_gradients") for s in SWITCH_SHAPES] + \
               [("gemm_position_gradients", 64, 1, 600, 64, 2, "causal_pad")]          # L > 512: the column groups against the GEMM launches


@pytest.mark.parametrize("switch,Dh,H,L,K,B,family", SWITCH_CASES)
def test_measurement_switches_agree_under_per_utterance_masks(switch, Dh, H, L, K, B, family, monkeypatch):
    """the A/B switches of test_flash_gpu.py, each with that file's tolerances, under masks that differ per utterance: option 14 = 0
    (tiled forward) bit-identical to the resident forward; option 0 = 1 (unfused chain): the fused kernels as accurate as the chain;
    option 8 = 0 (slab design) and option 11 = 1 (GEMM position gradients) within bf16 rounding of the default and equally far from the oracle"""
    from ttmi import ops
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    layer, x, cot, m, ref = _case(Dh, H, L, K, B, family)
    spec = _spec(m, B, L)
    _check_spec(spec, family, m, B, L)
    key, value, default = {"tiled_forward": (14, 0, 1), "unfused": (0, 1, 0), "slab": (8, 0, 1), "gemm_position_gradients": (11, 1, 0)}[switch]
    y1, dx1, g1 = _run(layer, x, cot, spec)
    try:
        ops.set_option(key, value)
        y0, dx0, g0 = _run(layer, x, cot, spec)
    finally:
        ops.set_option(key, default)
    e1, e0 = _errors(y1, dx1, g1, ref), _errors(y0, dx0, g0, ref)
    e10 = {n: rel_err(g1[n].cpu().numpy(), g0[n].cpu().numpy()) for n in g1}
    e_y, e_dx = rel_err(y1.cpu().numpy(), y0.cpu().numpy()), rel_err(dx1.cpu().numpy(), dx0.cpu().numpy())
    print("%s %s L=%d: default vs switch y %.2e dx %.2e grads %.2e" % (switch, family, L, e_y, e_dx, max(e10.values())))
    grads = lambda e: max(v for n, v in e.items() if n != "y")                                   # dx and the parameter gradients
    if switch == "tiled_forward":
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and max(e10.values()) < 1e-5
        assert e1["y"] < 3e-2
    elif switch == "unfused":
        assert e1["y"] < 3e-2 and grads(e1) < 8e-2
        assert e1["y"] < 2.5 * e0["y"] + 1e-3 and grads(e1) < 2.5 * grads(e0) + 1e-3
    elif switch == "slab":
        assert e_y < 5e-3 and e_dx < 2e-2 and max(e10.values()) < 4e-2
        assert e1["y"] < 3e-2 and grads(e1) < 8e-2
    else:
        assert torch.equal(y1, y0) and e_dx < 1e-2
        assert e1["dx"] < max(1.3 * e0["dx"], 5e-3)
        for n in g1:
            assert e10[n] < 1e-2 and e1[n] < max(1.3 * e0[n], 5e-3), (n, e10[n], e1[n], e0[n])


# --------------------------------------------------------------------------------------------------- batch slices of the attention backward
@pytest.mark.parametrize("B,L,K,family,gemm_launches", [
    (3, 129, 16, "none", 0), (4, 129, 16, "band", 0), (3, 129, 16, "keypad", 0), (4, 129, 16, "chunk_pad", 0), (4, 129, 16, "holes", 1),
    (3, 129, 16, "causal_pad", 1), (3, 600, 64, "none", 0), (4, 600, 64, "band", 1), (3, 600, 64, "holes", 0), (4, 600, 64, "causal_pad", 0),
    (4, 600, 64, "keypad", 0), (3, 600, 64, "chunk_pad", 1)])
def test_sliced_attention_backward_equals_the_unsliced_one(B, L, K, family, gemm_launches, monkeypatch):
    """ttmi_set_option(10, n), n in {2, 3, B + 1} with B = 3 and 4 (a ragged last slice, and more slices than utterances): the backward
    kernel and the position-gradient pass run per batch slice on the same rows with the same operands - y identical, dx bit-identical to
    the unsliced run, parameter gradients within 1e-5 (their f32 atomic sums arrive in another order), everything inside the oracle bounds
    of test_flash_gpu.py.  No mask, the parametric band, and per-utterance byte masks and interval tables, whose base pointer the slice
    loop advances by hand; L = 129 and 600: both forms of attn_dqde_kernel; gemm_launches: option 11 = 1, the GEMMs inside the slice loop."""
    from ttmi import ops
    from ttmi.ops import MaskSpec
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    Dh, H = 64, 2
    layer, x, cot, m, ref = _case(Dh, H, L, K, B, family)
    if family == "none":
        spec = MaskSpec(0)
    elif family == "band":
        spec = MaskSpec(2, left=20, right=3)
    else:
        spec = _spec(m, B, L)
        _check_spec(spec, family, m, B, L)
    try:
        ops.set_option(11, gemm_launches)
        y0, dx0, g0 = _run(layer, x, cot, spec)
        e0 = _errors(y0, dx0, g0, ref)
        assert e0["y"] < 3e-2 and max(v for n, v in e0.items() if n != "y") < 8e-2
        for n_slices in (2, 3, B + 1):
            ops.set_option(10, n_slices)
            y1, dx1, g1 = _run(layer, x, cot, spec)
            ops.set_option(10, 1)
            e1 = _errors(y1, dx1, g1, ref)
            worst = max(rel_err(g1[n].cpu().numpy(), g0[n].cpu().numpy()) for n in g1)
            print("%s L=%d B=%d slices=%d: dx equal %s (%.2e), grads %.2e" % (family, L, B, n_slices, torch.equal(dx1, dx0),
                                                                           rel_err(dx1.cpu().numpy(), dx0.cpu().numpy()), worst))
            assert torch.equal(y1, y0), n_slices
            assert torch.equal(dx1, dx0), n_slices
            for n in g1:
                assert rel_err(g1[n].cpu().numpy(), g0[n].cpu().numpy()) < 1e-5, (n_slices, n)
            assert e1["y"] < 3e-2 and max(v for n, v in e1.items() if n != "y") < 8e-2, n_slices
    finally:
        ops.set_option(10, 1)
        ops.set_option(11, 0)
