"""The FFN row reference of tests/ffn_oracle.py checks itself on the CPU: against float64 autograd of the module's formula, its inputs'
precondition at every GPU case, its comparator against the failures a whole-tensor norm lets through, and its tolerances against the
float32-to-float64 distance of the reference they are derived from."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ffn_oracle as R
from conftest import rel_err


@pytest.mark.parametrize("rows,d,Di", [(5, 8, 24), (67, 37, 20), (130, 264, 40)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_reference_equals_autograd_of_the_module_formula(rows, d, Di, p):
    """tt/transformer.py PositionwiseFF (one LayerNorm used twice: its gamma / beta gradients add) and the layer's dropout on its output"""
    case = R.ffn_case(rows, d, Di, p, 1234 + rows)
    masks = R.cpu_masks(case)
    got = R.ffn_ref(case, masks, None)
    t = {k: case[k].clone().requires_grad_(True) for k in ("y", "w1", "b1", "w2", "b2", "ln_g", "ln_b")}
    m_in, m_out, m_layer = masks if masks is not None else (1.0, 1.0, 1.0)
    h = F.layer_norm(t["y"], (d,), t["ln_g"], t["ln_b"], R.EPS)
    f = F.linear(torch.relu(F.linear(h, t["w1"], t["b1"])) * m_in, t["w2"], t["b2"]) * m_out
    z = F.layer_norm(t["y"] + f, (d,), t["ln_g"], t["ln_b"], R.EPS) * m_layer
    (z * case["dz"]).sum().backward()
    want = dict(z=z.detach(), dy=t["y"].grad, g_w1=t["w1"].grad, g_b1=t["b1"].grad, g_w2=t["w2"].grad, g_b2=t["b2"].grad,
                g_ln_g=t["ln_g"].grad, g_ln_b=t["ln_b"].grad)
    for k, (e_max, _) in R.errors(got, want).items():
        assert e_max < 1e-10, (k, e_max)


def test_every_gpu_case_meets_the_precondition():
    shapes = sorted({(c.rows, c.d, c.Di, c.p) for c in R.CASES})
    assert len(R.CASES) == len(set(R.CASES)) and len(shapes) >= 30
    for s in shapes:
        case = R.ffn_case(*s, R.case_seed(R.Case(*s[:3], 0, s[3], None)))        # asserts min |pre-activation| >= MIN_PRE itself
        assert case["min_pre"] >= R.MIN_PRE, (s, case["min_pre"])


def test_rounding_forms_round():
    """the two bf16 forms differ from the exact one by bf16-sized amounts - neither equal to it nor off by more than a rounding explains"""
    case = R.cached_case(1541, 136, 24, 0.1)
    masks = R.cpu_masks(case)
    exact = R.ffn_ref(case, masks, None)
    for rounding in ("fast", "operands"):
        e = R.errors(R.ffn_ref(case, masks, rounding), exact)
        worst = max(v[0] for v in e.values())
        assert 2.0 ** -12 < worst < 2.0 ** -4, (rounding, e)


def _corruptions(case, masks, want):
    cache = {}
    R.ffn_ref(case, masks, None, cache=cache)
    rows, d = case["rows"], case["d"]
    r = 700
    z = want["z"].clone()
    z[r] = z[r + 1]
    yield "one row of z replaced by its neighbour", "z", z
    m_layer = masks[2]
    dzm = case["dz"] * m_layer
    xh2 = (cache["s"] - cache["mean2"]) * cache["rstd2"]
    xh1 = (case["y"] - cache["mean1"]) * cache["rstd1"]
    yield "one row's contribution left out of g_ln_g", "g_ln_g", want["g_ln_g"] - (dzm[r] * xh2[r] + cache["dh"][r] * xh1[r])
    dy = want["dy"].clone()
    last = rows - 1
    dy[last] = R.ln_bwd_rows(cache["dh"][last:], case["y"][last:], cache["mean1"][last - 1:last], cache["rstd1"][last - 1:last], case["ln_g"])[0] + cache["dres"][last]
    yield "dy of the last row from the previous row's mean / rstd", "dy", dy
    dy = want["dy"].clone()
    dy[r, d - 4:] = 0
    yield "the last 4 columns of one row of dy zeroed", "dy", dy


def test_comparator_sees_what_a_whole_tensor_norm_lets_through():
    """the failures of a wave-per-row kernel - a wrong prefetched row, a column sum that misses a row, another row's statistics, a masked
    chunk that leaks - each fail the row-wise assertion of tests/test_ffn_rows_gpu.py at its LOOSEST bound and pass the suite's usual
    whole-tensor norm at 6e-2"""
    case = R.cached_case(1541, 136, 24, 0.1)
    masks = R.cpu_masks(case)
    want = R.ffn_ref(case, masks, None)
    loosest = max(R.TOL_MAX, R.TOL_EXACT)
    n = 0
    for what, key, bad in _corruptions(case, masks, want):
        assert not torch.equal(bad, want[key]), what
        e = R.rowwise_err(bad.numpy(), want[key].numpy())
        print("%s: worst row %.2e (bound %.2e)" % (what, e.max(), loosest))
        assert e.max() > loosest, (what, e.max())
        assert rel_err(bad.numpy(), want[key].numpy()) < 6e-2, what
        assert float(np.quantile(e, 0.9)) == 0.0 or key == "g_ln_g", what       # (and only the rows it touched)
        n += 1
    assert n == 4


def test_tolerances_are_tied_to_the_reference():
    """TOL_MAX and TOL_Q90 are 4 x the worst distance between the float32 and the float64 run of the reference over every prec-1 case (both
    bf16 forms): re-measured here, so that neither constant can drift from the reference it bounds."""
    gaps = R.reference_gaps()
    assert set(gaps) == {c for c in R.CASES if c.prec == 1}                   # no case excluded
    g_max, g_q90 = R.gap_summary(gaps)
    print("reference float32 vs float64: G_max %.3e G_q90 %.3e (TOL_MAX %.3e TOL_Q90 %.3e)" % (g_max, g_q90, R.TOL_MAX, R.TOL_Q90))
    assert 2 * g_max <= R.TOL_MAX <= 8 * g_max, (g_max, R.TOL_MAX)
    assert R.TOL_Q90 == 1e-5 or 2 * g_q90 <= R.TOL_Q90 <= 8 * g_q90, (g_q90, R.TOL_Q90)
    assert R.TOL_Q90 >= 1e-5
    assert R.TOL_MAX <= 1e-2                                                  # larger: a rounding point is missing from the reference
    assert R.TOL_EXACT == 1e-4
