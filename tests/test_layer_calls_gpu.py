"""The layer-level C entries (ttmi_layer_fwd / ttmi_layer_bwd: one call per encoder layer and direction) against the two
sub-layer calls they replace (ttmi_attn_* + ttmi_ffn_*): the same kernels apart from the passes the sub-layer boundary forced apart, so
outputs and every gradient agree to f32 rounding - with dropout on (same seeds, same masks), with and without deferred weight gradients'
bf16 input copy handed from layer to layer."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _run(stack, x, cot, mask, seed):
    torch.manual_seed(seed)                                   # the sub-layer calls draw their dropout seeds from torch's CPU generator
    for p in stack.parameters():
        p.grad = None
    xx = x.clone().requires_grad_(True)
    y = stack(xx, mask) if mask is not None else stack(xx)
    (y * cot).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xx.grad.detach(), {n: p.grad.detach().clone() for n, p in stack.named_parameters()}


@pytest.mark.parametrize("B,L,drop", [(2, 500, 0.1), (3, 70, 0.0), (1, 129, 0.2)])
def test_layer_calls_equal_the_sub_layer_calls(B, L, drop, monkeypatch):
    import tt.transformer as TT
    from tt.encoder import BuildEncoder
    from tt.utils import AttrDict
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    cfg = AttrDict(dict(enc=dict(n_layer=3, d_model=512, n_head=8, d_head=64, d_inner=1024, max_input_length=64), dropout=drop))
    torch.manual_seed(11)
    stack = BuildEncoder(cfg).cuda().train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, L, 512, generator=g).cuda()
    cot = torch.randn(B, L, 512, generator=g).cuda()
    assert stack.layers[0].MultiHeadAttention.fused()                   # three layers: the bf16 copy of the residual stream is handed on twice
    y1, dx1, g1 = _run(stack, x, cot, None, 123)
    monkeypatch.setattr(TT, "_SUBLAYER_CALLS", True)
    assert not stack.layers[0].MultiHeadAttention.fused()
    y0, dx0, g0 = _run(stack, x, cot, None, 123)
    e_y, e_dx = rel_err(y1.cpu().numpy(), y0.cpu().numpy()), rel_err(dx1.cpu().numpy(), dx0.cpu().numpy())
    e_g = {n: rel_err(g1[n].cpu().numpy(), g0[n].cpu().numpy()) for n in g1}
    worst = max(e_g, key=e_g.get)
    print("layer calls vs sub-layer calls (B=%d L=%d dropout %.1f): out %.2e dx %.2e worst gradient %s %.2e" % (B, L, drop, e_y, e_dx, worst, e_g[worst]))
    # same bf16 operands everywhere; what differs is f32 summation order inside the fused LayerNorm passes (and f32 atomics in the weight gradients)
    assert e_y < 1e-6 and e_dx < 1e-6 and e_g[worst] < 1e-5          # measured: 0, 0 and 5e-7 (atomic order of the LayerNorm parameter sums)


_WIDTHS = [(64, 2, 32, 96), (136, 2, 32, 96), (256, 4, 64, 128), (264, 4, 64, 128), (392, 2, 64, 128)]      # d, H, Dh, Di


@pytest.mark.parametrize("d,H,Dh,Di,B,L,grid", [w + bl + (None,) for w in _WIDTHS for bl in ((3, 70), (4, 400))] + [(136, 2, 32, 96, 3, 70, 3)])
def test_layer_calls_equal_the_sub_layer_calls_at_every_width(d, H, Dh, Di, B, L, grid, monkeypatch):
    """the same comparison at the other widths of the LayerNorm kernels the layer-level entries alone reach (ln_bwd_pair_kernel, the in-pass second
    norm of ln_fwd_row_kernel): one 256-column chunk partly and wholly filled, a second chunk partly filled (264, 392); 1600 rows = more than one
    pass of the pair kernel's grid-stride loop, and that loop at 3 blocks (option 12: 18 passes over 210 rows).  tests/test_ffn_rows_gpu.py
    holds the sub-layer calls themselves to a float64 reference row by row."""
    import tt.transformer as TT
    from tt.encoder import BuildEncoder
    from tt.utils import AttrDict
    from ttmi import ops
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    cfg = AttrDict(dict(enc=dict(n_layer=2, d_model=d, n_head=H, d_head=Dh, d_inner=Di, max_input_length=64), dropout=0.1))
    torch.manual_seed(11)
    stack = BuildEncoder(cfg).cuda().train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, L, d, generator=g).cuda()
    cot = torch.randn(B, L, d, generator=g).cuda()
    try:
        if grid is not None:
            ops.set_option(12, grid)
        assert stack.layers[0].MultiHeadAttention.fused()
        y1, dx1, g1 = _run(stack, x, cot, None, 123)
        monkeypatch.setattr(TT, "_SUBLAYER_CALLS", True)
        assert not stack.layers[0].MultiHeadAttention.fused()
        y0, dx0, g0 = _run(stack, x, cot, None, 123)
    finally:
        ops.set_option(12, 384)                                       # csrc/rowops.hip LN_BWD_GRID
    e_y, e_dx = rel_err(y1.cpu().numpy(), y0.cpu().numpy()), rel_err(dx1.cpu().numpy(), dx0.cpu().numpy())
    e_g = {n: rel_err(g1[n].cpu().numpy(), g0[n].cpu().numpy()) for n in g1}
    worst = max(e_g, key=e_g.get)
    print("layer calls vs sub-layer calls (d=%d B=%d L=%d grid %s): out %.2e dx %.2e worst gradient %s %.2e" % (d, B, L, grid, e_y, e_dx, worst, e_g[worst]))
    assert e_y < 1e-6 and e_dx < 1e-6 and e_g[worst] < 1e-5
