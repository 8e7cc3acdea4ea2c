"""The oracle under masks that differ per utterance, and the mask builders the GPU tests use (tests/mask_cases.py).  The golden fixtures
only hold masks shared by the batch; the oracle's (L, L, B) and (L, B) paths carry tests/test_masks_per_utterance_gpu.py, so they are
pinned here against the same functions run utterance by utterance with (L, L, 1) masks: no operation of a layer mixes batch elements."""
import numpy as np
import pytest

import mask_cases as MC
from oracle import tt_oracle as O

SHAPES = [(33, 2), (129, 3), (200, 4)]          # (L, B)


def _params(L, K, H, D, Di, seed):
    rng = np.random.default_rng(seed)
    d = H * D
    return dict(qkv_w=rng.standard_normal((3 * d, d)) / np.sqrt(d), o_w=rng.standard_normal((d, d)) / np.sqrt(d),
                ln_g=1 + 0.1 * rng.standard_normal(d), ln_b=0.1 * rng.standard_normal(d), r_emb=rng.standard_normal((K, H, D)),
                r_w_bias=rng.standard_normal((H, D)), r_bias=rng.standard_normal((K, H)),
                ff_w1=rng.standard_normal((Di, d)) / np.sqrt(d), ff_b1=0.1 * rng.standard_normal(Di),
                ff_w2=rng.standard_normal((d, Di)) / np.sqrt(Di), ff_b2=0.1 * rng.standard_normal(d),
                ff_ln_g=1 + 0.1 * rng.standard_normal(d), ff_ln_b=0.1 * rng.standard_normal(d))


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("L,B", SHAPES)
def test_builders_keep_a_key_per_row_and_the_interval_property(family, L, B):
    m, lens = MC.build(family, L, B)
    assert lens[0] == L and min(lens) in (1, 2) and len(lens) == B
    assert m.shape == ((L, B) if family == "keypad" else (L, L, B)) and m.dtype == bool
    assert MC.every_row_keeps_a_key(m, B, L)
    lo, hi, interval = MC.row_intervals(m, B, L)
    assert interval == (family != "holes")
    full = MC.per_row(m, B, L)
    assert not np.array_equal(full[0], full[1])                       # the tables differ per utterance
    i = np.arange(L)
    for b, n in enumerate(lens):
        if family == "keypad":
            assert (lo[b] == 0).all() and (hi[b] == n - 1).all()
        elif family == "causal_pad":
            assert (lo[b] == 0).all() and (hi[b] == np.minimum(i, n - 1)).all()
        elif family == "chunk_pad":
            base_lo = np.maximum((i // MC.CHUNK) * MC.CHUNK - MC.LEFT, 0)
            base_hi = np.minimum((i // MC.CHUNK + 1) * MC.CHUNK - 1, L - 1)
            assert (lo[b] == base_lo).all() and (hi[b] == np.where(i < n, np.minimum(base_hi, n - 1), base_hi)).all()
        else:
            assert not full[b][i, i].any()
    if family == "causal_pad":
        assert MC.reach(lo, hi) == (L - 1, 0)
    if family == "chunk_pad":
        assert MC.reach(lo, hi) == (min(MC.LEFT + MC.CHUNK - 1, L - 1), min(MC.CHUNK - 1, L - 1))


def test_single_utterance_view_of_a_mask():
    m, _ = MC.build("chunk_pad", 40, 3)
    assert np.array_equal(MC.per_row(MC.single(m, 2), 1, 40)[0], MC.per_row(m, 3, 40)[2])
    k, _ = MC.build("keypad", 40, 3)
    assert MC.single(k, 1).shape == (40, 1) and np.array_equal(MC.per_row(MC.single(k, 1), 1, 40)[0], MC.per_row(k, 3, 40)[1])


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("L,B,K", [(33, 2, 64), (70, 3, 16)])
def test_oracle_per_utterance_masks_equal_one_utterance_at_a_time(family, L, B, K):
    """rel_attn_fwd, layer_fwd and layer_bwd with an (L, L, B) / (L, B) mask against the same functions per utterance with that
    utterance's (L, L, 1) mask: outputs and dx per utterance, parameter gradients summed over the utterances, to 1e-12"""
    H, D, Di = 2, 8, 24
    p = _params(L, K, H, D, Di, seed=L)
    rng = np.random.default_rng(1)
    x, cot = rng.standard_normal((B, L, H * D)), rng.standard_normal((B, L, H * D))
    m, _ = MC.build(family, L, B)
    full = MC.per_row(m, B, L)
    a, _ = O.rel_attn_fwd(x, p, m)
    z, cache = O.layer_fwd(x, p, m)
    dx, g = O.layer_bwd(cot, cache, p)
    assert np.isfinite(z).all() and np.isfinite(dx).all()
    gsum = {n: np.zeros_like(v) for n, v in g.items()}
    for b in range(B):
        mb = np.ascontiguousarray(full[b][:, :, None])                                # (qlen, klen, 1)
        ab, _ = O.rel_attn_fwd(x[b:b + 1], p, mb)
        zb, cb = O.layer_fwd(x[b:b + 1], p, mb)
        dxb, gb = O.layer_bwd(cot[b:b + 1], cb, p)
        assert np.abs(ab[0] - a[b]).max() <= 1e-12 * max(np.abs(a[b]).max(), 1)
        assert np.abs(zb[0] - z[b]).max() <= 1e-12 * max(np.abs(z[b]).max(), 1)
        assert np.abs(dxb[0] - dx[b]).max() <= 1e-12 * max(np.abs(dx[b]).max(), 1)
        for n in gb:
            gsum[n] += gb[n]
    for n in g:
        assert np.abs(gsum[n] - g[n]).max() <= 1e-12 * max(np.abs(g[n]).max(), 1), n
    if family != "holes":              # a wrong broadcast would show: utterance 1 (length 1 or 2) is far from utterance 0's mask
        zw, _ = O.layer_fwd(x[1:2], p, np.ascontiguousarray(full[0][:, :, None]))
        assert np.abs(zw[0] - z[1]).max() > 1e-3
