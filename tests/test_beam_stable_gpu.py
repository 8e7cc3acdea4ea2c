"""ttmi_beam_stable_prefix on the device against the numpy restatement of its rule (tests/beam_stream_oracle.py), integers compared exactly.
Every case has B = 3 utterances; the words behind every slot's tokens are stale copies of the shared tokens (a kernel that ignored len would
count them), the words behind `stable` and behind the last hist row are guards that must come back intact, and two runs must agree."""
import math

import numpy as np
import pytest
import torch

import beam_stream_oracle as SO

pytestmark = pytest.mark.gpu

GUARD = -0x5a5a5a5a


def _beam(W, ld, seed, diverge=None, lens=None):
    """B = 3: per utterance a base row of random tokens; slot w spells the base up to diverge[b][w] tokens and differs from there on (None:
    drawn at random); lens[b][w] (None: drawn in [0, ld - 1]); the row behind len keeps the base's words; scores finite and descending"""
    rng = np.random.default_rng([seed, W, ld])
    B = 3
    hist = np.zeros((B, W, ld), dtype=np.int64)
    n_tok = np.zeros((B, W), dtype=np.int32)
    for b in range(B):
        base = rng.integers(1, 4000, ld)
        for w in range(W):
            hist[b, w] = base
            hist[b, w, 0] = 0
            d = int(rng.integers(0, ld)) if diverge is None else diverge[b][w]
            if d is not None and w > 0 and 1 + d < ld:
                hist[b, w, 1 + d:] += 1 + w
            n_tok[b, w] = int(rng.integers(0, ld)) if lens is None else lens[b][w]
    score = -np.arange(B * W, dtype=np.float64).reshape(B, W) / 8
    return score, n_tok, hist


def _run(score, n_tok, hist):
    from ttmi import ops
    B, W, ld = hist.shape
    flat = torch.full((B * W * ld + 64,), GUARD, dtype=torch.long)
    flat[:B * W * ld] = torch.from_numpy(hist).reshape(-1)
    flat = flat.cuda()
    out = torch.full((B + 64,), GUARD, dtype=torch.int32).cuda()
    s, n = torch.from_numpy(score).cuda(), torch.from_numpy(n_tok.astype(np.int32)).cuda()
    got = ops.beam_stable_prefix(s, n, flat[:B * W * ld].view(B, W, ld), out=out[:B])
    assert got.data_ptr() == out.data_ptr()
    first = out.cpu()
    ops.beam_stable_prefix(s, n, flat[:B * W * ld].view(B, W, ld), out=out[:B])
    assert torch.equal(first, out.cpu())                                  # two runs, the same bits
    assert (first[B:] == GUARD).all() and (flat[B * W * ld:].cpu() == GUARD).all()
    assert torch.equal(flat[:B * W * ld].cpu(), torch.from_numpy(hist).reshape(-1))
    return first[:B].tolist()


def _check(score, n_tok, hist, want=None):
    oracle = SO.stable_prefix(score, n_tok, hist).tolist()
    if want is not None:
        assert oracle == want, (oracle, want)                             # the case is the one it is meant to be
    got = _run(score, n_tok, hist)
    assert got == oracle, (got, oracle)
    return got


@pytest.mark.parametrize("ld", [5, 37, 131])
@pytest.mark.parametrize("W", [1, 4, 32])
def test_random_beams(W, ld):
    for seed in range(3):
        score, n_tok, hist = _beam(W, ld, seed)
        got = _check(score, n_tok, hist)
        if W == 1:
            assert got == n_tok[:, 0].tolist()
    score, n_tok, hist = _beam(W, ld, 7, lens=[[ld - 1] * W] * 3)       # full rows: the divergence alone decides
    _check(score, n_tok, hist)


@pytest.mark.parametrize("ld", [5, 37, 131])
def test_empty_slots(ld):
    W = 4
    full = [[ld - 1] * W] * 3
    div = [[None, ld // 2, 1, 3]] * 3
    score, n_tok, hist = _beam(W, ld, 1, diverge=div, lens=full)
    _check(score, n_tok, hist, [1, 1, 1])
    s = score.copy()
    s[:, 2] = -math.inf                                                   # the slot that differs first is empty
    _check(s, n_tok, hist, [min(3, ld // 2)] * 3)
    s[:, 0] = -math.inf                                                   # slot 0 empty: w0 = 1, which slot 3 leaves at min(3, ld // 2) too
    _check(s, n_tok, hist, [min(3, ld // 2)] * 3)
    s = score.copy()
    s[0, 2], s[1, 3], s[2, 1] = math.nan, math.nan, math.nan              # a NaN score is empty
    _check(s, n_tok, hist, [min(3, ld // 2), 1, 1])
    s = np.full_like(score, -math.inf)                                    # all slots empty
    s[1] = math.nan
    _check(s, n_tok, hist, [0, 0, 0])
    _check(score, np.zeros_like(n_tok), hist, [0, 0, 0])                  # len = 0 everywhere


@pytest.mark.parametrize("W", [4, 32])
def test_lane_stride_seams(W):
    """hypotheses that agree on 64, 65 and 129 tokens and differ at the next: the end of a pass of 64 lanes, the first lane of the next pass,
    the first lane of the third"""
    ld = 131
    agree = [64, 65, 129]
    div = [[None] + [agree[b] + 3 * (w - 1) for w in range(1, W)] for b in range(3)]
    score, n_tok, hist = _beam(W, ld, 2, diverge=div, lens=[[130] * W] * 3)
    _check(score, n_tok, hist, agree)
    div = [[None] + [agree[b] + 3 * (W - 1 - w) for w in range(1, W)] for b in range(3)]      # the last slot differs first
    score, n_tok, hist = _beam(W, ld, 3, diverge=div, lens=[[130] * W] * 3)
    _check(score, n_tok, hist, agree)
    n_tok[0, 1], n_tok[1, W - 1], n_tok[2, 2] = 63, 64, 128               # one live slot shorter than the others' agreement
    _check(score, n_tok, hist, [63, 64, 128])


@pytest.mark.parametrize("ld", [5, 37, 131])
def test_len_outside_the_row_is_clamped(ld):
    W = 4
    score, n_tok, hist = _beam(W, ld, 4, diverge=[[None] * W] * 3, lens=[[ld + 1000] * W, [2 ** 31 - 1] * W, [-5, ld, ld, ld]])
    _check(score, n_tok, hist, [ld - 1, ld - 1, 0])
