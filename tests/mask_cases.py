"""Attention masks that differ per utterance, in the reference's conventions (True / nonzero = masked; 2-D = (klen, bsz) key mask, 3-D =
(qlen, klen, bsz)), built from per-utterance lengths.  Plain numpy, shared by tests/test_oracle_masks.py (which pins the builders and the
oracle's handling of them on the CPU) and the GPU files, so the GPU tests cannot drift from what was checked without a GPU."""
import numpy as np

from oracle import tt_oracle as O

FAMILIES = ("keypad", "causal_pad", "chunk_pad", "holes")
INTERVAL_FAMILIES = ("causal_pad", "chunk_pad")          # every row's kept keys form one interval -> mask kind 4
CHUNK, LEFT = 16, 64


def lengths(L, B):
    """per-utterance lengths: utterance 0 full, utterance 1 of length 1 or 2, utterance 2 ending inside a 64-key tile and inside a
    128-key phase where the sequence has one (L = 500 -> 300 = 4 * 64 + 44 = 2 * 128 + 44); neighbours differ by more than a tile
    wherever L allows it"""
    assert L >= 3 and 2 <= B <= 4
    mid = (L * 3) // 5
    if mid % 64 == 0:
        mid += 7
    return [L, 1 + (L % 2), mid, max(L - 70, 3)][:B]


def key_padding(L, lens):
    """(klen, bsz): key j of utterance b is masked iff j >= len_b"""
    return np.arange(L)[:, None] >= np.asarray(lens)[None, :]


def causal_padding(L, lens):
    """(qlen, klen, bsz): row i of utterance b sees keys 0 .. min(i, len_b - 1) - causal, and no padded key on any row (rows inside the
    utterance never reach a padded key under a causal mask, so it is the padded rows on which the utterances differ)"""
    i, j = np.arange(L)[:, None, None], np.arange(L)[None, :, None]
    hi = np.minimum(i, np.asarray(lens)[None, None, :] - 1)
    return j > hi


def chunk_padding(L, lens, chunk=CHUNK, left=LEFT):
    """(qlen, klen, bsz): the chunk mask, with keys j >= len_b masked as well on the rows i < len_b; padded rows keep the chunk mask's row"""
    m = np.repeat(O.chunk_mask(L, chunk, left)[:, :, None], len(lens), 2)
    i, j = np.arange(L)[:, None, None], np.arange(L)[None, :, None]
    ln = np.asarray(lens)[None, None, :]
    return m | ((i < ln) & (j >= ln))


def holes(L, B, seed=0, p=0.5):
    """(qlen, klen, bsz): independent Bernoulli(p) masks per utterance, the diagonal kept"""
    m = np.random.default_rng(seed).random((L, L, B)) < p
    m[np.arange(L), np.arange(L), :] = False
    return m


def build(family, L, B, seed=0):
    """-> (mask in the reference's form, lens)"""
    lens = lengths(L, B)
    if family == "keypad":
        return key_padding(L, lens), lens
    if family == "causal_pad":
        return causal_padding(L, lens), lens
    if family == "chunk_pad":
        return chunk_padding(L, lens), lens
    if family == "holes":
        return holes(L, B, seed + L), lens
    raise ValueError(family)


def per_row(mask, B, L):
    """bool [B, L, L] (True = masked) of a reference-form mask, broadcast over whatever it leaves out"""
    return np.broadcast_to(O.normalize_mask(mask, B, L), (B, L, L))


def every_row_keeps_a_key(mask, B, L):
    return bool((~per_row(mask, B, L)).any(-1).all())


def row_intervals(mask, B, L):
    """-> (lo, hi int [B, L], is_interval): first / last kept key of every row and whether the kept keys are exactly lo .. hi on every row"""
    keep = ~per_row(mask, B, L)
    n = keep.sum(-1)
    lo = keep.argmax(-1)
    hi = L - 1 - keep[:, :, ::-1].argmax(-1)
    return lo, hi, bool(((n > 0) & (n == hi - lo + 1)).all())


def reach(lo, hi):
    """(left, right): how far the intervals reach from the diagonal, max(i - lo_i) and max(hi_i - i), not below 0"""
    i = np.arange(lo.shape[-1])[None, :]
    return max(int((i - lo).max()), 0), max(int((hi - i).max()), 0)


def single(mask, b):
    """utterance b's mask as a shared table: (klen, 1) or (qlen, klen, 1)"""
    return np.ascontiguousarray(mask[..., b:b + 1])
