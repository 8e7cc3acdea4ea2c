"""CPU-only: the edit-distance oracle against a brute force over all alignments; ttmi_edit_distance's argument validation through ctypes;
ttmi.metrics fails loudly without a device; the MWER weight rule against autograd."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest
import torch

from conftest import PKG
from edit_oracle import brute_force, edit_counts


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_oracle_against_every_alignment():
    """every pair with lengths 0..4 over an alphabet of 2: the tuple DP is the minimum over all alignments, and the identities hold"""
    seqs = [s for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(seqs) == 31
    for hyp in seqs:
        for ref in seqs:
            got = edit_counts(hyp, ref)
            assert got == brute_force(hyp, ref), (hyp, ref)
            dist, s, d, i = got
            assert dist == s + d + i and len(hyp) == len(ref) - d + i


def test_oracle_identities_on_longer_pairs():
    rng = random.Random(0)
    for _ in range(300):
        V = rng.choice((2, 3, 5))
        hyp = [rng.randrange(V) for _ in range(rng.randrange(13))]
        ref = [rng.randrange(V) for _ in range(rng.randrange(13))]
        dist, s, d, i = edit_counts(hyp, ref)
        assert dist == s + d + i and len(hyp) == len(ref) - d + i
        assert dist >= abs(len(hyp) - len(ref)) and dist <= max(len(hyp), len(ref))
    assert edit_counts([], []) == (0, 0, 0, 0)
    assert edit_counts([1, 2, 3], []) == (3, 0, 0, 3) and edit_counts([], [1, 2]) == (2, 0, 2, 0)
    assert edit_counts("kitten", "sitting") == (3, 2, 1, 0)


def _call(lib, hyp, ld_hyp, hyp_len, ref, ld_ref, ref_len, ref_index, P, n_ref, max_hyp, max_ref, out):
    return lib.ttmi_edit_distance(hyp, ctypes.c_long(ld_hyp), hyp_len, ref, ctypes.c_long(ld_ref), ref_len, ref_index, P, n_ref, max_hyp, max_ref,
                                  out, None)


def test_argument_validation_without_gpu():
    """every refusal comes before any launch: rc < 0 and a message, on a machine without a device"""
    lib = _lib()
    buf = (ctypes.c_int * 4096)()
    ok = dict(hyp=buf, ld_hyp=8, hyp_len=buf, ref=buf, ld_ref=8, ref_len=buf, ref_index=None, P=2, n_ref=2, max_hyp=8, max_ref=8, out=buf)
    for name in ("hyp", "hyp_len", "ref", "ref_len", "out"):
        rc = _call(lib, **dict(ok, **{name: None}))
        assert rc < 0 and b"null pointer" in lib.ttmi_last_error(), name
    rc = _call(lib, **dict(ok, max_ref=1025, ld_ref=2048))
    assert rc < 0 and b"1024" in lib.ttmi_last_error()
    rc = _call(lib, **dict(ok, max_hyp=1025, ld_hyp=2048))
    assert rc < 0 and b"1024" in lib.ttmi_last_error()
    rc = _call(lib, **dict(ok, max_hyp=9))
    assert rc < 0 and b"pitch" in lib.ttmi_last_error()
    rc = _call(lib, **dict(ok, max_ref=9))
    assert rc < 0 and b"pitch" in lib.ttmi_last_error()
    rc = _call(lib, **dict(ok, P=-1))
    assert rc < 0 and b"P=-1" in lib.ttmi_last_error()
    assert _call(lib, **dict(ok, P=0)) == 0                  # nothing to do: no launch, no device needed


def test_metrics_fail_loudly_without_device():
    from ttmi import metrics
    hyp, ref = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64)
    lens = torch.ones(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        metrics.edit_distance(hyp, lens, ref, lens)
    with pytest.raises(ValueError):
        metrics.edit_distance(hyp, lens, ref, lens, ref_index=torch.zeros(2, dtype=torch.int64))


def test_mwer_weights_are_the_gradient_of_the_expected_errors():
    """3 utterances with 4 / 1 / 2 hypotheses: the rule equals autograd of mean_b sum_i softmax(-c)_i W_i with respect to c"""
    from ttmi.metrics import mwer_weights
    g = torch.Generator().manual_seed(0)
    sizes, B = [4, 1, 2], 3
    row_utt = torch.tensor([b for b, n in enumerate(sizes) for _ in range(n)])
    c = (torch.rand(7, generator=g, dtype=torch.float64) * 30.0 + 5.0).requires_grad_(True)
    W = torch.tensor([3, 0, 7, 2, 5, 1, 4], dtype=torch.int32)
    total, start, want_P, want_E = 0.0, 0, [], []
    for n in sizes:
        P = torch.softmax(-c[start:start + n], dim=0)
        E = (P * W[start:start + n].double()).sum()
        want_P.append(P.detach())
        want_E.append(E.detach())
        total = total + E
        start += n
    want, = torch.autograd.grad(total / B, c)
    for kw in ({}, {"max_per_utt": 4}):
        got = mwer_weights(c.detach(), W, row_utt, B, **kw)
        assert got.weights.dtype is torch.float64 and got.weights.shape == (7,)
        assert (got.weights - want).abs().max() < 1e-12
        assert (got.posteriors - torch.cat(want_P)).abs().max() < 1e-12
        assert (got.expected_errors - torch.stack(want_E)).abs().max() < 1e-12
        start = 0
        for n in sizes:
            assert abs(float(got.weights[start:start + n].sum())) < 1e-15
            start += n
        assert float(got.weights[4]) == 0.0 and float(got.posteriors[4]) == 1.0        # the utterance with one hypothesis
    f32 = mwer_weights(c.detach().float(), W, row_utt, B)
    assert f32.weights.dtype is torch.float64
