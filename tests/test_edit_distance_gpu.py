"""ttmi_edit_distance / ttmi.metrics on the device: every output field exactly as the oracle (tests/edit_oracle.py) gives it."""
import functools
import random

import numpy as np
import pytest
import torch

from edit_oracle import edit_counts

pytestmark = pytest.mark.gpu


def _seq(rng, n, alphabet):
    return [rng.choice(alphabet) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """-> (hyps, refs, ref_of): pair p compares hyps[p] with refs[ref_of[p]]; refs[-1] is used by no pair"""
    rng = random.Random(name)
    hyps, refs, ref_of = [], [], []

    def add(hyp, ref, share=False):
        if not share:
            refs.append(ref)
        hyps.append(hyp)
        ref_of.append(len(refs) - 1)

    def lengths(cases, alphabet):
        for hl, rl in cases:
            ref = _seq(rng, rl, alphabet)
            add(_seq(rng, hl, alphabet), ref)
            add(_seq(rng, max(hl - 1, 0), alphabet), ref, share=True)        # a second hypothesis of the same transcript
    if name == "one_chunk":             # ref width 64: one column per lane
        lengths([(0, 0), (0, 5), (5, 0), (7, 63), (7, 64), (64, 64), (65, 7)], [1, 2, 3])
        add([5], [5])
        add([5], [6])
    elif name == "two_chunks":          # ref width 127: two columns per lane, the last lane's second column unused
        lengths([(0, 0), (0, 5), (5, 0), (7, 63), (7, 64), (7, 65), (65, 7), (64, 64), (130, 127)], [1, 2, 3])
        add([5], [5])
        add([5], [6])
    elif name == "limit":               # 16 columns per lane
        lengths([(1024, 1024)], [1, 2, 3, 4])
        add(_seq(rng, 1023, [1, 2]), _seq(rng, 1024, [1, 2]))
        add(_seq(rng, 1024, [1, 2, 3]), [2])
    elif name == "identical_200":       # 4 columns per lane
        ref = _seq(rng, 200, list(range(1, 30)))
        add(list(ref), ref)
        add(_seq(rng, 40, [1, 2]), _seq(rng, 300, [1, 2]))                     # 8 columns per lane
    elif name == "disjoint":
        add(_seq(rng, 50, [1, 2, 3]), _seq(rng, 80, [4, 5, 6]))
        add(_seq(rng, 80, [1, 2, 3]), _seq(rng, 50, [4, 5, 6]))
    elif name == "ties_257":            # alphabets of 2 and 3 symbols: the tie rule decides the counts; 65 workgroups
        for k in range(257):
            alphabet = [1, 2] if k % 2 else [0, 1, 2]
            add(_seq(rng, rng.randrange(41), alphabet), _seq(rng, rng.randrange(41), alphabet), share=(k % 3 == 1))
    elif name == "vocab_4334":
        for _ in range(3):
            ref = _seq(rng, rng.randrange(45, 56), list(range(4334)))
            hyp = [t if rng.random() < 0.8 else rng.randrange(4334) for t in ref if rng.random() < 0.9]
            add(hyp, ref)
    elif name == "single":
        add(_seq(rng, 9, [1, 2]), _seq(rng, 11, [1, 2]))
    else:
        raise KeyError(name)
    refs.append(_seq(rng, 3, [1, 2]))                                        # the row no pair reads
    want = np.array([edit_counts(h, refs[r]) for h, r in zip(hyps, ref_of)], dtype=np.int32)
    want.setflags(write=False)
    return tuple(map(tuple, hyps)), tuple(map(tuple, refs)), tuple(ref_of), want


def _matrix(rows, width, pitch, dtype, rng):
    """[len(rows), width] view of a [len(rows), pitch] buffer; row pads and the buffer's tail poisoned with tokens that occur in the rows"""
    seen = sorted({t for r in rows for t in r}) or [0]
    buf = np.array([[rng.choice(seen) for _ in range(pitch)] for _ in rows], dtype=np.int64).reshape(len(rows), pitch)
    for k, r in enumerate(rows):
        buf[k, :len(r)] = r
    return torch.tensor(buf, dtype=dtype, device="cuda")[:, :width]


def _run(hyps, refs, ref_of, use_index, dtype):
    from ttmi import metrics
    rng = random.Random(7)
    if not use_index:                  # pair p reads ref row p: one row per pair
        refs = [refs[r] for r in ref_of]
        ref_of = None
    Lh, Lr = max(len(h) for h in hyps), max(len(r) for r in refs)
    hyp = _matrix(hyps, Lh, Lh + 5, dtype, rng)
    ref = _matrix(refs, Lr, Lr + 3, dtype, rng)
    hl = torch.tensor([len(h) for h in hyps], dtype=dtype, device="cuda")
    rl = torch.tensor([len(r) for r in refs], dtype=dtype, device="cuda")
    ri = None if ref_of is None else torch.tensor(ref_of, dtype=dtype, device="cuda")
    out = metrics.edit_distance(hyp, hl, ref, rl, ri)
    assert all(t.dtype is torch.int32 and t.shape == (len(hyps),) and t.is_cuda for t in out)
    return torch.stack(list(out), dim=1)


CASES = [("one_chunk", True, torch.int32), ("one_chunk", False, torch.int64), ("two_chunks", False, torch.int32), ("two_chunks", True, torch.int64),
         ("limit", True, torch.int32), ("identical_200", False, torch.int32), ("disjoint", True, torch.int64), ("ties_257", True, torch.int32),
         ("ties_257", False, torch.int64), ("vocab_4334", False, torch.int64), ("single", True, torch.int64), ("single", False, torch.int32)]


@pytest.mark.parametrize("name,use_index,dtype", CASES, ids=["%s-%s-%s" % (n, "index" if u else "rows", str(d)[6:]) for n, u, d in CASES])
def test_every_field_matches_the_oracle(name, use_index, dtype):
    hyps, refs, ref_of, want = _batch(name)
    got = _run(hyps, refs, ref_of, use_index, dtype).cpu().numpy()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "pair %d (hyp %d, ref %d tokens): got %s, want %s" % (
        bad[0], len(hyps[bad[0]]), len(refs[ref_of[bad[0]]]), got[bad[0]], want[bad[0]])
    assert (got[:, 0] == got[:, 1:].sum(axis=1)).all()


def test_batch_sizes_cover_one_three_and_257_pairs():
    assert {len(_batch(n)[0]) for n in ("single", "vocab_4334", "ties_257")} == {1, 3, 257}


def test_same_bits_twice():
    hyps, refs, ref_of, _ = _batch("ties_257")
    assert torch.equal(_run(hyps, refs, ref_of, True, torch.int32), _run(hyps, refs, ref_of, True, torch.int32))


def test_out_of_contract_pairs_give_minus_one_and_leave_their_neighbours_alone():
    """hyp_len = max_hyp + 1, ref_index = n_ref and ref_len = -1, in tensors large enough that a kernel which followed the bad value would
    still stay inside the allocation"""
    from ttmi import metrics
    rng = random.Random(11)
    P, Lh, Lr = 9, 12, 10
    hyps = [_seq(rng, rng.randrange(1, Lh + 1), [1, 2, 3]) for _ in range(P)]
    refs = [_seq(rng, rng.randrange(1, Lr + 1), [1, 2, 3]) for _ in range(P)]
    hyp = _matrix(hyps, Lh, 2 * Lh + 8, torch.int32, rng)
    ref_all = _matrix(refs + [[1, 2, 3], [3, 2, 1]], Lr, 2 * Lr + 8, torch.int32, rng)
    ref = ref_all[:P]                                          # n_ref = P; rows P, P + 1 exist in memory behind it
    hl = torch.tensor([len(h) for h in hyps], dtype=torch.int32, device="cuda")
    rl = torch.tensor([len(r) for r in refs], dtype=torch.int32, device="cuda")
    ri = torch.arange(P, dtype=torch.int32, device="cuda")
    hl[2] = Lh + 1
    ri[4] = P
    rl[6] = -1
    out = torch.stack(list(metrics.edit_distance(hyp, hl, ref, rl, ri)), dim=1).cpu().numpy()
    for p in range(P):
        if p in (2, 4, 6):
            assert (out[p] == -1).all(), (p, out[p])
        else:
            assert tuple(out[p]) == edit_counts(hyps[p], refs[p]), p
    hl[:], rl[:] = -3, 2000                                    # every pair out of contract, without ref_index
    out = torch.stack(list(metrics.edit_distance(hyp, hl, ref, rl)), dim=1)
    assert (out == -1).all()


def test_empty_batch_and_zero_width():
    from ttmi import metrics
    z = torch.zeros(0, 5, dtype=torch.int64, device="cuda")
    zl = torch.zeros(0, dtype=torch.int64, device="cuda")
    out = metrics.edit_distance(z, zl, z, zl)
    assert all(t.shape == (0,) for t in out)
    hyp = torch.zeros(2, 0, dtype=torch.int64, device="cuda")
    ref = torch.tensor([[4, 5, 6], [7, 0, 0]], device="cuda")
    out = metrics.edit_distance(hyp, torch.zeros(2, dtype=torch.int64, device="cuda"), ref, torch.tensor([3, 1], device="cuda"))
    assert out.distance.tolist() == [3, 1] and out.deletions.tolist() == [3, 1] and out.insertions.tolist() == [0, 0]
    with pytest.raises(ValueError):
        metrics.edit_distance(torch.zeros(1, 1025, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"),
                              ref, torch.tensor([3, 1], device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))


def test_error_counts_and_computer_cer():
    from ttmi import metrics
    preds = [["a", "b", "c", "d", "e"], [], ["x", "y"], ["k", "i", "t", "t", "e", "n"]]
    labels = [["a", "c", "d"], ["p", "q"], ["x", "y"], ["s", "i", "t", "t", "i", "n", "g"]]       # a prediction longer than its label, an empty one
    want = [edit_counts(p, l) for p, l in zip(preds, labels)]
    c = metrics.error_counts(preds, labels)
    assert c.per_pair.tolist() == [list(w) for w in want]
    assert (c.distance, c.substitutions, c.deletions, c.insertions) == tuple(sum(w[k] for w in want) for k in range(4))
    assert c.ref_tokens == sum(len(l) for l in labels) and all(type(v) is int for v in c)
    assert metrics.computer_cer(preds, labels) == (sum(w[0] for w in want), sum(len(l) for l in labels))
    ints_p, ints_l = [[3, 1, 4, 1, 5], [9, 2, 6], []], [[3, 1, 4, 5], [9, 2, 6], [5, 3]]
    want = [edit_counts(p, l) for p, l in zip(ints_p, ints_l)]
    assert metrics.computer_cer(ints_p, ints_l) == (sum(w[0] for w in want), 9)
    assert metrics.computer_cer(["abc", "xyz"], ["abd", "xyz"]) == (1, 6)                       # strings as sequences of characters
    assert metrics.computer_cer([], []) == (0, 0)
