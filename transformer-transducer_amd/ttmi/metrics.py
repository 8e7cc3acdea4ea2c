"""Error counting on the device, and the weight rule of minimum word error rate (MWER) training.

edit_distance   device tensors in, device tensors out, no synchronisation (ttmi_edit_distance: one wave per pair)
error_counts    host lists of token sequences -> totals (one upload, one launch, one read-back)
computer_cer    the reference's tt/utils.py:46-50 on error_counts: `from ttmi.metrics import computer_cer` in place of
                `from tt.utils import computer_cer` lets the reference's eval() loop run where `editdistance` is not installed
mwer_weights    P_i = softmax_i(-c_i) per utterance, E_b = sum_i P_i W_i and the weights d mean_b E_b / d c_i (pure torch, float64)

The counts are unique: among all alignments the one that minimises (distance, substitutions, deletions, insertions) lexicographically
(include/ttmi.h has the rule).  A deletion is a ref token without a hyp counterpart, an insertion a hyp token without a ref counterpart."""
import collections

import numpy as np
import torch

from . import ops

EditStats = collections.namedtuple("EditStats", ["distance", "substitutions", "deletions", "insertions"])
MWERWeights = collections.namedtuple("MWERWeights", ["weights", "posteriors", "expected_errors"])


class ErrorCounts(collections.namedtuple("ErrorCounts", ["distance", "substitutions", "deletions", "insertions", "ref_tokens"])):
    """totals over the pairs of one error_counts call (python ints); `per_pair` = int array [pairs, 4] in the order of the first four fields"""
    per_pair = None


def _int32_rows(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype is torch.bool:
        raise ValueError("edit_distance: %s must be a 2-D integer tensor" % what)
    if t.dtype is not torch.int32:
        return t.to(torch.int32)                    # (a fresh dense tensor)
    return t if t.shape[1] <= 1 or t.stride(1) == 1 else t.contiguous()     # int32 rows are read where they are, at their own pitch


def _int32_vec(t, n, what):
    t = torch.as_tensor(t) if not isinstance(t, torch.Tensor) else t
    if t.dim() != 1 or t.shape[0] != n or t.dtype.is_floating_point:
        raise ValueError("edit_distance: %s must be an integer tensor of %d entries" % (what, n))
    return t.to(torch.int32).contiguous()


def edit_distance(hyp, hyp_lens, ref, ref_lens, ref_index=None):
    """hyp [P, Lh], ref [R, Lr]: device tensors of any integer dtype (compared as int32), Lh, Lr <= 1024; hyp_lens [P], ref_lens [R];
    ref_index [P] or None: the transcript row of every pair (None: pair p reads row p) -> EditStats of four int32 [P] device tensors.
    A pair whose lengths or ref_index are out of range gives -1 in every field.  Device only, no synchronisation; CPU tensors raise
    ValueError."""
    for t in (hyp, hyp_lens, ref, ref_lens, ref_index):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("edit_distance: inputs must be device tensors (the MI355X build has no CPU path)")
    hyp, ref = _int32_rows(hyp, "hyp"), _int32_rows(ref, "ref")
    hl, rl = _int32_vec(hyp_lens, hyp.shape[0], "hyp_lens"), _int32_vec(ref_lens, ref.shape[0], "ref_lens")
    ri = None if ref_index is None else _int32_vec(ref_index, hyp.shape[0], "ref_index")
    out = ops.edit_distance(hyp, hl, ref, rl, ri)
    return EditStats(*out.unbind(1))


def error_counts(hyps, refs, device=None):
    """hyps, refs: equally long host lists of sequences of hashable tokens (ids, or the strings dict_map produces); pair k compares hyps[k]
    with refs[k].  Tokens are interned to int32 ids on the host; one upload, one kernel launch, one read-back -> ErrorCounts."""
    hyps, refs = [list(h) for h in hyps], [list(r) for r in refs]
    if len(hyps) != len(refs):
        raise ValueError("error_counts: %d hypotheses for %d references" % (len(hyps), len(refs)))
    n = len(hyps)
    if n == 0:
        res = ErrorCounts(0, 0, 0, 0, 0)
        res.per_pair = np.zeros((0, 4), dtype=np.int64)
        return res
    ids = {}
    Lh, Lr = max(len(h) for h in hyps), max(len(r) for r in refs)
    if max(Lh, Lr) > 1024:
        raise ValueError("error_counts: sequences of more than 1024 tokens are not supported (longest: %d)" % max(Lh, Lr))
    pack = np.zeros((n, Lh + Lr + 2), dtype=np.int32)      # [hyp row | ref row | hyp length | ref length]: ONE host-to-device copy
    for k, (h, r) in enumerate(zip(hyps, refs)):
        pack[k, :len(h)] = [ids.setdefault(t, len(ids)) for t in h]
        pack[k, Lh:Lh + len(r)] = [ids.setdefault(t, len(ids)) for t in r]
        pack[k, Lh + Lr], pack[k, Lh + Lr + 1] = len(h), len(r)
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("error_counts: the kernel runs on the GPU (the MI355X build has no CPU path)")
    d = torch.from_numpy(pack).to(dev)
    out = ops.edit_distance(d[:, :Lh], d[:, Lh + Lr].contiguous(), d[:, Lh:Lh + Lr], d[:, Lh + Lr + 1].contiguous())
    per = out.cpu().numpy().astype(np.int64)
    res = ErrorCounts(*(int(v) for v in per.sum(0)), int(sum(len(r) for r in refs)))
    res.per_pair = per
    return res


def computer_cer(preds, labels):
    """the reference's tt/utils.py:46-50: -> (sum of the edit distances of every (label, pred) pair, sum of the label lengths)"""
    c = error_counts(preds, labels)
    return c.distance, c.ref_tokens


def mwer_weights(costs, errors, row_utt, B, max_per_utt=None):
    """The weight rule of MWER training.  costs [rows]: c_i = -log P(y_i | x) of every hypothesis row; errors [rows]: its error count W_i;
    row_utt [rows] (long): the utterance of every row, NON-DECREASING (an utterance's rows are adjacent); B utterances.  In float64:
        P_i = softmax over the rows of the utterance of (-c_i),   E_b = sum_i P_i W_i,   w_i = d (mean_b E_b) / d c_i = -P_i (W_i - E_b) / B
    -> MWERWeights(weights [rows], posteriors [rows], expected_errors [B]).  The weights of an utterance sum to zero; an utterance with one
    row has P = 1 and weight 0.  An utterance without a row has E_b = 0.  Nothing here is differentiated: the weights ARE the gradient.
    max_per_utt: the largest number of rows of one utterance when the caller knows it (else it is read from row_utt: one host read on a
    device tensor).  Every sum runs over a dense [B, max_per_utt] table in a fixed order: no atomics, two runs give the same bits."""
    c = costs.detach().to(torch.float64)
    W = errors.detach().to(torch.float64)
    row_utt = row_utt.long().contiguous()
    rows, dev = c.shape[0], c.device
    if rows == 0:
        z = torch.zeros(0, dtype=torch.float64, device=dev)
        return MWERWeights(z, z.clone(), torch.zeros(B, dtype=torch.float64, device=dev))
    start = torch.searchsorted(row_utt, torch.arange(B, device=dev))                   # first row of every utterance
    pos = torch.arange(rows, device=dev) - start[row_utt]
    N = int(pos.max()) + 1 if max_per_utt is None else int(max_per_utt)
    slot = row_utt * N + pos
    x = torch.full((B * N,), -float("inf"), dtype=torch.float64, device=dev)
    x[slot] = -c
    Wd = torch.zeros(B * N, dtype=torch.float64, device=dev)
    Wd[slot] = W
    x, Wd = x.view(B, N), Wd.view(B, N)
    m = x.max(dim=1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)                             # (an utterance without rows)
    e = torch.exp(x - m)
    s = e.sum(dim=1, keepdim=True)
    P = e / torch.where(s > 0, s, torch.ones_like(s))
    E = (P * Wd).sum(dim=1)
    w = -P * (Wd - E[:, None]) / B
    return MWERWeights(w.reshape(-1)[slot], P.reshape(-1)[slot], E)
