"""Drop-in for `warprnnt_pytorch` (HawkAaron/warp-transducer pytorch_binding), the
third-party loss the reference imports at train.py:13 and calls at train.py:53,231:

    criterion = RNNTLoss()                      # blank=0, reduction='mean'
    loss = criterion(logits, targets.int(), inputs_length.int(), targets_length.int())

Same call contract: un-normalised logits in, softmax taken
internally, int32 labels/lengths, gradient w.r.t. the logits, 'mean' divides by
the batch and returns shape [1].  The arithmetic runs in libttmi's HIP kernels
(csrc/rnnt.hip); there is no CPU path here.

`fastemit_lambda` (keyword-only, default 0.0) adds FastEmit latency
regularisation (Yu et al., ICASSP 2021) as the transducer-loss libraries
expose it: the gradient favours emitting a label over emitting blank, the
returned cost stays -log P(y|x).  Formula: include/ttmi.h.

`topology` (keyword-only, default "rnnt") selects the lattice: "rnnt" is the
standard one (a label keeps its frame; warp-transducer's), "monotonic" the
one-symbol-per-frame lattice of this package's decoders (Tripathi et al. 2019;
csrc/mono.hip, recursion in include/ttmi.h).  FastEmit is not built on it.

`rnnt_align` (no counterpart in warp-transducer, which returns costs only) is
forced alignment on the same arguments: the best path through the lattice
(frame of every label's emission), its log-probability, the cost, and on
request the expected emission frame of every label.  It takes `topology` too:
on the monotonic lattice the emission frames are strictly increasing.
"""
import os
import weakref
from typing import NamedTuple, Optional

import torch

from ttmi import ops

__all__ = ["RNNTLoss", "rnnt_loss", "rnnt_align", "AlignResult", "check_lengths", "check_monotonic_lengths"]


_max_cache = {}     # id(tensor) -> (weakref, tensor._version, max): the length check costs a device-to-host sync; a lengths tensor that
                    # is the SAME object with the SAME version counter as last time has the same contents, so its maximum is reused


def _cached_max(t):
    ent = _max_cache.get(id(t))
    if ent is not None and ent[0]() is t and ent[1] == t._version:
        return ent[2]
    v = int(t.max())
    if len(_max_cache) > 64:
        _max_cache.clear()
    _max_cache[id(t)] = (weakref.ref(t), t._version, v)
    return v


def check_monotonic_lengths(act_lens, label_lens):
    """the monotonic lattice has no path for an utterance with more labels than frames.  One device-to-host read, under check_lengths only,
    and like _cached_max not repeated for the SAME two tensor objects at the same version counters"""
    key = (id(act_lens), id(label_lens))
    ent = _max_cache.get(key)
    if ent is not None and ent[0]() is act_lens and ent[1]() is label_lens and ent[2] == (act_lens._version, label_lens._version):
        bad = ent[3]
    else:
        bad = bool((label_lens > act_lens).any())
        if len(_max_cache) > 64:
            _max_cache.clear()
        _max_cache[key] = (weakref.ref(act_lens), weakref.ref(label_lens), (act_lens._version, label_lens._version), bad)
    if bad:
        raise ValueError("topology='monotonic': an utterance has more labels than frames (label_lengths > lengths)")


def _certify(acts, labels, act_lens, label_lens, check_lengths):
    for name, t in (("labels", labels), ("label_lengths", label_lens), ("lengths", act_lens)):
        if t.dtype is not torch.int32:
            raise TypeError("%s must be int32" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if acts.dtype not in (torch.float32, torch.bfloat16):       # bf16: the MI355X bf16 pipeline's own logits
        raise TypeError("acts must be float32 (or the bf16 logits of the bf16 pipeline)")
    if acts.dim() != 4:
        raise ValueError("acts must have 4 dimensions (batch, T, U+1, vocab)")
    if labels.dim() != 2 or act_lens.dim() != 1 or label_lens.dim() != 1:
        raise ValueError("labels must be 2-D, lengths 1-D")
    if act_lens.shape[0] != acts.shape[0] or label_lens.shape[0] != acts.shape[0]:
        raise ValueError("must have a length per example")
    if labels.shape[0] != acts.shape[0] or labels.shape[1] != acts.shape[2] - 1:
        raise ValueError("labels must be [batch, U] with U+1 == acts.shape[2]")
    if check_lengths:   # one tiny D2H sync, as in warp-transducer's certify_inputs
        if _cached_max(act_lens) != acts.shape[1]:
            raise ValueError("Input length mismatch")
        if _cached_max(label_lens) + 1 != acts.shape[2]:
            raise ValueError("Output length mismatch")


def check_lengths(labels, act_lens, label_lens, B, T, U1, check_max):
    """the label / length part of warp-transducer's certify_inputs for callers that never hold an `acts` tensor (the fused joint + loss)"""
    for name, t in (("labels", labels), ("label_lengths", label_lens), ("lengths", act_lens)):
        if t.dtype is not torch.int32:
            raise TypeError("%s must be int32" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if labels.dim() != 2 or act_lens.dim() != 1 or label_lens.dim() != 1:
        raise ValueError("labels must be 2-D, lengths 1-D")
    if act_lens.shape[0] != B or label_lens.shape[0] != B:
        raise ValueError("must have a length per example")
    if labels.shape[0] != B or labels.shape[1] != U1 - 1:
        raise ValueError("labels must be [batch, U] with U+1 == acts.shape[2]")
    if check_max:
        if _cached_max(act_lens) != T:
            raise ValueError("Input length mismatch")
        if _cached_max(label_lens) + 1 != U1:
            raise ValueError("Output length mismatch")


class _LatticeLossFn(torch.autograd.Function):
    """the loss of either lattice on materialised logits; lat: its ops.Lattice record"""

    @staticmethod
    def forward(ctx, acts, labels, act_lens, label_lens, blank, reduction, fastemit_lambda, lat):
        B, T, U1, _ = acts.shape
        acts_c = acts if ops.row_pitch(acts) is not None else acts.contiguous()     # row-padded views are consumed in place
        ws = lat.workspace(B, T, U1, acts.device)
        costs = lat.loss_fwd(acts_c, labels, act_lens, label_lens, blank, ws)
        ctx.save_for_backward(acts_c, labels, act_lens, label_lens, ws)
        ctx.blank, ctx.reduction, ctx.fastemit_lambda, ctx.lat = blank, reduction, fastemit_lambda, lat
        return ops.reduce_costs(costs, reduction)

    @staticmethod
    def backward(ctx, grad_out):
        acts, labels, act_lens, label_lens, ws = ctx.saved_tensors
        grad = ctx.lat.loss_bwd(acts, labels, act_lens, label_lens, ctx.blank, ws, *ops.grad_out_args(grad_out, ctx.reduction, acts.shape[0]),
                                **ctx.lat.fastemit_kw(ctx.fastemit_lambda))
        return grad, None, None, None, None, None, None, None


def rnnt_loss(acts, labels, act_lens, label_lens, blank=0, reduction="mean", check_lengths=None, *, fastemit_lambda=0.0, topology="rnnt"):
    fastemit_lambda = ops.check_fastemit(fastemit_lambda)
    lat = ops.lattice(topology, fastemit_lambda)
    if check_lengths is None:
        check_lengths = os.environ.get("TTMI_CHECK_LENGTHS", "1") != "0"
    if not acts.is_cuda:
        raise ValueError("RNNTLoss: acts must live on the GPU (the MI355X build has no CPU path)")
    labels, act_lens, label_lens = (t.to(acts.device) for t in (labels, act_lens, label_lens))
    _certify(acts, labels, act_lens, label_lens, check_lengths)      # (shape / dtype queries only: a DeferredLogits handle stays a handle)
    if lat.label_takes_frame and check_lengths:
        check_monotonic_lengths(act_lens, label_lens)
    fused = getattr(acts, "rnnt_loss", None)
    if fused is not None:
        # `acts` is the handle Transducer.forward returns in the bf16 pipeline (tt.model.DeferredLogits): joint + loss run as one fused op on
        # the encoder states it carries and the logits are never formed - train.py:51-53 as written, on the path of Transducer.loss
        out = fused(labels, act_lens, label_lens, int(blank), reduction, fastemit_lambda=fastemit_lambda, topology=lat.name)
        if out is not None:
            return out
        acts = acts.materialize()           # (per-utterance costs with gradients, or a handle that was already used as a tensor)
    return _LatticeLossFn.apply(acts, labels, act_lens, label_lens, int(blank), reduction, fastemit_lambda, lat)


class AlignResult(NamedTuple):
    """frames int32 [B, U]: frames[b][u] = the frame at which label u+1 of utterance b is emitted on the best path (the path's move
    (t, u) -> (t, u+1)), non-decreasing in u, -1 for u >= U_b; score f32 [B]: log-probability of that path; cost f32 [B]: -log P(y|x), the
    bits RNNTLoss(reduction='none') returns; with stats=True expected_frames f32 [B, U] (posterior mean emission frame, -1 for u >= U_b) and
    mass f32 [B, U] (total emission posterior of the label: 1 for a healthy lattice, 0 for u >= U_b), else None.

    With topology='monotonic' the same five fields on the one-decision-per-frame lattice: frames[b][u] = the frame whose ONE decision is
    label u+1 (the move (t, u) -> (t+1, u+1)), STRICTLY increasing in u; score has no terminal blank; cost holds the bits
    RNNTLoss(reduction='none', topology='monotonic') returns; an utterance with more labels than frames has score -inf, cost +inf, every
    frames / expected_frames entry -1 and mass 0"""
    frames: torch.Tensor
    score: torch.Tensor
    cost: torch.Tensor
    expected_frames: Optional[torch.Tensor] = None
    mass: Optional[torch.Tensor] = None


def rnnt_align(acts, labels, act_lens, label_lens, blank=0, check_lengths=None, *, stats=False, topology="rnnt"):
    """Forced alignment: arguments as rnnt_loss -> AlignResult.  Forward only (runs under no_grad).  Tie rule: a label move is taken only
    when strictly better than the blank move (include/ttmi.h, ttmi_rnnt_align).  A DeferredLogits handle goes through the fused joint +
    loss path instead of being materialised, as in rnnt_loss.

    topology: 'rnnt' (the default: the standard lattice, the code and bits of before) or 'monotonic', the one-decision-per-frame lattice
    of RNNTLoss(topology='monotonic') and of the decoders (include/ttmi.h, ttmi_mono_align): `frames` is then STRICTLY increasing, `score`
    is comparable with the decoders' DecodeResult.score, and under check_lengths an utterance with more labels than frames is a
    ValueError."""
    lat = ops.lattice(topology)
    if check_lengths is None:
        check_lengths = os.environ.get("TTMI_CHECK_LENGTHS", "1") != "0"
    labels, act_lens, label_lens = (t.to(acts.device) for t in (labels, act_lens, label_lens))
    _certify(acts, labels, act_lens, label_lens, check_lengths)
    if not acts.is_cuda:
        raise ValueError("rnnt_align: acts must live on the GPU (the MI355X build has no CPU path)")
    if lat.label_takes_frame and check_lengths:
        check_monotonic_lengths(act_lens, label_lens)
    with torch.no_grad():
        fused = getattr(acts, "rnnt_align", None)
        if fused is not None:
            out = fused(labels, act_lens, label_lens, int(blank), stats=bool(stats), topology=lat.name)
            if out is not None:
                return out
            acts = acts.materialize()
        acts = acts.detach()
        B, T, U1, _ = acts.shape
        acts_c = acts if ops.row_pitch(acts) is not None else acts.contiguous()
        ws = lat.workspace(B, T, U1, acts.device)
        cost = lat.loss_fwd(acts_c, labels, act_lens, label_lens, int(blank), ws)
        frames, score = lat.align(ws, act_lens, label_lens, B, T, U1)
        expected, mass = lat.emit_stats(ws, act_lens, label_lens, B, T, U1) if stats else (None, None)
    return AlignResult(frames, score, cost, expected, mass)


class RNNTLoss(torch.nn.Module):
    """RNNTLoss(blank=0, reduction='mean', *, fastemit_lambda=0.0, topology='rnnt')(acts, labels, act_lens, label_lens)

    topology: 'rnnt' (the standard lattice, the default, bit for bit what it was) or 'monotonic' (one decision per frame, the lattice of
    this package's decoders; with the length check on, an utterance with more labels than frames is a ValueError, with it off such an
    utterance costs +inf and has a zero gradient).  'monotonic' with fastemit_lambda > 0 is a ValueError.

    fastemit_lambda: FastEmit regularisation weight (finite, >= 0; 0 is the plain loss, bit for bit).  It changes the gradient only.
    It reaches the kernels as a by-value argument, so a captured step (ttmi.train.GraphedStep) replays the value it was captured with:
    changing it means recapturing."""

    def __init__(self, blank=0, reduction="mean", check_lengths=None, *, fastemit_lambda=0.0, topology="rnnt"):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.blank, self.reduction, self.check_lengths = blank, reduction, check_lengths
        self.fastemit_lambda = ops.check_fastemit(fastemit_lambda)
        self.topology = ops.check_topology(topology, self.fastemit_lambda)

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss(acts, labels, act_lens, label_lens, self.blank, self.reduction, self.check_lengths,
                         fastemit_lambda=self.fastemit_lambda, topology=self.topology)
