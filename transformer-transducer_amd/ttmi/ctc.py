"""CTC loss and greedy CTC decoding on libttmi's HIP kernels (csrc/ctc.hip; formulas in include/ttmi.h).

For joint CTC - transducer training: a linear head on the audio encoder's output is trained with this loss next to the RNN-T loss
(`Transducer.loss(..., ctc_weight=w)`), and its argmax with repeats collapsed is a non-autoregressive recogniser
(`Transducer.recognize_ctc`).  There is no CPU path.
"""
import collections

import torch

from . import ops

__all__ = ["CTCLoss", "ctc_loss", "ctc_greedy_decode", "ctc_align", "CTCAlignment", "ctc_score"]

CTCAlignment = collections.namedtuple("CTCAlignment", "path spans score expected mass duration")


def _lengths(logits, labels, act_lens, label_lens):
    if not logits.is_cuda:
        raise ValueError("ctc: logits must live on the GPU (the MI355X build has no CPU path)")
    if logits.dim() != 3:
        raise ValueError("ctc: logits must be [batch, T, vocab]")
    dev = logits.device
    out = []
    for name, t in (("labels", labels), ("act_lens", act_lens), ("label_lens", label_lens)):
        if t is None:
            out.append(None)
            continue
        if t.is_floating_point():
            raise TypeError("ctc: %s must be an integer tensor" % name)
        out.append(t.to(device=dev, dtype=torch.int32).contiguous())
    labels, act_lens, label_lens = out
    B = logits.shape[0]
    if labels is not None and (labels.dim() != 2 or labels.shape[0] != B):
        raise ValueError("ctc: labels must be [batch, U]")
    for t in (act_lens, label_lens):
        if t is not None and (t.dim() != 1 or t.shape[0] != B):
            raise ValueError("ctc: must have a length per example")
    return labels, act_lens, label_lens


class _CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, reduction, zero_infinity):
        B, T, _ = logits.shape
        x = logits if (logits.dtype is torch.float32 and ops.row_pitch(logits) is not None) else logits.float().contiguous()
        ws = ops.ctc_workspace(B, T, labels.shape[1], x.device)
        costs = ops.ctc_loss_fwd(x, labels, act_lens, label_lens, blank, ws)
        ctx.save_for_backward(x, labels, act_lens, label_lens, ws)
        ctx.blank, ctx.reduction, ctx.in_dtype = blank, reduction, logits.dtype
        if zero_infinity:       # (the kernels give an infeasible utterance an all-zero gradient either way)
            costs = torch.where(torch.isinf(costs), torch.zeros_like(costs), costs)
        return ops.reduce_costs(costs, reduction)

    @staticmethod
    def backward(ctx, grad_out):
        x, labels, act_lens, label_lens, ws = ctx.saved_tensors
        grad = ops.ctc_loss_bwd(x, labels, act_lens, label_lens, ctx.blank, ws, *ops.grad_out_args(grad_out, ctx.reduction, x.shape[0]))
        return grad.to(ctx.in_dtype), None, None, None, None, None, None


def ctc_loss(logits, labels, act_lens, label_lens, blank=0, reduction="mean", zero_infinity=False):
    """-log P(labels | logits) under CTC.  logits: UN-normalised f32 [B, T, V] on the GPU (log_softmax is taken inside, as RNNTLoss does);
    labels integer [B, U]; act_lens / label_lens integer [B] (clamped to [1, T] / [0, U]).

    reduction: 'none' -> costs [B]; 'sum' -> [1]; 'mean' -> [1], the sum divided by the BATCH SIZE - the meaning it has in this
    package's RNNTLoss, so that the two losses add with one weight.  It is NOT torch.nn.functional.ctc_loss's 'mean', which divides
    every cost by its target length first.
    An utterance with no feasible alignment (fewer frames than labels plus adjacent repeats) costs +inf and has a zero gradient;
    zero_infinity=True turns that cost into 0."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    labels, act_lens, label_lens = _lengths(logits, labels, act_lens, label_lens)
    return _CTCLossFn.apply(logits, labels, act_lens, label_lens, int(blank), reduction, bool(zero_infinity))


class CTCLoss(torch.nn.Module):
    """CTCLoss(blank=0, reduction='mean', zero_infinity=False)(logits, labels, act_lens, label_lens): see ctc_loss ('mean' divides by the
    batch size, not by target lengths)"""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity

    def forward(self, logits, labels, act_lens, label_lens):
        return ctc_loss(logits, labels, act_lens, label_lens, self.blank, self.reduction, self.zero_infinity)


def ctc_greedy_decode(logits, act_lens=None, blank=0):
    """logits f32 [B, T, V] on the GPU, act_lens integer [B] (None: every utterance has T frames) -> list of B token lists: the argmax of
    every frame with repeats collapsed and blanks dropped.  One device-to-host transfer.  RuntimeError if a frame has no finite maximum
    (NaN logits), as Transducer.decode raises."""
    if act_lens is None:
        if not logits.is_cuda:
            raise ValueError("ctc: logits must live on the GPU (the MI355X build has no CPU path)")
        act_lens = torch.full((logits.shape[0],), logits.shape[1], dtype=torch.int32, device=logits.device)
    _, act_lens, _ = _lengths(logits, None, act_lens, None)
    x = logits.detach()
    if x.dtype is not torch.float32 or ops.row_pitch(x) is None:
        x = x.float().contiguous()
    tokens, count = ops.ctc_greedy(x, act_lens, int(blank))
    host = torch.cat([count[:, None], tokens], dim=1).cpu()
    out = []
    for b in range(host.shape[0]):
        n = int(host[b, 0])
        if n < 0:
            raise RuntimeError("CTC greedy decode: the head produced no finite maximum at frame %d of utterance %d (NaN logits?)" % (-n - 1, b))
        out.append(host[b, 1:1 + n].tolist())
    return out


@torch.no_grad()
def ctc_score(logits, hypotheses, act_lens=None, blank=0):
    """The CTC log-likelihood of every hypothesis on the logits of its utterance: logits f32 [B, T, V] on the GPU (un-normalised),
    hypotheses = per utterance a list of token lists (an utterance may have none), act_lens integer [B] (None: every utterance has T
    frames) -> f64 device tensor [P], the hypotheses in flattening order; -inf where no alignment is feasible (fewer frames than tokens
    plus adjacent repeats).  The logits are shared by an utterance's hypotheses, not expanded (include/ttmi.h, ttmi_ctc_score_hyps);
    the value is -ctc_loss(reduction='none') of the same tokens.  No host synchronisation."""
    if not logits.is_cuda:
        raise ValueError("ctc: logits must live on the GPU (the MI355X build has no CPU path)")
    if logits.dim() != 3:
        raise ValueError("ctc: logits must be [batch, T, vocab]")
    B, T, _ = logits.shape
    if len(hypotheses) != B:
        raise ValueError("ctc_score: one list of hypotheses per utterance, got %d for a batch of %d" % (len(hypotheses), B))
    if act_lens is None:
        act_lens = torch.full((B,), T, dtype=torch.int32, device=logits.device)
    _, act_lens, _ = _lengths(logits, None, act_lens, None)
    flat = [(b, [int(v) for v in h]) for b in range(B) for h in hypotheses[b]]
    if not flat:
        return torch.empty(0, dtype=torch.float64, device=logits.device)
    U = max(len(h) for _, h in flat)
    if U > 1023:
        raise ValueError("ctc_score: a hypothesis of %d tokens (at most 1023)" % U)
    host = torch.zeros(len(flat), U + 2, dtype=torch.int64)             # utterance | length | tokens: one transfer
    for p, (b, h) in enumerate(flat):
        host[p, 0], host[p, 1] = b, len(h)
        if h:
            host[p, 2:2 + len(h)] = torch.tensor(h, dtype=torch.int64)
    dev = host.to(logits.device)
    x = logits.detach()
    if x.dtype is not torch.float32 or ops.row_pitch(x) is None:
        x = x.float().contiguous()
    return ops.ctc_score_hyps(x, act_lens, dev[:, 2:], dev[:, 1].to(torch.int32), dev[:, 0].to(torch.int32), int(blank))


@torch.no_grad()
def ctc_align(logits, labels, act_lens, label_lens, blank=0, stats=False):
    """Forced alignment of `labels` on the CTC lattice of `logits` (f32 [B, T, V] on the GPU, un-normalised; lengths checked and clamped as
    by ctc_loss) -> CTCAlignment(path, spans, score, expected, mass, duration), all on the device:

    path      int32 [B, T]     the state of the extended label sequence (2u = the blank before label u, 2u+1 = label u) the best single
                               alignment sits in at every frame, -1 for t >= T_b
    spans     int32 [B, U, 2]  (first, last) frame of label u on that alignment, (-1, -1) for u >= U_b
    score     f32 [B]          its log-probability; -inf, with every path / spans entry -1, where no alignment is feasible
    expected  f32 [B, U]       stats=True: the expected onset frame of label u over ALL alignments (-1 for u >= U_b), else None
    mass      f32 [B, U]       stats=True: the total onset posterior, 1 for a healthy lattice (0 for u >= U_b), else None
    duration  f32 [B, U]       stats=True: the expected number of frames label u occupies (0 for u >= U_b), else None

    Forward only: the loss forward into a workspace of its own, then ttmi_ctc_align (and ttmi_ctc_emit_stats); include/ttmi.h has the
    recurrences and the tie rule.  No host synchronisation."""
    labels, act_lens, label_lens = _lengths(logits, labels, act_lens, label_lens)
    x = logits.detach()
    if x.dtype is not torch.float32 or ops.row_pitch(x) is None:
        x = x.float().contiguous()
    B, T, V = x.shape
    ws = ops.ctc_workspace(B, T, labels.shape[1], x.device)
    ops.ctc_loss_fwd(x, labels, act_lens, label_lens, int(blank), ws)
    path, spans, score = ops.ctc_align(ws, labels, act_lens, label_lens, B, T, V, int(blank))
    expected = mass = duration = None
    if stats:
        expected, mass, duration = ops.ctc_emit_stats(ws, labels, act_lens, label_lens, B, T, V, int(blank))
    return CTCAlignment(path, spans, score, expected, mass, duration)
