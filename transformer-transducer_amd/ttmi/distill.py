"""Transducer knowledge distillation on collapsed lattice posteriors (Panchapagesan et al., ICASSP 2021, "Efficient knowledge distillation
for RNN-transducer models"): every lattice node's distribution over the V outputs is collapsed to three classes - blank, the next label
y_{u+1}, everything else - and the student is trained with the KL divergence from the teacher's three probabilities to its own.  The teacher
hands over three floats per node ([B, T, U+1, 3], 9.8 MB for a whole C2 batch) instead of V logits, it can be computed once and cached, and it
need not share the student's vocabulary size.  include/ttmi.h has the arithmetic; the kernels are csrc/distill.hip.

    post = lattice_posteriors(teacher_logits, labels, act_lens, label_lens)            # the teacher, under no_grad
    kd = lattice_kd_loss(student_logits, post, labels, act_lens, label_lens)           # the student

`Transducer.lattice_posteriors` and `Transducer.loss(distill=post, distill_weight=w)` are the forms that never hold the logits."""
import torch

from . import ops


def _lattice_args(logits, labels, act_lens, label_lens, what):
    if not logits.is_cuda:
        raise ValueError("%s: logits must live on the GPU (the MI355X build has no CPU path)" % what)
    if hasattr(logits, "materialize"):          # a DeferredLogits handle (tt.model) is materialised like any other use of it
        logits = logits.materialize()
    labels, act_lens, label_lens = (t.to(device=logits.device, dtype=torch.int32).contiguous() for t in (labels, act_lens, label_lens))
    return logits, labels, act_lens, label_lens


def check_teacher(teacher_post, B, T, U1):
    """ValueError unless teacher_post is an f32 tensor [B, T, U1, 3] on the device (shape, then dtype, then device) -> it, detached and dense"""
    if not isinstance(teacher_post, torch.Tensor) or tuple(teacher_post.shape) != (B, T, U1, 3):
        raise ValueError("distill: teacher_post must have shape [%d, %d, %d, 3] (log P(blank), log P(next label), log P(other) per lattice "
                         "node), got %s" % (B, T, U1, list(getattr(teacher_post, "shape", ())) or type(teacher_post).__name__))
    if teacher_post.dtype != torch.float32:
        raise ValueError("distill: teacher_post must be float32, got %s" % teacher_post.dtype)
    if not teacher_post.is_cuda:
        raise ValueError("distill: teacher_post must live on the GPU (the MI355X build has no CPU path)")
    return teacher_post.detach().contiguous()


def lattice_posteriors(logits, labels, act_lens, label_lens, blank=0):
    """logits f32 / bf16 [B, T, U+1, V] (or a DeferredLogits handle) -> f32 [B, T, U+1, 3]: (log P(blank), log P(y_{u+1}), log P(anything
    else)) at every lattice node, each clamped below at -1e30, which is also what an empty class holds (the label class at u = U_b and for a
    label equal to blank); exact zeros outside the ragged lattice.  No gradient flows through it: it is the teacher's call"""
    with torch.no_grad():
        logits, labels, act_lens, label_lens = _lattice_args(logits, labels, act_lens, label_lens, "lattice_posteriors")
        x = logits.detach()
        if ops.row_pitch(x) is None:
            x = x.contiguous()
        return ops.kd_collapse(x, labels, act_lens, label_lens, int(blank))


class _LatticeKDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, teacher, labels, act_lens, label_lens, blank, reduction):
        B, T, U1, _ = acts.shape
        acts_c = acts if ops.row_pitch(acts) is not None else acts.contiguous()     # row-padded views are consumed in place
        ws = ops.kd_workspace(B, T, U1, acts.device)
        costs = ops.kd_loss_fwd(acts_c, labels, act_lens, label_lens, blank, teacher, ws)
        ctx.save_for_backward(acts_c, labels, act_lens, label_lens, ws)
        ctx.blank, ctx.reduction = blank, reduction
        return ops.reduce_costs(costs, reduction)

    @staticmethod
    def backward(ctx, grad_out):
        acts, labels, act_lens, label_lens, ws = ctx.saved_tensors
        grad = ops.kd_loss_bwd(acts, labels, act_lens, label_lens, ctx.blank, ws, *ops.grad_out_args(grad_out, ctx.reduction, acts.shape[0]))
        return grad, None, None, None, None, None, None


def lattice_kd_loss(logits, teacher_post, labels, act_lens, label_lens, blank=0, reduction="mean"):
    """KL(teacher || student) on the collapsed posteriors of every lattice node, summed over each utterance's nodes: [B] for reduction
    'none', their sum for 'sum', that over B for 'mean' ([1]).  logits: the student's, f32 / bf16 [B, T, U+1, V] on the device (a
    DeferredLogits handle is materialised); teacher_post: f32 [B, T, U+1, 3] as lattice_posteriors gives it, a constant (no gradient flows
    into it).  ValueError for a teacher_post of another shape, dtype or device"""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    if logits.dim() != 4:
        raise ValueError("lattice_kd_loss: logits must be [B, T, U+1, V]")
    teacher = check_teacher(teacher_post, *logits.shape[:3])
    logits, labels, act_lens, label_lens = _lattice_args(logits, labels, act_lens, label_lens, "lattice_kd_loss")
    return _LatticeKDFn.apply(logits, teacher, labels, act_lens, label_lens, int(blank), reduction)


class LatticeKDLoss(torch.nn.Module):
    """module form of lattice_kd_loss: LatticeKDLoss(blank, reduction)(logits, teacher_post, labels, act_lens, label_lens)"""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.blank, self.reduction = int(blank), reduction

    def forward(self, logits, teacher_post, labels, act_lens, label_lens):
        return lattice_kd_loss(logits, teacher_post, labels, act_lens, label_lens, self.blank, self.reduction)
