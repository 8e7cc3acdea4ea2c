"""Transducer / JointNet with the reference's API surface (tt/model.py): .encoder/.decoder/.joint,
forward(inputs[B,T,d], targets[B,U]) -> logits[B,T,U+1,V], decode/recognize (greedy), beam search."""
import collections
import copy
import heapq
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ttmi import ops
from ttmi.ops import MaskSpec
from tt.decoder import BuildDecoder
from tt.encoder import BuildEncoder
from tt.transformer import label_value_precision, default_precision, grad_targets
from tt.utils import context_mask, look_ahead_mask  # noqa: F401  (re-exported like the reference module)


class _JointFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, dec, wf, bf, wp, bp, prec):
        enc, dec = enc.contiguous(), dec.contiguous()
        params = (wf, bf, wp, bp)
        wf, bf, wp, bp = (t.detach() for t in (wf, bf, wp, bp))
        logits, saved = ops.joint_fwd(enc, dec, wf, bf, wp, bp, prec)
        ctx.save_for_backward(enc, dec, wf, wp, saved)
        ctx.prec = prec
        ctx.params = params
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        enc, dec, wf, wp, saved = ctx.saved_tensors
        g, rets, after = grad_targets(ctx.params, ("wf", "bf", "wp", "bp"))
        denc, ddec = ops.joint_bwd(dlogits, enc, dec, wf, wp, saved, ctx.prec, g)
        for cb in after:
            cb()
        return (denc, ddec, *rets, None)


class _ExpShift:
    """Range control of the exp-domain loss form, per JointNet module and device (never shared between models): the device scalars `cur`
    (shift subtracted before exp in this step) and `nxt` (gathered for the next one), and a sticky device `flag` the loss kernel raises when
    a lattice row's sum under- or overflowed.  No host synchronisation anywhere:

    * not `valid` (first use, after JointNet.load_state_dict - a hook invalidates it -, or after a flagged step): the step runs the plain
      fused form, whose log-sum-exp pass also seeds `nxt` (ttmi_rnnt_shift_seed); from the next step on the exp-domain kernels run.
      Weights overwritten behind the module's back (p.data.copy_) are caught by the flag if their logits left the 40 e-fold margin.
    * every exp step leaves max(log-sum-exp) - 40 in `nxt`; it becomes `cur` only if an exp (or seeding) chunk actually ran.
    * the flag is copied to pinned host memory on a side stream and looked at (event query, non-blocking) at the next calls; a flagged
      step's costs and gradients are NaN by construction (never finite and wrong) and the fused optimiser drops such a step."""

    def __init__(self, device):
        self.cur = torch.zeros(1, dtype=torch.float32, device=device)
        self.nxt = torch.zeros(1, dtype=torch.float32, device=device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.copy_stream = torch.cuda.Stream(device)
        self.pending = []               # (event, generation) of flag copies in flight
        self.valid, self.gen, self.flagged_steps = False, 0, 0

    def set(self, shift):
        """start from a known shift (tests, callers that know their logits' scale)"""
        self.cur.fill_(float(shift))
        self.nxt.zero_()
        self.valid = True

    def poll(self):
        """look at completed flag copies; a raised flag invalidates the shift (the next step re-seeds it in the plain form)"""
        while self.pending and self.pending[0][0].query():
            _, gen = self.pending.pop(0)
            if gen == self.gen and int(self.host[0]) != 0:
                import warnings
                self.gen += 1
                self.flagged_steps += 1
                self.valid = False
                self.flag.zero_()
                warnings.warn("exp-domain RNN-T loss: a lattice row's sum of exponentials under/overflowed (the logits moved by more than "
                              "the 40 e-fold margin within one step); that step's loss and gradients were NaN and FusedOptimizer dropped "
                              "it; the next step runs the plain fused form and re-seeds the shift")

    def watch(self):
        """queue an asynchronous copy of the flag behind the work issued so far"""
        main = torch.cuda.current_stream(self.cur.device)
        self.copy_stream.wait_stream(main)
        with torch.cuda.stream(self.copy_stream):
            self.host.copy_(self.flag, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.pending.append((ev, self.gen))
        if len(self.pending) > 8:       # bounded: the oldest copy finished long ago
            self.pending[0][0].synchronize()
            self.poll()


_warned_no_exp = set()


def _warn_no_exp(Bc, T, U1, J, V):
    """one warning per shape class: the exp-domain form was asked for and cannot run (the plain fused form runs instead - same loss and
    gradients up to bf16 rounding, about 4 ms slower per C2-sized step)"""
    key = (J, V, Bc * T * U1 < 32768)
    if key in _warned_no_exp:
        return
    _warned_no_exp.add(key)
    import warnings
    warnings.warn("exp-domain RNN-T loss form: a chunk of %d x %d x %d lattice rows with joint sizes J=%d, V=%d is outside the persistent "
                  "kernels' sizes (they need >= 32768 lattice rows per chunk, J a multiple of 64 and >= 256, V >= 1024); the plain fused "
                  "joint + loss form runs instead" % (Bc, T, U1, J, V))


def _scaled_param_grads(params, grads, gout):
    """the parameter part of what backward() of the fused loss ops returns: per parameter grads[i] * gout, or None where the product was
    added straight into the parameter's .grad (FlatModel's flat gradient buffer) and its gradient-ready callback run"""
    rets = []
    for prm, gp in zip(params, grads):
        if getattr(prm, "_ttmi_direct", False) and prm.grad is not None:       # FlatModel: accumulate into the flat gradient buffer
            prm.grad.addcmul_(gp, gout)
            rets.append(None)
            cb = getattr(prm, "_ttmi_on_grad", None)
            if cb is not None:
                cb()
        else:
            rets.append(gp * gout)
    return rets


class _JointLossFn(torch.autograd.Function):
    """joint network + RNN-T loss as ONE op that never holds the [B, T, U+1, V] logits: the batch is cut into chunks
    of utterances; per chunk the logits are produced (ttmi_joint_fwd), reduced to the lattice (ttmi_rnnt_loss_fwd), overwritten IN PLACE
    by their own gradient (ttmi_rnnt_loss_bwd, the same kernels as RNNTLoss) and consumed by the joint's backward (ttmi_joint_bwd) - in
    the forward pass, as warp-transducer itself forms its gradients - so one chunk's buffer is the whole footprint (C2: 14.2 GB of
    logits + gradient -> 0.44 GB per chunk of 2 utterances; C5: 55.8 GB -> 3.5 GB per utterance).  backward() only scales by the
    incoming gradient."""

    @staticmethod
    def forward(ctx, enc, dec, wf, bf, wp, bp, labels, act_lens, label_lens, prec, chunk, reduction, exp_state, grad_mode=True, blank=0,
                fastemit_lambda=0.0, weights=None, topology="rnnt", distill=None, distill_weight=0.0):
        """exp_state: None (plain fused form) or the JointNet's _ExpShift for this device (exp-domain form); fastemit_lambda: the FastEmit
        weight of the loss gradient (warprnnt_pytorch.RNNTLoss), in all three chunk forms; weights: None or a constant f32 [B] on the device,
        one factor per utterance: the result is sum_b w_b cost_b (times 1 / B for 'mean') and every chunk's loss-gradient call reads its slice
        of w as its upstream gradient (grad_out_stride = 1), so the gradients formed here are those of the weighted sum.  A chunk whose
        weights are all zero is NOT skipped: its costs are part of the result either way, and knowing that its weights are zero would take a
        host read of a device tensor - its gradient kernels run and add exact zeros; topology: 'rnnt', or 'monotonic' for the decoders'
        one-decision-per-frame lattice (ttmi_mono_loss_fwd / _bwd): that one has the plain chunk form only - joint_fwd, mono_loss_fwd,
        mono_loss_bwd in place, joint_bwd - no exp-domain form, no pre-split gradient planes and no shift seeding; distill (None, or with
        distill_weight 0: the code path and bits without it): the teacher's collapsed lattice posteriors, a constant f32 [B, T, U1, 3] on the
        device (ttmi.distill) - the result is the transducer term + distill_weight * KD under the same reduction (KD is not multiplied by
        `weights`).  A chunk then runs joint_fwd, the topology's loss forward, kd_loss_fwd, the topology's loss gradient OUT of place (FastEmit
        included; in the bf16x3 mode the f32 gradient goes through joint_bwd's own split pass, as on the monotonic lattice), kd_loss_bwd
        adding scale * distill_weight * d KD onto that gradient, joint_bwd.  A second chunk buffer is alive meanwhile; the 2 GB budget of
        default_loss_chunk leaves room for it, so the chunk size is the same.  No exp-domain form.  `topology` may also be a lattice RECORD
        instead of one of the two names: an ops.TDTLattice (token-and-duration transducer: wp has V + D rows, the loss entries are
        ttmi_tdt_loss_fwd / _bwd) runs the plain chunk form as 'monotonic' does; FastEmit and distillation are not built on it"""
        fe = ops.check_fastemit(fastemit_lambda)
        if isinstance(topology, str):
            lat = ops.lattice(topology, fe)
        else:
            lat = topology
            if fe > 0.0 or (distill is not None and float(distill_weight) != 0.0):
                raise ValueError("%s: FastEmit and distillation are not built on this lattice" % lat.name.upper())
        if not lat.has_exp_forms and exp_state is not None:
            raise ValueError("topology='%s' has no exp-domain form" % lat.name)
        kd = distill is not None and float(distill_weight) != 0.0
        if kd and exp_state is not None:
            raise ValueError("distill has no exp-domain form")
        enc, dec = enc.contiguous(), dec.contiguous()
        params = (wf, bf, wp, bp)
        wf_, bf_, wp_, bp_ = (t.detach() for t in params)
        B, T = enc.shape[0], enc.shape[1]
        U1 = dec.shape[1]
        need = grad_mode and any(ctx.needs_input_grad[:6])      # (needs_input_grad ignores torch.no_grad(); forward() itself always runs without grad mode)
        costs = torch.empty(B, dtype=torch.float32, device=enc.device)
        kd_costs = torch.empty(B, dtype=torch.float32, device=enc.device) if kd else None
        one = torch.ones(1, dtype=torch.float32, device=enc.device)
        scale = 1.0 / B if reduction == "mean" else 1.0
        if need:
            denc, ddec = torch.empty_like(enc), torch.empty_like(dec)
            g = {n: torch.zeros_like(t) for n, t in zip(("wf", "bf", "wp", "bp"), params)}
        J, V = wf.shape[0], wp.shape[0]

        def upstream(c0, c1):
            """(grad_out, grad_out_stride) of a chunk's loss-gradient call: the shared 1, or the chunk's utterance weights"""
            return (one, 0) if weights is None else (weights[c0:c1], 1)
        st = exp_state
        exp_ran = seeded = False
        capturing = enc.is_cuda and torch.cuda.is_current_stream_capturing()      # (ttmi.train.GraphedStep looks at the flag between replays)
        if st is not None and not capturing:
            st.poll()
        for c0 in range(0, B, chunk):
            c1 = min(B, c0 + chunk)
            lab, al, ll = labels[c0:c1], act_lens[c0:c1], label_lens[c0:c1]
            ws = lat.workspace(c1 - c0, T, U1, enc.device)
            kws = ops.kd_workspace(c1 - c0, T, U1, enc.device) if kd else None
            exp_ok = st is not None and ops.joint_exp_supported(c1 - c0, T, U1, J, V, prec, fwd_only=not need)
            if st is not None and not exp_ok:
                _warn_no_exp(c1 - c0, T, U1, J, V)
            if exp_ok and st.valid:
                # the projection stores exp(logit - shift) and row sums; the loss reads the sums and two f32 logits per row, its gradient
                # stays factored as (row factor) x P and is consumed in that form (include/ttmi.h, "fused joint + loss fast path")
                P, rowsum, saved, emis = ops.joint_fwd_exp(enc[c0:c1], dec[c0:c1], wf_, bf_, wp_, bp_, prec, st.cur, lab.contiguous(), blank)
                costs[c0:c1] = ops.rnnt_loss_fwd_exp(P, rowsum, lab, al, ll, blank, ws, st.cur, st.nxt, emis, st.flag)
                if need:
                    srow, srow16 = ops.rnnt_loss_bwd_exp(P, lab, al, ll, blank, ws, *upstream(c0, c1), scale, fastemit_lambda=fe)
                    ops.joint_bwd_exp(P, srow, srow16, enc[c0:c1], dec[c0:c1], wf_, wp_, saved, prec, g, out=(denc[c0:c1], ddec[c0:c1]))
                del P, rowsum, saved, emis
                exp_ran = True
                continue
            logits, saved = ops.joint_fwd(enc[c0:c1], dec[c0:c1], wf_, bf_, wp_, bp_, prec)
            costs[c0:c1] = lat.loss_fwd(logits, lab, al, ll, blank, ws)
            if kd:
                kd_costs[c0:c1] = ops.kd_loss_fwd(logits, lab, al, ll, blank, distill[c0:c1], kws)
            if st is not None and not st.valid:                 # the plain form's log-sum-exp pass seeds the shift for the next step
                ops.rnnt_shift_seed(ws, al, ll, c1 - c0, T, U1, st.nxt)
                seeded = True
            if need and lat.has_exp_forms and not kd and ops.joint_loss_split_supported(logits, wf_.shape[0], prec):
                # bf16x3: the gradient leaves the loss kernel as the two bf16 planes the joint's three-term backward multiplies (round 6: no split pass over d logits)
                planes = ops.rnnt_loss_bwd_split(logits, lab, al, ll, blank, ws, *upstream(c0, c1), scale, fastemit_lambda=fe)
                ops.joint_bwd_split(planes, enc[c0:c1], dec[c0:c1], wf_, wp_, saved, prec, g, out=(denc[c0:c1], ddec[c0:c1]))
            elif need:
                # in place, unless the KD gradient is to be added: that one needs the logits once more
                grad = lat.loss_bwd(logits, lab, al, ll, blank, ws, *upstream(c0, c1), scale, inplace=not kd, **lat.fastemit_kw(fe))
                if kd:
                    grad = ops.kd_loss_bwd(logits, lab, al, ll, blank, kws, one, 0, scale * float(distill_weight), accumulate=grad)
                ops.joint_bwd(grad, enc[c0:c1], dec[c0:c1], wf_, wp_, saved, prec, g, out=(denc[c0:c1], ddec[c0:c1]))
                if kd:
                    del grad                # (the second chunk buffer)
            del logits, saved
        if st is not None and (exp_ran or seeded):
            st.cur.copy_(st.nxt)
            st.nxt.zero_()
            st.valid = True
            if exp_ran and not capturing:
                st.watch()
        if need:
            ctx.save_for_backward(denc, ddec, *g.values())
        ctx.params = params
        if kd:
            if reduction == "none":
                return costs + float(distill_weight) * kd_costs
            total = (costs * weights).sum() if weights is not None else costs.sum()
            return (total + float(distill_weight) * kd_costs.sum()).reshape(1) * scale
        if reduction == "none":
            return costs
        if weights is not None:
            return (costs * weights).sum().reshape(1) * scale
        return costs.sum().reshape(1) * scale

    @staticmethod
    def backward(ctx, gout):
        denc, ddec, *gs = ctx.saved_tensors
        gout = gout.float()
        if gout.numel() != 1:
            raise NotImplementedError("fused joint + loss: per-utterance upstream gradients (reduction='none') are not supported; "
                                      "use model(inputs, targets) + RNNTLoss(reduction='none')")
        rets = _scaled_param_grads(ctx.params, gs, gout)
        return (denc * gout, ddec * gout, *rets, None, None, None, None, None, None, None, None, None, None, None, None, None, None)


class _CTCHeadLossFn(torch.autograd.Function):
    """auxiliary CTC head on the audio encoder's output + CTC loss as ONE op, in the manner of _JointLossFn: the [B, T, V] logits live in a
    row-padded buffer (ops.padded_empty) that the loss gradient overwrites in place (ttmi_ctc_loss_bwd) and the head's dgrad / wgrad /
    bias-sum products consume in the forward pass; backward() only scales by the incoming gradient.  Every product is the library's own
    GEMM (ops.linear_*): bf16 MFMA with f32 output in the bf16 mode, the exact-f32 / three-term paths in the fp32 / bf16x3 modes."""

    @staticmethod
    def forward(ctx, enc, w, b, labels, act_lens, label_lens, prec, reduction, grad_mode=True, blank=0):
        enc = enc.contiguous()
        B, T, d = enc.shape
        V = w.shape[0]
        w_, b_ = w.detach(), b.detach()
        x2 = enc.detach().reshape(B * T, d)
        buf, logits = ops.padded_empty((B, T, V), torch.float32, enc.device)
        l2 = buf.view(B * T, buf.shape[-1])[:, :V]
        ops.linear_nt(x2, w_, l2, bias=b_, prec=prec)
        ws = ops.ctc_workspace(B, T, labels.shape[1], enc.device)
        costs = ops.ctc_loss_fwd(logits, labels, act_lens, label_lens, blank, ws)
        need = grad_mode and any(ctx.needs_input_grad[:3])
        scale = 1.0 / B if reduction == "mean" else 1.0
        if need:
            one = torch.ones(1, dtype=torch.float32, device=enc.device)
            ops.ctc_loss_bwd(logits, labels, act_lens, label_lens, blank, ws, one, 0, scale, inplace=True)      # l2 now holds d loss / d logits
            denc, gw, gb = torch.empty_like(enc), torch.empty_like(w_), torch.empty_like(b_)
            ops.linear_nn(l2, w_, denc.view(B * T, d), prec=prec)
            ops.linear_tn(l2, x2, gw, prec=prec, accumulate=False)
            ops.linear_tn(l2, torch.ones(B * T, 1, dtype=torch.float32, device=enc.device), gb, prec=prec, accumulate=False)
            ctx.save_for_backward(denc, gw, gb)
        ctx.params = (w, b)
        if reduction == "none":
            return costs
        return costs.sum().reshape(1) * scale

    @staticmethod
    def backward(ctx, gout):
        denc, *gs = ctx.saved_tensors
        gout = gout.float()
        if gout.numel() != 1:
            raise NotImplementedError("fused CTC head + loss: per-utterance upstream gradients (reduction='none') are not supported; "
                                      "use model.ctc_head(enc_state) + ttmi.ctc.ctc_loss(reduction='none')")
        rets = _scaled_param_grads(ctx.params, gs, gout)
        return (denc * gout, *rets, None, None, None, None, None, None, None)


def _joint_align(joint, enc, dec, labels, act_lens, label_lens, prec, chunk, blank, exp_state, stats, topology="rnnt"):
    """joint network + loss forward + forced alignment, forward only, chunked over utterances as _JointLossFn.forward chunks: per chunk
    ttmi_joint_fwd + ttmi_rnnt_loss_fwd + ttmi_rnnt_align (+ ttmi_rnnt_emit_stats), or, with `exp_state` (the JointNet's _ExpShift) valid
    and the sizes supported, ttmi_joint_fwd_exp + ttmi_rnnt_loss_fwd_exp + the same two calls; the chunk's logits / P buffer is dropped
    before the next chunk.  The exp-domain form leaves the training state alone: it only READS exp_state.cur (and only when the state is
    valid), passes no shift_next and raises a flag of its own; chunks whose flag came back set are run again in the plain form (one host
    read per call).  topology='monotonic': per chunk ttmi_joint_fwd + ttmi_mono_loss_fwd + ttmi_mono_align (+ ttmi_mono_emit_stats) on the
    one-decision-per-frame lattice; that lattice has no exp-domain branch.  -> warprnnt_pytorch.AlignResult"""
    from warprnnt_pytorch import AlignResult
    lat = ops.lattice(topology)
    if not lat.has_exp_forms and exp_state is not None:
        raise ValueError("topology='%s' has no exp-domain form" % lat.name)
    with torch.no_grad():
        enc, dec = enc.detach().contiguous(), dec.detach().contiguous()
        wf, bf, wp, bp = (t.detach() for t in (joint.forward_layer.weight, joint.forward_layer.bias, joint.project_layer.weight,
                                               joint.project_layer.bias))
        B, T, U1 = enc.shape[0], enc.shape[1], dec.shape[1]
        J, V = wf.shape[0], wp.shape[0]
        dev = enc.device
        frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        cost = torch.empty(B, dtype=torch.float32, device=dev)
        expected = torch.empty(B, U1 - 1, dtype=torch.float32, device=dev) if stats else None
        mass = torch.empty(B, U1 - 1, dtype=torch.float32, device=dev) if stats else None
        starts = list(range(0, B, chunk))
        use_exp = exp_state is not None and exp_state.valid
        flags = torch.zeros(len(starts), dtype=torch.int32, device=dev) if use_exp else None

        def run(i, exp):
            c0 = starts[i]
            c1 = min(B, c0 + chunk)
            n = c1 - c0
            lab, al, ll = labels[c0:c1], act_lens[c0:c1], label_lens[c0:c1]
            ws = lat.workspace(n, T, U1, dev)
            if exp:
                P, rowsum, saved, emis = ops.joint_fwd_exp(enc[c0:c1], dec[c0:c1], wf, bf, wp, bp, prec, exp_state.cur, lab.contiguous(), blank)
                cost[c0:c1] = ops.rnnt_loss_fwd_exp(P, rowsum, lab, al, ll, blank, ws, exp_state.cur, None, emis, flags[i:i + 1])
                del P, rowsum, saved, emis
            else:
                logits, saved = ops.joint_fwd(enc[c0:c1], dec[c0:c1], wf, bf, wp, bp, prec)
                cost[c0:c1] = lat.loss_fwd(logits, lab, al, ll, blank, ws)
                del logits, saved
            frames[c0:c1], score[c0:c1] = lat.align(ws, al, ll, n, T, U1)
            if stats:
                expected[c0:c1], mass[c0:c1] = lat.emit_stats(ws, al, ll, n, T, U1)

        ran_exp = []
        for i, c0 in enumerate(starts):
            exp = use_exp and ops.joint_exp_supported(min(B, c0 + chunk) - c0, T, U1, J, V, prec, fwd_only=True)
            run(i, exp)
            if exp:
                ran_exp.append(i)
        if ran_exp:
            bad = flags.cpu()                       # a row sum left the range of the shift in use: that chunk again, in the plain form
            for i in ran_exp:
                if int(bad[i]) != 0:
                    run(i, False)
    return AlignResult(frames, score, cost, expected, mass)


def deferred_logits_enabled(config, prec):
    """does Transducer.forward hand out a DeferredLogits handle?  TTMI_DEFERRED_LOGITS=0 / 1 (read per call, like TTMI_PRECISION) or
    config.deferred_logits (True / False) decide; unset: on in the bf16 pipeline (the throughput mode - its logits are 7 GB of bf16 per
    C2 step that train.py:51-53 only ever hands to the loss) and, since round 6, in the bf16x3 mode (14 GB of f32 logits and 14 GB of gradient:
    fused, the loss gradient leaves its kernel as the bf16 planes the joint's three-term backward multiplies - 98.5 -> 93.4 ms per C2 step), off in
    the fp32 parity mode."""
    env = os.environ.get("TTMI_DEFERRED_LOGITS")
    if env is not None and env != "":
        return env != "0"
    if config is not None and config.deferred_logits is not None:
        return bool(config.deferred_logits)
    return prec in (1, 2)


def _meta_functions():
    """Tensor methods / property getters a DeferredLogits answers from its own metadata, without producing the logits"""
    T = torch.Tensor
    fns = {T.size, T.dim, T.ndimension, T.numel, T.nelement, T.element_size, T.is_floating_point, T.is_complex, T.get_device, T.__len__}
    # (not stride / is_contiguous: the eager logits are a [..., :V] view of a pitched buffer - those come from the real tensor)
    for name in ("shape", "dtype", "device", "ndim", "is_cuda", "is_cpu", "layout", "is_sparse", "is_quantized", "is_meta", "is_nested",
                 "requires_grad", "itemsize", "names"):
        # (grad_fn / is_leaf / grad are NOT answered here: they are the real logits' autograd state - a caller that checks `logits.grad_fn`
        # must see the joint's node - so they materialise, with the one-time warning below when that costs gigabytes)
        fns.add(getattr(T, name).__get__)
    return frozenset(fns)


class DeferredLogits(torch.Tensor):
    """What `logits = model(inputs, targets)` (train.py:51, tt/model.py:58-68) returns in the bf16 pipeline: a tensor-shaped HANDLE on the
    two encoder states.  train.py:53 hands it to `RNNTLoss` unchanged, and the `warprnnt_pytorch` shim then runs joint + loss as ONE fused
    op on those states (`_JointLossFn`: the exp-domain form when its kernels take the sizes, else the chunked memory form) - the
    [B, T, U+1, V] logits (7.1 GB of bf16 per C2 step, written once and walked twice by the loss) are never formed, which is what
    `Transducer.loss(..., exp_domain=True)` does for callers that changed their code.

    Any OTHER use - arithmetic, indexing, `.float()`, `softmax`, printing, `.data_ptr()`, `.stride()`, `torch.save`, a different loss -
    materialises exactly the tensor `model.joint(enc_state, dec_state)` returns today (same autograd graph into the encoders, same bits;
    produced once and kept) and carries on with it, and a handle that has been materialised is consumed by `RNNTLoss` as an ordinary
    logits tensor.  Metadata (`shape`, `size()`, `dim()`, `dtype`, `device`, `is_cuda`, `numel()`, `len()`, `requires_grad`) is answered
    from the handle.  Implementation: a storage-less wrapper subclass (`Tensor._make_wrapper_subclass`) whose `__torch_function__`
    swaps the handle for the real logits before any function that is not a metadata query runs."""

    _warned_big = False

    @staticmethod
    def __new__(cls, joint, enc_state, dec_state, prec):
        B, T = enc_state.shape[0], enc_state.shape[1]
        U1 = dec_state.shape[1]
        J, V = joint.forward_layer.out_features, joint.project_layer.out_features
        grad_mode = torch.is_grad_enabled()
        needs = grad_mode and (enc_state.requires_grad or dec_state.requires_grad or any(p.requires_grad for p in joint.parameters()))
        self = torch.Tensor._make_wrapper_subclass(cls, (B, T, U1, V), dtype=ops.joint_logits_dtype(prec, J), device=enc_state.device,
                                                   requires_grad=bool(needs))
        self._joint, self._enc, self._dec, self._prec, self._grad_mode, self._real = joint, enc_state, dec_state, prec, grad_mode, None
        if needs:
            # a gradient that arrives at the HANDLE (a caller below the Python API recorded it as an autograd input, e.g. a foreign
            # autograd.Function applied to it directly) belongs to the real logits: pass it on into their graph
            with torch._C.DisableTorchFunctionSubclass():
                torch.Tensor.register_hook(self, self._forward_gradient)
        return self

    def __init__(self, *args, **kwargs):
        pass

    def _forward_gradient(self, grad):
        if self._real is not None and self._real.requires_grad:
            torch.autograd.backward(self._real, grad)
        return None

    @property
    def is_materialized(self):
        return self._real is not None

    def _produce(self):
        j = self._joint
        ops.weights_fresh()
        return _JointFn.apply(self._enc, self._dec, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight,
                              j.project_layer.bias, self._prec)

    def materialize(self):
        """-> the real logits (produced on first use under the grad mode of the forward call that made the handle, then kept)"""
        if self._real is None:
            nbytes = self.numel() * self.element_size()
            if nbytes >= (1 << 30) and not DeferredLogits._warned_big:
                import warnings
                DeferredLogits._warned_big = True
                warnings.warn("DeferredLogits: a use other than RNNTLoss / shape queries is forming the real [B, T, U+1, V] logits (%.1f GB, kept "
                              "for the life of the handle); pass the handle straight to RNNTLoss to stay on the fused path, or set "
                              "TTMI_DEFERRED_LOGITS=0 if the logits are wanted anyway" % (nbytes / 2.0 ** 30))
            with torch.set_grad_enabled(self._grad_mode):
                self._real = self._produce()
        return self._real

    def rnnt_loss(self, labels, act_lens, label_lens, blank=0, reduction="mean", *, fastemit_lambda=0.0, topology="rnnt"):
        """the loss of train.py:53 on this handle's logits without forming them (called by warprnnt_pytorch.rnnt_loss; arguments already
        certified there).  None when this case has to go through the real logits (per-utterance costs that need gradients)."""
        if getattr(self._joint, "tdt_durations", None) is not None:
            raise ValueError("TDT: RNNTLoss on the logits of a token-and-duration model is not built (its rows are V + D wide): use "
                             "ttmi.tdt.TDTLoss or Transducer.loss")
        if self._real is not None:
            return None
        grad = self._grad_mode and torch.is_grad_enabled()
        if reduction == "none" and grad and self.requires_grad:
            return None                     # per-utterance upstream gradients cannot be folded into weight gradients formed in the forward pass
        j = self._joint
        B, T, U1 = self.shape[0], self.shape[1], self.shape[2]
        ops.weights_fresh()
        # (a lattice without the exp-domain form: the plain chunk form, at the memory form's chunk size)
        exp = ops.lattice(topology).has_exp_forms and self._prec == 1 and os.environ.get("TTMI_DEFERRED_EXP", "1") != "0"
        chunk = j.default_loss_chunk(B, T, U1, exp, self._prec)
        if exp and not ops.joint_exp_supported(chunk, T, U1, j.forward_layer.out_features, j.project_layer.out_features, self._prec,
                                               fwd_only=not (grad and self.requires_grad)):
            # the exp-domain kernels do not take this problem: the plain fused form runs, and ITS chunk is the memory form's (about 2 GB of
            # logits per chunk, not the 32 GB budget of the form that never holds them)
            chunk = j.default_loss_chunk(B, T, U1, False, self._prec)
        return _JointLossFn.apply(self._enc, self._dec, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight,
                                  j.project_layer.bias, labels, act_lens, label_lens, self._prec, int(chunk), reduction,
                                  j.exp_shift_state(self._enc.device) if exp else None, grad, int(blank), fastemit_lambda, None, topology)

    def rnnt_align(self, labels, act_lens, label_lens, blank=0, *, stats=False, topology="rnnt"):
        """forced alignment on this handle's logits without forming them (called by warprnnt_pytorch.rnnt_align; arguments already
        certified there): the chunked forward-only loop of Transducer.align.  None when the handle was already used as a tensor (the
        caller then aligns the real logits).  topology='monotonic': the same loop on the one-decision-per-frame lattice, in the plain
        chunk form at the memory form's chunk size (no exp-domain branch)."""
        if getattr(self._joint, "tdt_durations", None) is not None:
            raise ValueError("TDT: forced alignment is not built for a token-and-duration model")
        if self._real is not None:
            return None
        j = self._joint
        B, T, U1 = self.shape[0], self.shape[1], self.shape[2]
        ops.weights_fresh()
        exp = ops.lattice(topology).has_exp_forms and self._prec == 1 and os.environ.get("TTMI_DEFERRED_EXP", "1") != "0"
        st = j.exp_shift_state(self._enc.device) if exp else None
        exp = exp and st.valid
        chunk = j.default_loss_chunk(B, T, U1, exp, self._prec)
        if exp and not ops.joint_exp_supported(chunk, T, U1, j.forward_layer.out_features, j.project_layer.out_features, self._prec, fwd_only=True):
            exp, chunk = False, j.default_loss_chunk(B, T, U1, False, self._prec)
        return _joint_align(j, self._enc, self._dec, labels, act_lens, label_lens, self._prec, int(chunk), int(blank), st if exp else None,
                            stats, topology)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func in _META_FUNCTIONS:
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)

        def real(a):
            if isinstance(a, DeferredLogits):
                return a.materialize()
            if isinstance(a, (list, tuple)):
                return type(a)(real(x) for x in a)
            return a
        with torch._C.DisableTorchFunctionSubclass():
            return func(*real(args), **{k: real(v) for k, v in kwargs.items()})

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        # reached only by callers below the Python API (the handle has no storage): give them the real values.  Those values are
        # DETACHED - a foreign op applied at this level to a handle that needs gradients would silently cut the encoders off the graph,
        # so that case raises (grad mode on and the handle requires grad); inference / no_grad callers get the values
        import torch.utils._pytree as pytree

        def real(a):
            if a.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("DeferredLogits reached %s below the Python API while it requires grad: the op would run on detached "
                                   "logits and lose the gradient into the encoders.  Call logits.materialize() first (or set "
                                   "TTMI_DEFERRED_LOGITS=0)" % (func,))
            return a.materialize().detach()
        args, kwargs = pytree.tree_map_only(DeferredLogits, real, (args, kwargs or {}))
        return func(*args, **kwargs)


_META_FUNCTIONS = _meta_functions()


DecodeResult = collections.namedtuple("DecodeResult", ["tokens", "frames", "logprobs", "score"])
DecodeResult.__doc__ = """What greedy decoding returns per utterance with details=True (decode / decode_batch / recognize): `tokens` (list of int, what
details=False returns), `frames` (list of int, the frame at which each token was emitted: strictly increasing, < T_b), `logprobs` (list of float,
log P(token) on its emission frame) and `score` (float): the log-probability of the decisions the greedy decoder took, one term per frame of the
utterance - blank's log-probability against the label state current at that frame on a frame that does not emit, the token's on a frame that does.
That is the path of this decoder (at most one symbol per frame, the emitting frame is consumed), NOT a path of the RNN-T lattice, which follows a
label with a blank on the same frame: `score` is not comparable with `Transducer.align(...).score` on the default topology.  It IS a path of the
monotonic lattice: `Transducer.align_monotonic(inputs, ..., tokens, ...).score` is its upper bound, and equal to it where `frames` are
the aligned frames.
Beam decoding (beam_decode_batch / recognize_nbest) returns lists of the same type on the same probability model: there `score` is the log of the summed
probability of every decision sequence the beam kept for `tokens` (hypotheses spelling the same tokens are merged), `frames` and `logprobs` those of the
best single one of them."""


MWERDetails = collections.namedtuple("MWERDetails", ["hypotheses", "errors", "posteriors", "costs", "expected_errors"])
MWERDetails.__doc__ = """What Transducer.mwer_loss(details=True) returns beside the loss: `hypotheses` (the token lists used, per utterance), and over the rows
of the call (hypothesis rows utterance by utterance, then one transcript row per utterance when rnnt_weight > 0) `errors` (i32, edit distance to
the transcript), `posteriors` (f64, softmax of -cost within the utterance; 0 on a transcript row) and `costs` (f32, RNN-T lattice cost);
`expected_errors` (f64 [B]) = sum_i P_i W_i per utterance."""


class JointNet(nn.Module):
    """logits = project_layer(tanh(forward_layer(cat(enc, dec)))) evaluated in split-weight form
    (forward_layer.weight = [W_enc | W_dec]); accepts [B,T,de]/[B,U,dd] (lattice) or two 1-D vectors (decode)."""

    def __init__(self, input_size, inner_dim, vocab_size):
        super().__init__()
        self.forward_layer = nn.Linear(input_size, inner_dim, bias=True)
        self.tanh = nn.Tanh()
        self.project_layer = nn.Linear(inner_dim, vocab_size, bias=True)
        self._register_load_state_dict_pre_hook(self._new_weights)

    def _new_weights(self, *args):
        """load_state_dict: the logits' scale is unknown again - the exp-domain loss form re-seeds its shift at the next step"""
        for st in self.__dict__.get("_exp_shift", {}).values():
            st.valid = False

    def forward(self, enc_state, dec_state):
        ops.weights_fresh()
        if enc_state.dim() == 3 and dec_state.dim() == 3:
            squeeze = None
        else:
            assert enc_state.dim() == dec_state.dim()
            squeeze = enc_state.shape[:-1]
            enc_state = enc_state.reshape(-1, 1, enc_state.shape[-1])     # N vectors -> N lattices of 1 x 1
            dec_state = dec_state.reshape(-1, 1, dec_state.shape[-1])
        out = _JointFn.apply(enc_state, dec_state, self.forward_layer.weight, self.forward_layer.bias,
                             self.project_layer.weight, self.project_layer.bias, default_precision())
        return out if squeeze is None else out.reshape(*squeeze, out.shape[-1])

    def exp_shift_state(self, device):
        """this module's range-control state of the exp-domain loss form on `device` (_ExpShift; created on first use, not part of
        state_dict)"""
        states = self.__dict__.setdefault("_exp_shift", {})
        st = states.get(device)
        if st is None:
            st = states[device] = _ExpShift(device)
        return st

    def default_loss_chunk(self, B, T, U1, exp_domain=False, prec=None):
        """utterances per chunk of the fused joint + loss: about 2 GB of logits (the memory-saving form) or 32 GB (exp_domain: the speed
        form - every chunk boundary costs a pipeline fill of the three big GEMMs and one more lattice launch: C2 whole batch 35.0 ms per
        step, two halves 36.2; C5's 28 GB in one chunk 102.0 ms, in two 104.2 - on 288 GB of HBM the budget is not the constraint).  The
        chunks are balanced (B = 33 at a budget of 32 gives 17 + 16, not 32 + 1: every chunk stays above the persistent kernels' minimum
        row count).  Any row count runs the exp-domain kernels: the library pads the wgrad's reduction to its 64-row tile (round 3 needed
        chunk * T * U1 % 64 == 0 and fell back to the plain form otherwise - half of all real batches at B = 32).  With distillation
        (`loss(distill=...)`) a second chunk buffer, the out-of-place gradient, is alive beside the logits; the 2 GB budget leaves room for it
        and the chunk size is the same."""
        prec = default_precision() if prec is None else prec
        es = 2 if ops.joint_logits_dtype(prec, self.forward_layer.out_features) is torch.bfloat16 else 4
        budget = (32 << 30) if (exp_domain or prec == 2) else (2 << 30)     # (bf16x3: the speed form as well - C2 in eight chunks 108 ms, in one 93.4)
        chunk = max(1, min(B, int(budget // (es * T * U1 * self.project_layer.out_features))))
        n = -(-B // chunk)
        return -(-B // n)


class _LabelStateGraphs:
    """Greedy decoding re-runs the label encoder on the whole token history after every emitted symbol (tt/model.py:75,88 of the
    reference): ~100 tiny launches whose cost is the host issuing them.  One captured graph per history length L replays them with a
    single launch; the token histories live on the device (`master` [B, MAX_L]), each graph reads its own static copy and writes a static
    output.  B = 1: `Transducer.decode` (one utterance); B > 1: `Transducer.decode_batch` (every utterance of a batch in lockstep: all
    histories have the same length).  Graphs are captured lazily, share one memory pool and are dropped when the label encoder's
    parameter storage or the precision mode changes."""
    MAX_L = 128

    def __init__(self, model, device, batch=1):
        self.decoder, self.device, self.batch = model.decoder, device, batch
        self.master = torch.zeros(batch, self.MAX_L, dtype=torch.long, device=device)
        self.stream = torch.cuda.Stream(device)
        self.pool = torch.cuda.graph_pool_handle()
        self.graphs = {}
        self.key = self.weights_key(model)
        # every captured graph bakes in the address of this stream's scratch arena (ttmi.ops.scratch), which is re-allocated when a
        # longer history needs more: size it for MAX_L before the first capture, and drop the graphs should it ever move all the same
        cur = torch.cuda.current_stream(device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.decoder(torch.zeros(batch, self.MAX_L, dtype=torch.long, device=device))
        cur.wait_stream(self.stream)
        self.arena = ops.scratch_generation(device, self.stream)

    @staticmethod
    def weights_key(model):
        return tuple(p.data_ptr() for p in model.decoder.parameters()) + (default_precision(),)

    def set_token(self, pos, tok):
        self.master[0, pos] = tok                                   # a device fill, no synchronisation

    def state(self, L):
        """label-encoder output at the last position of master[:, :L] -> [B, 1, d] (static buffer of graph L)"""
        if ops.scratch_generation(self.device, self.stream) != self.arena:      # the arena moved: every graph points at freed memory
            self.graphs.clear()
            self.arena = ops.scratch_generation(self.device, self.stream)
        entry = self.graphs.get(L)
        if entry is None:
            tok = self.master[:, :L].clone()
            cur = torch.cuda.current_stream(self.device)
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                for _ in range(2):                                  # warm-up outside the capture: scratch arenas, kernel attributes
                    self.decoder(tok)
            cur.wait_stream(self.stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=self.pool, stream=self.stream):
                out = self.decoder(tok)[:, -1:, :].clone()       # (keeps [B, 1, d] alive per graph, not the stack's whole [B, L, d] output)
            assert ops.scratch_generation(self.device, self.stream) == self.arena, "scratch arena grew during a capture"
            entry = self.graphs[L] = (graph, tok, out)
        graph, tok, out = entry
        tok.copy_(self.master[:, :L])
        graph.replay()
        return out


class Transducer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.encoder = BuildEncoder(config)
        self.decoder = BuildDecoder(config)
        # token-and-duration transducer (ttmi.tdt; config.tdt_durations absent, None or empty: today's module, state_dict and bits): the joint's
        # projection gets D more rows, the duration logits, behind the vocab_size token rows
        self.tdt_durations = ops.check_durations(config.tdt_durations) if config.tdt_durations else None
        self.joint = JointNet(input_size=config.joint.input_size, inner_dim=config.joint.inner_size,
                              vocab_size=config.vocab_size + len(self.tdt_durations or ()))
        if self.tdt_durations is not None:
            self.joint.tdt_durations = self.tdt_durations      # (a DeferredLogits handle knows its joint only: RNNTLoss on it is refused)
        if config.share_embedding:
            # the reference's branch dereferences self.decoder.embedding, which does not exist (tt/model.py:53-56)
            raise AttributeError("'BuildDecoder' object has no attribute 'embedding' (share_embedding is broken upstream)")
        # optional auxiliary CTC head on the audio encoder's output (joint CTC - transducer training; config.ctc_weight absent, None or 0:
        # no head, the module and its state_dict are the reference's)
        self.ctc_weight = float(config.ctc_weight or 0.0)
        if self.ctc_weight < 0.0:
            raise ValueError("config.ctc_weight must be >= 0, got %r" % (config.ctc_weight,))
        if self.ctc_weight > 0.0:
            self.ctc_head = nn.Linear(config.enc.d_model, config.vocab_size)

    def forward(self, inputs, targets):
        """-> logits [B, T, U+1, V] (tt/model.py:58-68).  In the bf16 pipeline the return value is a DeferredLogits handle on the two
        encoder states: `RNNTLoss` (train.py:53) consumes it through the fused joint + loss kernels, anything else makes it produce
        the real logits first - train.py:51-53 runs unchanged and on the fast path (deferred_logits_enabled for the switches)."""
        enc_state, dec_state = self._encode(inputs, targets)
        if self.ctc_weight > 0.0:
            # the two-call form (train.py:51-53) reaches the head's input through here: ctc_loss_from_last_forward() consumes and releases it
            self.__dict__["_ctc_states"] = enc_state
        prec = default_precision()
        if enc_state.is_cuda and deferred_logits_enabled(self.config, prec):
            return DeferredLogits(self.joint, enc_state, dec_state, prec)
        return self.joint(enc_state, dec_state)

    def loss(self, inputs, inputs_length, targets, targets_length, reduction="mean", chunk=None, check_lengths=True, exp_domain=False, *,
             fastemit_lambda=0.0, ctc_weight=None, utterance_weights=None, topology="rnnt", distill=None, distill_weight=0.0):
        """Opt-in fused form of train.py:51-53 (`logits = model(inputs, targets); loss = criterion(logits, targets.int(),
        inputs_length.int(), targets_length.int())`) that never materialises the logits (API precedent: tt_espnet/model.py:35-81 returns
        the loss from forward).  Same numbers as the two-call form: the same kernels run, one chunk of `chunk` utterances at a time
        (default: about 2 GB of logits per chunk, adjusted to a row count the persistent wgrad kernel takes), and the chunk's buffer is overwritten by its gradient and consumed by the
        joint's backward before the next chunk starts.  Returns the loss ([1] for 'mean' / 'sum', [B] for 'none').

        exp_domain=True (bf16 mode, training-sized chunks; silently the form above otherwise): the projection stores exp(logit - shift) and
        per-row sums, so the loss never walks the lattice's rows and its gradient is consumed in factored form (include/ttmi.h).  Same
        loss and gradients up to bf16 rounding of different intermediates (tests/test_fused_loss_gpu.py states the tolerance).  The first
        call on a module (and the first after its joint weights were replaced) runs the form above and seeds the shift on the device
        (_ExpShift): no host synchronisation.

        fastemit_lambda: FastEmit regularisation of the gradient, as in warprnnt_pytorch.RNNTLoss (the loss value is unchanged).

        ctc_weight (None: config.ctc_weight): > 0 returns rnnt + ctc_weight * ctc, the CTC loss of the auxiliary head (`ctc_head`, built when
        config.ctc_weight > 0) on the same audio-encoder states - the encoder runs once.  ValueError on a module without the head.

        utterance_weights (None: today's code path and bits): an f32 / f64 tensor [B] on the device, one constant factor per utterance (no
        gradient flows into it; zero and negative entries are allowed).  The transducer term becomes sum_b w_b cost_b for 'sum' and that
        over B for 'mean'; its gradient is formed in the forward pass as always, each chunk's loss-gradient kernel reading its slice of w
        (all three chunk forms).  ValueError with reduction='none'.  The CTC term, when asked for, is not weighted.

        topology ('rnnt': today's code path and bits): 'monotonic' trains the one-decision-per-frame lattice the decoders of this class walk
        (warprnnt_pytorch.RNNTLoss has the same option) in the plain chunk form; ValueError together with exp_domain=True or
        fastemit_lambda > 0, and, under check_lengths, for an utterance with more labels than frames.

        distill, distill_weight (None, or a weight of 0: today's code path and bits): knowledge distillation from a teacher on collapsed
        lattice posteriors (ttmi.distill).  `distill` is what the teacher's `lattice_posteriors` returned for the same batch, a constant f32
        [B, T, U+1, 3] on the device; the call returns rnnt + distill_weight * KD with the reduction of the transducer term, KD being the KL
        divergence from the teacher's (blank, next label, other) probabilities to the student's, summed over each utterance's lattice nodes.
        Both topologies and FastEmit are supported.  Like the CTC term, the KD term is not multiplied by utterance_weights.  Per chunk the
        transducer gradient is written out of place and the KD gradient added to it, so a second chunk buffer is alive meanwhile:
        default_loss_chunk's 2 GB budget leaves room for it and the chunk size is unchanged.  ValueError together with exp_domain=True (the
        collapsed classes have no exp-domain form), for a distill_weight that is not a finite number >= 0, and for a `distill` of another
        shape, dtype or device."""
        from warprnnt_pytorch import check_lengths as certify, check_monotonic_lengths as monotonic_lengths
        fastemit_lambda = ops.check_fastemit(fastemit_lambda)
        if self.tdt_durations is not None:
            # token-and-duration model: the plain chunk form on its own lattice (joint_fwd, tdt_loss_fwd, tdt_loss_bwd in place, joint_bwd);
            # ctc_weight and utterance_weights live outside the lattice and work as always
            if topology != "rnnt":
                raise self._tdt_not_built("loss(topology=%r)" % (topology,))
            if exp_domain:
                raise self._tdt_not_built("the exp-domain loss form")
            if fastemit_lambda > 0.0:
                raise self._tdt_not_built("FastEmit")
            if distill is not None and self._distill_weight(distill_weight) != 0.0:
                raise self._tdt_not_built("distillation")
            lat = topology = ops.TDTLattice(self.tdt_durations)
        else:
            lat = ops.lattice(topology, fastemit_lambda)
        if exp_domain and not lat.has_exp_forms:
            raise ValueError("topology='%s' has no exp-domain form: leave exp_domain off" % lat.name)
        distill_weight = self._distill_weight(distill_weight)
        if distill is None or distill_weight == 0.0:
            distill, distill_weight = None, 0.0
        elif exp_domain:
            raise ValueError("distill has no exp-domain form: leave exp_domain off")
        ctc_weight = self._ctc_weight(ctc_weight)
        if utterance_weights is not None:
            utterance_weights = self._utterance_weights(utterance_weights, inputs.shape[0], reduction)
        enc_state, dec_state = self._encode(inputs, targets)
        B, T, U1 = enc_state.shape[0], enc_state.shape[1], dec_state.shape[1]
        labels, al, ll = (t.to(device=enc_state.device, dtype=torch.int32).contiguous() for t in (targets, inputs_length, targets_length))
        certify(labels, al, ll, B, T, U1, check_lengths)
        if lat.label_takes_frame and check_lengths:
            try:
                monotonic_lengths(al, ll)            # ValueError for an utterance with more labels than frames
            except ValueError:
                if self.tdt_durations is None:
                    raise
                raise ValueError("TDT: an utterance has more labels than frames (label_lengths > lengths)") from None
        ops.weights_fresh()
        prec = default_precision()
        if chunk is None:
            chunk = self.default_loss_chunk(B, T, U1, exp_domain)
        j = self.joint
        if distill is not None:
            from ttmi.distill import check_teacher
            distill = check_teacher(distill, B, T, U1)
        rnnt = _JointLossFn.apply(enc_state, dec_state, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight,
                                  j.project_layer.bias, labels, al, ll, prec, int(chunk), reduction,
                                  j.exp_shift_state(enc_state.device) if exp_domain and prec == 1 else None, torch.is_grad_enabled(), 0,
                                  fastemit_lambda, utterance_weights, topology, distill, distill_weight)
        if ctc_weight > 0.0:
            return rnnt + ctc_weight * self._ctc_from_states(enc_state, labels, al, ll, reduction)
        return rnnt

    @staticmethod
    def _tdt_not_built(what):
        """the error of every entry point that is not built for a token-and-duration model (config.tdt_durations)"""
        from ttmi.tdt import not_built
        return not_built(what)

    def _refuse_tdt(self, what):
        if self.tdt_durations is not None:
            raise self._tdt_not_built(what)

    @staticmethod
    def _distill_weight(w):
        """-> distill_weight as a float; ValueError unless it is a finite number >= 0"""
        try:
            v = float(w)
        except (TypeError, ValueError):
            raise ValueError("distill_weight must be a finite float >= 0, got %r" % (w,)) from None
        if not math.isfinite(v) or v < 0.0:
            raise ValueError("distill_weight must be a finite float >= 0, got %r" % (w,))
        return v

    def lattice_posteriors(self, inputs, inputs_length, targets, targets_length, chunk=None, check_lengths=True):
        """The teacher's call of knowledge distillation on collapsed lattice posteriors (ttmi.distill; `loss(distill=...)` is the student's):
        -> f32 [B, T, U+1, 3], (log P(blank), log P(y_{u+1}), log P(anything else)) at every lattice node of (inputs, targets), exact zeros
        outside the ragged lattice.  Under no_grad, without materialising the logits: per chunk of `loss()`'s plain form joint_fwd then
        kd_collapse, and the chunk's logits are dropped before the next chunk.  12 bytes per node (9.8 MB for a whole C2 batch): it can be
        computed once per utterance and cached.  The encoders run in whatever mode the module is in: call it in eval() mode."""
        self._refuse_tdt("lattice_posteriors / distillation")
        from warprnnt_pytorch import check_lengths as certify
        labels, al, ll = (t.to(dtype=torch.int32) for t in (targets, inputs_length, targets_length))
        certify(labels.contiguous(), al.contiguous(), ll.contiguous(), inputs.shape[0], 0, targets.shape[1] + 1, False)
        if not inputs.is_cuda:
            raise ValueError("Transducer.lattice_posteriors: inputs must live on the GPU (the MI355X build has no CPU path)")
        with torch.no_grad():
            enc_state, dec_state = self._encode(inputs, targets)
            B, T, U1 = enc_state.shape[0], enc_state.shape[1], dec_state.shape[1]
            labels, al, ll = (t.to(device=enc_state.device).contiguous() for t in (labels, al, ll))
            certify(labels, al, ll, B, T, U1, check_lengths)
            ops.weights_fresh()
            prec = default_precision()
            if chunk is None:
                chunk = self.default_loss_chunk(B, T, U1, False)
            chunk = int(chunk)
            enc, dec = enc_state.detach().contiguous(), dec_state.detach().contiguous()
            j = self.joint
            wf, bf, wp, bp = (t.detach() for t in (j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias))
            post = torch.empty(B, T, U1, 3, dtype=torch.float32, device=enc.device)
            for c0 in range(0, B, chunk):
                c1 = min(B, c0 + chunk)
                logits, saved = ops.joint_fwd(enc[c0:c1], dec[c0:c1], wf, bf, wp, bp, prec)
                post[c0:c1] = ops.kd_collapse(logits, labels[c0:c1], al[c0:c1], ll[c0:c1], 0)
                del logits, saved
        return post

    @staticmethod
    def _utterance_weights(w, B, reduction):
        """the per-utterance weights of `loss` as the kernels read them: a detached, dense f32 [B] on the device"""
        if reduction == "none":
            raise ValueError("utterance_weights need reduction='mean' or 'sum' (per-utterance costs are not weighted)")
        if not isinstance(w, torch.Tensor) or w.dtype not in (torch.float32, torch.float64) or tuple(w.shape) != (B,):
            raise ValueError("utterance_weights must be an f32 / f64 tensor of shape [%d]" % B)
        if not w.is_cuda:
            raise ValueError("utterance_weights must live on the GPU (the MI355X build has no CPU path)")
        return w.detach().to(torch.float32).contiguous()

    def _ctc_weight(self, ctc_weight):
        """the weight a call uses: None -> the config's; ValueError for a negative one, or a positive one on a module without the head"""
        w = self.ctc_weight if ctc_weight is None else float(ctc_weight)
        if not w >= 0.0:
            raise ValueError("ctc_weight must be >= 0, got %r" % (ctc_weight,))
        if w > 0.0 and getattr(self, "ctc_head", None) is None:
            raise ValueError("ctc_weight = %g on a Transducer without a CTC head: build it with config.ctc_weight > 0" % w)
        return w

    def _ctc_from_states(self, enc_state, labels, act_lens, label_lens, reduction):
        """CTC loss of the head on audio-encoder states [B, T, d] (head projection, loss and their backward as one op: _CTCHeadLossFn)"""
        if getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        if not enc_state.is_cuda:
            raise ValueError("Transducer.ctc_loss: inputs must live on the GPU (the MI355X build has no CPU path)")
        labels, act_lens, label_lens = (t.to(device=enc_state.device, dtype=torch.int32).contiguous() for t in (labels, act_lens, label_lens))
        ops.weights_fresh()
        return _CTCHeadLossFn.apply(enc_state, self.ctc_head.weight, self.ctc_head.bias, labels, act_lens, label_lens, default_precision(),
                                    reduction, torch.is_grad_enabled(), 0)

    def mwer_loss(self, inputs, inputs_length, targets, targets_length, *, beam_width=4, nbest=None, rnnt_weight=0.0, hypotheses=None,
                  chunk=None, fastemit_lambda=0.0, details=False, topology="rnnt"):
        """Minimum word error rate training on the N-best list (Prabhavalkar et al. 2018; Guo et al. 2020 for RNN-T), on tokens: utterance b
        has the distinct hypotheses y_1 .. y_n; c_i = the RNN-T lattice cost of (x_b, y_i), as loss(reduction='none') gives it;
        P_i = softmax_i(-c_i) in float64; W_i = the edit distance of y_i to the transcript; E_b = sum_i P_i W_i.  Returns, as an f64 [1],
            mean_b E_b + rnnt_weight * mean_b c(x_b, transcript_b)
        whose gradient is that of sum_r w_r c_r over the rows r of the call with the CONSTANT weights w = -P_i (W_i - E_b) / B on a hypothesis
        row (ttmi.metrics.mwer_weights) and rnnt_weight / B on a transcript row.

        hypotheses=None: the N-best of `beam_decode_batch(beam_width, nbest)` on the detached audio states, under no_grad and in eval mode
        (self.training is restored afterwards); else a list of token lists per utterance (ValueError for a duplicate within an utterance, an
        utterance without a hypothesis, a token outside [0, V)).  An empty hypothesis ([]) is an ordinary row; an utterance with one
        hypothesis adds its W_1 to the value and nothing to the gradient.

        The audio encoder runs once, with gradient; its states are gathered per row (index_select: their gradients add back per utterance),
        the label encoder runs on the row table (ragged: hypothesis rows b-major, then one transcript row per utterance when rnnt_weight > 0).
        W comes from ttmi.metrics.edit_distance on the device.  Then two passes of the fused, chunked joint + loss over the same states:
        pass 1 under no_grad gives c, pass 2 with utterance_weights = w forms the gradient - the [rows, T, U+1, V] logits never exist, one
        chunk of `chunk` ROWS at a time (default: default_loss_chunk of the row count).  fastemit_lambda acts on pass 2's gradient.

        topology ('rnnt' / 'monotonic', as in `loss`) is the lattice of both passes: with 'monotonic' the hypothesis costs c_i are taken on the
        lattice whose path sums ranked the N-best (the beam search's merged scores).  A hypothesis of the beam search never has more tokens
        than its utterance has frames; hypotheses passed in must not either (such a row has no path on this lattice: its cost is +inf).

        details=True: -> (loss, MWERDetails(hypotheses, errors i32 [rows], posteriors f64 [rows], costs f32 [rows], expected_errors f64 [B]));
        the per-row fields cover the whole row table: transcript rows carry errors 0 and posterior 0."""
        from ttmi import metrics
        self._refuse_tdt("MWER training (mwer_loss)")
        fastemit_lambda = ops.check_fastemit(fastemit_lambda)
        ops.check_topology(topology, fastemit_lambda)
        rnnt_weight = float(rnnt_weight)
        if not rnnt_weight >= 0.0:
            raise ValueError("mwer_loss: rnnt_weight must be >= 0, got %r" % (rnnt_weight,))
        if not (inputs.is_cuda and targets.is_cuda):
            raise ValueError("Transducer.mwer_loss: inputs and targets must live on the GPU (the MI355X build has no CPU path)")
        dev, B, V = inputs.device, inputs.shape[0], self.config.vocab_size
        enc_state = self.encoder(inputs, self._audio_mask(inputs))
        if hypotheses is None:
            was_training = self.training
            self.eval()
            try:
                with torch.no_grad():
                    nb = self.beam_decode_batch(enc_state.detach(), inputs_length, beam_width=beam_width, nbest=nbest)
            finally:
                self.train(was_training)
            hypotheses = [[list(h.tokens) for h in res] for res in nb]
        else:
            hypotheses = [[[int(t) for t in h] for h in hs] for hs in hypotheses]
            if len(hypotheses) != B:
                raise ValueError("mwer_loss: %d hypothesis lists for %d utterances" % (len(hypotheses), B))
        for b, hs in enumerate(hypotheses):
            if not hs:
                raise ValueError("mwer_loss: utterance %d has no hypothesis" % b)
            if len({tuple(h) for h in hs}) != len(hs):
                raise ValueError("mwer_loss: utterance %d holds the same hypothesis twice" % b)
            if any(not 0 <= t < V for h in hs for t in h):
                raise ValueError("mwer_loss: utterance %d has a token outside [0, %d)" % (b, V))
        # the row table.  The label matrix is padded with 0 to the longest row and to ONE column at least: the loss kernels take a label
        # pointer, which a [rows, 0] tensor does not have, so a call whose rows are all empty runs with U + 1 = 2 and label_lens = 0
        # (hence check_lengths=False: max(label_lens) + 1 need not be U + 1 here, nor max(act_lens) T)
        flat = [h for hs in hypotheses for h in hs]
        n_hyp, n_max = len(flat), max(len(hs) for hs in hypotheses)
        with_ref = rnnt_weight > 0.0
        U = max([1] + [len(h) for h in flat] + ([targets.shape[1]] if with_ref else []))
        host = np.zeros((n_hyp, U + 2), dtype=np.int64)                   # [labels | length | utterance]: one upload
        k = 0
        for b, hs in enumerate(hypotheses):
            for h in hs:
                host[k, :len(h)], host[k, U], host[k, U + 1] = h, len(h), b
                k += 1
        table = torch.from_numpy(host).to(dev)
        labels, ll, row_utt = table[:, :U], table[:, U], table[:, U + 1]
        tl = targets_length.to(device=dev, dtype=torch.long)
        if with_ref:
            tgt = F.pad(targets.long(), [0, U - targets.shape[1]])
            tgt = tgt * (torch.arange(U, device=dev)[None, :] < tl[:, None])
            labels, ll, row_all = torch.cat([labels, tgt]), torch.cat([ll, tl]), torch.cat([row_utt, torch.arange(B, device=dev)])
        else:
            row_all = row_utt
        rows = labels.shape[0]
        labels32, ll32 = labels.to(torch.int32).contiguous(), ll.to(torch.int32).contiguous()
        errors = metrics.edit_distance(labels32, ll32, targets, tl, row_all).distance          # W, on the device: no host read
        dec_rows = self._label_states(F.pad(labels, pad=[1, 0, 0, 0], value=0))
        enc_rows = enc_state.index_select(0, row_all)
        al32 = inputs_length.to(device=dev, dtype=torch.int32)[row_all].contiguous()
        T, U1 = enc_rows.shape[1], dec_rows.shape[1]
        ops.weights_fresh()
        prec = default_precision()
        chunk = self.default_loss_chunk(rows, T, U1) if chunk is None else int(chunk)
        j = self.joint

        def fused(reduction, grad, fe, w):
            return _JointLossFn.apply(enc_rows, dec_rows, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight,
                                      j.project_layer.bias, labels32, al32, ll32, prec, int(chunk), reduction, None, grad, 0, fe, w, topology)
        with torch.no_grad():
            costs = fused("none", False, 0.0, None)                                               # pass 1
        wt = metrics.mwer_weights(costs[:n_hyp], errors[:n_hyp], row_utt, B, max_per_utt=n_max)
        value = wt.expected_errors.mean()
        w, post = wt.weights, wt.posteriors
        if with_ref:
            value = value + rnnt_weight * costs[n_hyp:].double().mean()
            w = torch.cat([w, torch.full((B,), rnnt_weight / B, dtype=torch.float64, device=dev)])
            post = torch.cat([post, torch.zeros(B, dtype=torch.float64, device=dev)])
        out = value.reshape(1)
        if torch.is_grad_enabled():
            weighted = fused("sum", True, fastemit_lambda, w.to(torch.float32).contiguous())      # pass 2: the value is `value`, the graph pass 2's
            out = out + (weighted - weighted.detach()).double()
        if details:
            return out, MWERDetails(hypotheses, errors, post, costs, wt.expected_errors)
        return out

    def ctc_loss(self, inputs, inputs_length, targets, targets_length, reduction="mean"):
        """CTC loss of the auxiliary head alone (blank = 0, the transducer's): the audio encoder, the head and ttmi.ctc's kernels.
        reduction as in `loss` ('mean' divides by the batch size).  ValueError on a module without the head."""
        if getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        if not inputs.is_cuda:
            raise ValueError("Transducer.ctc_loss: inputs must live on the GPU (the MI355X build has no CPU path)")
        enc_state = self.encoder(inputs, self._audio_mask(inputs))
        return self._ctc_from_states(enc_state, targets, inputs_length, targets_length, reduction)

    def ctc_loss_from_last_forward(self, targets, inputs_length, targets_length, reduction="mean"):
        """the head's CTC loss on the audio states the last `forward` kept, for the two-call form `logits = model(x, y); loss =
        criterion(logits, ...)` (train.py:51-53; ttmi.dp_train wraps the criterion with it).  The reference is released here."""
        enc_state = self.__dict__.pop("_ctc_states", None)
        if enc_state is None:
            raise RuntimeError("ctc_loss_from_last_forward: no audio states kept (call the model first; one loss per forward)")
        return self._ctc_from_states(enc_state, targets, inputs_length, targets_length, reduction)

    def _ctc_head_logits(self, enc_state):
        """the CTC head on audio states [B, T, d] -> f32 logits [B, T, V], the [..., :V] view of a row-padded buffer (ops.linear_nt)"""
        enc_state = enc_state.contiguous()
        B, T, d = enc_state.shape
        V = self.ctc_head.out_features
        buf, logits = ops.padded_empty((B, T, V), torch.float32, enc_state.device)
        ops.weights_fresh()
        ops.linear_nt(enc_state.reshape(B * T, d), self.ctc_head.weight.detach(), buf.view(B * T, buf.shape[-1])[:, :V],
                      bias=self.ctc_head.bias.detach(), prec=default_precision())
        return logits

    @torch.no_grad()
    def recognize_ctc(self, inputs, inputs_length=None, audio_mask=None):
        """non-autoregressive recognition with the CTC head: per utterance the argmax of the head over its frames, repeats collapsed, blanks
        dropped (ttmi.ctc.ctc_greedy_decode) -> one token list per utterance"""
        from ttmi.ctc import ctc_greedy_decode
        if getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        if not inputs.is_cuda:
            raise ValueError("recognize_ctc: inputs must live on the GPU (the MI355X build has no CPU path)")
        enc_state = self.encoder(inputs, self._audio_mask(inputs) if audio_mask is None else audio_mask)
        logits = self._ctc_head_logits(enc_state)
        lens = None if inputs_length is None else torch.as_tensor(inputs_length).to(enc_state.device)
        return ctc_greedy_decode(logits, lens, blank=0)

    @torch.no_grad()
    def ctc_score(self, inputs, inputs_length, hypotheses, audio_mask=None):
        """The CTC head's log-likelihood of given token sequences (blank = 0): the audio encoder once, the head as `recognize_ctc` forms it,
        then ttmi.ctc.ctc_score, every hypothesis of an utterance on that utterance's logits.  hypotheses = per utterance a list of token
        lists -> the same nesting of floats (-inf where the utterance has fewer frames than the hypothesis needs).  It is the term
        `beam_decode_batch(ctc_weight=...)` adds to its ordering key.  ValueError on a module without the head."""
        from ttmi.ctc import ctc_score
        if getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        if not inputs.is_cuda:
            raise ValueError("Transducer.ctc_score: inputs must live on the GPU (the MI355X build has no CPU path)")
        enc_state = self.encoder(inputs, self._audio_mask(inputs) if audio_mask is None else audio_mask)
        lens = None if inputs_length is None else torch.as_tensor(inputs_length).to(enc_state.device)
        flat = ctc_score(self._ctc_head_logits(enc_state), hypotheses, lens, blank=0).cpu().tolist()
        out, i = [], 0
        for hyps in hypotheses:
            out.append(flat[i:i + len(hyps)])
            i += len(hyps)
        return out

    @torch.no_grad()
    def align_ctc(self, inputs, inputs_length, targets, targets_length, *, stats=False):
        """Forced alignment of `targets` to `inputs` on the CTC lattice of the auxiliary head (blank = 0): the audio encoder once, the head,
        then ttmi.ctc.ctc_align -> ttmi.ctc.CTCAlignment: `path` int32 [B, T] (state of the extended label sequence per frame), `spans`
        int32 [B, U, 2] ((first, last) frame of each label, -1 for u >= U_b), `score` [B] (log-probability of the best alignment) and, with
        stats=True, `expected` / `mass` / `duration` [B, U] (expected onset frame, onset mass - 1 for a healthy lattice - and expected
        number of frames of each label over all alignments).  The head's posteriors come from the audio encoder alone: compare `expected`
        with align(..., stats=True).expected_frames for the emission delay of the two heads.  ValueError on a module without the head."""
        from ttmi.ctc import ctc_align
        if getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        if not inputs.is_cuda:
            raise ValueError("Transducer.align_ctc: inputs must live on the GPU (the MI355X build has no CPU path)")
        logits = self._ctc_head_logits(self.encoder(inputs, self._audio_mask(inputs)))
        return ctc_align(logits, targets, inputs_length, targets_length, blank=0, stats=stats)

    def align(self, inputs, inputs_length, targets, targets_length, chunk=None, check_lengths=True, exp_domain=False, *, stats=False):
        """Forced alignment of `targets` to `inputs`: the best path through the RNN-T lattice, without materialising the logits (the chunked
        joint + loss forward of `loss()`, forward only, under no_grad; the reference has no counterpart).  -> warprnnt_pytorch.AlignResult:
        `frames` int32 [B, U] (frames[b][u] = the frame at which label u+1 of utterance b is emitted, non-decreasing, -1 for u >= U_b),
        `score` [B] (log-probability of that path), `cost` [B] (-log P(y|x), what loss(reduction='none') returns) and, with stats=True,
        `expected_frames` / `mass` [B, U] (posterior mean emission frame of each label; total emission posterior, 1 for a healthy lattice).
        Tie rule: a label move is taken only when strictly better than the blank move (include/ttmi.h, ttmi_rnnt_align).

        exp_domain=True (bf16 mode, training-sized chunks, and only once a training step has made the module's shift valid; the plain form
        otherwise): the exp-domain joint + loss forward.  It does not disturb training: the shift state of the joint (_ExpShift cur / nxt /
        flag / valid) is only read; an out-of-range chunk is detected by a flag of this call's own and run again in the plain form.

        The encoders run under no_grad in whatever mode the module is in: call it in eval() mode.  On a module in train() with
        dropout > 0 the alignment is taken on dropped-out encoder states and the call draws from the dropout generator like any other
        forward, so "does not disturb training" is a statement about the shift state only.

        This is the standard lattice; `align_monotonic` is the same call on the one-decision-per-frame lattice of the decoders."""
        return self._align("align", "rnnt", inputs, inputs_length, targets, targets_length, chunk, check_lengths, exp_domain, stats)

    def align_monotonic(self, inputs, inputs_length, targets, targets_length, chunk=None, check_lengths=True, *, stats=False):
        """`align` on the one-decision-per-frame lattice that loss(topology='monotonic') trains and that recognize / decode_batch / the beam
        search walk (include/ttmi.h, ttmi_mono_align): per chunk joint_fwd -> mono_loss_fwd -> mono_align (-> mono_emit_stats), forward
        only, under no_grad, at the chunk size of `loss()`'s plain form.  -> warprnnt_pytorch.AlignResult with the fields of `align`, where
        `frames` is STRICTLY increasing (frames[b][u] = the frame whose ONE decision is label u+1), `score` has no terminal blank and is
        comparable with DecodeResult.score - an upper bound of it for the same tokens - and `cost` is what
        loss(reduction='none', topology='monotonic') returns.  Same tie rule.  There is no exp_domain argument: this lattice has no
        exp-domain form.  Under check_lengths an utterance with more labels than frames is a ValueError; with the check off it has score
        -inf, cost +inf, every frames / expected_frames entry -1 and mass 0.  (A method of its own and not a keyword of `align`, whose
        parameter list is pinned; warprnnt_pytorch.rnnt_align takes topology='monotonic' for the same alignment on logits or a handle.)"""
        return self._align("align_monotonic", "monotonic", inputs, inputs_length, targets, targets_length, chunk, check_lengths, False, stats)

    def _align(self, method, topology, inputs, inputs_length, targets, targets_length, chunk, check_lengths, exp_domain, stats):
        """the body of align / align_monotonic (`method`: the caller's name, for its error message)"""
        from warprnnt_pytorch import check_lengths as certify, check_monotonic_lengths as monotonic_lengths
        self._refuse_tdt("forced alignment / emission statistics (%s)" % method)
        lat = ops.lattice(topology)
        labels, al, ll = (t.to(dtype=torch.int32) for t in (targets, inputs_length, targets_length))
        certify(labels.contiguous(), al.contiguous(), ll.contiguous(), inputs.shape[0], 0, targets.shape[1] + 1, False)
        if not inputs.is_cuda:
            raise ValueError("Transducer.%s: inputs must live on the GPU (the MI355X build has no CPU path)" % method)
        with torch.no_grad():
            enc_state, dec_state = self._encode(inputs, targets)
        B, T, U1 = enc_state.shape[0], enc_state.shape[1], dec_state.shape[1]
        labels, al, ll = (t.to(device=enc_state.device).contiguous() for t in (labels, al, ll))
        certify(labels, al, ll, B, T, U1, check_lengths)
        if lat.label_takes_frame and check_lengths:
            monotonic_lengths(al, ll)                # ValueError for an utterance with more labels than frames
        ops.weights_fresh()
        prec = default_precision()
        st = self.joint.exp_shift_state(enc_state.device) if exp_domain and lat.has_exp_forms and prec == 1 else None
        if st is not None and not st.valid:
            st = None
        if chunk is None:
            chunk = self.default_loss_chunk(B, T, U1, st is not None)
        return _joint_align(self.joint, enc_state, dec_state, labels, al, ll, prec, int(chunk), 0, st, stats, topology)

    def default_loss_chunk(self, B, T, U1, exp_domain=False):
        """utterances per chunk of `loss()` (JointNet.default_loss_chunk)"""
        return self.joint.default_loss_chunk(B, T, U1, exp_domain)

    def _encode(self, inputs, targets):
        """both encoders of forward() (tt/model.py:58-65): -> (enc_state [B,T,d], dec_state [B,U+1,d])"""
        targets = F.pad(targets, pad=[1, 0, 0, 0], value=0)                 # leading blank / SOS
        audio_mask = self._audio_mask(inputs)
        if self.config.overlap_label_encoder and inputs.is_cuda:
            # the label encoder (tiny, launch-latency-bound kernels) is independent of the audio encoder until the joint:
            # run it on a side stream so both fill the chip together; autograd replays the same streams in backward
            main, side = torch.cuda.current_stream(inputs.device), ops.side_stream(inputs.device)
            side.wait_stream(main)                                          # the side stream needs `targets`, nothing else
            # host order: the audio encoder's long kernels are queued FIRST, the label encoder's ~400 tiny launches are issued while the
            # GPU is busy with them (issued first, they left the chip nearly idle for the ~1 ms the host needs to enqueue them)
            enc_state = self.encoder(inputs, audio_mask)
            # `targets` lives in the main stream's pool but is read by side-stream kernels - in backward as late as the embedding
            # gradient, the label encoder's last launch: without this its block could be handed to a main-stream allocation (and
            # overwritten) as soon as autograd drops the graph, while that launch is still queued
            capturing = torch.cuda.is_current_stream_capturing()    # (a captured step's tensors live in the graph's own pool for its lifetime)
            if not capturing:
                targets.record_stream(side)
            with torch.cuda.stream(side):
                dec_state = self._label_states(targets)
            main.wait_stream(side)
            if not capturing:
                dec_state.record_stream(main)
        else:
            enc_state = self.encoder(inputs, audio_mask)
            dec_state = self._label_states(targets)
        return enc_state, dec_state

    def _label_states(self, targets):
        """the label encoder on the padded targets (mask == look_ahead_mask(targets)[:, :, None]).  With TTMI_LABEL_VALUE_PRECISION (tt.transformer.label_value_precision) the
        states' VALUE comes from a second, gradient-free pass in a parity mode, on the same dropout masks (the CPU generator the seeds are drawn from is rewound for it), and
        the gradient flows through the bf16 pass: one label state meets all T frames of its utterance in the joint, so the label encoder's bf16 rounding is one pattern in T
        lattice rows - and, while its outputs still resemble each other (the first steps of training), in every utterance of the batch (round 6)."""
        vp = label_value_precision()
        if vp is None or not targets.is_cuda:
            return self.decoder(targets, MaskSpec(1))
        rng = torch.get_rng_state()
        dec = self.decoder(targets, MaskSpec(1))
        after = torch.get_rng_state()
        torch.set_rng_state(rng)
        with torch.no_grad():
            hi = self.decoder(targets, MaskSpec(1), prec=vp)
        torch.set_rng_state(after)
        return dec + (hi - dec.detach())

    def _audio_mask(self, inputs):
        """Reference behaviour is audio_mask=None (tt/model.py:60-61).  Opt-in `config.streaming` (absent in the
        reference YAMLs => None => off): {'left': l, 'right': r} band mask or {'chunk': c, 'left': l} block mask."""
        s = self.config.streaming
        if not s:
            return None
        if "chunk" in s:
            # per-row key intervals of the block mask (tt.utils.chunk_mask), built once per (T, chunk, left, device) and handed to the kernels
            # as they are: no [T, T] tensor per forward and none of as_mask_spec's host synchronisations (they made the C4-chunk run host-bound)
            chunk, left, T = int(s["chunk"]), int(s.get("left", 0)), inputs.size(1)
            key = (T, chunk, left, str(inputs.device))
            cache = self.__dict__.setdefault("_chunk_specs", {})
            spec = cache.get(key)
            if spec is None:
                i = torch.arange(T, device=inputs.device)
                lo = ((i // chunk) * chunk - left).clamp_(min=0)
                hi = ((i // chunk + 1) * chunk - 1).clamp_(max=T - 1)
                spec = cache[key] = MaskSpec(4, left=left + chunk - 1, right=chunk - 1,
                                             tensor=torch.stack([lo, hi], -1).to(torch.int32)[None].contiguous())
            return spec
        return MaskSpec(2, left=int(s.get("left", 0)), right=int(s.get("right", 0)))

    @torch.no_grad()
    def decode(self, enc_state, lengths, block=64, details=False):
        """Greedy: <= 1 symbol per frame, label encoder re-run on the whole history WITHOUT look-ahead mask (tt/model.py:70-90).
        Same token sequence as the reference's per-frame loop, but frames are scored `block` at a time against the current
        label state and the first non-blank frame is found on the device (ttmi_greedy_scan): one host sync per emitted
        symbol instead of one per frame.  The label-encoder re-runs replay captured graphs (one per history length, see
        _LabelStateGraphs).  details=True: -> DecodeResult (tokens, emission frames, token log-probabilities, path score), from
        `decode_batch`'s device-side bookkeeping on a batch of one.  A token-and-duration model goes through `decode_batch` on a batch of
        one whatever `details` says (its jumps live in the TDT kernel pair)."""
        if self.tdt_durations is not None:
            return self.decode_batch(enc_state[None], [int(lengths)], block=block, details=details)[0]
        if details:
            return self.decode_batch(enc_state[None], [int(lengths)], block=block, details=True)[0]
        token_list = [0]
        dev = enc_state.device
        T = int(lengths)
        graphs = self._label_state_graphs(dev)

        def label_state():
            """label-encoder output for the current history -> [1, 1, d]"""
            L = len(token_list)
            if graphs is not None and L <= graphs.MAX_L:
                graphs.set_token(L - 1, token_list[-1])
                return graphs.state(L)
            return self.decoder(torch.tensor([token_list], dtype=torch.long, device=dev))[:, -1:, :]

        dec_state = label_state()
        t = 0
        while t < T:
            n = min(block, T - t)
            logits = self.joint(enc_state[t:t + n].unsqueeze(0), dec_state)                                  # [1, n, 1, V]
            row, tok = ops.greedy_scan(logits[0, :, 0, :])
            if tok is None:
                t += n
                continue
            if tok >= self.config.vocab_size:   # NaN logits (bad weights / inputs) come back as an impossible symbol: fail here, not later
                raise RuntimeError("greedy decode: the joint produced no finite maximum at frame %d (NaN logits?)" % (t + row))
            token_list.append(tok)
            dec_state = label_state()
            t += row + 1                                                    # the emitting frame is consumed
        return token_list[1:]

    def _label_state_graphs(self, dev, batch=1):
        """the per-model graph caches of `decode` / `decode_batch` (None: CPU tensors, or switched off with config.decode_graphs = False)"""
        if dev.type != "cuda" or self.config.decode_graphs is False:
            return None
        cache = self.__dict__.setdefault("_decode_graphs", {})
        g = cache.get(batch)
        if g is None or g.device != dev or g.key != _LabelStateGraphs.weights_key(self):
            if len(cache) > 4:
                cache.clear()                                       # (batch sizes come and go: keep a handful of graph sets)
            g = cache[batch] = _LabelStateGraphs(self, dev, batch)
        return g

    @torch.no_grad()
    def decode_batch(self, enc_states, lengths, block=None, details=False):
        """Greedy decoding of EVERY utterance of a batch at once: the token lists `decode(enc_states[b], lengths[b])` returns, for all b
        (tt/model.py:92-108 loops over the utterances, one host round trip per frame each).  The batch advances in lockstep over SYMBOL
        steps: in step s every utterance still decoding looks for its next non-blank frame (blocks of `block` frames from its own position,
        scored against its own label state: one joint call for the whole batch, ttmi_greedy_scan_batch / ttmi_greedy_advance keep positions,
        histories and flags on the device), then ONE label-encoder call of length s + 1 re-computes all label states (every history has
        exactly s + 1 tokens - the relative-position term depends on the sequence length, so utterances of different history lengths
        could not share a call).  Host synchronisations: one 8-byte read per scanned block of the whole batch (about one per symbol step)
        instead of one per symbol and utterance; label-encoder launches: one call per symbol step instead of one per symbol and
        utterance.  Utterances that have run out of frames LEAVE the batch (no extra host round trip: the count of the living comes with the
        flags, the rows from a stable sort on the device), so the long tail of a batch - the longest hypothesis of 32 synthetic utterances
        has 105 symbols, the mean 50 - runs on a handful of rows instead of 32.  Same arithmetic per utterance as `decode`: same tokens.
        block = frames scored per joint call (default 64).

        details=True: -> a list of DecodeResult.  ttmi_greedy_scan_batch_lp / ttmi_greedy_advance_lp run in place of the plain pair: the scan's
        one pass over each row of logits also yields log P(blank) and log P(argmax), the advance books the emission frame and log-probability
        of every token and the f64 log-probability of the greedy path (DecodeResult for what that score is and is not).  Same joint and
        label-encoder calls, same host reads; the details follow the rows through the shrinking batch like the histories and come back in
        the one transfer at the end.

        A token-and-duration model (config.tdt_durations) runs the same lockstep with ttmi_tdt_scan_batch / ttmi_tdt_advance: every decision
        jumps by the duration it predicts, a jump that leaves the block carries over into the next one, and details=True gives
        ttmi.tdt.TDTDecodeResult (the DecodeResult fields and the tokens' durations)."""
        if self.tdt_durations is not None:
            return self._decode_batch_tdt(enc_states, lengths, block, details)
        if details and not enc_states.is_cuda:
            raise ValueError("decode_batch(details=True): enc_states must live on the GPU (the MI355X build has no CPU path)")
        dev = enc_states.device
        B, T = enc_states.shape[0], enc_states.shape[1]
        block = 64 if block is None else block                       # frames scored per joint call
        T_len = torch.as_tensor(lengths, dtype=torch.int32).to(dev).clamp(max=T).contiguous()
        # Label-encoder graphs serve the symbol steps in which the batch is still COMPLETE (one replay instead of ~150 launches; a graph is
        # captured for a fixed row count); as soon as an utterance has finished the rows shrink and the calls are eager launches on the rows
        # still decoding - which is worth more than the replay (96 utt/s with a fixed batch of 32, 212 with shrinking rows).
        # config.decode_batch_graphs = False: eager launches throughout.  Round 4 had made the graphs opt-in because a third of the processes
        # came back from their first pure-replay pass with other tokens; round 5 found the cause - a hipMemset2DAsync NODE in the captured
        # label encoder (column 0 of the fp32 path's position slab) that ROCm 7.2's graph launch does not order against the kernels around
        # it - and removed every memset node from the library (csrc/rowops.hip fill_zero*, DESIGN.md section 4j,
        # tests/test_decode_graphs_gpu.py).
        graphs = self._label_state_graphs(dev, B) if self.config.decode_batch_graphs is not False else None
        final_hist = torch.zeros(B, T + 2, dtype=torch.long, device=dev)   # column 0 = the start symbol (blank); at most one symbol per frame
        final_count = torch.zeros(B, dtype=torch.int32, device=dev)
        hist = final_hist.clone()
        orig = torch.arange(B, device=dev)                           # the utterance each row of the (shrinking) batch belongs to
        t = torch.zeros(B, dtype=torch.int32, device=dev)
        need = torch.ones(B, dtype=torch.int32, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev)
        count = torch.zeros(B, dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        n_frames = block
        key = torch.full((B,), n_frames << 32, dtype=torch.int64, device=dev)
        rows = torch.arange(n_frames, device=dev, dtype=torch.long)[None, :]
        if details:                                                  # at most T symbols per utterance: column count[b] < T + 1
            final_frames = torch.zeros(B, T + 1, dtype=torch.int32, device=dev)
            final_lp = torch.zeros(B, T + 1, dtype=torch.float32, device=dev)
            final_score = torch.zeros(B, dtype=torch.float64, device=dev)
            frames, tok_lp, score = final_frames.clone(), final_lp.clone(), final_score.clone()
            lp = torch.empty(B, n_frames, 2, dtype=torch.float32, device=dev)

        def label_states(n_hist):
            """label-encoder outputs at the last position of every history (all of length n_hist) -> [rows of the batch, 1, d]"""
            if graphs is not None and n_hist <= graphs.MAX_L and hist.shape[0] == graphs.batch:
                graphs.master[:, :n_hist].copy_(hist[:, :n_hist])
                return graphs.state(n_hist)
            return self.decoder(hist[:, :n_hist].contiguous())[:, -1:, :]

        n_hist = 1
        dec_state = label_states(n_hist)
        while True:
            torch.sub(1, done, out=need)
            while True:
                idx = (t.long()[:, None] + rows).clamp_(max=T - 1)                             # frames t_b .. t_b + n_frames - 1 (beyond T_b: ignored by the scan)
                logits = self.joint(enc_states[orig[:, None], idx], dec_state)                    # [rows, n_frames, 1, V]
                if details:
                    ops.greedy_scan_batch_lp(logits[:, :, 0, :], t, T_len, need, key, lp)
                    ops.greedy_advance_lp(key, n_frames, n_hist, hist, t, T_len, need, done, count, flags, lp, frames, tok_lp, score)
                else:
                    ops.greedy_scan_batch(logits[:, :, 0, :], t, T_len, need, key)
                    ops.greedy_advance(key, n_frames, n_hist, hist, t, T_len, need, done, count, flags)
                pending, alive = flags.tolist()                                                   # the batch's one host round trip per block
                if pending == 0:
                    break
            if alive == 0:
                break
            if alive < hist.shape[0] and self.config.decode_batch_shrink is not False:
                # finished utterances leave the batch: every later label-encoder and joint call runs on the rows still decoding (per-utterance
                # arithmetic does not depend on who else is in the batch).  Their histories are kept; no host round trip - the row count is
                # `alive`, the rows are the first `alive` of a stable sort by the done flag
                final_hist.index_copy_(0, orig, hist)
                final_count.index_copy_(0, orig, count)
                keep = torch.argsort(done, stable=True)[:alive]
                if details:
                    final_frames.index_copy_(0, orig, frames)
                    final_lp.index_copy_(0, orig, tok_lp)
                    final_score.index_copy_(0, orig, score)
                    frames, tok_lp, score, lp = frames[keep], tok_lp[keep], score[keep], lp[:alive]
                hist, orig, t, T_len, count = hist[keep], orig[keep], t[keep].contiguous(), T_len[keep].contiguous(), count[keep].contiguous()
                need = torch.zeros(alive, dtype=torch.int32, device=dev)
                done = torch.zeros(alive, dtype=torch.int32, device=dev)
                key = torch.full((alive,), n_frames << 32, dtype=torch.int64, device=dev)
            n_hist += 1
            dec_state = label_states(n_hist)
        final_hist.index_copy_(0, orig, hist)
        final_count.index_copy_(0, orig, count)
        if details:
            final_frames.index_copy_(0, orig, frames)
            final_lp.index_copy_(0, orig, tok_lp)
            final_score.index_copy_(0, orig, score)
            # ONE transfer, as f64 (exact for token ids, counts, frames and f32 log-probabilities): count | score | tokens | frames | logprobs
            packed = torch.cat([final_count.double()[:, None], final_score[:, None], final_hist[:, 1:T + 2].double(), final_frames.double(),
                                final_lp.double()], dim=1).cpu()
            out = []
            for b in range(B):
                c = int(packed[b, 0])
                tok, frm, lpr = (packed[b, 2 + i * (T + 1):2 + i * (T + 1) + c].tolist() for i in range(3))
                out.append(DecodeResult([int(v) for v in tok], [int(v) for v in frm], lpr, float(packed[b, 1])))
            return out
        final = final_hist.cpu()
        counts = final_count.cpu().tolist()
        return [final[b, 1:1 + counts[b]].tolist() for b in range(B)]

    def _decode_batch_tdt(self, enc_states, lengths, block, details):
        """decode_batch for a token-and-duration model: the same symbol-step lockstep, shrinking batch and label-encoder graphs, with the TDT
        pair in place of the greedy pair.  There is one pair only, and it always books the details (frames, log-probabilities, durations,
        score); details=False returns the token lists alone.  block (default 64): the frames scored per joint call.  A jump skips rows
        the block has scored, so a TDT block of n frames holds n / (mean duration) decisions; 64 keeps the SPAN of a block, and with it the
        joint calls and host reads per symbol step, at what the frame-by-frame decoder has."""
        from ttmi.tdt import TDTDecodeResult
        if not enc_states.is_cuda:
            raise ValueError("decode_batch: a token-and-duration model decodes on the GPU only (the MI355X build has no CPU path)")
        durs = self.tdt_durations
        dev = enc_states.device
        B, T = enc_states.shape[0], enc_states.shape[1]
        n_frames = 64 if block is None else int(block)
        T_len = torch.as_tensor(lengths, dtype=torch.int32).to(dev).clamp(max=T).contiguous()
        graphs = self._label_state_graphs(dev, B) if self.config.decode_batch_graphs is not False else None
        final_hist = torch.zeros(B, T + 2, dtype=torch.long, device=dev)   # column 0 = the start symbol (blank); at most one symbol per frame
        final_count = torch.zeros(B, dtype=torch.int32, device=dev)
        final_frames = torch.zeros(B, T + 1, dtype=torch.int32, device=dev)
        final_lp = torch.zeros(B, T + 1, dtype=torch.float32, device=dev)
        final_dur = torch.zeros(B, T + 1, dtype=torch.int32, device=dev)
        final_score = torch.zeros(B, dtype=torch.float64, device=dev)
        hist, frames, tok_lp, tok_dur, score = (v.clone() for v in (final_hist, final_frames, final_lp, final_dur, final_score))
        orig = torch.arange(B, device=dev)                           # the utterance each row of the (shrinking) batch belongs to
        t = torch.zeros(B, dtype=torch.int32, device=dev)
        need = torch.ones(B, dtype=torch.int32, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev)
        count = torch.zeros(B, dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        rows = torch.arange(n_frames, device=dev, dtype=torch.long)[None, :]
        dec = torch.zeros(B, n_frames, 2, dtype=torch.int32, device=dev)
        lp = torch.zeros(B, n_frames, 2, dtype=torch.float32, device=dev)

        def label_states(n_hist):
            """label-encoder outputs at the last position of every history (all of length n_hist) -> [rows of the batch, 1, d]"""
            if graphs is not None and n_hist <= graphs.MAX_L and hist.shape[0] == graphs.batch:
                graphs.master[:, :n_hist].copy_(hist[:, :n_hist])
                return graphs.state(n_hist)
            return self.decoder(hist[:, :n_hist].contiguous())[:, -1:, :]

        def keep_results():
            for dst, src in ((final_hist, hist), (final_count, count), (final_frames, frames), (final_lp, tok_lp), (final_dur, tok_dur),
                             (final_score, score)):
                dst.index_copy_(0, orig, src)

        n_hist = 1
        dec_state = label_states(n_hist)
        while True:
            torch.sub(1, done, out=need)
            while True:
                idx = (t.long()[:, None] + rows).clamp_(max=T - 1)                             # frames t_b .. t_b + n_frames - 1 (beyond T_b: ignored by the scan)
                logits = self.joint(enc_states[orig[:, None], idx], dec_state)                    # [rows, n_frames, 1, V + D]
                ops.tdt_scan_batch(logits[:, :, 0, :], len(durs), t, T_len, need, dec, lp)
                ops.tdt_advance(dec, lp, durs, n_hist, hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, score)
                pending, alive = flags.tolist()                                                   # the batch's one host round trip per block
                if pending == 0:
                    break
            if alive == 0:
                break
            if alive < hist.shape[0] and self.config.decode_batch_shrink is not False:
                keep_results()
                keep = torch.argsort(done, stable=True)[:alive]
                hist, frames, tok_lp, tok_dur, score = hist[keep], frames[keep], tok_lp[keep], tok_dur[keep], score[keep]
                orig, t, T_len, count = orig[keep], t[keep].contiguous(), T_len[keep].contiguous(), count[keep].contiguous()
                dec, lp = dec[:alive], lp[:alive]
                need = torch.zeros(alive, dtype=torch.int32, device=dev)
                done = torch.zeros(alive, dtype=torch.int32, device=dev)
            n_hist += 1
            dec_state = label_states(n_hist)
        keep_results()
        if not details:
            final = final_hist.cpu()
            counts = final_count.cpu().tolist()
            return [final[b, 1:1 + counts[b]].tolist() for b in range(B)]
        # ONE transfer, as f64 (exact for token ids, counts, frames, durations and f32 log-probabilities)
        packed = torch.cat([final_count.double()[:, None], final_score[:, None], final_hist[:, 1:T + 2].double(), final_frames.double(),
                            final_lp.double(), final_dur.double()], dim=1).cpu()
        out = []
        for b in range(B):
            c = int(packed[b, 0])
            tok, frm, lpr, dur = (packed[b, 2 + i * (T + 1):2 + i * (T + 1) + c].tolist() for i in range(4))
            out.append(TDTDecodeResult([int(v) for v in tok], [int(v) for v in frm], lpr, [int(v) for v in dur], float(packed[b, 1])))
        return out

    @torch.no_grad()
    def recognize(self, inputs, inputs_length=None, audio_mask=None, details=False):
        """greedy recognition of a batch -> one token list per utterance; details=True -> one DecodeResult per utterance (tokens, emission
        frames, token log-probabilities, path score), every utterance through decode_batch's device-side bookkeeping (a batch of one too;
        with config.batched_decode = False one decode(details=True) per utterance).  A token-and-duration model (config.tdt_durations)
        always decodes through decode_batch's TDT pair, a batch of one included; details=True -> ttmi.tdt.TDTDecodeResult"""
        if self.tdt_durations is not None:
            if not inputs.is_cuda:
                raise ValueError("recognize: a token-and-duration model decodes on the GPU only (the MI355X build has no CPU path)")
            return self.decode_batch(self.encoder(inputs, audio_mask), inputs_length, details=details)
        if details:
            if not inputs.is_cuda:
                raise ValueError("recognize(details=True): inputs must live on the GPU (the MI355X build has no CPU path)")
            enc_states = self.encoder(inputs, audio_mask)
            if self.config.batched_decode is not False:
                return self.decode_batch(enc_states, inputs_length, details=True)
            return [self.decode(enc_states[b], inputs_length[b], details=True) for b in range(inputs.size(0))]
        enc_states = self.encoder(inputs, audio_mask)
        if enc_states.is_cuda and inputs.size(0) > 1 and self.config.batched_decode is not False:
            return self.decode_batch(enc_states, inputs_length)
        return [self.decode(enc_states[b], inputs_length[b]) for b in range(inputs.size(0))]

    @torch.no_grad()
    def beam_decode_batch(self, enc_states, lengths, beam_width=4, nbest=None, context=None, return_bias=False, lm=None, lm_weight=0.0,
                          ilm_weight=0.0, length_bonus=0.0, return_lm=False, ctc_weight=0.0, return_ctc=False):
        """Frame-synchronous beam search of EVERY utterance of a batch at once -> per utterance a list of at most `nbest` (default: beam_width)
        DecodeResult, best first.  The probability model is the greedy decoder's (`decode_batch`): each of an utterance's T_b frames takes one
        decision, blank or one symbol, against the label state of the tokens so far, and the emitting frame is consumed.  Unlike `beam_search`
        (the reference's, kept for token identity) every frame adds its term to every hypothesis, hypotheses that spell the same tokens are
        merged (their probabilities add), and the scores of the list are comparable: `score` = the log of the summed probability of the
        decision sequences the beam kept for these tokens, `frames` / `logprobs` = those of the best single one (include/ttmi.h,
        ttmi_beam_step, has the rule).  The loop runs over frames 0 .. max(lengths) - 1; per frame ONE joint call scores frame t of every
        utterance against the [B, beam_width, d] table of label states, ttmi_beam_step turns the logits into the next beam on the device
        (one workgroup per utterance), ONE host read brings the new slots' lengths and which of them are new sequences, and the label encoder
        runs on those only, one call per distinct history length (the relative-position term depends on the sequence length, see
        `decode_batch`); every other slot takes its parent's state by a gather on the device.  Finished utterances pass through unchanged.
        context = a ttmi.context.ContextGraph (hotword boosting): the same loop, but every slot also carries the automaton's state and its
        accumulated bias, and ttmi_beam_step_ctx selects by score + bias (include/ttmi.h has the rule), so a hotword whose first token ranks
        below the beam width on its score alone can stay in the beam.  After the last frame final_bias = bias + final_w[state] (a hotword
        begun and not finished keeps nothing) and the list is ordered by score + final_bias, descending, the slot ascending on ties, then cut
        to `nbest`.  `score` stays the model's log-probability (comparable with greedy scores, usable by mwer_loss).  return_bias=True ->
        (results, biases): biases[b][n] = the final bias of results[b][n], 0.0 without a context.  context=None runs ttmi_beam_step as before.
        lm = a language model scorer (ttmi.lm has the protocol and TransformerLM), fused into the search: with lm, ilm_weight or length_bonus
        given, every frame runs ttmi_beam_step_fuse (include/ttmi.h has the rule) on two more [B, W, V] row tables kept like the label
        states (gathered by `parent`, recomputed for `fresh` slots only, the LM called once per distinct history length): source 0 = the
        LM's rows at lm_weight, source 1 = the internal LM's rows self.joint(zero encoder state, label state) at -ilm_weight, renormalised
        without the blank (internal-LM subtraction), and length_bonus per emitted symbol.  The selection of every frame is by
        score + bias + fuse; after the last frame lm_total = fuse + lm_weight * log P_lm(eos | tokens) where lm.eos is not None, and the
        list is ordered by score + final_bias + lm_total.  `score` stays the model's log-probability.  return_lm=True appends the
        lm_totals to the return, as return_bias does the biases.  Hotwords and an n-gram automaton at once need a product automaton: one
        context= per call.  Without lm, ilm_weight and length_bonus the calls are the ones above, launch for launch.
        ctc_weight > 0 (a model with the CTC head): joint CTC - transducer rescoring of the final beam.  The search itself is untouched; after
        the last frame the head's logits are formed once from enc_states, ttmi_ctc_score_hyps gives ctc = the head's full-sum log-likelihood
        of the tokens of every one of the B x W slots, read from the beam's own arrays, and each list is ordered by
        score + final_bias + lm_total + ctc_weight * ctc (f64, added in that order), descending, the slot ascending on ties - before the cut
        to `nbest`, so the head can promote a hypothesis from anywhere in the beam.  A hypothesis the head finds infeasible (ctc = -inf:
        fewer frames than tokens plus adjacent repeats) or NaN comes after all others, in the order of the key without the CTC term, and
        is still returned.  `score` stays the model's log-probability.  return_ctc=True appends ctcs[b][n] to the return, after biases
        and lm_totals (with ctc_weight = 0 the values are computed and change no order).  With ctc_weight = 0 and return_ctc=False nothing
        of this runs.  ValueError on a module without the head, or when max(lengths) > 1023 (the scorer's longest hypothesis).
        The same search over frames that arrive in blocks: `beam_search_state` (ttmi.beam.BeamSearch; this loop stays beside it as it is).
        Not built: a cache of label states for sequences seen on earlier frames, a captured graph of the loop."""
        self._refuse_tdt("beam search (beam_decode_batch / recognize_nbest, ctc_weight= rescoring included)")
        if not enc_states.is_cuda:
            raise ValueError("beam_decode_batch: enc_states must live on the GPU (the MI355X build has no CPU path)")
        W = int(beam_width)
        nbest = W if nbest is None else int(nbest)
        if not 1 <= W <= 32 or nbest < 1:
            raise ValueError("beam_decode_batch: beam_width must be in [1, 32] and nbest >= 1, got %r and %r" % (beam_width, nbest))
        for name, v in (("lm_weight", lm_weight), ("ilm_weight", ilm_weight), ("length_bonus", length_bonus)):
            if not math.isfinite(float(v)) or (name != "length_bonus" and float(v) < 0.0):
                raise ValueError("beam_decode_batch: %s must be finite%s, got %r" % (name, "" if name == "length_bonus" else " and >= 0", v))
        lm_weight, ilm_weight, length_bonus = float(lm_weight), float(ilm_weight), float(length_bonus)
        if not math.isfinite(float(ctc_weight)) or float(ctc_weight) < 0.0:
            raise ValueError("beam_decode_batch: ctc_weight must be finite and >= 0, got %r" % (ctc_weight,))
        ctc_weight = float(ctc_weight)
        use_ctc = ctc_weight > 0.0 or bool(return_ctc)
        if use_ctc and getattr(self, "ctc_head", None) is None:
            raise ValueError("this Transducer has no CTC head: build it with config.ctc_weight > 0")
        fused = lm is not None or ilm_weight != 0.0 or length_bonus != 0.0
        if lm is not None:
            if lm.norm not in ops.BEAM_FUSE_NORMS:
                raise ValueError("beam_decode_batch: lm.norm must be one of %s, got %r" % (sorted(ops.BEAM_FUSE_NORMS), lm.norm))
            if isinstance(lm, nn.Module) and any(not p.is_cuda for p in lm.parameters()):
                raise ValueError("beam_decode_batch: the language model must live on the GPU (the MI355X build has no CPU path)")
        dev = enc_states.device
        B, T = enc_states.shape[0], enc_states.shape[1]
        lens = [T] * B if lengths is None else [min(int(v), T) for v in torch.as_tensor(lengths).tolist()]
        T_max = max(lens + [0])
        if use_ctc and T_max > 1023:
            raise ValueError("beam_decode_batch: CTC rescoring takes at most 1023 frames (the scorer's longest hypothesis), got %d" % T_max)
        T_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        t = torch.zeros(B, dtype=torch.int32, device=dev)
        ld_hist, ld_det = T_max + 2, T_max + 1                       # at most one symbol per frame; column 0 = the start symbol (blank)

        def beam():
            """score, (len | fresh) packed for the one host read, histories, emission frames, token log-probabilities"""
            return dict(score=torch.full((B, W), -math.inf, dtype=torch.float64, device=dev), meta=torch.zeros(2, B, W, dtype=torch.int32, device=dev),
                        hist=torch.zeros(B, W, ld_hist, dtype=torch.long, device=dev), frames=torch.zeros(B, W, ld_det, dtype=torch.int32, device=dev),
                        tok_lp=torch.zeros(B, W, ld_det, dtype=torch.float32, device=dev))

        def arrays(bm):
            return bm["score"], bm["meta"][0], bm["hist"], bm["frames"], bm["tok_lp"]
        cur, nxt = beam(), beam()
        cur["score"][:, 0] = 0.0                                     # slot 0 holds the start symbol, the other slots are empty
        if context is not None:
            context.validate(self.config.vocab_size).to(dev)
            for bm in (cur, nxt):
                bm["ctx"] = (torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev))
            ctx_ws = ops.beam_ctx_workspace(B, W, self.config.vocab_size, dev)
            if context.start:                                        # (an n-gram automaton starts in its <s> context)
                cur["ctx"][0][:, 0] = int(context.start)
        parent = torch.zeros(B, W, dtype=torch.int32, device=dev)
        start = self.decoder(torch.zeros(1, 1, dtype=torch.long, device=dev))[:, -1, :]
        states = start[None].expand(B, W, -1).contiguous()           # [B, W, d]; what an empty slot holds is never read by the kernel
        d = states.shape[-1]
        lm_rows = ilm_rows = None
        need_eos = lm is not None and lm.eos is not None
        if fused:
            V = self.config.vocab_size
            if context is None:                                      # the trivial automaton: the root alone, every weight 0
                tables = tuple(torch.zeros(n, dtype=dt, device=dev) for n, dt in ((2, torch.int32), (0, torch.int32), (0, torch.int32),
                                                                                   (0, torch.float32), (1, torch.int32), (1, torch.float32)))
                for bm in (cur, nxt):
                    bm["ctx"] = (torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev))
            else:
                tables = context.tables
            for bm in (cur, nxt):
                bm["fuse"] = torch.zeros(B, W, dtype=torch.float64, device=dev)
            fuse_ws = ops.beam_fuse_workspace(B, W, V, dev)
            zero_enc = torch.zeros(1, 1, enc_states.shape[-1], dtype=enc_states.dtype, device=dev)

            def lm_scores(hist):
                rows = lm.next_logits(hist)
                if not rows.is_cuda or rows.dim() != 2 or rows.shape[1] != V or rows.dtype not in (torch.float32, torch.bfloat16):
                    raise ValueError("beam_decode_batch: lm.next_logits must return [N, %d] f32 or bf16 rows on the GPU" % V)
                return rows

            def ilm_scores(st):
                """the joint without an encoder: the label encoder's own prior (internal LM), [N, d] -> [N, V]"""
                return self.joint(zero_enc, st[None].contiguous())[0, 0]
            if lm is not None:
                lm_rows = lm_scores(torch.zeros(1, 1, dtype=torch.long, device=dev))[None].expand(B, W, -1).contiguous()
            if ilm_weight != 0.0:
                ilm_rows = ilm_scores(start)[None].expand(B, W, -1).contiguous()
        for f in range(T_max):
            logits = self.joint(enc_states[:, f:f + 1].contiguous(), states)                      # [B, 1, W, V]
            if fused:
                ops.beam_step_fuse(logits[:, 0], t, T_len, arrays(cur), arrays(nxt), parent, nxt["meta"][1], tables, cur["ctx"], nxt["ctx"],
                                   fuse_ws, cur["fuse"], nxt["fuse"],
                                   sources=(None if lm is None else (lm_rows, lm_weight, ops.BEAM_FUSE_NORMS[lm.norm]),
                                            None if ilm_rows is None else (ilm_rows, -ilm_weight, 2)), sym_bonus=length_bonus, blank=0)
            elif context is None:
                ops.beam_step(logits[:, 0], t, T_len, arrays(cur), arrays(nxt), parent, nxt["meta"][1], blank=0)
            else:
                ops.beam_step_ctx(logits[:, 0], t, T_len, arrays(cur), arrays(nxt), parent, nxt["meta"][1], context.tables, cur["ctx"],
                                  nxt["ctx"], ctx_ws, blank=0)
            t += 1
            cur, nxt = nxt, cur
            if f == T_max - 1 and not need_eos:
                break
            n_tok, fresh = cur["meta"].cpu().tolist()                                             # the frame's one host round trip
            gather = parent.long()[:, :, None]
            if f < T_max - 1:
                states = states.gather(1, gather.expand(-1, -1, d))                               # a slot that keeps its tokens keeps its label state
                if ilm_rows is not None:
                    ilm_rows = ilm_rows.gather(1, gather.expand(-1, -1, V))
            if lm_rows is not None:
                lm_rows = lm_rows.gather(1, gather.expand(-1, -1, V))
            by_len, lm_only = {}, {}
            for b in range(B):
                # an utterance without frames left reads no label state again; its closing frame's new sequences still need the LM's eos term
                which = by_len if f + 1 < lens[b] else lm_only if (need_eos and f + 1 == lens[b]) else None
                if which is None or not any(fresh[b]):
                    continue
                for w in range(W):
                    if fresh[b][w]:
                        which.setdefault(n_tok[b][w], []).append(b * W + w)
            for n in sorted(set(by_len) | set(lm_only)):
                if n in by_len:
                    rows = torch.tensor(by_len[n], dtype=torch.long, device=dev)
                    hist = cur["hist"].view(B * W, ld_hist)[rows, :n + 1].contiguous()
                    st = self.decoder(hist)[:, -1, :]
                    states.view(B * W, d).index_copy_(0, rows, st)
                    if ilm_rows is not None:
                        ilm_rows.view(B * W, V).index_copy_(0, rows, ilm_scores(st).to(ilm_rows.dtype))
                if lm_rows is not None:
                    if n in lm_only:                                                              # one LM call per history length all the same
                        rows = torch.tensor(by_len.get(n, []) + lm_only[n], dtype=torch.long, device=dev)
                        hist = cur["hist"].view(B * W, ld_hist)[rows, :n + 1].contiguous()
                    lm_rows.view(B * W, V).index_copy_(0, rows, lm_scores(hist).to(lm_rows.dtype))
        # ONE transfer, as f64 (exact for token ids, counts, frames and f32 log-probabilities): score | len | tokens | frames | logprobs
        packed = torch.cat([cur["score"][:, :, None], cur["meta"][0].double()[:, :, None], cur["hist"][:, :, 1:].double(), cur["frames"].double(),
                            cur["tok_lp"].double()] +
                           ([] if context is None else [(cur["ctx"][1] + context.final_w[cur["ctx"][0].long()].double())[:, :, None]]), dim=2)
        if fused:
            from ttmi.lm import eos_logprob
            lm_total = cur["fuse"] + lm_weight * eos_logprob(lm_rows, lm.norm, lm.eos) if need_eos else cur["fuse"]
            packed = torch.cat([packed, lm_total[:, :, None]], dim=2)
        if use_ctc:
            # the head's log-likelihood of every slot's tokens: the head once on the audio states, then all B x W slots in one call, each
            # on its utterance's logits, straight from the beam's history and length arrays (an utterance has at most T_max tokens)
            ctc = ops.ctc_score_hyps(self._ctc_head_logits(enc_states), T_len,
                                     cur["hist"].view(B * W, ld_hist)[:, 1:1 + T_max], cur["meta"][0].reshape(B * W), None, blank=0)
            packed = torch.cat([packed, ctc.view(B, W, 1)], dim=2)
        packed = packed.cpu()
        lm_col = -1 - int(use_ctc)
        bias_col = lm_col - int(fused)
        out, biases, lms, ctcs = [], [], [], []
        for b in range(B):
            res, bias, lmt, ctl = [], [], [], []
            for w in range(W):
                score, c = float(packed[b, w, 0]), int(packed[b, w, 1])
                if not score > -math.inf:                            # an empty slot
                    continue
                tok, frm, lpr = (packed[b, w, 2 + i * ld_det:2 + i * ld_det + c].tolist() for i in range(3))
                res.append(DecodeResult([int(v) for v in tok], [int(v) for v in frm], lpr, score))
                bias.append(0.0 if context is None else float(packed[b, w, bias_col]))
                lmt.append(float(packed[b, w, lm_col]) if fused else 0.0)
                ctl.append(float(packed[b, w, -1]) if use_ctc else 0.0)
            if ctc_weight > 0.0:                                     # the head's term joins the key; what it cannot align comes last
                order = sorted(range(len(res)), key=lambda n: (0, -(res[n].score + bias[n] + lmt[n] + ctc_weight * ctl[n]), n) if math.isfinite(ctl[n])
                               else (1, -(res[n].score + bias[n] + lmt[n]), n))
                res, bias, lmt, ctl = ([v[n] for n in order] for v in (res, bias, lmt, ctl))
            elif fused:                                              # ... and so does the LM's closing term
                order = sorted(range(len(res)), key=lambda n: (-(res[n].score + bias[n] + lmt[n]), n))
                res, bias, lmt, ctl = ([v[n] for n in order] for v in (res, bias, lmt, ctl))
            elif context is not None:                                # the slots are in key order with the running bias; the final bias reorders
                order = sorted(range(len(res)), key=lambda n: (-(res[n].score + bias[n]), n))
                res, bias, ctl = ([v[n] for n in order] for v in (res, bias, ctl))
            if not res or not math.isfinite(res[0].score):
                raise RuntimeError("beam search: utterance %d has no hypothesis with a finite score (NaN logits?)" % b)
            out.append(res[:nbest])
            biases.append(bias[:nbest])
            lms.append(lmt[:nbest])
            ctcs.append(ctl[:nbest])
        ret = (out,) + ((biases,) if return_bias else ()) + ((lms,) if return_lm else ()) + ((ctcs,) if return_ctc else ())
        return ret if len(ret) > 1 else out

    def beam_search_state(self, B, beam_width=4, context=None, lm=None, lm_weight=0.0, ilm_weight=0.0, length_bonus=0.0, history="full",
                          max_history=40, capacity=None):
        """`beam_decode_batch`'s search of B utterances as an object that takes the encoder frames in blocks -> ttmi.beam.BeamSearch:
        advance(enc_frames [B, n, d], n_valid) as often as frames arrive, stable() = how many leading tokens of each utterance can no longer
        change, partial() = the currently best hypothesis, finish(nbest, return_bias, return_lm) = what beam_decode_batch returns for the same
        frames, bit for bit, however they were split.  context / lm / lm_weight / ilm_weight / length_bonus as there.  history = "full": the
        label state of a hypothesis is decoder([start] + tokens) as there; "stream": the streaming recogniser's rule, decoder(the last
        max_history tokens) without a leading start symbol.  capacity = the columns the history buffers start with (default 64; they grow)."""
        self._refuse_tdt("resumable beam search (beam_search_state, StreamingRecognizer)")
        from ttmi.beam import BeamSearch
        return BeamSearch(self, B, beam_width, context=context, lm=lm, lm_weight=lm_weight, ilm_weight=ilm_weight, length_bonus=length_bonus,
                          history=history, max_history=max_history, capacity=capacity)

    @torch.no_grad()
    def recognize_nbest(self, inputs, inputs_length=None, audio_mask=None, beam_width=4, nbest=None, context=None, return_bias=False, lm=None,
                        lm_weight=0.0, ilm_weight=0.0, length_bonus=0.0, return_lm=False, ctc_weight=0.0, return_ctc=False):
        """N-best recognition of a batch: the encoder, then `beam_decode_batch` -> per utterance a list of at most `nbest` (default:
        beam_width) DecodeResult, best first, with merged, comparable scores; `context` / `return_bias`: contextual biasing, `lm` /
        `lm_weight` / `ilm_weight` / `length_bonus` / `return_lm`: language-model fusion, `ctc_weight` / `return_ctc`: rescoring of the
        final beam with the CTC head, see there"""
        self._refuse_tdt("beam search (recognize_nbest)")
        if not inputs.is_cuda:
            raise ValueError("recognize_nbest: inputs must live on the GPU (the MI355X build has no CPU path)")
        enc_states = self.encoder(inputs, audio_mask)
        return self.beam_decode_batch(enc_states, inputs_length, beam_width=beam_width, nbest=nbest, context=context, return_bias=return_bias,
                                      lm=lm, lm_weight=lm_weight, ilm_weight=ilm_weight, length_bonus=length_bonus, return_lm=return_lm,
                                      ctc_weight=ctc_weight, return_ctc=return_ctc)

    @torch.no_grad()
    def beam_search(self, enc_state, lengths, beam_width=5, block=64):
        """The reference's beam search (tt/model.py:110-179), quirks included - frames advance on the currently most probable hypothesis;
        expansion happens only when that hypothesis predicts a non-blank; on an expanding frame every hypothesis contributes its top
        `beam_width` non-blank symbols; child token lists persist across expansions (appended to, never re-seeded from their parents) - with
        the device doing the per-frame work (round 5; the round-2 restatement, one label-encoder call and one `.item()` per hypothesis and
        frame, is `_beam_search_per_frame`, selected with block = 0):
          * every hypothesis has the same length (each expansion appends one symbol to every child list), so the `beam_width` label states
            come from ONE label-encoder call per expansion, and only change at expansions;
          * between expansions the lead hypothesis is fixed: `block` frames are scored against ITS label state in one joint call and the first
            non-blank frame is found on the device (ttmi_greedy_scan), as in `decode`;
          * on the expanding frame one joint call scores all hypotheses, softmax + top-(beam_width + 1) run on the device, and ONE host read
            brings the beam_width x (beam_width + 1) (probability, symbol) pairs back for the reference's own bookkeeping.
        Host reads: two per expansion + one per scanned block, instead of (1 + beam_width) per frame."""
        self._refuse_tdt("beam search (beam_search)")
        if not enc_state.is_cuda or not block:
            return self._beam_search_per_frame(enc_state, lengths, beam_width)
        dev, W, T = enc_state.device, beam_width, int(lengths)
        hyps = [[0] for _ in range(W)]
        score = np.zeros((W,), dtype=float)
        child = [[[0] for _ in range(W)] for _ in range(W)]
        child_score = np.zeros((W, W), dtype=float)
        first = True

        def label_states():
            """[W, d]: the label encoder (no look-ahead mask, tt/model.py:118) on the W histories, all of one length"""
            return self.decoder(torch.tensor(hyps, dtype=torch.long, device=dev))[:, -1, :]

        dec = label_states()
        t = 0
        while t < T:
            lead = int(score.argmax())
            n = min(block, T - t)
            logits = self.joint(enc_state[t:t + n].unsqueeze(0), dec[lead:lead + 1].unsqueeze(0))          # [1, n, 1, V]
            row, tok = ops.greedy_scan(logits[0, :, 0, :])
            if tok is None:                                     # the lead hypothesis predicts blank on all n frames
                t += n
                continue
            if tok >= self.config.vocab_size:
                raise RuntimeError("beam search: the joint produced no finite maximum at frame %d (NaN logits?)" % (t + row))
            te = t + row
            z = self.joint(enc_state[te:te + 1].unsqueeze(0), dec.unsqueeze(0))[0, 0]                     # [W, V]: every hypothesis on the expanding frame
            values, indices = torch.topk(F.softmax(z.float(), dim=-1), k=W + 1, dim=-1)
            both = torch.cat([values.double(), indices.double()], dim=1).cpu().tolist()                   # ONE host read per expansion
            for k in range(W):
                vals, idxs = both[k][:W + 1], [int(v) for v in both[k][W + 1:]]
                drop = idxs.index(0) if 0 in idxs else len(idxs) - 1
                idxs.pop(drop)
                vals.pop(drop)
                for i, sym in enumerate(idxs):
                    if first:
                        child[i][k].append(sym)
                    else:
                        child[k][i].append(sym)
                if first:
                    child_score[:, k] = np.log(vals)
                else:
                    child_score[k] = score[k] + np.log(vals)
            if first:
                first = False
                for i in range(W):
                    hyps[i] = copy.deepcopy(child[i][0])
                    score[i] = child_score[i, 0]
            else:
                best = heapq.nlargest(W, range(W ** 2), child_score.take)
                for i, idx in enumerate(best):
                    score[i] = child_score[idx // W, idx % W]
                    hyps[i] = copy.deepcopy(child[idx // W][idx % W])
            dec = label_states()
            t = te + 1
        return hyps[int(score.argmax())][1:]

    @torch.no_grad()
    def _beam_search_per_frame(self, enc_state, lengths, beam_width=5):
        """(round 2; `beam_search(block=0)`) Restatement of the reference's beam search (tt/model.py:110-179) including its quirks: frames advance on the
        currently most probable hypothesis; expansion happens only when that hypothesis predicts a non-blank; child
        token lists persist across expansions (they are appended to, never re-seeded from their parents)."""
        self._refuse_tdt("beam search (beam_search)")
        dev = enc_state.device

        def posterior(tokens, t):
            d = self.decoder(torch.tensor([tokens], dtype=torch.long, device=dev))[:, -1, :]
            return F.softmax(self.joint(enc_state[t].view(-1), d.view(-1)), dim=0)

        hyps = [[0] for _ in range(beam_width)]
        score = np.zeros((beam_width,), dtype=float)
        child = [[[0] for _ in range(beam_width)] for _ in range(beam_width)]
        child_score = np.zeros((beam_width, beam_width), dtype=float)
        first = True
        for t in range(int(lengths)):
            lead = int(score.argmax())
            if int(torch.argmax(posterior(hyps[lead], t)).item()) == 0:
                continue
            for k in range(beam_width):
                values, indices = torch.topk(posterior(hyps[k], t), k=beam_width + 1, dim=0)
                values, indices = values.tolist(), indices.tolist()
                drop = indices.index(0) if 0 in indices else len(indices) - 1
                indices.pop(drop)
                values.pop(drop)
                for i, tok in enumerate(indices):
                    if first:
                        child[i][k].append(tok)
                    else:
                        child[k][i].append(tok)
                if first:
                    child_score[:, k] = np.log(values)
                else:
                    child_score[k] = score[k] + np.log(values)
            if first:
                first = False
                for i in range(beam_width):
                    hyps[i] = copy.deepcopy(child[i][0])
                    score[i] = child_score[i, 0]
            else:
                best = heapq.nlargest(beam_width, range(beam_width ** 2), child_score.take)
                for i, idx in enumerate(best):
                    score[i] = child_score[idx // beam_width, idx % beam_width]
                    hyps[i] = copy.deepcopy(child[idx // beam_width][idx % beam_width])
        return hyps[int(score.argmax())][1:]

    @torch.no_grad()
    def recognize_beam_search(self, inputs, inputs_length, audio_mask=None):
        self._refuse_tdt("beam search (recognize_beam_search)")
        enc_states = self.encoder(inputs, audio_mask)
        return [self.beam_search(enc_states[b], inputs_length[b], beam_width=5) for b in range(inputs.size(0))]
