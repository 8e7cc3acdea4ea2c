"""Thin typed wrappers: torch tensors -> raw device pointers -> libttmi C ABI.

torch is plumbing only (device memory, current stream).  Every function here
launches hand-written HIP kernels; none has a PyTorch/CPU fallback.
"""
import ctypes
import math
import os
import sys

import torch

from . import check, lib

c_int, c_long, c_float, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p


_TRACE = bool(os.environ.get("TTMI_TRACE_CALLS"))       # debugging: name and shape of every layer-level call on stderr before it is issued


def _trace(name, *dims):
    if _TRACE:
        print("[ttmi] %s %s stream %x" % (name, dims, torch.cuda.current_stream().cuda_stream), file=sys.stderr, flush=True)


def _p(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def weights_fresh():
    """called at the module-level entry points (BuildEncoder / BuildDecoder / JointNet forward, Transducer.loss) before weights are handed
    to the library: if a ttmi.train.FlatModel keeps bf16 weight shadows and a parameter was changed through torch since their last
    refresh, they are rebuilt first.  Free when no shadows exist."""
    import sys
    tr = sys.modules.get("ttmi.train")
    if tr is not None and tr._shadowed:
        tr.ensure_fresh()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("ttmi ops need device tensors (no CPU fallback); got a %s tensor" % t.device)


# ----------------------------------------------------------------------------- row-padded views
def row_pitch(t):
    """t [..., V] -> pitch (elements between consecutive rows) if t is a dense tensor or a [..., :V] view of a dense
    [..., pitch] buffer (what the bf16 joint produces: pitch = V rounded up to 64); else None."""
    if t.dim() < 2 or t.stride(-1) != 1:
        return None
    ld = t.stride(-2)
    if ld < t.shape[-1]:
        return None
    for i in range(t.dim() - 2):
        if t.shape[i] > 1 and t.stride(i) != t.stride(i + 1) * t.shape[i + 1]:
            return None
    return ld


def padded_empty(shape, dtype, device, multiple=64):
    """dense [..., roundup(V, multiple)] buffer and its [..., :V] view"""
    V = shape[-1]
    Vp = (V + multiple - 1) // multiple * multiple
    buf = torch.empty(*shape[:-1], Vp, dtype=dtype, device=device)
    return buf, buf[..., :V]


# gradients written by rnnt_loss_bwd carry exact zeros in their pad columns; the joint's fast dgrad relies on that.  The guarantee is
# attached to the gradient's TENSOR OBJECT (attribute `_ttmi_zero_pad` = its pitch), never to a raw address: a foreign gradient that the
# caching allocator happens to place where an earlier one lived must not inherit it.


def _sized(name, *args, restype=ctypes.c_size_t):
    """call a library entry that does not return an int status: a byte / float / row count (size_t unless `restype` says otherwise).  The
    restype is set the first time the symbol is used and found in place afterwards"""
    f = getattr(lib(), name)
    if f.restype is not restype:
        f.restype = restype
    return f(*args)


def grad_buffer(logits, inplace=False, zero_pad=True):
    """where a loss gradient of `logits` ([..., V], dense or row-padded view) goes -> (grad, pitch): the logits themselves (inplace), a dense
    tensor when the logits are dense, else the [..., :V] view of a new buffer of the logits' pitch.  zero_pad: the kernel that fills it
    writes exact zeros into the pad columns, so a padded `grad` carries the `_ttmi_zero_pad` mark (above)"""
    V, ld = logits.shape[-1], row_pitch(logits)
    assert ld is not None
    if inplace:
        grad = logits
    elif ld == V:
        grad = torch.empty_like(logits)
    else:
        grad = torch.empty(*logits.shape[:-1], ld, dtype=logits.dtype, device=logits.device)[..., :V]
    if zero_pad and ld != V:
        grad._ttmi_zero_pad = ld
    return grad, ld


def reduce_costs(costs, reduction):
    """the two-call losses' reduction of per-utterance costs [B]: 'none' -> costs, 'sum' -> [1], 'mean' -> [1], the sum DIVIDED by B (the
    fused ops of tt.model multiply by 1 / B instead: the last bit differs, and each keeps its own)"""
    if reduction == "none":
        return costs
    out = costs.sum().reshape(1)
    return out / costs.shape[0] if reduction == "mean" else out


def grad_out_args(grad_out, reduction, B):
    """the upstream gradient of reduce_costs' result -> the (grad_out, grad_out_stride, scale) arguments of a *_loss_bwd call"""
    return grad_out.contiguous().float(), 1 if reduction == "none" else 0, 1.0 / B if reduction == "mean" else 1.0


# ----------------------------------------------------------------------------- the transducer lattices (RNN-T loss, alignment, statistics)
def check_fastemit(fastemit_lambda):
    """-> fastemit_lambda as a float; ValueError unless it is a finite number >= 0 (the library checks again)"""
    try:
        v = float(fastemit_lambda)
    except (TypeError, ValueError):
        raise ValueError("fastemit_lambda must be a finite float >= 0, got %r" % (fastemit_lambda,)) from None
    if not math.isfinite(v) or v < 0.0:
        raise ValueError("fastemit_lambda must be a finite float >= 0, got %r" % (fastemit_lambda,))
    return v


class Lattice:
    """One transducer lattice the loss kernels walk: the library symbols of its six entries and the facts callers branch on.  The
    underscored methods are the wrappers of both lattices, one body each; what differs between the lattices is said in each docstring.
    lat.workspace / .loss_fwd / .loss_bwd / .align / .emit_stats are this module's rnnt_* / mono_* functions below."""
    __slots__ = ("name", "prefix", "takes_fastemit", "has_exp_forms", "label_takes_frame", "symbols")
    ENTRIES = ("workspace", "loss_fwd", "loss_bwd", "align", "emit_stats")

    def __init__(self, name, prefix, takes_fastemit, has_exp_forms, label_takes_frame, **symbols):
        # takes_fastemit: the gradient entry ends in a FastEmit weight; has_exp_forms: the exp-domain and bf16x3 split-plane chunk forms
        # (rnnt_loss_fwd_exp / _bwd_exp / _bwd_split, rnnt_shift_seed below) exist for it; label_takes_frame: an utterance with more labels
        # than frames has no path (the callers' length checks refuse it)
        self.name, self.prefix, self.symbols = name, prefix, symbols
        self.takes_fastemit, self.has_exp_forms, self.label_takes_frame = takes_fastemit, has_exp_forms, label_takes_frame

    def __getattr__(self, entry):
        # looked up by name at call time: whoever wraps ops.rnnt_loss_bwd (tests count calls that way) sees the calls made through a record too
        if entry in Lattice.ENTRIES:
            return globals()["%s_%s" % (self.prefix, entry)]
        raise AttributeError(entry)

    def fastemit_kw(self, fastemit_lambda):
        """the keyword of lat.loss_bwd that only a lattice with a FastEmit gradient takes"""
        return {"fastemit_lambda": fastemit_lambda} if self.takes_fastemit else {}

    def _call(self, entry, *args):
        sym = self.symbols[entry]
        check(getattr(lib(), sym)(*args, _stream()), sym)

    def _workspace(self, B, T, U1, device):
        n = _sized(self.symbols["workspace"], c_int(B), c_int(T), c_int(U1))
        return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)

    def _loss_fwd(self, logits, labels, act_lens, label_lens, blank, workspace):
        """logits: f32/bf16 [B,T,U1,V], dense or row-padded view -> costs f32 [B]; 'monotonic': on the decoders' one-symbol-per-frame lattice
        (include/ttmi.h)"""
        _need_cuda(logits, labels, act_lens, label_lens, workspace)
        B, T, U1, V = logits.shape
        ld = row_pitch(logits)
        assert ld is not None
        costs = torch.empty(B, dtype=torch.float32, device=logits.device)
        self._call("loss_fwd", _p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                   c_int(U1), c_int(V), c_int(blank), _p(workspace), _p(costs))
        return costs

    def _loss_bwd(self, logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False, fastemit_lambda=0.0):
        """inplace: the gradient overwrites the logits (same dtype and pitch; the fused joint + loss path needs them only once).
        fastemit_lambda > 0: the FastEmit gradient (include/ttmi.h, ttmi_rnnt_loss_bwd_fe); 'monotonic' has none: neither ttmi_mono_loss_bwd
        nor mono_loss_bwd takes such an argument"""
        fe = check_fastemit(fastemit_lambda)
        _need_cuda(logits, labels, act_lens, label_lens, workspace, grad_out)
        B, T, U1, V = logits.shape
        grad, ld = grad_buffer(logits, inplace)
        self._call("loss_bwd", _p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                   c_int(U1), c_int(V), c_int(blank), _p(workspace), _p(grad_out), c_int(grad_out_stride), c_float(scale), _p(grad), c_long(ld),
                   *((c_float(fe),) if self.takes_fastemit else ()))
        return grad

    def _align(self, workspace, act_lens, label_lens, B, T, U1):
        """best path through the lattice a finished loss_fwd (or rnnt_loss_fwd_exp) left in `workspace` (read only) -> (frames int32
        [B, U1-1], -1 for u >= U_b; score f32 [B]: the path's log-probability).  'rnnt': frames[u] = the frame at which label u+1 is emitted,
        non-decreasing.  'monotonic': the frame whose one decision is label u+1, STRICTLY increasing; score -inf with all frames -1 for an
        utterance with more labels than frames.  The label move is taken only when strictly greater (a tie goes to blank); include/ttmi.h,
        ttmi_rnnt_align / ttmi_mono_align"""
        _need_cuda(workspace, act_lens, label_lens)
        _trace(self.symbols["align"][5:], B, T, U1)
        n = _sized(self.symbols["align_workspace"], c_int(B), c_int(T), c_int(U1))
        aws = torch.empty((n + 7) // 8, dtype=torch.int64, device=workspace.device)
        frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=workspace.device)
        score = torch.empty(B, dtype=torch.float32, device=workspace.device)
        self._call("align", _p(workspace), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(U1), _p(aws), _p(frames), _p(score))
        return frames, score

    def _emit_stats(self, workspace, act_lens, label_lens, B, T, U1):
        """per label, from the alpha / beta of a finished forward in `workspace` (read only) -> (expected f32 [B, U1-1]: expected emission frame,
        -1 for u >= U_b; mass f32 [B, U1-1]: total emission posterior, 1 for a healthy lattice, 0 for u >= U_b); 'monotonic': an utterance
        without a path has 0 / -1 in every entry"""
        _need_cuda(workspace, act_lens, label_lens)
        _trace(self.symbols["emit_stats"][5:], B, T, U1)
        expected = torch.empty(B, U1 - 1, dtype=torch.float32, device=workspace.device)
        mass = torch.empty(B, U1 - 1, dtype=torch.float32, device=workspace.device)
        self._call("emit_stats", _p(workspace), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(U1), _p(expected), _p(mass))
        return expected, mass


LATTICES = {
    "rnnt": Lattice("rnnt", "rnnt", True, True, False, workspace="ttmi_rnnt_workspace_bytes", loss_fwd="ttmi_rnnt_loss_fwd", loss_bwd="ttmi_rnnt_loss_bwd_fe",
                    align_workspace="ttmi_rnnt_align_workspace_bytes", align="ttmi_rnnt_align", emit_stats="ttmi_rnnt_emit_stats"),
    "monotonic": Lattice("monotonic", "mono", False, False, True, workspace="ttmi_mono_workspace_bytes", loss_fwd="ttmi_mono_loss_fwd",
                         loss_bwd="ttmi_mono_loss_bwd", align_workspace="ttmi_mono_align_workspace_bytes", align="ttmi_mono_align",
                         emit_stats="ttmi_mono_emit_stats"),
}
TOPOLOGIES = tuple(LATTICES)


def check_topology(topology, fastemit_lambda=0.0):
    """-> topology; ValueError unless it names a lattice the loss kernels walk, or for FastEmit on the monotonic one (not built)"""
    if topology not in TOPOLOGIES:
        raise ValueError("topology must be 'rnnt' or 'monotonic', got %r" % (topology,))
    if topology == "monotonic" and fastemit_lambda > 0.0:
        raise ValueError("topology='monotonic' does not take fastemit_lambda > 0 (FastEmit is defined on the standard lattice here)")
    return topology


def lattice(topology, fastemit_lambda=0.0):
    """-> the Lattice record of `topology`, after check_topology's checks"""
    return LATTICES[check_topology(topology, fastemit_lambda)]


# the per-lattice names of the wrappers above: what a record's entries resolve to, and what tests and tools call
_RNNT, _MONO = LATTICES["rnnt"], LATTICES["monotonic"]


def rnnt_workspace(B, T, U1, device):
    return _RNNT._workspace(B, T, U1, device)


def rnnt_loss_fwd(logits, labels, act_lens, label_lens, blank, workspace):
    return _RNNT._loss_fwd(logits, labels, act_lens, label_lens, blank, workspace)


def rnnt_loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False, fastemit_lambda=0.0):
    return _RNNT._loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace, fastemit_lambda)


def rnnt_align(workspace, act_lens, label_lens, B, T, U1):
    return _RNNT._align(workspace, act_lens, label_lens, B, T, U1)


def rnnt_emit_stats(workspace, act_lens, label_lens, B, T, U1):
    return _RNNT._emit_stats(workspace, act_lens, label_lens, B, T, U1)


def mono_workspace(B, T, U1, device):
    return _MONO._workspace(B, T, U1, device)


def mono_loss_fwd(logits, labels, act_lens, label_lens, blank, workspace):
    return _MONO._loss_fwd(logits, labels, act_lens, label_lens, blank, workspace)


def mono_loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False):
    return _MONO._loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace)


def mono_align(workspace, act_lens, label_lens, B, T, U1):
    return _MONO._align(workspace, act_lens, label_lens, B, T, U1)


def mono_emit_stats(workspace, act_lens, label_lens, B, T, U1):
    return _MONO._emit_stats(workspace, act_lens, label_lens, B, T, U1)


# ----------------------------------------------------------------------------- token-and-duration transducer (csrc/tdt.hip)
TDT_MAX_DURATION = 8


def check_durations(durations):
    """-> durations as a tuple of ints; ValueError unless they are distinct integers in [1, 8], at most 8 of them, in strictly increasing
    order.  Duration 0 (several tokens on one frame) is refused: every decoder of this library consumes the emitting frame."""
    try:
        ds = tuple(durations)
    except TypeError:
        raise ValueError("TDT durations must be a sequence of integers in [1, %d], got %r" % (TDT_MAX_DURATION, durations)) from None
    if not 1 <= len(ds) <= TDT_MAX_DURATION:
        raise ValueError("TDT durations: between 1 and %d durations, got %d" % (TDT_MAX_DURATION, len(ds)))
    for d in ds:
        if isinstance(d, bool) or not isinstance(d, int):
            raise ValueError("TDT durations must be integers, got %r" % (d,))
        if d == 0:
            raise ValueError("TDT duration 0 (several tokens on one frame) is not built: every decoder here consumes the emitting frame; "
                             "durations must lie in [1, %d]" % TDT_MAX_DURATION)
        if not 1 <= d <= TDT_MAX_DURATION:
            raise ValueError("TDT duration %d outside [1, %d]" % (d, TDT_MAX_DURATION))
    if any(b <= a for a, b in zip(ds, ds[1:])):
        raise ValueError("TDT durations must be strictly increasing, got %r" % (ds,))
    return ds


def _c_durations(durations):
    ds = check_durations(durations)
    return (c_int * len(ds))(*ds), c_int(len(ds))


def _tdt_args(logits, D):
    if logits.dim() != 4 or logits.dtype not in _DT or _DT[logits.dtype] > 1:
        raise ValueError("TDT: logits must be an f32 / bf16 tensor [B, T, U1, V + D]")
    B, T, U1, W = logits.shape
    if W - D < 1:
        raise ValueError("TDT: the last dimension (%d) must hold at least one token column and the %d duration columns" % (W, D))
    ld = row_pitch(logits)
    if ld is None:
        raise ValueError("TDT: logits must be dense or a row-padded [..., :V + D] view")
    return B, T, U1, W - D, ld


def tdt_workspace(B, T, U1, D, device):
    n = _sized("ttmi_tdt_workspace_bytes", c_int(B), c_int(T), c_int(U1), c_int(D))
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)


def tdt_loss_fwd(logits, labels, act_lens, label_lens, blank, durations, workspace):
    """logits: f32 / bf16 [B, T, U1, V + D], dense or row-padded view: V token columns, then the D = len(durations) duration columns -> costs
    f32 [B] on the token-and-duration lattice (include/ttmi.h: ttmi_tdt_loss_fwd); +inf for an utterance without a path"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace)
    dur, D = _c_durations(durations)
    B, T, U1, V, ld = _tdt_args(logits, D.value)
    _trace("tdt_loss_fwd", B, T, U1, V, D.value)
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(lib().ttmi_tdt_loss_fwd(_p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                                  c_int(U1), c_int(V), c_int(blank), dur, D, _p(workspace), _p(costs), _stream()), "ttmi_tdt_loss_fwd")
    return costs


def tdt_loss_bwd(logits, labels, act_lens, label_lens, blank, durations, workspace, grad_out, grad_out_stride, scale, inplace=False):
    """scale * grad_out[b * grad_out_stride] * d costs[b] / d logits over all V + D columns, with the logits' pitch (pad columns zero);
    inplace: written over the logits (ttmi_tdt_loss_bwd)"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace, grad_out)
    dur, D = _c_durations(durations)
    B, T, U1, V, ld = _tdt_args(logits, D.value)
    _trace("tdt_loss_bwd", B, T, U1, V, D.value)
    grad, ld = grad_buffer(logits, inplace)
    check(lib().ttmi_tdt_loss_bwd(_p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                                  c_int(U1), c_int(V), c_int(blank), dur, D, _p(workspace), _p(grad_out), c_int(grad_out_stride),
                                  c_float(scale), _p(grad), c_long(ld), _stream()), "ttmi_tdt_loss_bwd")
    return grad


def tdt_scan_batch(logits, D, t, T_len, need, dec, lp):
    """logits [B, n, V + D] (f32 / bf16, row pitch = stride(-2)): for every existing row of the block, dec [B, n, 2] (i32) = (argmax token,
    argmax duration index) and lp [B, n, 2] (f32) = their log-probabilities, each sub-row normalised by itself (include/ttmi.h:
    ttmi_tdt_scan_batch); rows it skips keep what dec / lp held; device only, no synchronisation"""
    B, n, W = logits.shape
    _need_cuda(logits, t, T_len, need, dec, lp)
    assert dec.dtype is torch.int32 and dec.is_contiguous() and tuple(dec.shape) == (B, n, 2)
    assert lp.dtype is torch.float32 and lp.is_contiguous() and tuple(lp.shape) == (B, n, 2)
    check(lib().ttmi_tdt_scan_batch(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(n), c_int(W - D), c_int(D),
                                    _p(t), _p(T_len), _p(need), _p(dec), _p(lp), _stream()), "ttmi_tdt_scan_batch")


def tdt_advance(dec, lp, durations, n_hist, hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, score, blank=0):
    """follow the jumps through the scanned block (ttmi_tdt_advance): histories, frame positions (a jump that leaves the block carries over)
    and the need / done flags move on the device; frames (i32) / tok_lp (f32) / tok_dur (i32) [B, ld_det] get the emission frame,
    log-probability and duration of the symbol appended at column count[b]; score (f64 [B]) the log-probability of the decisions taken;
    flags[0] = utterances that still need a symbol in this step, flags[1] = utterances not finished"""
    B, n = dec.shape[0], dec.shape[1]
    _need_cuda(dec, lp, hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, score)
    dur, D = _c_durations(durations)
    assert hist.dtype is torch.long and hist.stride(1) == 1
    assert dec.dtype is torch.int32 and dec.is_contiguous() and lp.dtype is torch.float32 and lp.is_contiguous() and tuple(lp.shape) == (B, n, 2)
    assert frames.dtype is torch.int32 and tok_lp.dtype is torch.float32 and tok_dur.dtype is torch.int32
    assert frames.stride(1) == 1 and tok_lp.stride(1) == 1 and tok_dur.stride(1) == 1 and frames.shape[0] == B
    assert tok_lp.shape == frames.shape and tok_dur.shape == frames.shape and frames.stride(0) == tok_lp.stride(0) == tok_dur.stride(0)
    assert score.dtype is torch.float64 and score.is_contiguous() and score.shape[0] == B
    check(lib().ttmi_tdt_advance(_p(dec), _p(lp), c_int(B), c_int(n), c_int(blank), dur, D, c_int(n_hist), _p(hist), c_long(hist.stride(0)),
                                 _p(t), _p(T_len), _p(need), _p(done), _p(count), _p(flags), _p(frames), _p(tok_lp), _p(tok_dur),
                                 c_long(frames.stride(0)), _p(score), _stream()), "ttmi_tdt_advance")


class TDTLattice:
    """The token-and-duration lattice as a record that quacks like `Lattice` for _LatticeLossFn (warprnnt_pytorch) and _JointLossFn
    (tt.model): .workspace / .loss_fwd / .loss_bwd with their signatures, and the facts callers branch on.  It is NOT in LATTICES: it is no
    topology of the same logits (its rows are V + D wide) and carries its durations.  Alignment and emission statistics are not built."""
    name, takes_fastemit, has_exp_forms, label_takes_frame = "tdt", False, False, True

    def __init__(self, durations):
        self.durations = check_durations(durations)

    def fastemit_kw(self, fastemit_lambda):
        return {}

    def workspace(self, B, T, U1, device):
        return tdt_workspace(B, T, U1, len(self.durations), device)

    def loss_fwd(self, logits, labels, act_lens, label_lens, blank, workspace):
        return tdt_loss_fwd(logits, labels, act_lens, label_lens, blank, self.durations, workspace)

    def loss_bwd(self, logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False):
        return tdt_loss_bwd(logits, labels, act_lens, label_lens, blank, self.durations, workspace, grad_out, grad_out_stride, scale, inplace)

    def align(self, *args, **kwargs):
        raise ValueError("TDT: forced alignment is not built on the token-and-duration lattice")

    def emit_stats(self, *args, **kwargs):
        raise ValueError("TDT: emission statistics are not built on the token-and-duration lattice")


# ----------------------------------------------------------------------------- distillation on collapsed lattice posteriors (csrc/distill.hip)
def kd_workspace(B, T, U1, device):
    n = _sized("ttmi_kd_workspace_bytes", c_int(B), c_int(T), c_int(U1))
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)


def _kd_args(logits, labels, act_lens, label_lens):
    if logits.dim() != 4 or logits.dtype not in _DT or _DT[logits.dtype] > 1:
        raise ValueError("kd: logits must be an f32 / bf16 tensor [B, T, U1, V]")
    B, T, U1, V = logits.shape
    if V < 2:
        raise ValueError("kd: V = %d < 2 (a blank and at least one label)" % V)
    ld = row_pitch(logits)
    if ld is None:
        raise ValueError("kd: logits must be dense or a row-padded [..., :V] view")
    for name, t, shape in (("labels", labels, (B, U1 - 1)), ("act_lens", act_lens, (B,)), ("label_lens", label_lens, (B,))):
        if t.dtype != torch.int32 or not t.is_contiguous() or (tuple(t.shape) != shape and not (name == "labels" and U1 == 1)):
            raise ValueError("kd: %s must be a contiguous int32 tensor %s" % (name, list(shape)))
    return B, T, U1, V, ld


def _kd_post(t, name, B, T, U1):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, T, U1, 3):
        raise ValueError("kd: %s must have shape [%d, %d, %d, 3]" % (name, B, T, U1))
    if t.dtype != torch.float32:
        raise ValueError("kd: %s must be float32, got %s" % (name, t.dtype))
    if not t.is_cuda:
        raise ValueError("kd: %s must live on the GPU (no CPU fallback)" % name)
    return t.contiguous()


def kd_collapse(logits, labels, act_lens, label_lens, blank=0):
    """logits f32 / bf16 [B,T,U1,V], dense or row-padded view -> f32 [B,T,U1,3]: (log P(blank), log P(y_{u+1}), log P(anything else)) of every
    lattice node, zeros outside the ragged lattice (include/ttmi.h, ttmi_kd_collapse)"""
    _need_cuda(logits, labels, act_lens, label_lens)
    B, T, U1, V, ld = _kd_args(logits, labels, act_lens, label_lens)
    _trace("kd_collapse", B, T, U1, V)
    post = torch.empty(B, T, U1, 3, dtype=torch.float32, device=logits.device)
    check(lib().ttmi_kd_collapse(_p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens),
                                 c_int(B), c_int(T), c_int(U1), c_int(V), c_int(blank), _p(post), _stream()), "ttmi_kd_collapse")
    return post


def kd_loss_fwd(logits, labels, act_lens, label_lens, blank, teacher, workspace):
    """-> costs f32 [B]: the KL divergence from the teacher's collapsed posteriors (f32 [B,T,U1,3], as kd_collapse gives them) to the
    student's, summed over each utterance's lattice nodes"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace)
    B, T, U1, V, ld = _kd_args(logits, labels, act_lens, label_lens)
    teacher = _kd_post(teacher, "teacher", B, T, U1)
    _trace("kd_loss_fwd", B, T, U1, V)
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(lib().ttmi_kd_loss_fwd(_p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens),
                                 c_int(B), c_int(T), c_int(U1), c_int(V), c_int(blank), _p(teacher), _p(workspace), _p(costs), _stream()),
          "ttmi_kd_loss_fwd")
    return costs


def kd_loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False, accumulate=None):
    """accumulate=None: the gradient is written - over the logits (inplace, same dtype and pitch) or to a new buffer of the logits' pitch, as
    in mono_loss_bwd.  accumulate=<tensor>: a gradient of the logits' shape and dtype (dense or row-padded) to which this one is ADDED over
    the lattice's rows, columns [0, V); no other byte of it is touched; the library refuses the logits themselves (ValueError)"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace, grad_out, accumulate)
    B, T, U1, V, ld = _kd_args(logits, labels, act_lens, label_lens)
    if accumulate is not None:
        if inplace:
            raise ValueError("kd_loss_bwd: accumulate and inplace exclude each other")
        if accumulate.shape != logits.shape or accumulate.dtype != logits.dtype or row_pitch(accumulate) is None:
            raise ValueError("kd_loss_bwd: accumulate must have the logits' shape and dtype (dense or row-padded)")
        grad, ldg = accumulate, row_pitch(accumulate)
    else:
        grad, ldg = grad_buffer(logits, inplace)
    _trace("kd_loss_bwd", B, T, U1, V)
    check(lib().ttmi_kd_loss_bwd(_p(logits), c_int(_DT[logits.dtype]), c_long(ld), _p(labels), _p(act_lens), _p(label_lens),
                                 c_int(B), c_int(T), c_int(U1), c_int(V), c_int(blank), _p(workspace), _p(grad_out),
                                 c_int(grad_out_stride), c_float(scale), _p(grad), c_long(ldg), c_int(0 if accumulate is None else 1),
                                 _stream()), "ttmi_kd_loss_bwd")
    return grad


# ----------------------------------------------------------------------------- CTC loss / greedy decode (auxiliary head on the audio encoder)
def ctc_workspace(B, T, U, device):
    n = _sized("ttmi_ctc_workspace_bytes", c_int(B), c_int(T), c_int(U))
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)


def _ctc_labels(labels, B):
    if labels.dim() != 2 or labels.shape[0] != B or labels.dtype is not torch.int32 or (labels.numel() and not labels.is_contiguous()):
        raise ValueError("ctc: labels must be contiguous int32 [B, U]")
    return labels.shape[1]


def _ctc_args(logits, labels):
    if logits.dim() != 3 or logits.dtype is not torch.float32:
        raise ValueError("ctc: logits must be f32 [B, T, V], got %s %s" % (logits.dtype, tuple(logits.shape)))
    ld = row_pitch(logits)
    if ld is None:
        raise ValueError("ctc: logits must be dense or a [..., :V] view of a row-padded buffer")
    _ctc_labels(labels, logits.shape[0])
    return ld


def ctc_loss_fwd(logits, labels, act_lens, label_lens, blank, workspace):
    """logits: f32 [B, T, V], dense or row-padded view; labels int32 [B, U] -> costs f32 [B] (include/ttmi.h: ttmi_ctc_loss_fwd)"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace)
    ld = _ctc_args(logits, labels)
    B, T, V = logits.shape
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(lib().ttmi_ctc_loss_fwd(_p(logits), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(labels.shape[1]),
                                  c_int(V), c_int(blank), _p(workspace), _p(costs), _stream()), "ttmi_ctc_loss_fwd")
    return costs


def ctc_loss_bwd(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, inplace=False):
    """scale * grad_out[b * grad_out_stride] * d costs[b] / d logits, with the logits' pitch (pad columns zero); inplace: written over the
    logits"""
    _need_cuda(logits, labels, act_lens, label_lens, workspace, grad_out)
    ld = _ctc_args(logits, labels)
    B, T, V = logits.shape
    grad, _ = grad_buffer(logits, inplace, zero_pad=False)
    check(lib().ttmi_ctc_loss_bwd(_p(logits), c_long(ld), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(labels.shape[1]),
                                  c_int(V), c_int(blank), _p(workspace), _p(grad_out), c_int(grad_out_stride), c_float(scale), _p(grad),
                                  c_long(ld), _stream()), "ttmi_ctc_loss_bwd")
    return grad


def ctc_greedy(logits, act_lens, blank=0):
    """logits f32 [B, T, V] (row pitch = stride(-2)), act_lens int32 [B] -> (tokens int32 [B, T], count int32 [B]): per utterance the
    argmax of its frames with repeats collapsed and blanks dropped in tokens[b, :count[b]]; count[b] = -(1 + t) when frame t has no
    finite maximum (include/ttmi.h: ttmi_ctc_greedy).  Device only, no synchronisation."""
    _need_cuda(logits, act_lens)
    if logits.dim() != 3 or logits.dtype is not torch.float32 or row_pitch(logits) is None:
        raise ValueError("ctc_greedy: logits must be f32 [B, T, V], dense or row-padded")
    B, T, V = logits.shape
    tokens = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    count = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib().ttmi_ctc_greedy(_p(logits), c_long(row_pitch(logits)), _p(act_lens), c_int(B), c_int(T), c_int(V), c_int(blank), _p(tokens),
                                _p(count), _stream()), "ttmi_ctc_greedy")
    return tokens, count


def ctc_align_workspace(B, T, U, device):
    """scratch of ctc_align (decision words when they do not fit LDS): int64 words, never empty (the entry wants a pointer whatever the shape)"""
    n = _sized("ttmi_ctc_align_workspace_bytes", c_int(B), c_int(T), c_int(U))
    return torch.empty(max((n + 7) // 8, 1), dtype=torch.int64, device=device)


def ctc_align(workspace, labels, act_lens, label_lens, B, T, V, blank=0, align_workspace=None):
    """the best path through the lattice a finished ctc_loss_fwd left in `workspace` (read only); labels int32 [B, U] -> (path int32 [B, T]:
    the state index of l' at every frame, -1 for t >= T_b; spans int32 [B, U, 2]: (first, last) frame of label u, -1 for u >= U_b; score
    f32 [B]: the path's log-probability).  An utterance with no feasible alignment: score -inf, every path / spans entry -1.  Predecessors
    are tried in the order s, s-1, s-2 and replaced only when strictly greater (include/ttmi.h, ttmi_ctc_align)"""
    _need_cuda(workspace, labels, act_lens, label_lens)
    U = _ctc_labels(labels, B)
    _trace("ctc_align", B, T, U)
    aws = ctc_align_workspace(B, T, U, workspace.device) if align_workspace is None else align_workspace
    path = torch.empty(B, T, dtype=torch.int32, device=workspace.device)
    spans = torch.empty(B, U, 2, dtype=torch.int32, device=workspace.device)
    score = torch.empty(B, dtype=torch.float32, device=workspace.device)
    check(lib().ttmi_ctc_align(_p(workspace), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(U), c_int(V), c_int(blank),
                               _p(aws), _p(path), _p(spans), _p(score), _stream()), "ttmi_ctc_align")
    return path, spans, score


def ctc_emit_stats(workspace, labels, act_lens, label_lens, B, T, V, blank=0):
    """from the alpha / beta of a finished ctc_loss_fwd in `workspace` (read only) -> (expected f32 [B, U]: expected onset frame of label u,
    -1 for u >= U_b; mass f32 [B, U]: total onset posterior, 1 for a healthy lattice; duration f32 [B, U]: expected number of frames the
    label occupies); an utterance with no feasible alignment has -1 / 0 / 0 in every entry (include/ttmi.h, ttmi_ctc_emit_stats)"""
    _need_cuda(workspace, labels, act_lens, label_lens)
    U = _ctc_labels(labels, B)
    _trace("ctc_emit_stats", B, T, U)
    expected, mass, duration = (torch.empty(B, U, dtype=torch.float32, device=workspace.device) for _ in range(3))
    check(lib().ttmi_ctc_emit_stats(_p(workspace), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(U), c_int(V),
                                    c_int(blank), _p(expected), _p(mass), _p(duration), _stream()), "ttmi_ctc_emit_stats")
    return expected, mass, duration


def ctc_score_workspace(B, T, device):
    """scratch of ctc_score_hyps (the log-sum-exp of every row): f32 words, never empty (the entry wants a pointer whatever the shape)"""
    n = _sized("ttmi_ctc_score_ws_bytes", c_int(B), c_int(T))
    return torch.empty(max((n + 3) // 4, 1), dtype=torch.float32, device=device)


def ctc_score_hyps(logits, act_lens, hyp, hyp_len, utt=None, blank=0, workspace=None):
    """logits f32 [B, T, V] (dense or row-padded view), act_lens int32 [B]; hyp int64 [P, U] (row pitch = stride(0): a column view of a
    beam's histories goes in as it is), hyp_len int32 [P], utt int32 [P] or None (None: P = B * N, pair p belongs to utterance p // N) ->
    score f64 [P]: the CTC log-likelihood of hypothesis p on the logits of its utterance, -inf where no alignment is feasible
    (include/ttmi.h: ttmi_ctc_score_hyps).  Device only, no synchronisation."""
    _need_cuda(logits, act_lens, hyp, hyp_len, utt, workspace)
    if logits.dim() != 3 or logits.dtype is not torch.float32:
        raise ValueError("ctc: logits must be f32 [B, T, V], got %s %s" % (logits.dtype, tuple(logits.shape)))
    ld = row_pitch(logits)
    if ld is None:
        raise ValueError("ctc: logits must be dense or a [..., :V] view of a row-padded buffer")
    B, T, V = logits.shape
    if hyp.dim() != 2 or hyp.dtype is not torch.int64 or (hyp.numel() and hyp.stride(1) != 1) or (hyp.shape[0] > 1 and hyp.stride(0) < hyp.shape[1]):
        raise ValueError("ctc_score_hyps: hyp must be int64 [P, U] with unit column stride")
    P, U = hyp.shape
    for name, t, n in (("act_lens", act_lens, B), ("hyp_len", hyp_len, P), ("utt", utt, P)):
        if t is not None and (t.dim() != 1 or t.shape[0] != n or t.dtype is not torch.int32 or not t.is_contiguous()):
            raise ValueError("ctc_score_hyps: %s must be contiguous int32 [%d]" % (name, n))
    _trace("ctc_score_hyps", B, T, P, U)
    ws = ctc_score_workspace(B, T, logits.device) if workspace is None else workspace
    score = torch.empty(P, dtype=torch.float64, device=logits.device)
    check(lib().ttmi_ctc_score_hyps(_p(logits), c_long(ld), _p(act_lens), c_int(B), c_int(T), c_int(V), c_int(blank), _p(hyp),
                                    c_long(hyp.stride(0) if P > 1 else max(U, 1)), _p(hyp_len), _p(utt), c_int(P), c_int(U), _p(ws), _p(score),
                                    _stream()), "ttmi_ctc_score_hyps")
    return score


def linear_nt(x, w, out, bias=None, prec=0, accumulate=False):
    """out[M, N] (f32, row pitch = out.stride(0)) (+)= x[M, K] @ w[N, K]^T (+ bias): the library's generic GEMM on f32 operands - exact-f32
    MFMA in the fp32 mode, the three-term bf16 split in the bf16x3 mode, bf16 MFMA with f32 accumulation and output in the bf16 mode"""
    M, K = x.shape
    N = w.shape[0]
    flags = GEMM_A_KMAJOR | GEMM_B_KMAJOR | (GEMM_BIAS if bias is not None else 0) | _PREC_FLAG[prec]
    return gemm(x, w, out, M, N, K, x.stride(0), w.stride(0), out.stride(0), flags, bias=bias, beta=1.0 if accumulate else 0.0)


def linear_nn(g, w, out, prec=0):
    """out[M, K] (f32) = g[M, N] @ w[N, K] (a linear layer's input gradient)"""
    M, N = g.shape
    K = w.shape[1]
    return gemm(g, w, out, M, K, N, g.stride(0), w.stride(0), out.stride(0), GEMM_A_KMAJOR | _PREC_FLAG[prec])


def linear_tn(g, x, out, prec=0, accumulate=True):
    """out[N, K] (f32) (+)= g[M, N]^T @ x[M, K] (a linear layer's weight gradient; x [M, 1] of ones: its bias gradient, the column sums
    of g).  One workgroup walks the whole reduction of a tile: no split along M, no atomics, the same bits in every run."""
    M, N = g.shape
    K = x.shape[1]
    return gemm(g, x, out, N, K, M, g.stride(0), x.stride(0), out.stride(0) if out.dim() == 2 else 1, _PREC_FLAG[prec],
                beta=1.0 if accumulate else 0.0)


# ----------------------------------------------------------------------------- generic GEMM (tests / bring-up)
GEMM_BIAS, GEMM_RELU, GEMM_ATOMIC, GEMM_MASK_AUX, GEMM_A_KMAJOR, GEMM_B_KMAJOR, GEMM_BF16_MFMA, GEMM_BF16X3 = 1, 2, 4, 8, 16, 32, 64, 128
_DT = {torch.float32: 0, torch.bfloat16: 1}
_PREC_FLAG = {0: 0, 1: GEMM_BF16_MFMA, 2: GEMM_BF16X3}       # precision code (tt.transformer.default_precision) -> compute flag of the generic GEMM


def gemm(A, B, C, M, N, K, lda, ldb, ldc, flags, bias=None, aux=None, alpha=1.0, beta=0.0, nz1=1, nz2=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), splitk=1):
    _need_cuda(A, B, C, bias, aux)
    check(lib().ttmi_gemm(_p(A), _p(B), _p(C), _p(bias), _p(aux), c_int(_DT[A.dtype]), c_int(_DT[B.dtype]),
                          c_int(_DT[C.dtype]), c_int(M), c_int(N), c_int(K), c_long(lda), c_long(ldb), c_long(ldc),
                          c_int(nz1), c_int(nz2), c_long(sA[0]), c_long(sA[1]), c_long(sB[0]), c_long(sB[1]),
                          c_long(sC[0]), c_long(sC[1]), c_float(alpha), c_float(beta), c_int(flags), c_int(splitk),
                          _stream()), "ttmi_gemm")
    return C


# ----------------------------------------------------------------------------- grouped weight gradients
class WgradDesc(ctypes.Structure):
    """ttmi_wgrad_desc (include/ttmi.h)"""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("colsum", c_void_p), ("M", c_int), ("N", c_int), ("K", c_int),
                ("lda", c_long), ("ldb", c_long), ("ldc", c_long)]


class _WgradLane:
    __slots__ = ("stream", "descs", "alive", "after")

    def __init__(self, stream):
        self.stream, self.descs, self.alive, self.after = stream, [], [], []


class WgradQueue:
    """Weight-gradient GEMMs of audio-sized encoder layers, held back until `group` layers' worth (4 problems each) are waiting and
    then launched together: 4 layers x 64 tiles = one 256 x 128 tile per CU over the whole reduction, no atomics (ttmi_wgrad_group).
    Holds the operand buffers alive until then; `after` callbacks (gradient-ready hooks of the deferred parameters) run after the launch.
    One lane per stream: a layer's problems are launched on the stream that produced their operands (the label encoder's backward pass
    runs on a side stream beside the audio encoder's; their entries never share a launch)."""

    def __init__(self, group=4, immediate_first_layer=False):
        self.limit = 4 * group
        # data-parallel runs: the first layer's gradients are the last of the step - whatever is reduced after them overlaps nothing.  Left
        # out of the groups they are ready as early as before; the layers behind them are launched when the first layer's backward STARTS.
        self.immediate_first_layer = immediate_first_layer
        self.lanes = {}

    def _lane(self):
        st = torch.cuda.current_stream()
        key = (st.device.index, st.cuda_stream)
        lane = self.lanes.get(key)
        if lane is None:
            lane = self.lanes[key] = _WgradLane(st)
        return lane

    @property
    def descs(self):
        return self._lane().descs

    def push(self, descs, tensors):
        lane = self._lane()
        lane.descs.extend(WgradDesc.from_buffer_copy(d) for d in descs)
        lane.alive.append(tensors)

    def add_callbacks(self, cbs):
        self._lane().after.extend(cbs)

    def maybe_flush(self, force=False):
        """the current stream's lane: launch if `group` layers wait (or anything at all with force)"""
        lane = self._lane()
        if lane.descs and (force or len(lane.descs) >= self.limit):
            arr = (WgradDesc * len(lane.descs))(*lane.descs)
            check(lib().ttmi_wgrad_group(arr, c_int(len(lane.descs)), _stream()), "ttmi_wgrad_group")
            cbs = lane.after
            lane.descs, lane.alive, lane.after = [], [], []
            for cb in cbs:
                cb()

    def flush_all(self):
        for lane in list(self.lanes.values()):
            if lane.descs:
                with torch.cuda.stream(lane.stream):
                    self.maybe_flush(force=True)

    def discard(self):
        """an aborted backward pass leaves entries behind: drop them (their gradients are lost with the step)"""
        self.lanes = {}


wgrad_queue = None          # set by ttmi.train.FlatModel.enable_grouped_wgrads(); read by the sub-layer backward passes


def wgrad_defer_supported(rows, d, H, Dh, Di, prec):
    return bool(lib().ttmi_wgrad_defer_supported(c_long(rows), c_int(d), c_int(H), c_int(Dh), c_int(Di), c_int(prec)))


def wgrad_flush(every_stream=False):
    """launch the weight gradients still queued on the current stream (end of an encoder's backward pass), or on every stream"""
    if wgrad_queue is not None:
        if every_stream:
            wgrad_queue.flush_all()
        else:
            wgrad_queue.maybe_flush(force=True)


# ----------------------------------------------------------------------------- sub-layers
class MaskSpec:
    """Attention mask handed to the kernels as parameters: kind 0 none, 1 causal
    (look_ahead_mask), 2 band (context_mask left/right), 3 arbitrary uint8 tensor [B|1, L, L], 4 per-row key intervals: int32 tensor
    [B|1, L, 2] of (lo, hi), key j of query i is masked iff j < lo or j > hi."""
    __slots__ = ("kind", "left", "right", "tensor")

    def __init__(self, kind=0, left=None, right=None, tensor=None):
        unknown = -1 if kind == 4 else 0
        self.kind, self.tensor = kind, tensor
        self.left = unknown if left is None else left
        self.right = unknown if right is None else right

    def args(self):
        t = self.tensor
        if self.kind == 4:
            # left / right: bounds on how far the intervals reach from the diagonal (-1 = not known)
            return c_int(4), c_int(self.left), c_int(self.right), _p(t), c_long(t.stride(0) if t.shape[0] > 1 else 0), c_long(2)
        if self.kind != 3:
            return c_int(self.kind), c_int(self.left), c_int(self.right), c_void_p(0), c_long(0), c_long(0)
        sb = t.stride(0) if t.shape[0] > 1 else 0
        si = t.stride(1) if t.shape[1] > 1 else 0
        return c_int(3), c_int(0), c_int(0), _p(t), c_long(sb), c_long(si)


def _f32(n, device):
    return torch.empty(int(n), dtype=torch.float32, device=device)


_ws_cache = {}
_side_streams = {}


def scratch(n, device):
    """One grow-only scratch arena per (device, stream): sub-layer drivers run back to back on a stream, so the
    scratch of one call is dead when the next call on that stream starts; concurrent streams get their own arena."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _ws_cache.get(key)
    if t is None or t.numel() < n:
        t = _ws_cache[key] = _f32(max(int(n), 1 << 20), device)
    return t


def scratch_generation(device, stream):
    """identity of `stream`'s scratch arena (its base address, None before first use): captured graphs hold this pointer, so whoever
    replays them must notice a re-allocation (the arena only ever grows)"""
    t = _ws_cache.get((device.type, device.index, stream.cuda_stream))
    return None if t is None else t.data_ptr()


def attn_fwd(x, p, mask, prec, p_drop=0.0, seed=0):
    """p: dict of parameter tensors (qkv_w, o_w, ln_g, ln_b, r_emb, r_w_bias, r_bias)."""
    _trace("attn_fwd", tuple(x.shape))
    _need_cuda(x)
    B, L, d = x.shape
    K, H, Dh = p["r_emb"].shape
    L_ = lib()
    ctx = _f32(_sized("ttmi_attn_ctx_floats", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(prec)), x.device)
    ws = scratch(_sized("ttmi_attn_ws_floats", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(prec)), x.device)
    y = torch.empty_like(x)
    check(L_.ttmi_attn_fwd(_p(x), _p(p["qkv_w"]), _p(p["o_w"]), _p(p["ln_g"]), _p(p["ln_b"]), _p(p["r_emb"]),
                           _p(p["r_w_bias"]), _p(p["r_bias"]), c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(K),
                           *mask.args(), c_int(prec), c_float(p_drop), ctypes.c_uint(seed), _p(ctx), _p(ws), _p(y), _stream()),
          "ttmi_attn_fwd")
    return y, ctx


def attn_bwd(dy, x, p, ctx, prec, grads, p_drop=0.0, seed=0, mask=None, defer=None):
    """grads: dict of ZERO-INITIALISED (or running) f32 buffers, accumulated into.  defer: a WgradQueue - the two weight-gradient GEMMs
    are queued for a grouped launch instead of run here (their gradients appear when the queue is flushed)."""
    _trace("attn_bwd", tuple(x.shape))
    B, L, d = x.shape
    K, H, Dh = p["r_emb"].shape
    L_ = lib()
    ws = scratch(_sized("ttmi_attn_ws_floats", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(prec)), x.device)
    dx = torch.empty_like(x)
    if defer is not None:
        keep = torch.empty(_sized("ttmi_attn_bwd_keep_bytes", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh)), dtype=torch.uint8, device=x.device)
        out = (WgradDesc * 2)()
        check(L_.ttmi_attn_bwd_defer(_p(dy), _p(x), _p(p["qkv_w"]), _p(p["o_w"]), _p(p["ln_g"]), _p(p["r_emb"]), _p(p["r_w_bias"]), _p(p["r_bias"]),
                                     c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(K), *(mask or MaskSpec()).args(), c_int(prec),
                                     c_float(p_drop), ctypes.c_uint(seed), _p(ctx), _p(ws), _p(dx),
                                     _p(grads["qkv_w"]), _p(grads["o_w"]), _p(grads["ln_g"]), _p(grads["ln_b"]), _p(grads["r_emb"]),
                                     _p(grads["r_w_bias"]), _p(grads["r_bias"]), _p(keep), out, _stream()), "ttmi_attn_bwd_defer")
        defer.push(out, (keep, ctx, grads["qkv_w"], grads["o_w"]))
        return dx
    check(L_.ttmi_attn_bwd(_p(dy), _p(x), _p(p["qkv_w"]), _p(p["o_w"]), _p(p["ln_g"]), _p(p["r_emb"]), _p(p["r_w_bias"]), _p(p["r_bias"]),
                           c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(K), *(mask or MaskSpec()).args(), c_int(prec),
                           c_float(p_drop), ctypes.c_uint(seed), _p(ctx), _p(ws), _p(dx),
                           _p(grads["qkv_w"]), _p(grads["o_w"]), _p(grads["ln_g"]), _p(grads["ln_b"]), _p(grads["r_emb"]),
                           _p(grads["r_w_bias"]), _p(grads["r_bias"]), _stream()), "ttmi_attn_bwd")
    return dx


def ffn_fwd(y, p, prec, p_drop=0.0, p_layer=0.0, seed=0):
    _trace("ffn_fwd", tuple(y.shape))
    rows, d = y.numel() // y.shape[-1], y.shape[-1]
    Di = p["ff_w1"].shape[0]
    L_ = lib()
    ctx = _f32(_sized("ttmi_ffn_ctx_floats", c_long(rows), c_int(d), c_int(Di), c_int(prec)), y.device)
    ws = scratch(_sized("ttmi_ffn_ws_floats", c_long(rows), c_int(d), c_int(Di), c_int(prec)), y.device)
    z = torch.empty_like(y)
    check(L_.ttmi_ffn_fwd(_p(y), _p(p["ff_w1"]), _p(p["ff_b1"]), _p(p["ff_w2"]), _p(p["ff_b2"]), _p(p["ff_ln_g"]),
                          _p(p["ff_ln_b"]), c_long(rows), c_int(d), c_int(Di), c_int(prec), c_float(p_drop), c_float(p_layer),
                          ctypes.c_uint(seed), _p(ctx), _p(ws), _p(z), _stream()),
          "ttmi_ffn_fwd")
    return z, ctx


def ffn_bwd(dz, y, p, ctx, prec, grads, p_drop=0.0, p_layer=0.0, seed=0, defer=None):
    _trace("ffn_bwd", tuple(y.shape))
    rows, d = y.numel() // y.shape[-1], y.shape[-1]
    Di = p["ff_w1"].shape[0]
    L_ = lib()
    ws = scratch(_sized("ttmi_ffn_ws_floats", c_long(rows), c_int(d), c_int(Di), c_int(prec)), y.device)
    dy = torch.empty_like(y)
    if defer is not None:
        keep = torch.empty(_sized("ttmi_ffn_bwd_keep_bytes", c_long(rows), c_int(d), c_int(Di)), dtype=torch.uint8, device=y.device)
        out = (WgradDesc * 2)()
        check(L_.ttmi_ffn_bwd_defer(_p(dz), _p(y), _p(p["ff_w1"]), _p(p["ff_w2"]), _p(p["ff_ln_g"]), c_long(rows), c_int(d), c_int(Di),
                                    c_int(prec), c_float(p_drop), c_float(p_layer), ctypes.c_uint(seed), _p(ctx), _p(ws), _p(dy),
                                    _p(grads["ff_w1"]), _p(grads["ff_b1"]), _p(grads["ff_w2"]), _p(grads["ff_b2"]), _p(grads["ff_ln_g"]),
                                    _p(grads["ff_ln_b"]), _p(keep), out, _stream()), "ttmi_ffn_bwd_defer")
        defer.push(out, (keep, ctx, grads["ff_w1"], grads["ff_b1"], grads["ff_w2"]))
        return dy
    check(L_.ttmi_ffn_bwd(_p(dz), _p(y), _p(p["ff_w1"]), _p(p["ff_w2"]), _p(p["ff_ln_g"]), c_long(rows), c_int(d), c_int(Di),
                          c_int(prec), c_float(p_drop), c_float(p_layer), ctypes.c_uint(seed), _p(ctx), _p(ws), _p(dy), _p(grads["ff_w1"]), _p(grads["ff_b1"]), _p(grads["ff_w2"]),
                          _p(grads["ff_b2"]), _p(grads["ff_ln_g"]), _p(grads["ff_ln_b"]), _stream()), "ttmi_ffn_bwd")
    return dy


def layer_fused(d, H, Dh, Di, prec):
    """do the layer-level calls share passes between the sub-layers (bf16 pipeline at these widths) - i.e. may x16 / z16 be passed?"""
    return bool(lib().ttmi_layer_fused(c_int(d), c_int(H), c_int(Dh), c_int(Di), c_int(prec)))


def _layer_ws(B, L, d, H, Dh, Di, prec, device):
    return scratch(_sized("ttmi_layer_ws_floats", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(Di), c_int(prec)), device)


def layer_fwd(x, x16, pa, pf, mask, prec, p_attn=0.0, seed_attn=0, p_ffn=0.0, p_layer=0.0, seed_ffn=0, want16=False):
    """one encoder layer (attention sub-layer + FFN) in one call: -> (y, z, z16 or None, ctx_attn, ctx_ffn).  pa / pf: the parameter
    dicts of attn_fwd / ffn_fwd; x16: bf16 copy of x from the previous layer's z16 (or None); want16: also return bf16(z)."""
    _trace("layer_fwd", tuple(x.shape))
    _need_cuda(x)
    B, L, d = x.shape
    K, H, Dh = pa["r_emb"].shape
    Di = pf["ff_w1"].shape[0]
    L_ = lib()
    ctx_a = _f32(_sized("ttmi_attn_ctx_floats", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(prec)), x.device)
    ctx_f = _f32(_sized("ttmi_ffn_ctx_floats", c_long(B * L), c_int(d), c_int(Di), c_int(prec)), x.device)
    ws = _layer_ws(B, L, d, H, Dh, Di, prec, x.device)
    y, z = torch.empty_like(x), torch.empty_like(x)
    z16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want16 else None
    check(L_.ttmi_layer_fwd(_p(x), _p(x16), _p(pa["qkv_w"]), _p(pa["o_w"]), _p(pa["ln_g"]), _p(pa["ln_b"]), _p(pa["r_emb"]), _p(pa["r_w_bias"]),
                            _p(pa["r_bias"]), _p(pf["ff_w1"]), _p(pf["ff_b1"]), _p(pf["ff_w2"]), _p(pf["ff_b2"]), _p(pf["ff_ln_g"]),
                            _p(pf["ff_ln_b"]), c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh), c_int(K), c_int(Di), *mask.args(), c_int(prec),
                            c_float(p_attn), ctypes.c_uint(seed_attn), c_float(p_ffn), c_float(p_layer), ctypes.c_uint(seed_ffn), _p(ctx_a),
                            _p(ctx_f), _p(ws), _p(y), _p(z), _p(z16), _stream()), "ttmi_layer_fwd")
    return y, z, z16, ctx_a, ctx_f


def layer_bwd(dz, x, x16, y, pa, pf, ctx_a, ctx_f, prec, grads, mask=None, p_attn=0.0, seed_attn=0, p_ffn=0.0, p_layer=0.0, seed_ffn=0, defer=None):
    """backward of layer_fwd -> dx; grads: running f32 buffers by parameter name (both sub-layers'), accumulated into.  defer: a WgradQueue
    that takes the layer's four weight-gradient GEMMs."""
    _trace("layer_bwd", tuple(x.shape))
    B, L, d = x.shape
    K, H, Dh = pa["r_emb"].shape
    Di = pf["ff_w1"].shape[0]
    L_ = lib()
    ws = _layer_ws(B, L, d, H, Dh, Di, prec, x.device)
    dx = torch.empty_like(x)
    keep_a = keep_f = out = None
    if defer is not None:
        keep_a = torch.empty(_sized("ttmi_attn_bwd_keep_bytes", c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh)), dtype=torch.uint8, device=x.device)
        keep_f = torch.empty(_sized("ttmi_ffn_bwd_keep_bytes", c_long(B * L), c_int(d), c_int(Di)), dtype=torch.uint8, device=x.device)
        out = (WgradDesc * 4)()
    for nm, t in (("dz", dz), ("x", x), ("y", y), ("ctx_attn", ctx_a), ("ctx_ffn", ctx_f), ("ws", ws), ("dx", dx)):
        if t is None or t.data_ptr() == 0:      # (round 6: one bench run in ~40 died here with the library's anonymous "null pointer"; name the tensor next time)
            raise ValueError("layer_bwd: %s is %s (x %s, prec %d, stream %#x)" % (nm, "None" if t is None else "an empty tensor of shape %s" % (tuple(t.shape),),
                                                                                 tuple(x.shape), prec, torch.cuda.current_stream(x.device).cuda_stream))
    check(L_.ttmi_layer_bwd(_p(dz), _p(x), _p(x16), _p(y), _p(pa["qkv_w"]), _p(pa["o_w"]), _p(pa["ln_g"]), _p(pa["r_emb"]), _p(pa["r_w_bias"]),
                            _p(pa["r_bias"]), _p(pf["ff_w1"]), _p(pf["ff_w2"]), _p(pf["ff_ln_g"]), c_int(B), c_int(L), c_int(d), c_int(H), c_int(Dh),
                            c_int(K), c_int(Di), *(mask or MaskSpec()).args(), c_int(prec), c_float(p_attn), ctypes.c_uint(seed_attn),
                            c_float(p_ffn), c_float(p_layer), ctypes.c_uint(seed_ffn), _p(ctx_a), _p(ctx_f), _p(ws), _p(dx),
                            _p(grads["qkv_w"]), _p(grads["o_w"]), _p(grads["ln_g"]), _p(grads["ln_b"]), _p(grads["r_emb"]), _p(grads["r_w_bias"]),
                            _p(grads["r_bias"]), _p(grads["ff_w1"]), _p(grads["ff_b1"]), _p(grads["ff_w2"]), _p(grads["ff_b2"]),
                            _p(grads["ff_ln_g"]), _p(grads["ff_ln_b"]), _p(keep_a), _p(keep_f), out, _stream()), "ttmi_layer_bwd")
    if defer is not None:
        defer.push(out, (keep_a, keep_f, ctx_a, ctx_f, x16, grads["qkv_w"], grads["o_w"], grads["ff_w1"], grads["ff_b1"], grads["ff_w2"]))
    return dx


def joint_logits_dtype(prec, J):
    return torch.bfloat16 if lib().ttmi_joint_logits_dtype(c_int(prec), c_int(J)) == 1 else torch.float32


def joint_fwd(enc, dec, wf, bf, wp, bp, prec):
    """-> logits [B,T,U1,V] (f32: prec 0 / 2, bf16: prec 1), a [..., :V] view of a pitch-roundup(V,64) buffer"""
    B, T, de = enc.shape
    U1, dd = dec.shape[1], dec.shape[2]
    J, V = wf.shape[0], wp.shape[0]
    L_ = lib()
    ctx = _f32(_sized("ttmi_joint_ctx_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(prec)), enc.device)
    ws = scratch(_sized("ttmi_joint_ws_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec)), enc.device)
    dt = joint_logits_dtype(prec, J)
    # (f32 logits too: rows of V = 4334 floats start 8 bytes off every second time - the projection's epilogue then stores float by float, 12 of
    # the bf16x3 mode's 21 ms forward GEMM at C2; on a pitch of roundup(V, 64) every row piece is whole 16-byte stores.  The loss and its
    # gradient take the pitch as they do for bf16 logits)
    buf, logits = padded_empty((B, T, U1, V), dt, enc.device)
    ldv = buf.shape[-1]
    check(L_.ttmi_joint_fwd(_p(enc), _p(dec), _p(wf), _p(bf), _p(wp), _p(bp), c_int(B), c_int(T), c_int(U1), c_int(de),
                            c_int(dd), c_int(J), c_int(V), c_int(prec), _p(ctx), _p(ws), _p(logits), c_long(ldv), _stream()),
          "ttmi_joint_fwd")
    return logits, ctx


def joint_bwd(dlogits, enc, dec, wf, wp, ctx, prec, grads, out=None):
    """out: optional (denc, ddec) buffers to write the input gradients into"""
    B, T, de = enc.shape
    U1, dd = dec.shape[1], dec.shape[2]
    J, V = wf.shape[0], wp.shape[0]
    L_ = lib()
    ws = scratch(_sized("ttmi_joint_ws_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec)), enc.device)
    dt = joint_logits_dtype(prec, J)
    ldg = row_pitch(dlogits)
    if dt is torch.bfloat16:
        ok = (dlogits.dtype is dt and ldg is not None and ldg % 8 == 0 and dlogits.data_ptr() % 16 == 0 and
              (ldg == V or getattr(dlogits, "_ttmi_zero_pad", None) == ldg))
        if not ok:                                  # foreign gradient: repack into a zero-padded bf16 buffer
            buf, view = padded_empty((B, T, U1, V), dt, enc.device)
            buf.zero_()
            view.copy_(dlogits)
            dlogits, ldg = view, buf.shape[-1]
    else:
        if dlogits.dtype is not dt or ldg is None:
            dlogits = dlogits.to(dt).contiguous()
            ldg = V
    denc, ddec = (torch.empty_like(enc), torch.empty_like(dec)) if out is None else out
    assert denc.is_contiguous() and ddec.is_contiguous() and denc.shape == enc.shape and ddec.shape == dec.shape
    check(L_.ttmi_joint_bwd(_p(dlogits), c_long(ldg), _p(enc), _p(dec), _p(wf), _p(wp), c_int(B), c_int(T), c_int(U1), c_int(de),
                            c_int(dd), c_int(J), c_int(V), c_int(prec), _p(ctx), _p(ws), _p(denc), _p(ddec), _p(grads["wf"]),
                            _p(grads["bf"]), _p(grads["wp"]), _p(grads["bp"]), _stream()), "ttmi_joint_bwd")
    return denc, ddec


def joint_loss_split_supported(logits, J, prec):
    """bf16x3 mode: may the loss gradient be written over the f32 logits as the two bf16 planes the joint's backward multiplies (no split pass over d logits)?"""
    if prec != 2 or logits.dtype is not torch.float32 or os.environ.get("TTMI_X3_SPLIT_GRAD", "1") == "0":
        return False
    B, T, U1, V = logits.shape
    ld = row_pitch(logits)
    return (ld is not None and bool(lib().ttmi_rnnt_loss_bwd_split_ok(c_long(ld), _p(logits))) and
            bool(lib().ttmi_joint_bwd_split_ok(c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec), c_long(ld))))


def rnnt_loss_bwd_split(logits, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, fastemit_lambda=0.0):
    """the f32 logits are REPLACED by their gradient's bf16 planes [hi | lo] per row (ttmi_rnnt_loss_bwd_split); -> the same tensor, to be handed to
    joint_bwd_split only"""
    fe = check_fastemit(fastemit_lambda)
    _need_cuda(logits, labels, act_lens, label_lens, workspace, grad_out)
    B, T, U1, V = logits.shape
    check(lib().ttmi_rnnt_loss_bwd_split_fe(_p(logits), c_long(row_pitch(logits)), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                                            c_int(U1), c_int(V), c_int(blank), _p(workspace), _p(grad_out), c_int(grad_out_stride), c_float(scale),
                                            c_float(fe), _stream()),
          "ttmi_rnnt_loss_bwd_split_fe")
    return logits


def joint_bwd_split(planes, enc, dec, wf, wp, ctx, prec, grads, out=None):
    """joint_bwd for d logits that rnnt_loss_bwd_split left as bf16 planes in the logits' own buffer"""
    B, T, de = enc.shape
    U1, dd = dec.shape[1], dec.shape[2]
    J, V = wf.shape[0], wp.shape[0]
    L_ = lib()
    ws = scratch(_sized("ttmi_joint_ws_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec)), enc.device)
    denc, ddec = (torch.empty_like(enc), torch.empty_like(dec)) if out is None else out
    assert denc.is_contiguous() and ddec.is_contiguous() and denc.shape == enc.shape and ddec.shape == dec.shape
    check(L_.ttmi_joint_bwd_split(_p(planes), c_long(row_pitch(planes)), _p(enc), _p(dec), _p(wf), _p(wp), c_int(B), c_int(T), c_int(U1), c_int(de),
                                  c_int(dd), c_int(J), c_int(V), c_int(prec), _p(ctx), _p(ws), _p(denc), _p(ddec), _p(grads["wf"]),
                                  _p(grads["bf"]), _p(grads["wp"]), _p(grads["bp"]), _stream()), "ttmi_joint_bwd_split")
    return denc, ddec


# ---- fused joint + loss fast path (exp-domain forms, include/ttmi.h)
def joint_exp_supported(B, T, U1, J, V, prec, fwd_only=False):
    ldv = (V + 63) // 64 * 64
    fn = lib().ttmi_joint_exp_fwd_supported if fwd_only else lib().ttmi_joint_exp_supported
    return bool(fn(c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec), c_long(ldv)))


def exp_padded_rows(B, T, U1):
    return int(_sized("ttmi_joint_exp_padded_rows", c_int(B), c_int(T), c_int(U1), restype=c_long))


def joint_fwd_exp(enc, dec, wf, bf, wp, bp, prec, shift=None, labels=None, blank=0):
    """-> (P bf16 [B,T,U1,V] view of a pitch-roundup(V,64) buffer = exp(logits - shift), rowsum f32 [nparts, B*T*U1], ctx, emis).
    labels (int32 [B, U1-1]) given: emis f32 [B*T*U1, 4] = the blank's and the next label's logit of every lattice row (from the GEMM's bf16
    operands, then from f32 operands), else None"""
    B, T, de = enc.shape
    U1, dd = dec.shape[1], dec.shape[2]
    J, V = wf.shape[0], wp.shape[0]
    L_ = lib()
    ctx = _f32(_sized("ttmi_joint_ctx_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(prec)), enc.device)
    ws = scratch(_sized("ttmi_joint_ws_floats_prec", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(prec)), enc.device)
    # room for the lattice rows padded to the wgrad's 64-row reduction tile (ttmi_joint_bwd_exp zero-fills the pad rows: include/ttmi.h)
    rows, ldv = B * T * U1, (V + 63) // 64 * 64
    rows_p = exp_padded_rows(B, T, U1)
    buf = torch.empty(rows_p * ldv, dtype=torch.bfloat16, device=enc.device)[:rows * ldv].view(B, T, U1, ldv)
    P = buf[..., :V]
    nparts = L_.ttmi_joint_exp_nparts(c_int(V))
    rowsum = torch.empty(nparts, B * T * U1, dtype=torch.float32, device=enc.device)
    emis = None
    if labels is not None:
        _need_cuda(labels)
        assert labels.dtype is torch.int32 and labels.is_contiguous() and tuple(labels.shape) == (B, U1 - 1)
        emis = torch.empty(B * T * U1, 4, dtype=torch.float32, device=enc.device)
    check(L_.ttmi_joint_fwd_exp(_p(enc), _p(dec), _p(wf), _p(bf), _p(wp), _p(bp), c_int(B), c_int(T), c_int(U1), c_int(de),
                                c_int(dd), c_int(J), c_int(V), c_int(prec), _p(ctx), _p(ws), _p(P), c_long(buf.shape[-1]),
                                _p(rowsum), c_int(nparts), _p(shift), _p(labels), c_int(blank), _p(emis), _stream()), "ttmi_joint_fwd_exp")
    return P, rowsum, ctx, emis


def rnnt_loss_fwd_exp(P, rowsum, labels, act_lens, label_lens, blank, workspace, shift_cur=None, shift_next=None, emis=None, flag=None):
    """emis: f32 [rows, 4] from joint_fwd_exp (the emission log-probs then come from f32 logits, not from bf16 entries of P); flag: device
    int32 [1], bit 0 set when a row sum under- / overflowed (that step's costs and gradients are NaN)"""
    _need_cuda(P, rowsum, labels, act_lens, label_lens, workspace, emis, flag)
    B, T, U1, V = P.shape
    costs = torch.empty(B, dtype=torch.float32, device=P.device)
    check(lib().ttmi_rnnt_loss_fwd_exp(_p(P), c_long(row_pitch(P)), _p(rowsum), c_int(rowsum.shape[0]), _p(labels), _p(act_lens),
                                       _p(label_lens), c_int(B), c_int(T), c_int(U1), c_int(V), c_int(blank), _p(workspace),
                                       _p(costs), _p(shift_cur), _p(shift_next), _p(emis), _p(flag), _stream()), "ttmi_rnnt_loss_fwd_exp")
    return costs


def rnnt_shift_seed(workspace, act_lens, label_lens, B, T, U1, shift_next):
    """shift_next = max(shift_next, max log-sum-exp - 40) over the lattice rows of a PLAIN rnnt_loss_fwd's workspace (device only)"""
    check(lib().ttmi_rnnt_shift_seed(_p(workspace), _p(act_lens), _p(label_lens), c_int(B), c_int(T), c_int(U1), _p(shift_next), _stream()),
          "ttmi_rnnt_shift_seed")


def rnnt_loss_bwd_exp(P, labels, act_lens, label_lens, blank, workspace, grad_out, grad_out_stride, scale, fastemit_lambda=0.0):
    """patches P in place -> (srow f32 [rows], srow16 bf16 [rows]): d logits = srow[r] * P[r, :]"""
    fe = check_fastemit(fastemit_lambda)
    B, T, U1, V = P.shape
    rows = B * T * U1
    srow = torch.empty(rows, dtype=torch.float32, device=P.device)
    srow16 = torch.empty(exp_padded_rows(B, T, U1), dtype=torch.bfloat16, device=P.device)[:rows]      # (pad rows: zero-filled by ttmi_joint_bwd_exp)
    check(lib().ttmi_rnnt_loss_bwd_exp_fe(_p(P), c_long(row_pitch(P)), _p(labels), _p(act_lens), _p(label_lens), c_int(B), c_int(T),
                                          c_int(U1), c_int(V), c_int(blank), _p(workspace), _p(grad_out), c_int(grad_out_stride),
                                          c_float(scale), _p(srow), _p(srow16), c_float(fe), _stream()), "ttmi_rnnt_loss_bwd_exp_fe")
    return srow, srow16


def joint_bwd_exp(P, srow, srow16, enc, dec, wf, wp, ctx, prec, grads, out=None):
    B, T, de = enc.shape
    U1, dd = dec.shape[1], dec.shape[2]
    J, V = wf.shape[0], wp.shape[0]
    L_ = lib()
    ws = scratch(_sized("ttmi_joint_ws_floats", c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V)), enc.device)
    denc, ddec = (torch.empty_like(enc), torch.empty_like(dec)) if out is None else out
    assert denc.is_contiguous() and ddec.is_contiguous() and denc.shape == enc.shape and ddec.shape == dec.shape
    check(L_.ttmi_joint_bwd_exp(_p(P), c_long(row_pitch(P)), _p(srow), _p(srow16), _p(enc), _p(dec), _p(wf), _p(wp), c_int(B),
                                c_int(T), c_int(U1), c_int(de), c_int(dd), c_int(J), c_int(V), c_int(prec), _p(ctx), _p(ws),
                                _p(denc), _p(ddec), _p(grads["wf"]), _p(grads["bf"]), _p(grads["wp"]), _p(grads["bp"]), _stream()),
          "ttmi_joint_bwd_exp")
    return denc, ddec


def embed_fwd(tokens, W):
    _need_cuda(tokens, W)
    if tokens.dtype is not torch.long:          # the kernel reads int64 ids; nn.Embedding (tt/decoder.py:26) also takes int32
        if tokens.dtype is not torch.int32:
            raise TypeError("embedding indices must be int64 or int32, got %s" % tokens.dtype)
        tokens = tokens.long()
    tokens = tokens.contiguous()
    n, (V, d) = tokens.numel(), W.shape
    out = torch.empty(*tokens.shape, d, dtype=torch.float32, device=W.device)
    check(lib().ttmi_embed_fwd(_p(tokens), _p(W), c_long(n), c_int(d), c_int(V), _p(out), _stream()), "ttmi_embed_fwd")
    return out


def embed_bwd(tokens, dout, V, padding_idx, gW):
    n, d = tokens.numel(), dout.shape[-1]
    check(lib().ttmi_embed_bwd(_p(tokens), _p(dout), c_long(n), c_int(d), c_int(V), c_int(padding_idx), _p(gW), _stream()),
          "ttmi_embed_bwd")
    return gW


# ----------------------------------------------------------------------------- optimiser tail / probes
def sumsq(x, out):
    check(lib().ttmi_sumsq(_p(x), c_long(x.numel()), _p(out), _stream()), "ttmi_sumsq")


def sgd_step(p, g, mom, lr, momentum, weight_decay, nesterov, max_norm, normsq, grad_scale, hyper=None):
    """hyper: device f32 [2] = (learning rate, steps taken), read (and the count advanced) by the kernels at run time - see include/ttmi.h"""
    check(lib().ttmi_sgd_step(_p(p), _p(g), _p(mom), c_long(p.numel()), c_float(lr), c_float(momentum), c_float(weight_decay),
                              c_int(1 if nesterov else 0), c_float(max_norm), _p(normsq), c_float(grad_scale), _p(hyper), _stream()),
          "ttmi_sgd_step")


def adam_step(p, g, m, v, lr, betas, eps, weight_decay, step, max_norm, normsq, grad_scale, hyper=None):
    check(lib().ttmi_adam_step(_p(p), _p(g), _p(m), _p(v), c_long(p.numel()), c_float(lr), c_float(betas[0]), c_float(betas[1]),
                               c_float(eps), c_float(weight_decay), c_int(step), c_float(max_norm), _p(normsq),
                               c_float(grad_scale), _p(hyper), _stream()), "ttmi_adam_step")


def adadelta_step(p, g, sq, acc, lr, rho, eps, weight_decay, max_norm, normsq, grad_scale, hyper=None):
    check(lib().ttmi_adadelta_step(_p(p), _p(g), _p(sq), _p(acc), c_long(p.numel()), c_float(lr), c_float(rho), c_float(eps),
                                   c_float(weight_decay), c_float(max_norm), _p(normsq), c_float(grad_scale), _p(hyper), _stream()), "ttmi_adadelta_step")


def probe_arm(slot=0):
    check(lib().ttmi_probe_arm(c_int(slot)), "ttmi_probe_arm")


def probe_read_ms(slot=0, point=0):
    """duration of probe `point` (0 joint projection, 1 RNN-T loss forward, 2 RNN-T loss backward) armed in `slot`; < 0 = never fired"""
    return float(_sized("ttmi_probe_point_read_ms", c_int(point), c_int(slot), restype=ctypes.c_float))


# ----------------------------------------------------------------------------- throughput bf16 GEMMs (tests / tools)
def gemm_nt_bf16(A, B, C, bias=None):
    """C[M,N] = A[M,K] @ B[N,K]^T (+bias).  A, B bf16 row-major (row pitch = stride(0)); C f32 or bf16."""
    M, K = A.shape
    N = B.shape[0]
    check(lib().ttmi_gemm_nt_bf16(_p(A), _p(B), _p(C), c_int(_DT[C.dtype]), _p(bias), c_int(M), c_int(N), c_int(K),
                                  c_long(A.stride(0)), c_long(B.stride(0)), c_long(C.stride(0)), _stream()), "ttmi_gemm_nt_bf16")
    return C


def gemm_nt_bf16_two_term(A, B, B_lo, C, bias=None, relu=False, k_lo=0):
    """C[M,N] = act(A[M,K] @ (B + B_lo)[N,K]^T + bias) in one launch; k_lo != 0: B_lo meets A's first k_lo columns only."""
    M, K = A.shape
    N = B.shape[0]
    assert B_lo.shape[0] == B.shape[0] and B_lo.stride(0) == B.stride(0)
    if k_lo:
        check(lib().ttmi_gemm_nt_bf16_two_term_klo(_p(A), _p(B), _p(B_lo), _p(C), c_int(_DT[C.dtype]), _p(bias), c_int(1 if relu else 0), c_int(M),
                                                   c_int(N), c_int(K), c_int(k_lo), c_long(A.stride(0)), c_long(B.stride(0)), c_long(C.stride(0)), _stream()),
              "ttmi_gemm_nt_bf16_two_term_klo")
        return C
    check(lib().ttmi_gemm_nt_bf16_two_term(_p(A), _p(B), _p(B_lo), _p(C), c_int(_DT[C.dtype]), _p(bias), c_int(1 if relu else 0), c_int(M),
                                           c_int(N), c_int(K), c_long(A.stride(0)), c_long(B.stride(0)), c_long(C.stride(0)), _stream()),
          "ttmi_gemm_nt_bf16_two_term")
    return C


def gemm_tn_bf16(A, B, C, accumulate=False, colsum_a=None):
    """C[M,N] (f32) (+)= A[K,M]^T @ B[K,N].  A, B bf16 row-major.  colsum_a (f32 [M]) += column sums of A."""
    K, M = A.shape
    N = B.shape[1]
    check(lib().ttmi_gemm_tn_bf16(_p(A), _p(B), _p(C), c_int(M), c_int(N), c_int(K), c_long(A.stride(0)), c_long(B.stride(0)),
                                  c_long(C.stride(0)), c_int(1 if accumulate else 0), _p(colsum_a), _stream()), "ttmi_gemm_tn_bf16")
    return C


def dropout_multipliers(n, p, seed, device):
    """the exact 0 / 1/(1-p) multipliers the fused sub-layers use for dropout site `seed` (tests, debugging)"""
    ones = torch.ones(n, dtype=torch.float32, device=device)
    out = torch.empty_like(ones)
    check(lib().ttmi_dropout_apply(_p(ones), c_long(n), c_float(p), ctypes.c_uint(seed), _p(out), _stream()), "ttmi_dropout_apply")
    return out


_salt_keep = [None]


def set_dropout_salt(t):
    """t: int32 / uint32 device tensor [1] (or None): a word every dropout site mixes into its seed at kernel start; bump it on the device
    between steps when the step is replayed from a captured graph (ttmi.train.GraphedStep)"""
    if t is not None:
        _need_cuda(t)
        assert t.numel() == 1 and t.element_size() == 4
    _salt_keep[0] = t                       # the library holds the raw pointer: keep the tensor alive
    check(lib().ttmi_set_dropout_salt(_p(t)), "ttmi_set_dropout_salt")


def set_option(key, value):
    """process-wide A/B switches (key 0: 1 disables the fused attention kernels of the bf16 pipeline)"""
    check(lib().ttmi_set_option(c_int(key), c_int(value)), "ttmi_set_option")


def reserve_cus(n, device=None):
    """CUs the encoder-sized persistent GEMMs leave free on the CURRENT stream and on the label encoder's side stream (data-parallel
    backward: RCCL's kernels run beside it).  Per-stream state in the library, read at launch time; 0 = whole chip."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    check(lib().ttmi_stream_reserve_cus(c_void_p(torch.cuda.current_stream(device).cuda_stream), c_int(n)), "ttmi_stream_reserve_cus")
    st = _side_streams.get((device.type, device.index))
    if st is not None:
        check(lib().ttmi_stream_reserve_cus(c_void_p(st.cuda_stream), c_int(n)), "ttmi_stream_reserve_cus")


def side_stream(device):
    """the per-device side stream on which the label encoder runs concurrently with the audio encoder"""
    key = (device.type, device.index)
    st = _side_streams.get(key)
    if st is None:
        # TTMI_SIDE_STREAM_PRIORITY (A/B knob, round 6): torch clamps it to the device's range; lower number = served first
        st = _side_streams[key] = torch.cuda.Stream(device=device, priority=int(os.environ.get("TTMI_SIDE_STREAM_PRIORITY", "0")))
        # a second-level stream (forked from the caller's main stream): library calls on it never fork again inside a stream capture
        check(lib().ttmi_stream_set_nofork(c_void_p(st.cuda_stream), c_int(1)), "ttmi_stream_set_nofork")
    return st


def join_side_streams():
    """make the current stream wait for everything queued on the side streams (call before consuming gradients that
    backward nodes running on a side stream wrote in place, e.g. before the optimiser step / gradient all-reduce)"""
    for st in _side_streams.values():
        torch.cuda.current_stream(st.device).wait_stream(st)


def greedy_scan(logits2d, blank=0):
    """logits2d [n, V] (f32/bf16, row pitch = stride(0)) -> (first row whose argmax != blank, symbol) or (n, None); one 8-byte
    D2H read."""
    n, V = logits2d.shape
    out = torch.empty(1, dtype=torch.int64, device=logits2d.device)
    check(lib().ttmi_greedy_scan(_p(logits2d), c_int(_DT[logits2d.dtype]), c_long(logits2d.stride(0)), c_int(n), c_int(V),
                                 c_int(blank), _p(out), _stream()), "ttmi_greedy_scan")
    key = int(out.item())
    row, tok = key >> 32, key & 0xffffffff
    return (row, tok) if row < n else (n, None)


def greedy_scan_batch(logits, t, T_len, need, key, blank=0):
    """logits [B, n, V] (f32 / bf16, row pitch = stride(-2)): per utterance the first existing frame of the block whose argmax is not blank
    -> key[b] (include/ttmi.h: ttmi_greedy_scan_batch); device only, no synchronisation"""
    B, n, V = logits.shape
    _need_cuda(logits, t, T_len, need, key)
    check(lib().ttmi_greedy_scan_batch(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(n), c_int(V), c_int(blank),
                                       _p(t), _p(T_len), _p(need), _p(key), _stream()), "ttmi_greedy_scan_batch")


def greedy_advance(key, n, n_hist, hist, t, T_len, need, done, count, flags):
    """consume key (ttmi_greedy_advance): histories, frame positions and the need / done flags move on the device; flags[0] = utterances
    that still need a symbol in this step, flags[1] = utterances not finished"""
    B = key.shape[0]
    assert hist.dtype is torch.long and hist.stride(1) == 1
    check(lib().ttmi_greedy_advance(_p(key), c_int(B), c_int(n), c_int(n_hist), _p(hist), c_long(hist.stride(0)), _p(t), _p(T_len), _p(need),
                                    _p(done), _p(count), _p(flags), _stream()), "ttmi_greedy_advance")


def greedy_scan_batch_lp(logits, t, T_len, need, key, lp, blank=0):
    """greedy_scan_batch (same key) that also writes lp [B, n, 2] (f32) = log P(blank), log P(argmax) of every row it walks, from the same
    single pass over the row (include/ttmi.h: ttmi_greedy_scan_batch_lp); rows it skips keep what lp held; device only, no synchronisation"""
    B, n, V = logits.shape
    _need_cuda(logits, t, T_len, need, key, lp)
    assert lp.dtype is torch.float32 and lp.is_contiguous() and tuple(lp.shape) == (B, n, 2)
    check(lib().ttmi_greedy_scan_batch_lp(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(n), c_int(V), c_int(blank),
                                          _p(t), _p(T_len), _p(need), _p(key), _p(lp), _stream()), "ttmi_greedy_scan_batch_lp")


def greedy_advance_lp(key, n, n_hist, hist, t, T_len, need, done, count, flags, lp, frames, tok_lp, score):
    """greedy_advance (same state, same flags) that also books the block's decisions from the scan's lp (ttmi_greedy_advance_lp): frames
    (i32) / tok_lp (f32) [B, ld_det] get the emission frame and log-probability of the symbol appended at column count[b], score (f64 [B])
    the log-probability of the frames consumed - the greedy decoder's own path, not a path of the RNN-T lattice"""
    B = key.shape[0]
    _need_cuda(key, hist, lp, frames, tok_lp, score)
    assert hist.dtype is torch.long and hist.stride(1) == 1
    assert lp.dtype is torch.float32 and lp.is_contiguous() and tuple(lp.shape) == (B, n, 2)
    assert frames.dtype is torch.int32 and tok_lp.dtype is torch.float32 and frames.stride(1) == 1 and tok_lp.stride(1) == 1
    assert frames.shape[0] == B and tok_lp.shape == frames.shape and frames.stride(0) == tok_lp.stride(0)
    assert score.dtype is torch.float64 and score.is_contiguous() and score.shape[0] == B
    check(lib().ttmi_greedy_advance_lp(_p(key), c_int(B), c_int(n), c_int(n_hist), _p(hist), c_long(hist.stride(0)), _p(t), _p(T_len), _p(need),
                                       _p(done), _p(count), _p(flags), _p(lp), _p(frames), _p(tok_lp), c_long(frames.stride(0)), _p(score),
                                       _stream()), "ttmi_greedy_advance_lp")


def beam_step(logits, t, T_len, beam_in, beam_out, parent, fresh, blank=0):
    """one frame of the frame-synchronous beam search of every utterance (include/ttmi.h: ttmi_beam_step, the rule is written there).
    logits [B, W, V] (f32 / bf16, row pitch = stride(-2)) = the joint of frame t[b] against the label state of every hypothesis; beam_in /
    beam_out = (score f64 [B, W], len i32 [B, W], hist i64 [B, W, ld_hist], frames i32 [B, W, ld_det] or None, tok_lp f32 [B, W, ld_det] or
    None), two sets of buffers the caller swaps; parent / fresh i32 [B, W].  Device only, no synchronisation."""
    B, W, V = logits.shape
    (s0, n0, h0, f0, l0), (s1, n1, h1, f1, l1) = beam_in, beam_out
    _need_cuda(logits, t, T_len, s0, n0, h0, f0, l0, s1, n1, h1, f1, l1, parent, fresh)
    if logits.stride(-1) != 1 or (B > 1 and logits.stride(0) != W * logits.stride(1)):
        raise ValueError("beam_step: logits rows must be evenly pitched ([B, W, V] with stride(0) = W * stride(1))")
    for x in (t, T_len):
        assert x.dtype is torch.int32 and x.is_contiguous() and x.shape[0] == B
    for s, n, h, f, l in (beam_in, beam_out):
        assert s.dtype is torch.float64 and s.is_contiguous() and tuple(s.shape) == (B, W)
        assert n.dtype is torch.int32 and n.is_contiguous() and tuple(n.shape) == (B, W)
        assert h.dtype is torch.long and h.is_contiguous() and tuple(h.shape[:2]) == (B, W) and h.shape == h0.shape
        assert (f is None) == (l is None) == (f0 is None)
        if f is not None:
            assert f.dtype is torch.int32 and l.dtype is torch.float32 and f.is_contiguous() and l.is_contiguous()
            assert tuple(f.shape[:2]) == (B, W) and f.shape == l.shape == f0.shape
    for x in (parent, fresh):
        assert x.dtype is torch.int32 and x.is_contiguous() and tuple(x.shape) == (B, W)
    check(lib().ttmi_beam_step(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(W), c_int(V), c_int(blank), _p(t),
                               _p(T_len), _p(s0), _p(n0), _p(h0), _p(f0), _p(l0), _p(s1), _p(n1), _p(h1), _p(f1), _p(l1), c_long(h0.shape[2]),
                               c_long(f0.shape[2] if f0 is not None else 0), _p(parent), _p(fresh), _stream()), "ttmi_beam_step")


def beam_ctx_workspace(B, W, V, device):
    """the workspace of beam_step_ctx for [B, W, V] logits (ttmi_beam_ctx_ws_bytes): allocate once per decoding run, nothing is kept in it"""
    return torch.empty(_sized("ttmi_beam_ctx_ws_bytes", c_int(B), c_int(W), c_int(V)), dtype=torch.uint8, device=device)


def beam_step_ctx(logits, t, T_len, beam_in, beam_out, parent, fresh, tables, ctx_in, ctx_out, ws, blank=0):
    """beam_step with contextual biasing (include/ttmi.h: ttmi_beam_step_ctx, the rule and the automaton's contract are written there).
    tables = (arc_off i32 [S + 1], arc_sym i32 [A], arc_next i32 [A], arc_w f32 [A], fail i32 [S], fail_w f32 [S]) on the device
    (ttmi.context.ContextGraph.to(device).tables); ctx_in / ctx_out = (state i32 [B, W], bias f64 [B, W]), swapped with the beam;
    ws = beam_ctx_workspace(B, W, V, device).  Device only, no synchronisation."""
    B, W, V = logits.shape
    (s0, n0, h0, f0, l0), (s1, n1, h1, f1, l1) = beam_in, beam_out
    arc_off, arc_sym, arc_next, arc_w, fail, fail_w = tables
    _need_cuda(logits, t, T_len, s0, n0, h0, f0, l0, s1, n1, h1, f1, l1, parent, fresh, *tables, *ctx_in, *ctx_out, ws)
    if logits.stride(-1) != 1 or (B > 1 and logits.stride(0) != W * logits.stride(1)):
        raise ValueError("beam_step_ctx: logits rows must be evenly pitched ([B, W, V] with stride(0) = W * stride(1))")
    for x in (t, T_len):
        assert x.dtype is torch.int32 and x.is_contiguous() and x.shape[0] == B
    for s, n, h, f, l in (beam_in, beam_out):
        assert s.dtype is torch.float64 and s.is_contiguous() and tuple(s.shape) == (B, W)
        assert n.dtype is torch.int32 and n.is_contiguous() and tuple(n.shape) == (B, W)
        assert h.dtype is torch.long and h.is_contiguous() and tuple(h.shape[:2]) == (B, W) and h.shape == h0.shape
        assert (f is None) == (l is None) == (f0 is None)
        if f is not None:
            assert f.dtype is torch.int32 and l.dtype is torch.float32 and f.is_contiguous() and l.is_contiguous()
            assert tuple(f.shape[:2]) == (B, W) and f.shape == l.shape == f0.shape
    for x in (parent, fresh):
        assert x.dtype is torch.int32 and x.is_contiguous() and tuple(x.shape) == (B, W)
    S, A = fail.shape[0], arc_sym.shape[0]
    for x, dt, n in ((arc_off, torch.int32, S + 1), (arc_sym, torch.int32, A), (arc_next, torch.int32, A), (arc_w, torch.float32, A),
                     (fail, torch.int32, S), (fail_w, torch.float32, S)):
        assert x.dtype is dt and x.is_contiguous() and tuple(x.shape) == (n,)
    for state, bias in (ctx_in, ctx_out):
        assert state.dtype is torch.int32 and state.is_contiguous() and tuple(state.shape) == (B, W)
        assert bias.dtype is torch.float64 and bias.is_contiguous() and tuple(bias.shape) == (B, W)
    assert (ws.is_contiguous() and ws.numel() * ws.element_size() >= _sized("ttmi_beam_ctx_ws_bytes", c_int(B), c_int(W), c_int(V)) and
            ws.data_ptr() % 8 == 0)
    check(lib().ttmi_beam_step_ctx(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(W), c_int(V), c_int(blank),
                                   _p(t), _p(T_len), _p(s0), _p(n0), _p(h0), _p(f0), _p(l0), _p(s1), _p(n1), _p(h1), _p(f1), _p(l1),
                                   c_long(h0.shape[2]), c_long(f0.shape[2] if f0 is not None else 0), _p(parent), _p(fresh), c_int(S), c_int(A),
                                   _p(arc_off), _p(arc_sym), _p(arc_next), _p(arc_w), _p(fail), _p(fail_w), _p(ctx_in[0]), _p(ctx_in[1]),
                                   _p(ctx_out[0]), _p(ctx_out[1]), _p(ws), _stream()), "ttmi_beam_step_ctx")


BEAM_FUSE_NORMS = {"logprob": 0, "softmax": 1, "softmax_no_blank": 2}


def beam_fuse_workspace(B, W, V, device):
    """the workspace of beam_step_fuse for [B, W, V] logits (ttmi_beam_fuse_ws_bytes): allocate once per decoding run, nothing is kept in it"""
    return torch.empty(_sized("ttmi_beam_fuse_ws_bytes", c_int(B), c_int(W), c_int(V)), dtype=torch.uint8, device=device)


def beam_step_fuse(logits, t, T_len, beam_in, beam_out, parent, fresh, tables, ctx_in, ctx_out, ws, fuse_in, fuse_out, sources=(),
                   sym_bonus=0.0, blank=0):
    """beam_step_ctx with dense external scores (include/ttmi.h: ttmi_beam_step_fuse, the rule is written there): language-model fusion and
    internal-LM subtraction.  The arguments of beam_step_ctx (tables: a search without hotwords passes the trivial automaton, S = 1, A = 0),
    ws = beam_fuse_workspace(B, W, V, device), then fuse_in / fuse_out f64 [B, W], swapped with the beam, and `sources`: at most two
    entries, source 0 and source 1, each None (absent) or (rows, weight, norm) with rows [B, W, V] f32 / bf16 (row (b, w) scores the hypothesis of slot w; row pitch = stride(-2)), weight a float
    and norm 0 / 1 / 2 (BEAM_FUSE_NORMS: the row holds log-probabilities / logits to normalise / logits to normalise without the blank).
    Device only, no synchronisation."""
    B, W, V = logits.shape
    (s0, n0, h0, f0, l0), (s1, n1, h1, f1, l1) = beam_in, beam_out
    arc_off, arc_sym, arc_next, arc_w, fail, fail_w = tables
    sources = list(sources)
    if len(sources) > 2:
        raise ValueError("beam_step_fuse: at most two sources, got %d" % len(sources))
    _need_cuda(logits, t, T_len, s0, n0, h0, f0, l0, s1, n1, h1, f1, l1, parent, fresh, *tables, *ctx_in, *ctx_out, ws, fuse_in, fuse_out,
               *[src[0] for src in sources if src is not None])
    if logits.stride(-1) != 1 or (B > 1 and logits.stride(0) != W * logits.stride(1)):
        raise ValueError("beam_step_fuse: logits rows must be evenly pitched ([B, W, V] with stride(0) = W * stride(1))")
    for x in (t, T_len):
        assert x.dtype is torch.int32 and x.is_contiguous() and x.shape[0] == B
    for s, n, h, f, l in (beam_in, beam_out):
        assert s.dtype is torch.float64 and s.is_contiguous() and tuple(s.shape) == (B, W)
        assert n.dtype is torch.int32 and n.is_contiguous() and tuple(n.shape) == (B, W)
        assert h.dtype is torch.long and h.is_contiguous() and tuple(h.shape[:2]) == (B, W) and h.shape == h0.shape
        assert (f is None) == (l is None) == (f0 is None)
        if f is not None:
            assert f.dtype is torch.int32 and l.dtype is torch.float32 and f.is_contiguous() and l.is_contiguous()
            assert tuple(f.shape[:2]) == (B, W) and f.shape == l.shape == f0.shape
    for x in (parent, fresh):
        assert x.dtype is torch.int32 and x.is_contiguous() and tuple(x.shape) == (B, W)
    S, A = fail.shape[0], arc_sym.shape[0]
    for x, dt, n in ((arc_off, torch.int32, S + 1), (arc_sym, torch.int32, A), (arc_next, torch.int32, A), (arc_w, torch.float32, A),
                     (fail, torch.int32, S), (fail_w, torch.float32, S)):
        assert x.dtype is dt and x.is_contiguous() and tuple(x.shape) == (n,)
    for state, bias in (ctx_in, ctx_out):
        assert state.dtype is torch.int32 and state.is_contiguous() and tuple(state.shape) == (B, W)
        assert bias.dtype is torch.float64 and bias.is_contiguous() and tuple(bias.shape) == (B, W)
    for x in (fuse_in, fuse_out):
        assert x.dtype is torch.float64 and x.is_contiguous() and tuple(x.shape) == (B, W)
    assert (ws.is_contiguous() and ws.numel() * ws.element_size() >= _sized("ttmi_beam_fuse_ws_bytes", c_int(B), c_int(W), c_int(V)) and
            ws.data_ptr() % 8 == 0)
    ext = []
    for src in sources + [None] * (2 - len(sources)):
        if src is None:
            ext += [c_void_p(0), c_int(0), c_long(0), ctypes.c_double(0.0), c_int(0)]
            continue
        rows, weight, norm = src
        if rows.dtype not in _DT or tuple(rows.shape) != (B, W, V) or rows.stride(-1) != 1 or (B > 1 and rows.stride(0) != W * rows.stride(1)):
            raise ValueError("beam_step_fuse: a source is [B, W, V] f32 / bf16 rows, evenly pitched (stride(0) = W * stride(1)), last stride 1")
        ext += [_p(rows), c_int(_DT[rows.dtype]), c_long(rows.stride(-2)), ctypes.c_double(float(weight)), c_int(int(norm))]
    check(lib().ttmi_beam_step_fuse(_p(logits), c_int(_DT[logits.dtype]), c_long(logits.stride(-2)), c_int(B), c_int(W), c_int(V), c_int(blank),
                                    _p(t), _p(T_len), _p(s0), _p(n0), _p(h0), _p(f0), _p(l0), _p(s1), _p(n1), _p(h1), _p(f1), _p(l1),
                                    c_long(h0.shape[2]), c_long(f0.shape[2] if f0 is not None else 0), _p(parent), _p(fresh), c_int(S), c_int(A),
                                    _p(arc_off), _p(arc_sym), _p(arc_next), _p(arc_w), _p(fail), _p(fail_w), _p(ctx_in[0]), _p(ctx_in[1]),
                                    _p(ctx_out[0]), _p(ctx_out[1]), _p(ws), _p(fuse_in), _p(fuse_out), ctypes.c_double(float(sym_bonus)), *ext,
                                    _stream()), "ttmi_beam_step_fuse")


def beam_stable_prefix(score, n_tok, hist, out=None):
    """one beam as beam_step leaves it (score f64 [B, W], len i32 [B, W], hist i64 [B, W, ld_hist]) -> stable i32 [B]: how many leading tokens
    every live slot of the utterance shares (include/ttmi.h: ttmi_beam_stable_prefix, the rule and why the prefix is permanent are written
    there).  Device only, no synchronisation; `out` = a buffer to write into."""
    _need_cuda(score, n_tok, hist, out)
    B, W = score.shape
    assert score.dtype is torch.float64 and score.is_contiguous()
    assert n_tok.dtype is torch.int32 and n_tok.is_contiguous() and tuple(n_tok.shape) == (B, W)
    assert hist.dtype is torch.long and hist.is_contiguous() and tuple(hist.shape[:2]) == (B, W)
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=score.device)
    assert out.dtype is torch.int32 and out.is_contiguous() and tuple(out.shape) == (B,)
    check(lib().ttmi_beam_stable_prefix(_p(score), _p(n_tok), _p(hist), c_long(hist.shape[2]), c_int(B), c_int(W), _p(out), _stream()),
          "ttmi_beam_stable_prefix")
    return out


# ----------------------------------------------------------------------------- error counting (ttmi.metrics)
def edit_distance(hyp, hyp_len, ref, ref_len, ref_index=None):
    """hyp i32 [P, Lh] / ref i32 [R, Lr] (last stride 1, any row pitch), hyp_len i32 [P], ref_len i32 [R], ref_index i32 [P] or None
    -> out i32 [P, 4] = (distance, substitutions, deletions, insertions) per pair (include/ttmi.h: ttmi_edit_distance, the tie rule is
    written there); device only, no synchronisation"""
    _need_cuda(hyp, hyp_len, ref, ref_len, ref_index)
    P, Lh = hyp.shape
    R, Lr = ref.shape
    for x, n in ((hyp_len, P), (ref_len, R)) + (((ref_index, P),) if ref_index is not None else ()):
        assert x.dtype is torch.int32 and x.is_contiguous() and tuple(x.shape) == (n,)
    for x in (hyp, ref):
        assert x.dtype is torch.int32 and (x.shape[1] <= 1 or x.stride(1) == 1)
    ld_hyp = hyp.stride(0) if P > 1 and Lh > 0 else Lh          # (the pitch of a single row, or of empty rows, is never used)
    ld_ref = ref.stride(0) if R > 1 and Lr > 0 else Lr
    out = torch.empty(P, 4, dtype=torch.int32, device=hyp.device)
    check(lib().ttmi_edit_distance(_p(hyp), c_long(ld_hyp), _p(hyp_len), _p(ref), c_long(ld_ref), _p(ref_len), _p(ref_index), c_int(P), c_int(R),
                                   c_int(Lh), c_int(Lr), _p(out), _stream()), "ttmi_edit_distance")
    return out
