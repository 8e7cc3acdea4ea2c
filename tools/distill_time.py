"""The distillation kernels against the monotonic loss pair, same process, same bf16 logits: kd_collapse, kd_loss_fwd
and kd_loss_bwd(accumulate=1), and ttmi_mono_loss_fwd / ttmi_mono_loss_bwd as the yardstick, on the loss shape of one chunk of BASELINE
configs[1] (8 x T 500 x U + 1 = 51 x V 4334, bf16, row pitch 4352 - the chunk Transducer.loss picks for B = 32 in the bf16 mode).  The five
calls alternate; every call is timed by its own device events; median (minimum - maximum) of 20 after 5 warm-ups.  The monotonic gradient
is written out of place, as the distillation path of the fused joint + loss runs it, so that no call changes the logits.  The achieved
bandwidth counts the logits' and gradient's bytes at their pitch (what the row walks touch is V of every 4352 columns: 0.4 % less) plus
the per-row records.

    python tools/distill_time.py [--batch 32] [--reps 20] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
import torch

from ttmi import ops

T, U1, V = 500, 51, 4334


def chunk_size(B):
    """what Transducer.loss picks in the bf16 mode (JointNet.default_loss_chunk needs only the joint's sizes)"""
    from tt.model import JointNet
    return JointNet(1024, 1024, V).default_loss_chunk(B, T, U1, False, 1)


def timed(fns, reps, warmup):
    """fns: {name: callable}; they alternate.  -> {name: [ms] * reps}"""
    out = {k: [] for k in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_time: needs the GPU (a timing anywhere else says nothing)")
    Bc = chunk_size(a.batch)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    buf, logits = ops.padded_empty((Bc, T, U1, V), torch.bfloat16, dev)
    buf.zero_()
    logits.copy_(torch.randn(Bc, T, U1, V, device=dev, generator=g).to(torch.bfloat16))
    tbuf, tlogits = ops.padded_empty((Bc, T, U1, V), torch.bfloat16, dev)
    tbuf.zero_()
    tlogits.copy_(torch.randn(Bc, T, U1, V, device=dev, generator=g).to(torch.bfloat16))
    gbuf, grad = ops.padded_empty((Bc, T, U1, V), torch.bfloat16, dev)
    gbuf.zero_()
    y = torch.randint(1, V, (Bc, U1 - 1), device=dev, generator=g, dtype=torch.int32)
    tl = torch.full((Bc,), T, dtype=torch.int32, device=dev)
    ul = torch.full((Bc,), U1 - 1, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    wm, wk = ops.mono_workspace(Bc, T, U1, dev), ops.kd_workspace(Bc, T, U1, dev)
    post = ops.kd_collapse(tlogits, y, tl, ul, 0)
    ops.mono_loss_fwd(logits, y, tl, ul, 0, wm)
    ops.kd_loss_fwd(logits, y, tl, ul, 0, post, wk)
    rows, plane = Bc * T * U1, buf.numel() * 2
    fns = {
        "mono_loss_fwd": lambda: ops.mono_loss_fwd(logits, y, tl, ul, 0, wm),
        "mono_loss_bwd": lambda: ops.mono_loss_bwd(logits, y, tl, ul, 0, wm, one, 0, 1.0 / a.batch),
        "kd_collapse": lambda: ops.kd_collapse(logits, y, tl, ul, 0),
        "kd_loss_fwd": lambda: ops.kd_loss_fwd(logits, y, tl, ul, 0, post, wk),
        "kd_loss_bwd acc": lambda: ops.kd_loss_bwd(logits, y, tl, ul, 0, wk, one, 0, 1.0 / a.batch, accumulate=grad),
    }
    # bytes moved: logits planes read / gradient planes read and written, and the per-row tables of each call
    moved = {
        "mono_loss_fwd": plane + rows * 12 * 2 + Bc * (T + 1) * U1 * 16,          # lse, lpb, lpl written and the tables read back; alpha, beta written
        "mono_loss_bwd": 2 * plane + rows * 4 + Bc * (T + 1) * U1 * 16,
        "kd_collapse": plane + rows * 12,
        "kd_loss_fwd": plane + rows * (12 + 20 + 4),
        "kd_loss_bwd acc": 3 * plane + rows * 16,
    }
    print("chunk of %d utterances (batch %d): logits bf16 [%d, %d, %d, %d], pitch %d, %.2f GB per plane" % (Bc, a.batch, Bc, T, U1, V, buf.shape[-1], plane / 1e9))
    res = timed(fns, a.reps, a.warmup)
    for name, ms in res.items():
        med = statistics.median(ms)
        print("%-16s median %.3f ms (%.3f - %.3f), %d runs; %.2f GB moved, %.2f TB/s" % (name, med, min(ms), max(ms), len(ms), moved[name] / 1e9, moved[name] / med / 1e9))
    mf, mb = statistics.median(res["mono_loss_fwd"]), statistics.median(res["mono_loss_bwd"])
    for name, base, k in (("kd_collapse", mf, 1.0), ("kd_loss_fwd", mf, 1.0), ("kd_loss_bwd acc", mb, 1.5)):
        med = statistics.median(res[name])
        print("%-16s %.3f x its yardstick (a pass that moves %.1f x the yardstick's bytes)" % (name, med / base, k))


if __name__ == "__main__":
    main()
