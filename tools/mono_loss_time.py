"""Monotonic against standard RNN-T loss kernels, same process, same bf16 logits: mono_loss_fwd + mono_loss_bwd and
rnnt_loss_fwd + rnnt_loss_bwd on the loss shape of one chunk of BASELINE configs[1] (T 500, U + 1 = 51, V 4334, row pitch 4352, the chunk size
Transducer.loss picks for B = 32 in the bf16 mode), the gradient written in place as the fused joint + loss does.  The two pairs alternate;
every call pair is timed by its own device events (the logits are restored outside the timed window); median, minimum and maximum of 20
after 5 warm-ups.  The lattice kernels alone are timed the way tools/bench_lattice.py times them: the forward on logits with a vocabulary of
8, where the log-sum-exp pass is negligible.

    python tools/mono_loss_time.py [--batch 32] [--reps 20] [--warmup 5]
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


def timed(fns, reps, warmup, before=None):
    """fns: {name: callable}; they alternate.  -> {name: [ms] * reps}"""
    out = {k: [] for k in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def report(title, res):
    for name, ms in res.items():
        print("%-28s %-10s median %.3f ms  min %.3f  max %.3f  (%d runs)" % (title, name, statistics.median(ms), min(ms), max(ms), len(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mono_loss_time: needs the GPU (a timing anywhere else says nothing)")
    Bc = chunk_size(a.batch)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    src = torch.randn(Bc, T, U1, V, device=dev, generator=g).to(torch.bfloat16)
    buf, logits = ops.padded_empty((Bc, T, U1, V), torch.bfloat16, dev)
    buf.zero_()
    y = torch.randint(1, V, (Bc, U1 - 1), device=dev, generator=g, dtype=torch.int32)
    tl = torch.full((Bc,), T, dtype=torch.int32, device=dev)
    ul = torch.full((Bc,), U1 - 1, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    wm, wr = ops.mono_workspace(Bc, T, U1, dev), ops.rnnt_workspace(Bc, T, U1, dev)

    def mono():
        ops.mono_loss_fwd(logits, y, tl, ul, 0, wm)
        ops.mono_loss_bwd(logits, y, tl, ul, 0, wm, one, 0, 1.0 / a.batch, inplace=True)

    def rnnt():
        ops.rnnt_loss_fwd(logits, y, tl, ul, 0, wr)
        ops.rnnt_loss_bwd(logits, y, tl, ul, 0, wr, one, 0, 1.0 / a.batch, inplace=True)

    print("chunk of %d utterances (batch %d): logits bf16 [%d, %d, %d, %d], pitch %d, %.2f GB" % (Bc, a.batch, Bc, T, U1, V, buf.shape[-1], buf.numel() * 2 / 1e9))
    report("loss fwd + bwd (in place)", timed({"monotonic": mono, "standard": rnnt}, a.reps, a.warmup, before=lambda: logits.copy_(src)))
    small = torch.randn(Bc, T, U1, 8, device=dev, generator=g)
    ys = torch.randint(1, 8, (Bc, U1 - 1), device=dev, generator=g, dtype=torch.int32)
    report("lattice alone (fwd, V = 8)", timed({"monotonic": lambda: ops.mono_loss_fwd(small, ys, tl, ul, 0, wm),
                                                 "standard": lambda: ops.rnnt_loss_fwd(small, ys, tl, ul, 0, wr)}, a.reps, a.warmup))
    steps = {"monotonic": T, "standard": T + U1 - 2}
    print("serial steps of the recursion: monotonic %d frames, standard %d anti-diagonals" % (steps["monotonic"], steps["standard"]))


if __name__ == "__main__":
    main()
