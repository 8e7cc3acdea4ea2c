"""Monotonic against standard forced alignment, same process: ttmi_mono_align and ttmi_rnnt_align alternating, each on
the workspace its own loss forward filled from the same f32 logits (vocabulary of 8: the aligners read the emission tables, never the
logits), with the emission-statistics kernels beside them.  Two shapes: the loss chunk of BASELINE configs[1] (8 x T 500 x U + 1 = 51) and
C5's lattice (8 x T 2000 x U + 1 = 201), full lengths.  Both decision-word placements are timed: where the shape puts them (LDS for both
shapes) and the caller's workspace (ttmi_set_option(23, 1)); option 23 = 2 gives the forward walk without the backtrace.  Every call is timed
by its own device events; median, minimum and maximum of 20 after 5 warm-ups.

    python tools/mono_align_time.py [--reps 20] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
import torch

from ttmi import ops

SHAPES = [("configs[1] loss chunk", 8, 500, 51), ("C5 lattice", 8, 2000, 201)]
PLACEMENTS = [("words by shape (LDS)", 0), ("words in workspace", 1), ("LDS, no backtrace", 2)]


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


def report(title, res):
    for name, ms in res.items():
        print("%-46s %-10s median %.3f ms  min %.3f  max %.3f  (%d runs)" % (title, name, statistics.median(ms), min(ms), max(ms), len(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mono_align_time: needs the GPU (a timing anywhere else says nothing)")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    for title, B, T, U1 in SHAPES:
        x = torch.randn(B, T, U1, 8, device=dev, generator=g)
        y = torch.randint(1, 8, (B, U1 - 1), device=dev, generator=g, dtype=torch.int32)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        ul = torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
        wm, wr = ops.mono_workspace(B, T, U1, dev), ops.rnnt_workspace(B, T, U1, dev)
        ops.mono_loss_fwd(x, y, tl, ul, 0, wm)
        ops.rnnt_loss_fwd(x, y, tl, ul, 0, wr)
        torch.cuda.synchronize()
        head = "%s [%d, %d, %d]" % (title, B, T, U1)
        for pname, bits in PLACEMENTS:
            ops.set_option(23, bits)
            try:
                report("%s align, %s" % (head, pname), timed({"monotonic": lambda: ops.mono_align(wm, tl, ul, B, T, U1),
                                                              "standard": lambda: ops.rnnt_align(wr, tl, ul, B, T, U1)}, a.reps, a.warmup))
            finally:
                ops.set_option(23, 0)
        report("%s emit_stats" % head, timed({"monotonic": lambda: ops.mono_emit_stats(wm, tl, ul, B, T, U1),
                                              "standard": lambda: ops.rnnt_emit_stats(wr, tl, ul, B, T, U1)}, a.reps, a.warmup))
        print("%s serial steps of the walk: monotonic %d frames, standard %d anti-diagonals" % (head, T, T + U1 - 2))


if __name__ == "__main__":
    main()
