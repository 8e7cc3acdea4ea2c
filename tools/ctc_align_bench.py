"""Device time of ttmi_ctc_align and ttmi_ctc_emit_stats beside ttmi_ctc_loss_fwd on the same inputs, at the CTC head of
BASELINE configs[1]: B 32, T 500, U 50, V 4334, full lengths.  The aligner's yardstick is the forward's alpha walk - the same dynamic programme
over the same emission table - which the forward runs after its log-sum-exp pass over the [B, T, V] logits; the forward is therefore timed
a second time on a vocabulary of 8, where that pass is next to nothing and the lattice walk (alpha and beta side by side, one workgroup each)
is what remains.  Both decision-word placements are timed: where the shape puts them (LDS) and the caller's workspace
(ttmi_set_option(23, 1)); option 23 = 2 gives the forward walk without the backtrace.  The calls alternate, every call is timed by its own
device events; median, minimum and maximum of 20 after 5 warm-ups.

    python tools/ctc_align_bench.py [--reps 20] [--warmup 5]

The per-kernel times beside them in profiles/ctc_align_bench.log are those of a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace -- python tools/ctc_align_bench.py --reps 10).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
import torch

from ttmi import ops

B, T, U, V = 32, 500, 50, 4334
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_align_bench: needs the GPU (a timing anywhere else says nothing)")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, T, V, device=dev, generator=g)
    x8 = x[..., :8].contiguous()
    y = torch.randint(1, 8, (B, U), device=dev, generator=g, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U, dtype=torch.int32, device=dev)
    ws, ws8 = ops.ctc_workspace(B, T, U, dev), ops.ctc_workspace(B, T, U, dev)
    aws = ops.ctc_align_workspace(B, T, U, dev)
    ops.ctc_loss_fwd(x, y, tl, ul, 0, ws)
    ops.ctc_loss_fwd(x8, y, tl, ul, 0, ws8)
    torch.cuda.synchronize()
    fns = {"ctc_loss_fwd, V %d" % V: lambda: ops.ctc_loss_fwd(x, y, tl, ul, 0, ws),
           "ctc_loss_fwd, V 8 (the lattice walk)": lambda: ops.ctc_loss_fwd(x8, y, tl, ul, 0, ws8),
           "ctc_emit_stats": lambda: ops.ctc_emit_stats(ws, y, tl, ul, B, T, V, 0)}
    res = {}
    for pname, bits in PLACEMENTS:
        ops.set_option(23, bits)
        try:
            key = "ctc_align, %s" % pname
            r = timed(dict(fns, **{key: lambda: ops.ctc_align(ws, y, tl, ul, B, T, V, 0, align_workspace=aws)}), a.reps, a.warmup)
        finally:
            ops.set_option(23, 0)
        res[key] = r[key]
        for k in fns:
            res.setdefault(k, []).extend(r[k])
    print("CTC head of configs[1]: B %d, T %d, U %d, V %d, full lengths" % (B, T, U, V))
    for name, ms in res.items():
        print("%-40s median %.3f ms  min %.3f  max %.3f  (%d runs)" % (name, statistics.median(ms), min(ms), max(ms), len(ms)))
    walk = statistics.median(res["ctc_loss_fwd, V 8 (the lattice walk)"])
    for pname, _ in PLACEMENTS:
        print("ctc_align, %s / lattice walk of the forward: %.2f" % (pname, statistics.median(res["ctc_align, %s" % pname]) / walk))


if __name__ == "__main__":
    main()
