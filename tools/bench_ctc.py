"""What the CTC auxiliary head costs (bench.py is not involved):

  1. the loss launches alone at B=32, T=500, U=50, V=4334 (pitch 4352): ttmi_ctc_loss_fwd (symbol chains, log-sum-exp + gather pass,
     lattice walk: timed together, they are one call) and ttmi_ctc_loss_bwd (the gradient pass) - HIP events around `reps` calls after
     warm-up;
  2. a C2 training step (bench.py's model, bf16 mode, exp-domain loss) through Transducer.loss with ctc_weight 0 and 0.3, alternating in
     one process on the same module.

Bytes per second are the bytes the algorithm needs (computed here from the shapes) over the measured time; nothing is compared against a
threshold.  Writes profiles/ctc_bench.log.

    python tools/bench_ctc.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "transformer-transducer_amd")]
os.environ.setdefault("TTMI_PRECISION", "bf16")
import torch

import bench
from tt.model import Transducer
from ttmi import ops


def timed(fn, reps=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(out, B=32, T=500, U=50, V=4334):
    g = torch.Generator(device="cuda").manual_seed(1)
    buf, logits = ops.padded_empty((B, T, V), torch.float32, "cuda")
    buf.normal_(generator=g)
    ld = buf.shape[-1]
    y = torch.randint(1, V, (B, U), device="cuda", generator=g).int()
    al = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ul = torch.full((B,), U, dtype=torch.int32, device="cuda")
    one = torch.ones(1, device="cuda")
    ws = ops.ctc_workspace(B, T, U, "cuda")
    grad = torch.empty_like(buf)[..., :V]
    L = ops.lib()

    def fwd(lens):
        costs = torch.empty(B, device="cuda")       # (allocation from the caching allocator: no device work)
        ops.check(L.ttmi_ctc_loss_fwd(ops._p(logits), ops.c_long(ld), ops._p(y), ops._p(lens), ops._p(ul), B, T, U, V, 0, ops._p(ws),
                                      ops._p(costs), ops._stream()), "ttmi_ctc_loss_fwd")

    def bwd():
        ops.check(L.ttmi_ctc_loss_bwd(ops._p(logits), ops.c_long(ld), ops._p(y), ops._p(al), ops._p(ul), B, T, U, V, 0, ops._p(ws), ops._p(one),
                                      0, ops.c_float(1.0 / B), ops._p(grad), ops.c_long(ld), ops._stream()), "ttmi_ctc_loss_bwd")

    t_fwd = timed(lambda: fwd(al))
    fwd(al)
    t_bwd = timed(bwd)
    S = 2 * U + 1
    rows = B * T
    lse_bytes = rows * V * 4 + rows * S * 4                                   # logits read once, emission table written
    walk_bytes = 2 * rows * S * (4 + 8)                                       # both directions: emission table read, alpha / beta written
    grad_bytes = rows * V * 4 + rows * ld * 4 + rows * S * (8 + 8 + 4)        # logits read, gradient written, alpha / beta / table read
    out.append("CTC loss kernels alone, B=%d T=%d U=%d V=%d (pitch %d), f32 logits, %d reps after 5 warm-up calls, HIP events" % (B, T, U, V, ld, 50))
    out.append("  ttmi_ctc_loss_fwd (symbol chains + log-sum-exp / gather + lattice walk, 3 launches): %.4f ms" % t_fwd)
    out.append("    bytes needed: log-sum-exp / gather %.1f MB, walk %.1f MB -> forward as a whole %.1f GB/s "
               "(the walk is latency-bound: %d dependent frames per direction)" % (lse_bytes / 1e6, walk_bytes / 1e6, (lse_bytes + walk_bytes) / t_fwd / 1e6, T))
    out.append("  ttmi_ctc_loss_bwd (gradient pass, 1 launch): %.4f ms, %.1f MB needed -> %.1f GB/s" % (t_bwd, grad_bytes / 1e6, grad_bytes / t_bwd / 1e6))
    return t_fwd, t_bwd


def step(out, B=32, T=500, U=50, rounds=6, reps=5):
    cfg = bench.c2_config()
    cfg["ctc_weight"] = 0.3
    torch.manual_seed(0)
    model = Transducer(cfg).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, T, 512, device="cuda", generator=g)
    y = torch.randint(1, 4334, (B, U), device="cuda", generator=g)
    al = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ul = torch.full((B,), U, dtype=torch.int32, device="cuda")

    def run(w):
        model.zero_grad(set_to_none=False)
        model.loss(x, al, y, ul, check_lengths=False, exp_domain=True, ctc_weight=w).backward()

    for w in (0.0, 0.3, 0.0, 0.3):          # the first step seeds the exp-domain shift; every shape of both forms warmed
        run(w)
    t = {0.0: [], 0.3: []}
    for _ in range(rounds):                  # alternating, same process, same module
        for w in (0.0, 0.3):
            t[w].append(timed(lambda: run(w), reps=reps, warmup=1))
    m0, m1 = (sorted(t[w])[len(t[w]) // 2] for w in (0.0, 0.3))
    out.append("C2 training step through Transducer.loss (forward + backward, no optimiser), B=%d T=%d U=%d, %s mode, exp-domain RNN-T loss, "
               "%d alternating rounds of %d steps, medians" % (B, T, U, os.environ["TTMI_PRECISION"], rounds, reps))
    out.append("  ctc_weight 0:   %.3f ms  (rounds: %s)" % (m0, " ".join("%.3f" % v for v in t[0.0])))
    out.append("  ctc_weight 0.3: %.3f ms  (rounds: %s)" % (m1, " ".join("%.3f" % v for v in t[0.3])))
    out.append("  difference: %+.3f ms per step" % (m1 - m0))
    return m1 - m0


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc.py needs the GPU: nothing is measured without it")
    out = []
    t_fwd, t_bwd = kernels(out)
    diff = step(out)
    rows, V, d = 32 * 500, 4334, 512
    out.append("arithmetic for the step: head GEMMs 3 x %.1f GFLOP (projection, dgrad, wgrad); loss kernels alone %.3f ms; "
               "step difference minus loss kernels %.3f ms (the three GEMMs on the generic kernel, the bias column sums and the host's launches)"
               % (2.0 * rows * V * d / 1e9, t_fwd + t_bwd, diff - (t_fwd + t_bwd)))
    text = "\n".join(out)
    print(text)
    with open(os.path.join(ROOT, "profiles", "ctc_bench.log"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
