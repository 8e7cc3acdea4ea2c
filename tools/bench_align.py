"""What forced alignment adds on top of a forward: `Transducer.align` at C2 (B=32, T=500, U=50, the bench.py model) in the bf16 exp-domain
form against a no-grad `Transducer.loss` forward of the same form (the loss path is the one of the commit before the alignment feature:
nothing on it changed).  HIP events around 20 calls after 3 warm-up calls, the protocol of tools/bench_lattice.py:

    python tools/bench_align.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "transformer-transducer_amd")]
os.environ["TTMI_PRECISION"] = "bf16"
import torch

import bench
from tt.model import Transducer


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(B=32, T=500, U=50):
    torch.manual_seed(0)
    model = Transducer(bench.c2_config()).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, T, 512, device="cuda", generator=g)
    y = torch.randint(1, 4334, (B, U), device="cuda", generator=g)
    al = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ll = torch.full((B,), U, dtype=torch.int32, device="cuda")
    for _ in range(2):          # the first step runs the plain form and seeds the shift, the second is the exp-domain form
        model.zero_grad()
        model.loss(x, al, y, ll, check_lengths=False, exp_domain=True).backward()
    model.eval()

    def loss_fwd():
        with torch.no_grad():
            return model.loss(x, al, y, ll, check_lengths=False, exp_domain=True, reduction="none")

    t_loss = timed(loss_fwd)
    t_align = timed(lambda: model.align(x, al, y, ll, check_lengths=False, exp_domain=True))
    t_stats = timed(lambda: model.align(x, al, y, ll, check_lengths=False, exp_domain=True, stats=True))
    st = model.joint.exp_shift_state(x.device)
    print("C2 B=%d T=%d U=%d bf16 exp-domain (shift valid: %s): no-grad Transducer.loss forward %.3f ms, Transducer.align %.3f ms (%+.3f), "
          "with stats %.3f ms (%+.3f)" % (B, T, U, st.valid, t_loss, t_align, t_align - t_loss, t_stats, t_stats - t_loss))


if __name__ == "__main__":
    main()
