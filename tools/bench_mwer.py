#!/usr/bin/env python3
"""MWER training (Transducer.mwer_loss) and its edit-distance kernel, measured in one process; the log goes to profiles/mwer_bench.log.

1. ttmi_edit_distance alone, HIP events around `--reps` back-to-back calls after a warm-up, at (P, length) = (128, 50), (1024, 200) and (32, 1024):
   random hypotheses against random transcripts of that length over 4334 symbols (every cell of every row is computed whatever the tokens are).
2. One training step (forward + backward, no optimiser) of `mwer_loss` beside one step of `Transducer.loss` on the same C2 model and batch,
   alternating, `--steps` of each after `--warmup`; host clock around work that ends in a device synchronise.
3. The split of the MWER step: the beam search alone (on encoder states computed beforehand), `mwer_loss(hypotheses=...)` under no_grad (audio
   encoder + label encoder on the rows + edit distances + pass 1) and the whole step with given hypotheses (those + pass 2 + backward).

    python tools/bench_mwer.py [--batch 4] [--T 100] [--U 10] [--beam 4] [--precision bf16] [--steps 5] [--warmup 2] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def bench_kernel(P, length, reps, dev):
    from ttmi import ops
    g = torch.Generator(device=dev).manual_seed(P + length)
    hyp = torch.randint(0, 4334, (P, length), device=dev, generator=g, dtype=torch.int32)
    ref = torch.randint(0, 4334, (P, length), device=dev, generator=g, dtype=torch.int32)
    lens = torch.full((P,), length, dtype=torch.int32, device=dev)
    for _ in range(3):
        ops.edit_distance(hyp, lens, ref, lens)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        out = ops.edit_distance(hyp, lens, ref, lens)
    stop.record()
    torch.cuda.synchronize()
    us = 1e3 * start.elapsed_time(stop) / reps
    return {"P": P, "length": length, "us_per_call": round(us, 1), "cells_per_us": round(P * length * length / us, 1),
            "mean_distance": round(float(out[:, 0].double().mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--U", type=int, default=10)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mwer_bench.log"))
    a = ap.parse_args()
    os.environ["TTMI_PRECISION"] = a.precision
    from bench import c2_config
    from tt.model import Transducer
    dev = torch.device("cuda", 0)
    out = {"edit_distance_kernel": [bench_kernel(P, n, a.reps, dev) for P, n in ((128, 50), (1024, 200), (32, 1024))]}

    cfg = c2_config()
    torch.manual_seed(1)
    model = Transducer(cfg).to(dev).train()
    B, T, U, W = a.batch, a.T, a.U, a.beam
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(B, T, cfg["enc"]["d_model"], device=dev, generator=g)
    y = torch.randint(1, cfg["vocab_size"], (B, U), device=dev, generator=g)
    al = torch.full((B,), T, dtype=torch.int32, device=dev)
    ll = torch.full((B,), U, dtype=torch.int32, device=dev)
    with torch.no_grad():
        # blank bias such that about U of the T frames emit (tools/bench_decode.py): hypotheses of the transcripts' length, not of T symbols
        z = model.joint(model.encoder(x[:1], None), model.decoder(torch.zeros(1, 1, dtype=torch.long, device=dev)))[0, :, 0, :].float()
        model.joint.project_layer.bias[0] += torch.quantile(z[:, 1:].max(dim=1).values - z[:, 0], 1.0 - U / T)

    def step_rnnt():
        model.zero_grad()
        model.loss(x, al, y, ll).backward()

    def step_mwer(**kw):
        model.zero_grad()
        model.mwer_loss(x, al, y, ll, beam_width=W, **kw).backward()

    for _ in range(a.warmup):
        step_rnnt()
        step_mwer()
    t_rnnt, t_mwer = [], []
    for _ in range(a.steps):                                   # alternating: both see the same machine
        t_rnnt.append(timed(step_rnnt)[1])
        t_mwer.append(timed(step_mwer)[1])
    # the split, on the hypotheses of one more search
    model.eval()
    with torch.no_grad():
        enc = model.encoder(x, None)
        model.beam_decode_batch(enc, al, beam_width=W)
        nbest, t_search = timed(lambda: model.beam_decode_batch(enc, al, beam_width=W))
    model.train()
    hyps = [[list(h.tokens) for h in res] for res in nbest]
    t_fwd, t_given = [], []
    for _ in range(a.steps):
        with torch.no_grad():
            t_fwd.append(timed(lambda: model.mwer_loss(x, al, y, ll, hypotheses=hyps))[1])
        t_given.append(timed(lambda: step_mwer(hypotheses=hyps))[1])
    med = statistics.median
    out["workload"] = ("C2 model (12 / 6 layers, V = 4334, dropout 0.1, train mode), %s, B = %d, T = %d, U = %d, beam %d -> %d hypothesis rows of at most %d tokens"
                       % (a.precision, B, T, U, W, sum(len(h) for h in hyps), max(len(t) for h in hyps for t in h)))
    out["step_ms"] = {"rnnt_loss": round(med(t_rnnt), 2), "mwer_loss": round(med(t_mwer), 2), "rnnt_all": [round(v, 2) for v in t_rnnt],
                      "mwer_all": [round(v, 2) for v in t_mwer], "steps": a.steps, "warmup": a.warmup}
    out["mwer_split_ms"] = {"search": round(t_search, 2), "encoders_edit_distance_pass1_no_grad": round(med(t_fwd), 2),
                            "step_with_given_hypotheses": round(med(t_given), 2),
                            "pass2_and_backward_by_difference": round(med(t_given) - med(t_fwd), 2)}
    line = json.dumps(out)
    print(line, flush=True)
    with open(a.log, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
