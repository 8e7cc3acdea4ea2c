#!/usr/bin/env python3
"""Wall time per window of the DECODE part of ttmi.streaming.StreamingRecognizer (the encoder excluded) on the recorded stream of
tests/golden/streaming.npz with test_frontend_gpu.py's model: the greedy recogniser beside the beam search at the given widths (and, with
--context, a beam of four with one hotword phrase), interleaved in this process, --repeats passes each after one warm-up pass.  A window
carries 15 519 new samples = 0.97 s of audio.  The clock is the host's around work that ends in a device synchronise; the stable-prefix kernel
is timed by device events as well.  One JSON line.

    python tools/bench_streaming_nbest.py [--widths 1,4] [--repeats 7] [--context]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed_decode(rec, times):
    """wrap the recogniser's decode step (greedy or beam) in a synchronised host clock; one entry per window that decodes frames"""
    name = "_greedy" if rec.search is None else "_beam"
    inner = getattr(rec, name)

    def outer(eff, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inner(eff, *args)
        torch.cuda.synchronize()
        if eff.shape[0]:
            times.append((eff.shape[0], 1e3 * (time.perf_counter() - t0)))
    setattr(rec, name, outer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="1,4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--context", action="store_true")
    a = ap.parse_args()
    from test_frontend_gpu import _streaming_model
    from ttmi import ops
    from ttmi.context import ContextGraph
    from ttmi.streaming import StreamingRecognizer
    z = np.load(os.path.join(ROOT, "tests", "golden", "streaming.npz"))
    model = _streaming_model(z)
    n = int(z["n_windows"])
    wins = [torch.tensor(z["win%d" % i]).cuda() for i in range(n)]
    tokens = z["tokens"].tolist()
    configs = {"greedy": {}}
    for W in [int(w) for w in a.widths.split(",")]:
        configs["beam_%d" % W] = dict(beam_width=W)
    if a.context:
        configs["beam_4_hotword"] = dict(beam_width=4, context=ContextGraph([tokens[40:43]], boost=2.0))
    times, results = {name: [] for name in configs}, {}
    for rep in range(a.repeats + 1):
        for name, kw in configs.items():
            rec = StreamingRecognizer(model, **kw)
            per = []
            timed_decode(rec, per)
            for i in range(n):
                rec.feed(wins[i], last=(i == n - 1))
            results[name] = rec
            if rep:                                                   # pass 0 warms every shape up
                times[name].append(per)
    out = {"workload": "streaming.npz: %d windows, %d decoded frames, %d greedy tokens; a window = 0.97 s of audio" % (n, results["greedy"].pos, len(tokens)),
           "repeats": a.repeats, "decode_ms_per_window": {}}
    for name, passes in times.items():
        per_window = [ms for p in passes for _, ms in p]
        per_pass = [sum(ms for _, ms in p) for p in passes]
        frames = sum(f for f, _ in passes[0])
        out["decode_ms_per_window"][name] = {
            "median": round(statistics.median(per_window), 3), "min": round(min(per_window), 3), "max": round(max(per_window), 3),
            "windows_timed_per_pass": len(passes[0]), "ms_per_frame": round(statistics.median(per_pass) / frames, 4),
            "pass_ms_median": round(statistics.median(per_pass), 2), "pass_ms_min": round(min(per_pass), 2), "pass_ms_max": round(max(per_pass), 2),
            "share_of_audio": round(statistics.median(per_window) / 970.0, 5),
            "tokens_equal_greedy": results[name].result == results["greedy"].result}
    # the stable-prefix kernel alone, on the final beam of the widest search: device events, 10 rounds of 10 calls
    search = StreamingRecognizer(model, beam_width=max(int(w) for w in a.widths.split(",")))
    for i in range(n - 1):
        search.feed(wins[i])
    cur = search.search.cur
    buf = torch.empty(1, dtype=torch.int32, device="cuda")
    ev_times = []
    ops.beam_stable_prefix(cur["score"], cur["meta"][0], cur["hist"], out=buf)
    for _ in range(10):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
        ev[0].record()
        for i in range(10):
            ops.beam_stable_prefix(cur["score"], cur["meta"][0], cur["hist"], out=buf)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ev_times += [1e3 * x.elapsed_time(y) for x, y in zip(ev, ev[1:])]
    out["stable_prefix_kernel_us"] = {"median": round(statistics.median(ev_times), 2), "min": round(min(ev_times), 2),
                                      "W": search.beam_width, "ld_hist": int(cur["hist"].shape[2]), "stable": int(buf.item())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
