"""Device time of the token-and-duration loss beside the monotonic loss (the yardstick: existing code on the same lattice shape), and greedy
decoding of a TDT model beside the same model without the key.

Loss: the benchmark's lattice, B 32, T 500, U1 51, V 4334, bf16 logits in the joint's row-padded buffer (pitch 4352), full lengths, 50 labels.
ttmi_tdt_loss_fwd + _bwd with durations (1, 2, 3, 4) on the V + 4 live columns; ttmi_mono_loss_fwd + _bwd on the same buffer's first V
columns.  The gradient is written in place, as Transducer.loss does, so the logits are restored from a copy before every timed pair (outside
the timed window).  The two losses alternate; forward and backward are timed by their own device events; median, minimum and maximum of
--reps after --warmup.  The forward is two kernels (log-sum-exp + gather, alpha / beta): after the event timings the same calls run
--reps more rounds under torch's profiler (device activity only) and every tdt_* / mono_* kernel is reported by itself.  A kernel trace
of this tool in a run of its own (rocprofv3 --kernel-trace --stats -f csv -- python tools/tdt_time.py --reps 10 --no-decode --no-kernels) gives the
same table from another source.

Decode: Transducer.recognize on the benchmark's decode workload (tools/bench_decode.py: the C2 model, 32 utterances of 500 frames, fp32,
blank bias for about one symbol in ten frames against the start state) for a model with tdt_durations = [1, 2, 3, 4] and for the same config
without the key, alternating, wall time with a synchronisation on either side.  The weights are random: the durations such a model picks say
nothing about a trained model's.

    python tools/tdt_time.py [--reps 20] [--warmup 5] [--decode-reps 3] [--no-decode] [--no-loss] [--no-kernels]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
import torch

from ttmi import ops

B, T, U1, V = 32, 500, 51, 4334
DUR = (1, 2, 3, 4)


def stats(ms):
    return "median %.3f ms  min %.3f  max %.3f  (%d runs)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def loss_times(reps, warmup, kernels=True):
    dev = "cuda"
    D = len(DUR)
    pitch = (V + D + 63) // 64 * 64
    g = torch.Generator(device=dev).manual_seed(1)
    master = torch.randn(B, T, U1, pitch, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    buf = torch.empty_like(master)
    labels = torch.randint(1, V, (B, U1 - 1), device=dev, generator=g, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    ws_t, ws_m = ops.tdt_workspace(B, T, U1, D, dev), ops.mono_workspace(B, T, U1, dev)
    tdt, mono = buf[..., :V + D], buf[..., :V]

    def run_tdt():
        c = ops.tdt_loss_fwd(tdt, labels, tl, ul, 0, DUR, ws_t)
        return c, lambda: ops.tdt_loss_bwd(tdt, labels, tl, ul, 0, DUR, ws_t, one, 0, 1.0 / B, inplace=True)

    def run_mono():
        c = ops.mono_loss_fwd(mono, labels, tl, ul, 0, ws_m)
        return c, lambda: ops.mono_loss_bwd(mono, labels, tl, ul, 0, ws_m, one, 0, 1.0 / B, inplace=True)

    out = {"tdt fwd (lse + alpha/beta)": [], "tdt bwd (gradient)": [], "mono fwd (lse + alpha/beta)": [], "mono bwd (gradient)": []}
    costs = {}
    for i in range(warmup + reps):
        for name, fn in (("tdt", run_tdt), ("mono", run_mono)):
            buf.copy_(master)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            c, bwd = fn()
            ev[1].record()
            bwd()
            ev[2].record()
            torch.cuda.synchronize()
            costs[name] = float(c.double().mean())
            if i >= warmup:
                out[name + " fwd (lse + alpha/beta)"].append(ev[0].elapsed_time(ev[1]))
                out[name + " bwd (gradient)"].append(ev[1].elapsed_time(ev[2]))
    print("loss: B %d, T %d, U1 %d, V %d, bf16, pitch %d, full lengths; TDT durations %s on V + %d columns, monotonic on the first V"
          % (B, T, U1, V, pitch, DUR, D))
    print("mean cost: TDT %.3f, monotonic %.3f (random logits)" % (costs["tdt"], costs["mono"]))
    for name, ms in out.items():
        print("%-32s %s" % (name, stats(ms)))
    tot = {k: statistics.median(out[k + " fwd (lse + alpha/beta)"]) + statistics.median(out[k + " bwd (gradient)"]) for k in ("tdt", "mono")}
    print("whole loss (medians): TDT %.3f ms, monotonic %.3f ms, ratio %.2f" % (tot["tdt"], tot["mono"], tot["tdt"] / tot["mono"]))

    def one_round():
        for fn in (run_tdt, run_mono):
            buf.copy_(master)
            fn()[1]()
    if kernels:
        kernel_times(one_round, reps)


def kernel_times(one_round, reps):
    """per kernel: the device time of every tdt_* / mono_* kernel over `reps` more rounds of the same calls, from torch's profiler (device
    activity only), after the event timings so that the tracing does not touch them"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            one_round()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.events():
        name = ev.name
        if "tdt_" not in name and "mono_" not in name:
            continue
        us = getattr(ev, "device_time", None)
        if us is None:
            us = getattr(ev, "cuda_time", 0.0)
        if not us:
            us = ev.time_range.elapsed_us()
        short = name[name.index("tdt_") if "tdt_" in name else name.index("mono_"):]
        for cut in ("IfEEvPK", "ItEEvPK", "ILi", "EPK", "Ev"):       # mangled names: keep the kernel's own name
            if cut in short:
                short = short[:short.index(cut)]
                break
        rows.setdefault(short.split("<")[0].split("(")[0], []).append(float(us))
    print("per kernel (torch profiler, device time, %d launches each):" % reps)
    if not rows:
        print("  the profiler returned no tdt_* / mono_* kernel records")
    for name in sorted(rows):
        v = rows[name]
        print("  %-24s median %.3f ms  min %.3f  max %.3f  (%d launches)" % (name, statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3, len(v)))


def decode_times(reps):
    os.environ["TTMI_PRECISION"] = "fp32"
    from bench import c2_config
    from tt.model import Transducer
    dev = torch.device("cuda", 0)
    utts, emit_rate = 32, 0.1
    models = {}
    for name, extra in (("TDT, durations %s" % (list(DUR),), dict(tdt_durations=list(DUR))), ("same config without the key", {})):
        cfg = c2_config()
        cfg.update(extra)
        torch.manual_seed(1)
        models[name] = Transducer(cfg).to(dev).eval()
    d = models[next(iter(models))].config.enc.d_model
    g = torch.Generator(device=dev).manual_seed(1234)
    feats = torch.randn(utts, T, 80, device=dev, generator=g)
    proj = torch.randn(80, d, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) / 80 ** 0.5
    inputs = feats @ proj
    lens = [T] * utts
    out = {k: [] for k in models}
    res = {}
    with torch.no_grad():
        for model in models.values():                                # tools/bench_decode.py's blank bias, on the token columns
            enc = model.encoder(inputs[:1], None)
            z = model.joint(enc, model.decoder(torch.zeros(1, 1, dtype=torch.long, device=dev)))[0, :, 0, :V].float()
            model.joint.project_layer.bias[0] += torch.quantile(z[:, 1:].max(dim=1).values - z[:, 0], 1.0 - emit_rate)
        for i in range(1 + reps):                                    # (the first round is the warm-up: graphs, first launches)
            for name, model in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = model.recognize(inputs, lens, details=True)
                torch.cuda.synchronize()
                if i:
                    out[name].append(time.perf_counter() - t0)
    print("decode: recognize(details=True), C2 model (random weights), %d utterances of %d frames, fp32, emit rate target %.2f" % (utts, T, emit_rate))
    for name, secs in out.items():
        r = res[name]
        nsym = sum(len(u.tokens) for u in r)
        line = "%-36s %.1f utt/s (median of %d; min %.1f, max %.1f), %.1f symbols per utterance" % (
            name, utts / statistics.median(secs), len(secs), utts / max(secs), utts / min(secs), nsym / utts)
        if hasattr(r[0], "durations"):
            line += ", mean duration of the tokens' decisions %.2f" % (sum(sum(u.durations) for u in r) / max(nsym, 1))
        print(line)
    print("random weights: the durations chosen here say nothing about a trained model's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decode-reps", type=int, default=3)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-loss", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="skip the profiler pass (for a run under an external kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tdt_time: needs the GPU (a timing anywhere else says nothing)")
    if not a.no_loss:
        loss_times(a.reps, a.warmup, not a.no_kernels)
        torch.cuda.empty_cache()
    if not a.no_decode:
        decode_times(a.decode_reps)


if __name__ == "__main__":
    main()
