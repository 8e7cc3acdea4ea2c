"""Device time and peak memory of ttmi_ctc_score_hyps beside the only route there was before it - the utterances' logits gathered into a
[B * W, T, V] batch and ttmi_ctc_loss_fwd on it - at the CTC head of BASELINE configs[1] under a beam of four: B 32,
T 500, V 4334, W 4, hypotheses of 40 to 60 tokens, full lengths.  The scorer is timed at U = 63 (the hypotheses' own width: one wave per
pair) and at U = T (what beam_decode_batch passes, the beam's history pitch: eight waves per pair).  The calls alternate, every call is timed
by its own device events; median, minimum and maximum of 20 after 5 warm-ups.  Peak device memory of each route: torch's allocator peak over
one call, above what is resident before it (logits, hypotheses, lengths).  Then one whole Transducer.beam_decode_batch of the C2 model with a
CTC head (8 utterances of 500 frames, W 4, wall time with a synchronisation on either side) with and without ctc_weight, alternating.

    python tools/ctc_rescore_bench.py [--reps 20] [--warmup 5] [--search-reps 3] [--no-search]

The per-kernel times beside them in profiles/ctc_rescore_time.log are those of a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/ctc_rescore_bench.py --reps 10 --no-search).
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

B, T, V, W = 32, 500, 4334, 4


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


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def search_times(reps):
    """wall ms of beam_decode_batch on the C2 model with a CTC head, 8 utterances of 500 frames, W 4: plain and with ctc_weight, alternating"""
    os.environ["TTMI_PRECISION"] = "fp32"
    from bench import c2_config
    from tt.model import Transducer
    cfg = c2_config()
    cfg["ctc_weight"] = 0.3
    torch.manual_seed(1)
    model = Transducer(cfg).cuda().eval()
    utts = 8
    g = torch.Generator(device="cuda").manual_seed(1234)
    inputs = torch.randn(utts, T, 80, device="cuda", generator=g) @ (torch.randn(80, 512, device="cuda", generator=g) / 80 ** 0.5)
    lens = [T] * utts
    with torch.no_grad():
        enc = model.encoder(inputs[:1], None)
        z = model.joint(enc, model.decoder(torch.zeros(1, 1, dtype=torch.long, device="cuda")))[0, :, 0, :].float()
        model.joint.project_layer.bias[0] += torch.quantile(z[:, 1:].max(dim=1).values - z[:, 0], 0.9)      # about one symbol in ten frames
        enc = model.encoder(inputs, None)
        configs = {"beam_decode_batch, plain": {}, "beam_decode_batch, ctc_weight 0.3": dict(ctc_weight=0.3)}
        out = {k: [] for k in configs}
        res = {}
        for i in range(1 + reps):
            for name, kw in configs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = model.beam_decode_batch(enc, lens, beam_width=W, **kw)
                torch.cuda.synchronize()
                if i:
                    out[name].append(1e3 * (time.perf_counter() - t0))
    a, b = res.values()
    print("C2 model with a CTC head (random weights), %d utterances of %d frames, W %d; %.1f tokens in the best hypothesis; the head changes the "
          "1-best of %d utterances" % (utts, T, W, sum(len(u[0].tokens) for u in a) / utts, sum(x[0].tokens != y[0].tokens for x, y in zip(a, b))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--search-reps", type=int, default=3)
    ap.add_argument("--no-search", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_rescore_bench: needs the GPU (a timing anywhere else says nothing)")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, T, V, device=dev, generator=g)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    P = B * W
    hist = torch.randint(1, V, (P, T + 2), device=dev, generator=g, dtype=torch.int64)       # the beam's history buffer: column 0 = start symbol
    hl = torch.randint(40, 61, (P,), device=dev, generator=g, dtype=torch.int32)
    narrow, wide = hist[:, 1:64], hist[:, 1:1 + T]
    ws = ops.ctc_score_workspace(B, T, dev)
    idx = torch.arange(P, device=dev) // W

    def expand():
        big = x[idx]                                                                         # [B * W, T, V]
        lab = narrow.to(torch.int32).contiguous()
        return ops.ctc_loss_fwd(big, lab, tl[idx], hl, 0, ops.ctc_workspace(P, T, 63, dev))

    fns = {"ctc_score_hyps, U 63 (one wave per pair)": lambda: ops.ctc_score_hyps(x, tl, narrow, hl, None, 0, workspace=ws),
           "ctc_score_hyps, U %d (the beam's pitch)" % T: lambda: ops.ctc_score_hyps(x, tl, wide, hl, None, 0, workspace=ws),
           "gather to [B*W, T, V] + ctc_loss_fwd": expand}
    got = [fn() for fn in fns.values()]
    torch.cuda.synchronize()
    same = torch.equal(got[0], got[1]) and torch.equal((-got[0]).float(), got[2])
    res = timed(fns, a.reps, a.warmup)
    print("CTC head of configs[1] under a beam: B %d, T %d, V %d, W %d (P %d), hypotheses of 40..60 tokens, full lengths" % (B, T, V, W, P))
    print("the three routes give the same bits: %s" % same)
    for name, ms in res.items():
        print("%-44s median %.3f ms  min %.3f  max %.3f  (%d runs)" % (name, statistics.median(ms), min(ms), max(ms), len(ms)))
    new, old = statistics.median(res["ctc_score_hyps, U %d (the beam's pitch)" % T]), statistics.median(res["gather to [B*W, T, V] + ctc_loss_fwd"])
    print("expand route / ctc_score_hyps at the beam's pitch: %.2f" % (old / new))
    print("resident before either route (logits, histories): %.1f MiB" % (torch.cuda.memory_allocated() / 2.0 ** 20))
    print("peak device memory above that: ctc_score_hyps (workspace included) %.2f MiB, expand route %.1f MiB"
          % (peak_mib(lambda: ops.ctc_score_hyps(x, tl, wide, hl, None, 0)), peak_mib(expand)))
    del x, got
    torch.cuda.empty_cache()
    if not a.no_search:
        for name, ms in search_times(a.search_reps).items():
            print("%-44s median %.1f ms  min %.1f  max %.1f  (%d runs, wall)" % (name, statistics.median(ms), min(ms), max(ms), len(ms)))


if __name__ == "__main__":
    main()
