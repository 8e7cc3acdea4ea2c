#!/usr/bin/env python3
"""Frame-synchronous beam search (Transducer.beam_decode_batch) at tools/bench_decode.py's workload - the C2 model on synthetic utterances,
blank bias set for the emit rate - for beam widths 1, 4 and 8, beside greedy decode_batch (plain and details=True) measured in the same process
on the same encoder states.  Utterances/s include the encoder's time, as bench_decode.py's do.  One JSON line.

--context N adds contextual biasing: N phrases of 2 to 4 tokens are drawn from the greedy hypotheses of the run's own
utterances, and per beam width three configurations are timed interleaved in this process, --repeats times each: no context (ttmi_beam_step),
the phrases' graph with every weight 0 (ttmi_beam_step_ctx searching exactly the same hypotheses: the kernel's extra work alone) and the
boosted graph.  Reported: median, min and max of the ms per frame, and the two kernels' own times by device events on the same beam and logits.

--lm adds language-model fusion: a random two-layer ttmi.lm.TransformerLM of the label encoder's width, internal-LM
subtraction on, timed per beam width interleaved with the plain search, --repeats times each; and the device-event times of
ttmi_beam_step_ctx with the zero-weight graph beside ttmi_beam_step_fuse with 0, 1 and 2 sources on the same beam and logits, at W = 4 and 8.

    python tools/bench_beam.py [--utts 8] [--T 500] [--emit-rate 0.1] [--precision fp32] [--widths 1,4,8] [--context 100 [--boost 1.0] [--repeats 5]]
                               [--lm [--lm-weight 0.3] [--ilm-weight 0.1]]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "transformer-transducer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def draw_phrases(hyps, n, seed=0):
    """n phrases of 2 to 4 tokens cut from the hypotheses (token lists) at seeded random places"""
    rng = random.Random(seed)
    pool = [list(h) for h in hyps if len(h) >= 2]
    if not pool:
        raise SystemExit("--context: no hypothesis with two tokens to draw phrases from")
    out = []
    for _ in range(n):
        h = rng.choice(pool)
        length = rng.randint(2, min(4, len(h)))
        start = rng.randrange(len(h) - length + 1)
        out.append([int(k) for k in h[start:start + length]])
    return out


def kernel_times(W, V, B, graphs, frames=20, reps=50):
    """device-event time of one ttmi_beam_step / ttmi_beam_step_ctx call, us, on a beam that `frames` steps on random logits have filled:
    every kernel reads the same beam and the same logits, `reps` calls each, interleaved in rounds of 10"""
    from ttmi import ops
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ld_hist, ld_det = frames + 3, frames + 2

    def beam():
        return (torch.full((B, W), -float("inf"), dtype=torch.float64, device=dev), torch.zeros(B, W, dtype=torch.int32, device=dev),
                torch.zeros(B, W, ld_hist, dtype=torch.long, device=dev), torch.zeros(B, W, ld_det, dtype=torch.int32, device=dev),
                torch.zeros(B, W, ld_det, dtype=torch.float32, device=dev))

    def ctx():
        return torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev)
    cur, nxt, cur_x, nxt_x = beam(), beam(), ctx(), ctx()
    cur[0][:, 0] = 0.0
    t = torch.zeros(B, dtype=torch.int32, device=dev)
    T_len = torch.full((B,), frames + 1, dtype=torch.int32, device=dev)
    parent, fresh = torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.int32, device=dev)
    ws = ops.beam_ctx_workspace(B, W, V, dev)
    zero = graphs["zero_weight"]
    for _ in range(frames):                                              # fill the beam; the zero-weight graph keeps the states current
        logits = 3.0 * torch.randn(B, W, V, device=dev, generator=gen)
        ops.beam_step_ctx(logits, t, T_len, cur, nxt, parent, fresh, zero.tables, cur_x, nxt_x, ws)
        t += 1
        cur, nxt, cur_x, nxt_x = nxt, cur, nxt_x, cur_x
    logits = 3.0 * torch.randn(B, W, V, device=dev, generator=gen)
    calls = {"no_context": lambda: ops.beam_step(logits, t, T_len, cur, nxt, parent, fresh)}
    for name, g in graphs.items():
        calls[name] = lambda g=g: ops.beam_step_ctx(logits, t, T_len, cur, nxt, parent, fresh, g.tables, cur_x, nxt_x, ws)
    times = {name: [] for name in calls}
    for fn in calls.values():
        fn()
    for _ in range(reps // 10):
        for name, fn in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
            ev[0].record()
            for i in range(10):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[name] += [1e3 * a.elapsed_time(b) for a, b in zip(ev, ev[1:])]
    return {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for name, v in times.items()}


def fuse_kernel_times(W, V, B, zero, frames=20, rounds=10):
    """device-event time, us, of ttmi_beam_step_ctx with the zero-weight graph and of ttmi_beam_step_fuse with 0, 1 and 2 f32 sources (norm 1
    and norm 2, as the fused search passes them) on the same beam, logits and graph: `rounds` interleaved rounds of 10 calls each.  Per
    configuration the median and minimum over all calls and the spread of the rounds' medians; the zero-source call is held against the
    spread of the ctx kernel's rounds"""
    from ttmi import ops
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ld_hist, ld_det = frames + 3, frames + 2

    def beam():
        return (torch.full((B, W), -float("inf"), dtype=torch.float64, device=dev), torch.zeros(B, W, dtype=torch.int32, device=dev),
                torch.zeros(B, W, ld_hist, dtype=torch.long, device=dev), torch.zeros(B, W, ld_det, dtype=torch.int32, device=dev),
                torch.zeros(B, W, ld_det, dtype=torch.float32, device=dev))

    def ctx():
        return torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev)
    cur, nxt, cur_x, nxt_x = beam(), beam(), ctx(), ctx()
    cur[0][:, 0] = 0.0
    t = torch.zeros(B, dtype=torch.int32, device=dev)
    T_len = torch.full((B,), frames + 1, dtype=torch.int32, device=dev)
    parent, fresh = torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.int32, device=dev)
    ws = ops.beam_fuse_workspace(B, W, V, dev)
    fuse_in, fuse_out = torch.zeros(B, W, dtype=torch.float64, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev)
    for _ in range(frames):
        logits = 3.0 * torch.randn(B, W, V, device=dev, generator=gen)
        ops.beam_step_ctx(logits, t, T_len, cur, nxt, parent, fresh, zero.tables, cur_x, nxt_x, ws)
        t += 1
        cur, nxt, cur_x, nxt_x = nxt, cur, nxt_x, cur_x
    logits = 3.0 * torch.randn(B, W, V, device=dev, generator=gen)
    lm_rows = 2.0 * torch.randn(B, W, V, device=dev, generator=gen)
    ilm_rows = 2.0 * torch.randn(B, W, V, device=dev, generator=gen)
    srcs = {"fuse_0_sources": (), "fuse_1_source": ((lm_rows, 0.3, 1),), "fuse_2_sources": ((lm_rows, 0.3, 1), (ilm_rows, -0.1, 2))}
    calls = {"ctx_zero_weight": lambda: ops.beam_step_ctx(logits, t, T_len, cur, nxt, parent, fresh, zero.tables, cur_x, nxt_x, ws)}
    for name, src in srcs.items():
        calls[name] = lambda src=src: ops.beam_step_fuse(logits, t, T_len, cur, nxt, parent, fresh, zero.tables, cur_x, nxt_x, ws, fuse_in,
                                                         fuse_out, sources=src)
    times = {name: [] for name in calls}
    for fn in calls.values():
        fn()
    for _ in range(rounds):
        for name, fn in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
            ev[0].record()
            for i in range(10):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[name].append([1e3 * a.elapsed_time(b) for a, b in zip(ev, ev[1:])])
    out = {}
    for name, v in times.items():
        meds = [statistics.median(r) for r in v]
        out[name] = {"median_us": round(statistics.median(sum(v, [])), 2), "min_us": round(min(sum(v, [])), 2),
                     "round_median_min_us": round(min(meds), 2), "round_median_max_us": round(max(meds), 2)}
    out["zero_source_within_ctx_spread"] = out["fuse_0_sources"]["median_us"] <= out["ctx_zero_weight"]["round_median_max_us"]
    for name in ("fuse_1_source", "fuse_2_sources"):
        out[name]["over_zero_sources_us"] = round(out[name]["median_us"] - out["fuse_0_sources"]["median_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--emit-rate", type=float, default=0.1)
    ap.add_argument("--precision", default="fp32", choices=["bf16", "fp32"])
    ap.add_argument("--widths", default="1,4,8")
    ap.add_argument("--context", type=int, default=0, help="number of hotword phrases drawn from the run's own hypotheses (0: no biasing runs)")
    ap.add_argument("--boost", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lm", action="store_true", help="language-model fusion: a random two-layer TransformerLM, internal-LM subtraction on")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--ilm-weight", type=float, default=0.1)
    a = ap.parse_args()
    import bench_decode
    base, model, inputs, lens, hyps = bench_decode.run(a.utts, a.T, a.emit_rate, a.precision)       # builds the model, sets the blank bias, warms up
    with torch.no_grad():
        enc_states, t_enc = timed(lambda: model.encoder(inputs, None))
        _, t_greedy = timed(lambda: model.decode_batch(enc_states, lens))
        model.decode_batch(enc_states, lens, details=True)
        greedy, t_details = timed(lambda: model.decode_batch(enc_states, lens, details=True))
        out = {"workload": base["workload"].replace("greedy decode", "beam decode"), "encoder_ms": round(1e3 * t_enc, 2),
               "decode_batch": {"utt_per_s": round(a.utts / (t_enc + t_greedy), 3), "decode_ms_per_utt": round(1e3 * t_greedy / a.utts, 2)},
               "decode_batch_details": {"utt_per_s": round(a.utts / (t_enc + t_details), 3), "decode_ms_per_utt": round(1e3 * t_details / a.utts, 2)},
               "symbols_per_utt": round(sum(len(h) for h in hyps) / a.utts, 1), "beam": {}}
        calls = [0]
        decoder_forward = model.decoder.forward
        model.decoder.forward = lambda *x, **k: (calls.__setitem__(0, calls[0] + 1), decoder_forward(*x, **k))[1]
        for W in [int(w) for w in a.widths.split(",")]:
            model.beam_decode_batch(enc_states, lens, beam_width=W)                                 # warm-up: first launches at this width
            calls[0] = 0
            res, t_beam = timed(lambda: model.beam_decode_batch(enc_states, lens, beam_width=W))
            out["beam"][str(W)] = {"utt_per_s": round(a.utts / (t_enc + t_beam), 3), "decode_ms_per_utt": round(1e3 * t_beam / a.utts, 2),
                                   "ms_per_frame": round(1e3 * t_beam / max(lens), 3), "label_encoder_calls_per_frame": round(calls[0] / max(lens), 2),
                                   "best_equals_greedy_tokens": sum(r[0].tokens == g.tokens for r, g in zip(res, greedy)),
                                   "mean_best_score_per_frame": round(sum(r[0].score for r in res) / sum(lens), 4),
                                   "mean_greedy_score_per_frame": round(sum(g.score for g in greedy) / sum(lens), 4)}
        model.decoder.forward = decoder_forward
        if a.context > 0:
            from ttmi.context import ContextGraph
            V = model.config.vocab_size
            phrases = draw_phrases(hyps, a.context)
            boosted = ContextGraph(phrases, boost=a.boost).validate(V).to(enc_states.device)
            arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w = boosted.cpu_tables()
            zero = ContextGraph.from_tables(arc_off, arc_sym, arc_next, torch.zeros_like(arc_w), fail, torch.zeros_like(fail_w),
                                            torch.zeros_like(final_w)).validate(V).to(enc_states.device)
            configs = {"no_context": None, "zero_weight": zero, "boosted": boosted}
            out["context"] = {"phrases": len(phrases), "states": boosted.S, "arcs": boosted.A, "boost": a.boost, "repeats": a.repeats, "widths": {}}
            for W in [int(w) for w in a.widths.split(",")]:
                res, times = {}, {name: [] for name in configs}
                for name, g in configs.items():                                                     # warm-up of every configuration
                    model.beam_decode_batch(enc_states, lens, beam_width=W, context=g)
                for _ in range(a.repeats):
                    for name, g in configs.items():
                        res[name], dt = timed(lambda: model.beam_decode_batch(enc_states, lens, beam_width=W, context=g, return_bias=True))
                        times[name].append(1e3 * dt / max(lens))
                row = {name: {"ms_per_frame_median": round(statistics.median(v), 4), "ms_per_frame_min": round(min(v), 4),
                              "ms_per_frame_max": round(max(v), 4)} for name, v in times.items()}
                row["zero_weight_over_no_context"] = round(statistics.median(times["zero_weight"]) / statistics.median(times["no_context"]), 4)
                row["zero_weight_equals_no_context"] = res["zero_weight"][0] == res["no_context"][0]
                row["boosted_best_differs_in"] = sum(x[0].tokens != y[0].tokens for x, y in zip(res["boosted"][0], res["no_context"][0]))
                row["boosted_mean_best_bias"] = round(sum(u[0] for u in res["boosted"][1]) / a.utts, 2)
                row["kernel_us"] = kernel_times(W, V, a.utts, {"zero_weight": zero, "boosted": boosted})
                out["context"]["widths"][str(W)] = row
        if a.lm:
            from ttmi.context import ContextGraph
            from ttmi.lm import TransformerLM
            V, dec = model.config.vocab_size, model.config.dec
            torch.manual_seed(1)
            lm = TransformerLM(dict(vocab_size=V, n_layer=2, d_model=dec.d_model, n_head=dec.n_head, d_head=dec.d_head, d_inner=dec.d_inner,
                                    max_target_length=dec.max_target_length, dropout=0.0)).to(enc_states.device).eval()
            arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w = ContextGraph(draw_phrases(hyps, a.context or 100)).cpu_tables()
            zero = ContextGraph.from_tables(arc_off, arc_sym, arc_next, torch.zeros_like(arc_w), fail, torch.zeros_like(fail_w),
                                            torch.zeros_like(final_w)).validate(V).to(enc_states.device)
            # "weightless": both sources present at weights that leave every key as it was (0 and 1e-300), so the fused machinery - the
            # kernel's extra reads, the LM's and the internal LM's calls, the gathers - runs on exactly the hypotheses of the plain search
            configs = {"no_lm": {}, "weightless": dict(lm=lm, lm_weight=0.0, ilm_weight=1e-300),
                       "lm_and_ilm": dict(lm=lm, lm_weight=a.lm_weight, ilm_weight=a.ilm_weight)}
            out["lm"] = {"lm_weight": a.lm_weight, "ilm_weight": a.ilm_weight, "lm_layers": 2, "repeats": a.repeats, "widths": {}, "kernel_us": {}}
            for W in [int(w) for w in a.widths.split(",")]:
                res, times = {}, {name: [] for name in configs}
                for kw in configs.values():                                                         # warm-up of every configuration
                    model.beam_decode_batch(enc_states, lens, beam_width=W, **kw)
                for _ in range(a.repeats):
                    for name, kw in configs.items():
                        res[name], dt = timed(lambda: model.beam_decode_batch(enc_states, lens, beam_width=W, return_lm=True, **kw))
                        times[name].append(1e3 * dt / max(lens))
                row = {name: {"ms_per_frame_median": round(statistics.median(v), 4), "ms_per_frame_min": round(min(v), 4),
                              "ms_per_frame_max": round(max(v), 4)} for name, v in times.items()}
                row["weightless_over_no_lm"] = round(statistics.median(times["weightless"]) / statistics.median(times["no_lm"]), 4)
                row["weightless_equals_no_lm"] = res["weightless"][0] == res["no_lm"][0]
                row["mean_best_tokens"] = {name: round(sum(len(u[0].tokens) for u in res[name][0]) / a.utts, 1) for name in configs}
                row["fused_best_differs_in"] = sum(x[0].tokens != y[0].tokens for x, y in zip(res["lm_and_ilm"][0], res["no_lm"][0]))
                row["fused_mean_best_lm_total"] = round(sum(u[0] for u in res["lm_and_ilm"][1]) / a.utts, 2)
                out["lm"]["widths"][str(W)] = row
            for W in (4, 8):
                out["lm"]["kernel_us"][str(W)] = fuse_kernel_times(W, V, a.utts, zero)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
