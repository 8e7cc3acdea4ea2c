#!/usr/bin/env python3
"""Frame-synchronous beam search (Transducer.beam_decode_batch) at tools/bench_decode.py's workload - the C2 model on synthetic utterances,
blank bias set for the emit rate - for beam widths 1, 4 and 8, beside greedy decode_batch (plain and details=True) measured in the same process
on the same encoder states.  Utterances/s include the encoder's time, as bench_decode.py's do.  One JSON line.

    python tools/bench_beam.py [--utts 8] [--T 500] [--emit-rate 0.1] [--precision fp32] [--widths 1,4,8]
"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--emit-rate", type=float, default=0.1)
    ap.add_argument("--precision", default="fp32", choices=["bf16", "fp32"])
    ap.add_argument("--widths", default="1,4,8")
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
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
