"""Numpy restatement of the stable prefix of a beam (include/ttmi.h, ttmi_beam_stable_prefix) and a driver that steps beam_oracle.step frame
by frame under either label-history rule of ttmi.beam.BeamSearch and records the stable count after every frame.  A helper, not a test
module (like beam_oracle.py).

stable_prefix()  the rule on one beam's arrays, as the kernel reads them; `defect` plants one of three mistakes (for the oracle's own tests)
fed_ids()        what the label encoder is fed for a hypothesis: history "full" = start symbol + tokens, "stream" = the start symbol alone
                 without tokens, else the last max_history tokens and no start symbol
to_arrays()      a beam of beam_oracle.Hyp -> (score, len, hist) arrays
drive()          a whole utterance -> (final beam, the stable count after every frame, the beam after every frame)"""
import math

import numpy as np

import beam_oracle as BO

DEFECTS = ("empty_live", "column_0", "first_len")


def stable_prefix(score, n_tok, hist, defect=None):
    """score f64 [B, W], n_tok int [B, W], hist int [B, W, ld_hist] (column 0 = the start symbol) -> int64 [B]: the largest n such that every
    live slot (score > -inf; NaN and -inf are empty) has at least n tokens and the same first n tokens as the first live slot; 0 without a
    live slot.  Lengths are clamped to [0, ld_hist - 1]."""
    score, n_tok, hist = np.asarray(score, dtype=np.float64), np.asarray(n_tok), np.asarray(hist)
    B, W = score.shape
    ld = hist.shape[2]
    assert defect in (None,) + DEFECTS
    out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        live = [w for w in range(W) if defect == "empty_live" or score[b, w] > -math.inf]
        if not live:
            continue
        lens = [min(max(int(n_tok[b, w]), 0), ld - 1) for w in live]
        if defect == "first_len":
            lens = [lens[0]] * len(lens)
        first = 0 if defect == "column_0" else 1
        n = 0
        while n < min(lens) and first + n < ld and all(hist[b, w, first + n] == hist[b, live[0], first + n] for w in live):
            n += 1
        out[b] = n
    return out


def fed_ids(tokens, history="full", max_history=40, start=0):
    tokens = tuple(tokens)
    if history == "full":
        return (start,) + tokens
    assert history == "stream"
    return tokens[-max_history:] if tokens else (start,)


def to_arrays(beam, W, ld_hist, fill=0):
    """one utterance's beam (Hyp or None per slot) -> score [1, W], len [1, W], hist [1, W, ld_hist] as ttmi_beam_step leaves them"""
    score = np.full((1, W), -math.inf)
    n_tok = np.zeros((1, W), dtype=np.int64)
    hist = np.full((1, W, ld_hist), fill, dtype=np.int64)
    for w, h in enumerate(beam):
        if h is None:
            continue
        score[0, w], n_tok[0, w] = h.score, len(h.tokens)
        hist[0, w, :len(h.tokens) + 1] = (0,) + tuple(h.tokens)
    return score, n_tok, hist


def drive(logits, b, T, W, history="full", max_history=40, blank=0):
    """logits(b, t, ids) -> the V logits of frame t of utterance b against the label state of the fed ids (fed_ids).  Steps beam_oracle.step
    over frames 0 .. T - 1 -> (final beam: W slots, Hyp or None; counts[t] = the stable prefix after frame t; beams[t] = the beam after it)"""
    beam = list(BO.START) + [None] * (W - 1)
    counts, beams = [], []
    for t in range(T):
        rows = [logits(b, t, fed_ids(h.tokens, history, max_history)) if h is not None else None for h in beam]
        beam = BO.step(beam, rows, t, W, blank)[0]
        counts.append(int(stable_prefix(*to_arrays(beam, W, T + 2))[0]))
        beams.append(beam)
    return beam, counts, beams
