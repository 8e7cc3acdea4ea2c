"""Token-and-duration transducer (TDT; Xu et al., ICML 2023, "Efficient Sequence Transduction by Jointly Predicting Tokens and Durations").

The joint predicts a token AND the number of frames that decision consumes: a row of logits is V token columns followed by
D = len(durations) duration columns, each sub-row normalised by itself.  Training is the forward-backward over a lattice whose moves jump
d frames (csrc/tdt.hip; the recursion is in include/ttmi.h); decoding jumps instead of scoring every frame
(`tt.model.Transducer.recognize` on a model built with `config.tdt_durations`).

Durations are distinct integers in [1, 8], at most 8, strictly increasing.  Duration 0 is refused: every decoder of this library consumes
the emitting frame.  With `durations=(1,)` the lattice is the monotonic one (`RNNTLoss(topology='monotonic')` on the token columns).  A
path lands exactly on the last frame: a move that would overshoot does not exist in the lattice, so an utterance whose length is not a sum
of durations (or that has more labels than frames) has no path - cost +inf, zero gradient.

Not built for TDT: the exp-domain form, FastEmit, alignment / emission statistics, distillation, MWER, beam search, streaming, the
paper's logit under-normalisation (sigma)."""
import collections
import os

import torch

from .ops import TDTLattice, check_durations

__all__ = ["check_durations", "tdt_loss", "TDTLoss", "TDTDecodeResult", "TDTLattice", "not_built"]


TDTDecodeResult = collections.namedtuple("TDTDecodeResult", ["tokens", "frames", "logprobs", "durations", "score"])
TDTDecodeResult.__doc__ = """What greedy decoding of a TDT model returns per utterance with details=True: `tokens` (list of int), `frames` (the frame
each token was emitted on, strictly increasing), `logprobs` (log P(token) of each, from the token sub-row), `durations` (the frames each
token's decision consumed) and `score`: the log-probability of every decision taken, blanks included, token and duration terms both - a
path of the TDT lattice when the last jump lands exactly on the utterance's end."""


def not_built(what):
    """the one error of every entry point a TDT model reaches and that is not built for it"""
    return ValueError("TDT: %s is not built for a token-and-duration model (config.tdt_durations); greedy decoding and the loss are" % what)


def tdt_loss(logits, labels, act_lens, label_lens, durations, blank=0, reduction="mean", check_lengths=None):
    """logits: f32 / bf16 [B, T, U+1, V + D] on the device (un-normalised; V token columns, then D duration columns), labels int32 [B, U],
    act_lens / label_lens int32 [B] -> the TDT loss under `reduction` ('mean' divides by the batch and returns shape [1], as RNNTLoss),
    with the gradient w.r.t. the logits.  check_lengths (default: on unless TTMI_CHECK_LENGTHS=0): the length checks of RNNTLoss, and an
    utterance with more labels than frames is a ValueError; with it off such an utterance costs +inf and has a zero gradient.  A
    DeferredLogits handle is materialised first."""
    import warprnnt_pytorch as wp
    lat = TDTLattice(durations)
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("reduction must be 'mean', 'sum' or 'none'")
    if check_lengths is None:
        check_lengths = os.environ.get("TTMI_CHECK_LENGTHS", "1") != "0"
    if not logits.is_cuda:
        raise ValueError("TDTLoss: logits must live on the GPU (the MI355X build has no CPU path)")
    labels, act_lens, label_lens = (t.to(logits.device) for t in (labels, act_lens, label_lens))
    wp._certify(logits, labels, act_lens, label_lens, check_lengths)
    if logits.shape[-1] <= len(lat.durations):
        raise ValueError("TDTLoss: the last dimension (%d) must hold the token columns and %d duration columns"
                         % (logits.shape[-1], len(lat.durations)))
    if not 0 <= int(blank) < logits.shape[-1] - len(lat.durations):
        raise ValueError("TDTLoss: blank %d outside the %d token columns" % (blank, logits.shape[-1] - len(lat.durations)))
    if check_lengths:
        try:
            wp.check_monotonic_lengths(act_lens, label_lens)
        except ValueError:
            raise ValueError("TDT: an utterance has more labels than frames (label_lengths > lengths)") from None
    materialize = getattr(logits, "materialize", None)
    if materialize is not None:
        logits = materialize()
    return wp._LatticeLossFn.apply(logits, labels, act_lens, label_lens, int(blank), reduction, 0.0, lat)


class TDTLoss(torch.nn.Module):
    """TDTLoss(durations, blank=0, reduction='mean')(logits, labels, act_lens, label_lens): `tdt_loss` as a criterion with RNNTLoss's call
    contract, on logits whose last D = len(durations) columns are the duration logits."""

    def __init__(self, durations, blank=0, reduction="mean", check_lengths=None):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.durations = check_durations(durations)
        self.blank, self.reduction, self.check_lengths = blank, reduction, check_lengths

    def forward(self, logits, labels, act_lens, label_lens):
        return tdt_loss(logits, labels, act_lens, label_lens, self.durations, self.blank, self.reduction, self.check_lengths)
