"""The frame-synchronous beam search as an object that can be resumed: Transducer.beam_search_state() -> BeamSearch.

Transducer.beam_decode_batch needs the encoder states of the whole utterance before its first frame is searched.  BeamSearch holds what
that loop keeps in locals - the two beams (score / len / hist / frames / tok_lp), parent / fresh, the [B, W, d] table of label states, the
automaton's state and bias, the fuse accumulator with the LM's and the internal LM's row tables, the per-utterance clock - so the frames can
come in blocks: advance(block) as often as there is audio, stable() / partial() in between, finish() once.  Per frame the calls are the
one-shot loop's: one joint call, one beam-step kernel of the same flavour (ttmi_beam_step / _ctx / _fuse), one host read, the label encoder
and the LM on fresh slots only.  What follows a frame - the host read, the gathers by `parent`, the new label states and LM rows - is done
lazily, before the next frame that reads it (or in finish(), for the LM's closing term), so a search that ends computes nothing the one-shot
loop would not have computed; a block split anywhere gives the bits of the unsplit run.

The total number of frames is unknown: the history and detail buffers start at `capacity` columns and grow (reallocate and copy, at least
doubling) before a block that could break the kernels' requirement ld_hist >= largest len + 2, ld_det >= largest len + 1.  Nothing the
kernels compute depends on the pitch.

history = "full": the label state of a hypothesis is decoder([start] + tokens)[:, -1] (beam_decode_batch's rule).  history = "stream": the
streaming recogniser's rule (ttmi.streaming): decoder([[start]]) without tokens, else decoder(tokens[-max_history:])[:, -1], no leading start
symbol; fresh slots are grouped by the length actually fed.  The internal-LM rows follow the label state; the external LM always sees the
full history.

stable(): how many leading tokens every live hypothesis shares (ttmi_beam_stable_prefix, include/ttmi.h has the rule and why such a prefix
can no longer change) - one launch and one host read per call.
"""
import math

import torch
import torch.nn as nn

from . import ops


class BeamSearch:
    def __init__(self, model, B, beam_width=4, context=None, lm=None, lm_weight=0.0, ilm_weight=0.0, length_bonus=0.0, history="full",
                 max_history=40, capacity=None):
        if getattr(model, "tdt_durations", None) is not None:
            from .tdt import not_built
            raise not_built("resumable beam search (BeamSearch)")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise ValueError("beam_search_state: the model must live on the GPU (the MI355X build has no CPU path)")
        W, B = int(beam_width), int(B)
        if not 1 <= W <= 32 or B < 1:
            raise ValueError("beam_search_state: beam_width must be in [1, 32] and B >= 1, got %r and %r" % (beam_width, B))
        if history not in ("full", "stream") or int(max_history) < 1:
            raise ValueError("beam_search_state: history is 'full' or 'stream' and max_history >= 1, got %r and %r" % (history, max_history))
        for name, v in (("lm_weight", lm_weight), ("ilm_weight", ilm_weight), ("length_bonus", length_bonus)):
            if not math.isfinite(float(v)) or (name != "length_bonus" and float(v) < 0.0):
                raise ValueError("beam_search_state: %s must be finite%s, got %r" % (name, "" if name == "length_bonus" else " and >= 0", v))
        capacity = 64 if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError("beam_search_state: capacity must be >= 1, got %r" % (capacity,))
        self.model, self.dev, self.B, self.W, self.V = model, dev, B, W, model.config.vocab_size
        self.context, self.lm = context, lm
        self.lm_weight, self.ilm_weight, self.length_bonus = float(lm_weight), float(ilm_weight), float(length_bonus)
        self.history, self.max_history = history, int(max_history)
        self.fused = lm is not None or self.ilm_weight != 0.0 or self.length_bonus != 0.0
        if lm is not None:
            if lm.norm not in ops.BEAM_FUSE_NORMS:
                raise ValueError("beam_search_state: lm.norm must be one of %s, got %r" % (sorted(ops.BEAM_FUSE_NORMS), lm.norm))
            if isinstance(lm, nn.Module) and any(not p.is_cuda for p in lm.parameters()):
                raise ValueError("beam_search_state: the language model must live on the GPU (the MI355X build has no CPU path)")
        self.need_eos = lm is not None and lm.eos is not None
        self.cap = capacity                                          # ld_det; ld_hist = cap + 1 (column 0 = the start symbol)
        self.clock = [0] * B                                         # frames consumed per utterance
        self.t = torch.zeros(B, dtype=torch.int32, device=dev)
        self.cur, self.nxt = self._beam(), self._beam()
        self.cur["score"][:, 0] = 0.0                                # slot 0 holds the start symbol, the other slots are empty
        with torch.no_grad():
            self._setup()
        self.pending = False                                         # a frame was stepped and what follows it is still to do
        self.was_active = [False] * B                                # ... for these utterances
        self.stale_state = [[False] * W for _ in range(B)]           # slots whose label state (and internal-LM row) is not computed yet
        self.stale_lm = [[False] * W for _ in range(B)]              # ... whose LM row is not
        self.n_tok = [[0] * W for _ in range(B)]                     # the lengths the last host read brought
        self.stable_count = [0] * B
        self.finished = False

    def _beam(self):
        """score, (len | fresh) packed for the one host read, histories, emission frames, token log-probabilities"""
        B, W, dev = self.B, self.W, self.dev
        return dict(score=torch.full((B, W), -math.inf, dtype=torch.float64, device=dev), meta=torch.zeros(2, B, W, dtype=torch.int32, device=dev),
                    hist=torch.zeros(B, W, self.cap + 1, dtype=torch.long, device=dev), frames=torch.zeros(B, W, self.cap, dtype=torch.int32, device=dev),
                    tok_lp=torch.zeros(B, W, self.cap, dtype=torch.float32, device=dev))

    @staticmethod
    def _arrays(bm):
        return bm["score"], bm["meta"][0], bm["hist"], bm["frames"], bm["tok_lp"]

    def _setup(self):
        model, context, lm, dev, B, W, V = self.model, self.context, self.lm, self.dev, self.B, self.W, self.V
        cur, nxt = self.cur, self.nxt
        if context is not None:
            context.validate(V).to(dev)
            for bm in (cur, nxt):
                bm["ctx"] = (torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev))
            self.ctx_ws = ops.beam_ctx_workspace(B, W, V, dev)
            if context.start:                                        # (an n-gram automaton starts in its <s> context)
                cur["ctx"][0][:, 0] = int(context.start)
        self.parent = torch.zeros(B, W, dtype=torch.int32, device=dev)
        start = model.decoder(torch.zeros(1, 1, dtype=torch.long, device=dev))[:, -1, :]
        self.states = start[None].expand(B, W, -1).contiguous()      # [B, W, d]; what an empty slot holds is never read by the kernel
        self.d = self.states.shape[-1]
        self.lm_rows = self.ilm_rows = None
        if self.fused:
            if context is None:                                      # the trivial automaton: the root alone, every weight 0
                self.tables = tuple(torch.zeros(n, dtype=dt, device=dev) for n, dt in ((2, torch.int32), (0, torch.int32), (0, torch.int32),
                                                                                        (0, torch.float32), (1, torch.int32), (1, torch.float32)))
                for bm in (cur, nxt):
                    bm["ctx"] = (torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.float64, device=dev))
            else:
                self.tables = context.tables
            for bm in (cur, nxt):
                bm["fuse"] = torch.zeros(B, W, dtype=torch.float64, device=dev)
            self.fuse_ws = ops.beam_fuse_workspace(B, W, V, dev)
            self.zero_enc = None                                     # made on the first block: it takes the encoder states' dtype
            if lm is not None:
                self.lm_rows = self._lm_scores(torch.zeros(1, 1, dtype=torch.long, device=dev))[None].expand(B, W, -1).contiguous()
            self.start_state = start

    def _lm_scores(self, hist):
        rows = self.lm.next_logits(hist)
        if not rows.is_cuda or rows.dim() != 2 or rows.shape[1] != self.V or rows.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("beam search: lm.next_logits must return [N, %d] f32 or bf16 rows on the GPU" % self.V)
        return rows

    def _ilm_scores(self, st):
        """the joint without an encoder: the label encoder's own prior (internal LM), [N, d] -> [N, V]"""
        return self.model.joint(self.zero_enc, st[None].contiguous())[0, 0]

    def _grow(self, need):
        """make room for histories of `need` - 1 symbols and one more (the kernels' requirement, with the one-shot loop's slack)"""
        if need <= self.cap:
            return
        old, self.cap = self.cap, max(2 * self.cap, need)
        for bm in (self.cur, self.nxt):
            for name, cols in (("hist", old + 1), ("frames", old), ("tok_lp", old)):
                was = bm[name]
                bm[name] = torch.zeros(self.B, self.W, self.cap + cols - old, dtype=was.dtype, device=self.dev)
                bm[name][:, :, :cols] = was

    def _refresh(self, active):
        """what follows the last frame stepped, for the frame to come (active[b]: utterance b takes part in it; all False: finish()): the frame's
        one host read, the gathers by `parent`, label states / internal-LM rows of the fresh slots of the active utterances and LM rows of
        those, and - where the LM has a closing term, which needs the row of every final slot - of the utterances that sit the frame out too;
        one label-encoder call per distinct length fed, one LM call per distinct history length"""
        B, W, V, d, dev, cur = self.B, self.W, self.V, self.d, self.dev, self.cur
        closing = not any(active)
        if self.pending:
            if closing and not self.need_eos:
                return
            n_tok, fresh = cur["meta"].cpu().tolist()                                             # the frame's one host round trip
            gather = self.parent.long()[:, :, None]
            if not closing:
                self.states = self.states.gather(1, gather.expand(-1, -1, d))                     # a slot that keeps its tokens keeps its label state
                if self.ilm_rows is not None:
                    self.ilm_rows = self.ilm_rows.gather(1, gather.expand(-1, -1, V))
            if self.lm_rows is not None:
                self.lm_rows = self.lm_rows.gather(1, gather.expand(-1, -1, V))
            for b in range(B):                                       # (an utterance that sat the frame out was copied through: nothing of it moved)
                if self.was_active[b]:
                    self.n_tok[b] = n_tok[b]
                    self.stale_state[b] = [bool(v) for v in fresh[b]]
                    self.stale_lm[b] = [bool(v) for v in fresh[b]] if self.lm_rows is not None else [False] * W
            self.pending = False
        by_fed, lm_first, lm_rest = {}, {}, {}                       # length fed -> [(row, first column)]; history length -> rows
        for b in range(B):
            if not active[b] and not self.need_eos:
                continue
            for w in range(W):
                n = self.n_tok[b][w]
                if active[b] and self.stale_state[b][w]:
                    if self.history == "full":
                        by_fed.setdefault(n + 1, []).append((b * W + w, 0))
                    else:
                        fed = min(n, self.max_history)
                        by_fed.setdefault(fed, []).append((b * W + w, n + 1 - fed))
                    self.stale_state[b][w] = False
                if self.stale_lm[b][w]:
                    (lm_first if active[b] else lm_rest).setdefault(n, []).append(b * W + w)
                    self.stale_lm[b][w] = False
        hist2d = cur["hist"].view(B * W, self.cap + 1)
        for fed in sorted(by_fed):
            rows = torch.tensor([r for r, _ in by_fed[fed]], dtype=torch.long, device=dev)
            first = {c for _, c in by_fed[fed]}
            if len(first) == 1:
                c = first.pop()
                hist = hist2d[rows, c:c + fed].contiguous()
            else:                                                    # (history = "stream" past max_history: windows that start at different columns)
                cols = torch.tensor([c for _, c in by_fed[fed]], dtype=torch.long, device=dev)[:, None] + torch.arange(fed, device=dev)[None]
                hist = hist2d[rows[:, None], cols].contiguous()
            st = self.model.decoder(hist)[:, -1, :]
            self.states.view(B * W, d).index_copy_(0, rows, st)
            if self.ilm_rows is not None:
                self.ilm_rows.view(B * W, V).index_copy_(0, rows, self._ilm_scores(st).to(self.ilm_rows.dtype))
        for n in sorted(set(lm_first) | set(lm_rest)):               # one LM call per history length, the active utterances' rows first
            rows = torch.tensor(lm_first.get(n, []) + lm_rest.get(n, []), dtype=torch.long, device=dev)
            hist = hist2d[rows, :n + 1].contiguous()
            self.lm_rows.view(B * W, V).index_copy_(0, rows, self._lm_scores(hist).to(self.lm_rows.dtype))

    @torch.no_grad()
    def advance(self, enc_frames, n_valid=None):
        """enc_frames [B, n, d] on the GPU: the next n encoder frames of every utterance; n_valid int [B] (default n for all): utterance b
        consumes frames 0 .. n_valid[b] - 1 of the block and its clock moves on by n_valid[b].  Within the block an utterance past its
        n_valid is finished to the kernel and copied through; a later advance takes it up again.  n = 0 does nothing."""
        if self.finished:
            raise RuntimeError("BeamSearch.advance: the search was finished")
        if not enc_frames.is_cuda:
            raise ValueError("BeamSearch.advance: enc_frames must live on the GPU (the MI355X build has no CPU path)")
        if enc_frames.dim() != 3 or enc_frames.shape[0] != self.B:
            raise ValueError("BeamSearch.advance: enc_frames is [%d, n, d], got %s" % (self.B, tuple(enc_frames.shape)))
        B, n = self.B, enc_frames.shape[1]
        nv = [n] * B if n_valid is None else [int(v) for v in torch.as_tensor(n_valid).tolist()]
        if len(nv) != B or any(not 0 <= v <= n for v in nv):
            raise ValueError("BeamSearch.advance: n_valid holds %d counts in [0, %d], got %r" % (B, n, nv))
        steps = max(nv + [0])
        if steps == 0:
            return
        ends = [c + v for c, v in zip(self.clock, nv)]
        self._grow(max(ends) + 1)                                    # at most one symbol per frame
        T_len = torch.tensor(ends, dtype=torch.int32, device=self.dev)
        if self.fused and self.zero_enc is None:
            self.zero_enc = torch.zeros(1, 1, enc_frames.shape[-1], dtype=enc_frames.dtype, device=self.dev)
            if self.ilm_weight != 0.0:
                self.ilm_rows = self._ilm_scores(self.start_state)[None].expand(B, self.W, -1).contiguous()
        lm, context = self.lm, self.context
        for j in range(steps):
            active = [j < v for v in nv]
            self._refresh(active)
            cur, nxt = self.cur, self.nxt
            logits = self.model.joint(enc_frames[:, j:j + 1].contiguous(), self.states)           # [B, 1, W, V]
            if self.fused:
                ops.beam_step_fuse(logits[:, 0], self.t, T_len, self._arrays(cur), self._arrays(nxt), self.parent, nxt["meta"][1], self.tables,
                                   cur["ctx"], nxt["ctx"], self.fuse_ws, cur["fuse"], nxt["fuse"],
                                   sources=(None if lm is None else (self.lm_rows, self.lm_weight, ops.BEAM_FUSE_NORMS[lm.norm]),
                                            None if self.ilm_rows is None else (self.ilm_rows, -self.ilm_weight, 2)),
                                   sym_bonus=self.length_bonus, blank=0)
            elif context is None:
                ops.beam_step(logits[:, 0], self.t, T_len, self._arrays(cur), self._arrays(nxt), self.parent, nxt["meta"][1], blank=0)
            else:
                ops.beam_step_ctx(logits[:, 0], self.t, T_len, self._arrays(cur), self._arrays(nxt), self.parent, nxt["meta"][1], context.tables,
                                  cur["ctx"], nxt["ctx"], self.ctx_ws, blank=0)
            self.t += 1
            self.cur, self.nxt = nxt, cur
            self.pending, self.was_active = True, active
        self.clock = ends
        if any(v != steps for v in nv):                              # the device clock ran on for the utterances that sat frames out
            self.t.copy_(T_len)

    @torch.no_grad()
    def stable(self):
        """per utterance, how many leading tokens every live hypothesis shares (they can no longer change); the count never decreases (a beam
        without a live slot, which reports 0, keeps what it had)"""
        cur = self.cur
        got = ops.beam_stable_prefix(cur["score"], cur["meta"][0], cur["hist"]).tolist()
        self.stable_count = [max(a, int(b)) for a, b in zip(self.stable_count, got)]
        return list(self.stable_count)

    @torch.no_grad()
    def partial(self):
        """per utterance the DecodeResult of the currently best slot under the running key (slot 0: the kernels order the slots by it); no
        final bias, no eos term.  An utterance without a live slot gives an empty result with score -inf."""
        from tt.model import DecodeResult
        cur, c = self.cur, self.cap
        packed = torch.cat([cur["score"][:, :1], cur["meta"][0][:, :1].double(), cur["hist"][:, 0, 1:].double(), cur["frames"][:, 0].double(),
                            cur["tok_lp"][:, 0].double()], dim=1).cpu()
        out = []
        for b in range(self.B):
            score, n = float(packed[b, 0]), int(packed[b, 1])
            if not score > -math.inf:
                out.append(DecodeResult([], [], [], -math.inf))
                continue
            tok, frm, lpr = (packed[b, 2 + i * c:2 + i * c + n].tolist() for i in range(3))
            out.append(DecodeResult([int(v) for v in tok], [int(v) for v in frm], lpr, score))
        return out

    @torch.no_grad()
    def finish(self, nbest=None, return_bias=False, return_lm=False):
        """what Transducer.beam_decode_batch returns for the frames advanced so far: the final bias, the LM's eos term, the ordering, the cut to
        `nbest` and the RuntimeError for an utterance without a finite score.  The object takes no frames afterwards."""
        from tt.model import DecodeResult
        if self.finished:
            raise RuntimeError("BeamSearch.finish: the search was finished")
        W, B, context, fused, ld_det = self.W, self.B, self.context, self.fused, self.cap
        nbest = W if nbest is None else int(nbest)
        if nbest < 1:
            raise ValueError("BeamSearch.finish: nbest must be >= 1, got %r" % (nbest,))
        self._refresh([False] * B)
        self.finished = True
        cur = self.cur
        # ONE transfer, as f64 (exact for token ids, counts, frames and f32 log-probabilities): score | len | tokens | frames | logprobs
        packed = torch.cat([cur["score"][:, :, None], cur["meta"][0].double()[:, :, None], cur["hist"][:, :, 1:].double(), cur["frames"].double(),
                            cur["tok_lp"].double()] +
                           ([] if context is None else [(cur["ctx"][1] + context.final_w[cur["ctx"][0].long()].double())[:, :, None]]), dim=2)
        if fused:
            from .lm import eos_logprob
            lm_total = cur["fuse"] + self.lm_weight * eos_logprob(self.lm_rows, self.lm.norm, self.lm.eos) if self.need_eos else cur["fuse"]
            packed = torch.cat([packed, lm_total[:, :, None]], dim=2)
        packed = packed.cpu()
        bias_col = -1 - int(fused)
        out, biases, lms = [], [], []
        for b in range(B):
            res, bias, lmt = [], [], []
            for w in range(W):
                score, c = float(packed[b, w, 0]), int(packed[b, w, 1])
                if not score > -math.inf:                            # an empty slot
                    continue
                tok, frm, lpr = (packed[b, w, 2 + i * ld_det:2 + i * ld_det + c].tolist() for i in range(3))
                res.append(DecodeResult([int(v) for v in tok], [int(v) for v in frm], lpr, score))
                bias.append(0.0 if context is None else float(packed[b, w, bias_col]))
                lmt.append(float(packed[b, w, -1]) if fused else 0.0)
            if fused:                                                # the final bias reorders, and so does the LM's closing term
                order = sorted(range(len(res)), key=lambda n: (-(res[n].score + bias[n] + lmt[n]), n))
                res, bias, lmt = [res[n] for n in order], [bias[n] for n in order], [lmt[n] for n in order]
            elif context is not None:                                # the slots are in key order with the running bias; the final bias reorders
                order = sorted(range(len(res)), key=lambda n: (-(res[n].score + bias[n]), n))
                res, bias = [res[n] for n in order], [bias[n] for n in order]
            if not res or not math.isfinite(res[0].score):
                raise RuntimeError("beam search: utterance %d has no hypothesis with a finite score (NaN logits?)" % b)
            out.append(res[:nbest])
            biases.append(bias[:nbest])
            lms.append(lmt[:nbest])
        ret = (out,) + ((biases,) if return_bias else ()) + ((lms,) if return_lm else ())
        return ret if len(ret) > 1 else out
