"""Language models for the fused beam search (Transducer.beam_decode_batch(lm=...), include/ttmi.h: ttmi_beam_step_fuse).

The scorer protocol: any object with
    next_logits(hist)   hist i64 [N, n + 1] on the device, column 0 the start symbol 0 -> [N, V] f32 or bf16 rows with last stride 1: the
                        scores of every next symbol after each history
    norm                "logprob" (the rows are log-probabilities), "softmax" (logits, normalised over all V entries by the kernel) or
                        "softmax_no_blank" (logits, normalised without the blank)
    eos                 the token whose probability closes a hypothesis after the last frame, or None

TransformerLM(config)      a small Transformer LM on the project's own label-encoder stack
NGramLM.from_arpa(...)     a back-off n-gram model compiled into the automaton ttmi_beam_step_ctx already walks: pass it as context="""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .context import ContextGraph
from .ops import MaskSpec


class TransformerLM(nn.Module):
    """tt.decoder.BuildDecoder on an LM config (vocab_size, n_layer, d_model, n_head, d_head, d_inner, max_target_length, dropout) plus a
    linear head.  Token 0 is both the start and the end symbol, as in the label encoder."""
    norm = "softmax"
    eos = 0

    def __init__(self, config):
        super().__init__()
        from tt.decoder import BuildDecoder
        from tt.utils import AttrDict
        get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
        self.vocab_size, self.max_target_length = int(get("vocab_size")), int(get("max_target_length"))
        self.decoder = BuildDecoder(AttrDict(dict(vocab_size=self.vocab_size, dropout=float(get("dropout")),
                                                  dec=dict(n_layer=int(get("n_layer")), d_model=int(get("d_model")), n_head=int(get("n_head")),
                                                           d_head=int(get("d_head")), d_inner=int(get("d_inner")),
                                                           max_target_length=self.max_target_length))))
        self.head = nn.Linear(int(get("d_model")), self.vocab_size)

    def forward(self, tokens):
        """tokens i64 [B, U], column 0 the start symbol -> [B, U, V] logits of the next symbol at every position (causal mask)"""
        return self.head(self.decoder(tokens, MaskSpec(1)).float())

    def loss(self, tokens, lengths):
        """tokens i64 [B, U] (the symbols, no start symbol; padding beyond lengths[b] is ignored), lengths [B] -> the mean next-token cross
        entropy over every symbol and the closing 0 of every sequence"""
        B, U = tokens.shape
        lengths = torch.as_tensor(lengths, device=tokens.device).long()
        pos = torch.arange(U + 1, device=tokens.device)[None, :]
        inputs = torch.cat([tokens.new_zeros(B, 1), tokens], dim=1)
        inputs = torch.where(pos <= lengths[:, None], inputs, torch.zeros_like(inputs))
        targets = torch.cat([tokens, tokens.new_zeros(B, 1)], dim=1)
        targets = torch.where(pos < lengths[:, None], targets, torch.zeros_like(targets))      # position lengths[b] predicts the closing 0
        targets = torch.where(pos <= lengths[:, None], targets, torch.full_like(targets, -100))
        return F.cross_entropy(self.forward(inputs).reshape(B * (U + 1), -1), targets.reshape(-1), ignore_index=-100)

    @torch.no_grad()
    def next_logits(self, hist):
        """the last position of forward(hist).  Under the causal mask, as in training: the last position itself sees every key with or without
        a mask, but from the second layer on it attends to the earlier positions' states, and without a mask those have looked ahead (the
        label encoder's decoding calls carry that quirk over from the reference; a language model scored on prefixes must not)"""
        return self.head(self.decoder(hist.contiguous(), MaskSpec(1))[:, -1, :].float())


def eos_logprob(rows, norm, eos, blank=0):
    """log P(eos | history) of every row of a source, in f64, under the source's norm"""
    x = rows.double()
    if norm == "logprob":
        return x[..., eos]
    if norm == "softmax_no_blank":
        keep = torch.ones(x.shape[-1], dtype=torch.bool, device=x.device)
        keep[blank] = False
        return x[..., eos] - torch.logsumexp(x[..., keep], dim=-1)
    return x[..., eos] - torch.logsumexp(x, dim=-1)


class NGramLM:
    """A back-off n-gram language model in ARPA format as a ContextGraph (the automaton's contract: include/ttmi.h)."""

    @staticmethod
    def parse_arpa(text):
        """-> {order: {words tuple: (log10 p, log10 back-off)}}"""
        grams, order = {}, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line.startswith("ngram ") or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                order = int(line[1:line.index("-")])
                grams[order] = {}
                continue
            if order is None:
                continue
            f = line.split()
            if len(f) < order + 1:
                raise ValueError("NGramLM: bad ARPA line %r" % line)
            grams[order][tuple(f[1:order + 1])] = (float(f[0]), float(f[order + 1]) if len(f) > order + 1 else 0.0)
        if 1 not in grams:
            raise ValueError("NGramLM: no \\1-grams: section")
        return grams

    @classmethod
    def from_arpa(cls, text_or_path, symbols, weight=1.0, unk_log10=-10.0):
        """ARPA text (or the path of a file holding it) -> a ContextGraph for context=.  symbols: {word: token id} (or a list, the index the
        id; the blank's entry, id 0, is ignored).  States are the model's contexts, numbered by (length, tuple), so fail[s] < s; an arc is an
        explicit n-gram at weight * ln10 * log10 p and leads to the longest suffix of context + word that is a context; fail_w is the
        back-off weight, fail_w[0] the unigram of <unk> (unk_log10 where there is none): what a symbol without a unigram costs;
        final_w[s] = weight * log P(</s> | s) through the back-off chain.  Words outside `symbols` are dropped.  The search starts in the
        <s> context (.start)."""
        text = text_or_path
        if "\n" not in text_or_path and "\\data\\" not in text_or_path:
            with open(text_or_path) as fh:
                text = fh.read()
        if not isinstance(symbols, dict):
            symbols = {w: i for i, w in enumerate(symbols)}
        ids = {w: int(i) for w, i in symbols.items() if int(i) != 0}
        ids["<s>"] = -1                                              # a context symbol only: never on an arc
        c = float(weight) * math.log(10.0)
        if not math.isfinite(c) or weight < 0:
            raise ValueError("NGramLM: weight must be finite and >= 0, got %r" % (weight,))
        grams = cls.parse_arpa(text)
        top = max(grams)
        prob, backoff = {}, {}                                       # on id tuples; </s> kept aside
        eos = {}
        for n, table in grams.items():
            for words, (lp, bo) in table.items():
                if words[-1] == "</s>":
                    if all(w in ids for w in words[:-1]):
                        eos[tuple(ids[w] for w in words[:-1])] = lp
                    continue
                if not all(w in ids for w in words):
                    continue
                key = tuple(ids[w] for w in words)
                if key[-1] != -1:
                    prob[key] = lp
                backoff[key] = bo
        # contexts: every n-gram below the top order (it may carry a back-off weight), every prefix of an explicit n-gram (of a </s> one
        # too), the <s> context, and the suffixes that keep the set closed
        contexts = {(), (-1,)} | set(backoff) | {key[:-1] for key in prob} | set(eos)
        contexts = {x for x in contexts if len(x) < top and all(k != -1 or i == 0 for i, k in enumerate(x))}
        for x in list(contexts):                                     # a back-off chain walks through every suffix
            for i in range(1, len(x) + 1):
                contexts.add(x[i:])
        nodes = sorted(contexts, key=lambda x: (len(x), x))
        index = {x: i for i, x in enumerate(nodes)}

        def longest(seq):
            for i in range(len(seq) + 1):
                if seq[i:] in index:
                    return index[seq[i:]]
            raise AssertionError("the empty context is a state")

        unk = grams[1].get(("<unk>",), (unk_log10, 0.0))[0]
        arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w = [0], [], [], [], [], [], []
        for x in nodes:
            for key in sorted(k for k in prob if k[:-1] == x):
                arc_sym.append(key[-1])
                arc_next.append(longest(key))
                arc_w.append(c * prob[key])
            arc_off.append(len(arc_sym))
            fail.append(longest(x[1:]) if x else 0)
            fail_w.append(c * (backoff.get(x, 0.0) if x else unk))
            acc, y = 0.0, x                                          # log P(</s> | x) through the back-off chain
            while y not in eos and y:
                acc += backoff.get(y, 0.0)
                y = y[1:]
            final_w.append(c * (acc + eos.get(y, unk_log10)))
        g = ContextGraph.from_tables(arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w)
        g.start = index[(-1,)]
        return g
