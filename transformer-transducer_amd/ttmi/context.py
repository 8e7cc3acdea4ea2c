"""Contextual biasing (hotword boosting) for the frame-synchronous beam search: a set of token phrases compiled into the deterministic weighted
automaton with failure links that ttmi_beam_step_ctx walks (include/ttmi.h has the automaton's contract and the transition rule).

ContextGraph(phrases, boost)     the hotword compiler: phrase trie + Aho-Corasick failure links
ContextGraph.from_tables(...)    any automaton that meets the contract
.validate(V)                     checks the CPU copy of the tables before any launch
.to(device)                      uploads the tables once; .tables / .final_w are then device tensors
.start                           the state slot 0 starts in: 0, the root (ttmi.lm.NGramLM.from_arpa sets the <s> context)

What the compiled weights mean.  A finished phrase p is worth boost_p * len(p), counted once per occurrence in the token sequence, overlapping
occurrences included.  A phrase that has been begun is paid in advance, boost * (tokens matched so far), so that its first token already rises
in the beam; the advance is pi(n) = beta(n) * depth(n) for a trie node n with children (beta(n) = the largest boost of a phrase that strictly
extends n), 0 for a leaf.  After tokens y the running bias is
    sum_p boost_p * len(p) * occurrences(p in y)  +  pi(the longest suffix of y that is a trie node)
and the final bias (final_w[n] = -pi(n) takes the advance back) is the first term alone: a hotword begun and not finished keeps nothing."""
import collections
import math

import torch

BLANK = 0


class ContextGraph:
    def __init__(self, phrases, boost=1.0):
        phrases = [list(p) for p in phrases]
        try:
            boosts = [float(b) for b in boost]
        except TypeError:
            boosts = [float(boost)] * len(phrases)
        if len(boosts) != len(phrases):
            raise ValueError("ContextGraph: boost is one float or one per phrase (%d phrases, %d boosts)" % (len(phrases), len(boosts)))
        for b in boosts:
            if not math.isfinite(b) or b <= 0.0:
                raise ValueError("ContextGraph: a boost must be finite and > 0, got %r" % (b,))
        for p in phrases:
            if not p:
                raise ValueError("ContextGraph: an empty phrase")
            for k in p:
                if int(k) != k or k < 0 or k == BLANK:
                    raise ValueError("ContextGraph: a phrase holds non-negative token ids other than the blank (%d), got %r" % (BLANK, p))
        # the trie, nodes in insertion order first
        children, depth, end, beta = [{}], [0], [0.0], [0.0]
        for p, b in zip(phrases, boosts):
            n = 0
            for i, k in enumerate(p):
                beta[n] = max(beta[n], b)                            # p strictly extends every node on its path but the last
                if int(k) not in children[n]:
                    children[n][int(k)] = len(children)
                    children.append({})
                    depth.append(i + 1)
                    end.append(0.0)
                    beta.append(0.0)
                n = children[n][int(k)]
            end[n] += b * len(p)                                     # duplicates add up
        # renumbered breadth first, children by ascending symbol: a failure link points to a shallower node, so fail[s] < s
        order, queue = [], collections.deque([0])
        while queue:
            n = queue.popleft()
            order.append(n)
            queue.extend(children[n][k] for k in sorted(children[n]))
        new = {n: i for i, n in enumerate(order)}
        S = len(order)
        kids = [{k: new[c] for k, c in children[n].items()} for n in order]
        depth, end, beta = [depth[n] for n in order], [end[n] for n in order], [beta[n] for n in order]
        pi = [beta[s] * depth[s] if kids[s] else 0.0 for s in range(S)]
        fail, out = [0] * S, list(end)
        for s in range(S):                                           # parents come before children: fail and out of s are final here
            for k, c in kids[s].items():
                f = fail[s]
                while s != 0 and f != 0 and k not in kids[f]:
                    f = fail[f]
                fail[c] = kids[f][k] if s != 0 and k in kids[f] else 0
                out[c] = end[c] + out[fail[c]]
        arc_off, arc_sym, arc_next, arc_w = [0], [], [], []
        for s in range(S):
            for k in sorted(kids[s]):
                c = kids[s][k]
                arc_sym.append(k)
                arc_next.append(c)
                arc_w.append(pi[c] - pi[s] + out[c])
            arc_off.append(len(arc_sym))
        fail_w = [0.0] + [pi[fail[s]] - pi[s] for s in range(1, S)]
        self._set(arc_off, arc_sym, arc_next, arc_w, fail, fail_w, [-v for v in pi])

    @classmethod
    def from_tables(cls, arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w):
        """an automaton given by its tables (lists or tensors; the contract: include/ttmi.h); checked by validate(V)"""
        g = cls.__new__(cls)
        g._set(arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w)
        return g

    def _set(self, arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w):
        def as_tensor(x, dtype):
            return torch.as_tensor(x, device="cpu").to(dtype).contiguous().reshape(-1)
        self._cpu = tuple(as_tensor(x, dt) for x, dt in ((arc_off, torch.int32), (arc_sym, torch.int32), (arc_next, torch.int32),
                                                         (arc_w, torch.float32), (fail, torch.int32), (fail_w, torch.float32)))
        self._cpu_final = as_tensor(final_w, torch.float32)
        self.tables, self.final_w = self._cpu, self._cpu_final
        self.S, self.A = int(self._cpu[4].shape[0]), int(self._cpu[1].shape[0])
        self._device = {}
        self.start = 0                                               # the state the search starts in: the root for everything built here

    def cpu_tables(self):
        """(arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w) as CPU tensors"""
        return self._cpu + (self._cpu_final,)

    def validate(self, V):
        """ValueError unless the CPU copy of the tables meets the contract for a vocabulary of V symbols (no launch is made)"""
        arc_off, arc_sym, arc_next, arc_w, fail, fail_w = (x.tolist() for x in self._cpu)
        final_w = self._cpu_final.tolist()
        S, A = self.S, self.A
        if S < 1 or len(arc_off) != S + 1 or len(fail_w) != S or len(final_w) != S or len(arc_next) != A or len(arc_w) != A:
            raise ValueError("ContextGraph: table sizes do not fit each other (S = %d, A = %d)" % (S, A))
        if arc_off[0] != 0 or arc_off[-1] != A or any(a > b for a, b in zip(arc_off, arc_off[1:])):
            raise ValueError("ContextGraph: arc_off must rise from 0 to the number of arcs")
        for s in range(S):
            syms = arc_sym[arc_off[s]:arc_off[s + 1]]
            if any(a >= b for a, b in zip(syms, syms[1:])):
                raise ValueError("ContextGraph: the arcs of state %d are not sorted by strictly ascending symbol" % s)
            for k in syms:
                if k == BLANK or not 0 <= k < V:
                    raise ValueError("ContextGraph: state %d has an arc on %d: symbols lie in [0, %d) and are never the blank" % (s, k, V))
            if s > 0 and not 0 <= fail[s] < s:
                raise ValueError("ContextGraph: fail[%d] = %d, a failure link must point to a lower state" % (s, fail[s]))
        if any(not 0 <= n < S for n in arc_next):
            raise ValueError("ContextGraph: an arc leads outside the %d states" % S)
        if not all(math.isfinite(w) for w in arc_w + fail_w + final_w):
            raise ValueError("ContextGraph: every weight must be finite")
        return self

    def to(self, device):
        """the same graph with .tables / .final_w on `device`; a device's copy is made once"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = (tuple(x.to(device) for x in self._cpu), self._cpu_final.to(device))
        self.tables, self.final_w = self._device[device]
        return self
