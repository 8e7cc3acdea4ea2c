"""CPU-only side of contextual biasing: the hotword compiler (ttmi/context.py) against a brute force by substring counting and against the
rule restated in tests/beam_ctx_oracle.py, ContextGraph.validate, the biased oracle with a zero-weight graph against beam_oracle.step,
ttmi_beam_step_ctx's argument validation without a GPU, and biased beam decoding on CPU tensors being an error.

The compiler case: four symbols 1 .. 4, every sequence of length 0 .. 6 (5461 of them), five phrases with five boosts - [1, 2] is a prefix of
[1, 2, 3], [2, 3] a suffix of it, [1, 1] overlaps itself in 1 1 1, [3] is a single token and a suffix of two others.  The boosts are multiples
of 1/4, so every weight and every sum is exact in f32 and f64 and the comparison is for equality."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import beam_ctx_oracle as CO
import beam_oracle as BO
from conftest import PKG

PHRASES = [[1, 2], [1, 2, 3], [2, 3], [1, 1], [3]]
BOOSTS = [1.5, 0.75, 2.0, 1.25, 0.5]


def _graph_tables(g):
    return CO.Tables(*(x.numpy() for x in g.cpu_tables()))


def test_compiler_against_brute_force():
    from ttmi.context import ContextGraph
    g = ContextGraph(PHRASES, boost=BOOSTS).validate(5)
    tb = _graph_tables(g)
    want = CO.compile_tables(PHRASES, BOOSTS)
    for got, ref in zip(tb, want):                            # the compiler's tables are the restated rule's, bit for bit
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (got, ref)
    assert g.S == len(tb.fail) == 8 and g.A == len(tb.arc_sym) == 7
    assert all(tb.fail[s] < s for s in range(1, g.S)) and float(tb.fail_w[0]) == 0.0
    n = 0
    for length in range(7):
        for y in itertools.product([1, 2, 3, 4], repeat=length):
            _, running, final = CO.fsa_run(tb, y)
            assert (running, final) == CO.brute_bias(PHRASES, BOOSTS, y), y
            n += 1
    assert n == 5461
    # a hotword begun and not finished keeps nothing; a finished one keeps boost * len, per occurrence, overlaps counted
    assert CO.fsa_run(tb, (4, 1))[1:] == (1.5, 0.0)
    assert CO.fsa_run(tb, (1, 1, 1))[2] == 2 * 1.25 * 2
    assert CO.fsa_run(tb, (1, 2, 3))[2] == 1.5 * 2 + 0.75 * 3 + 2.0 * 2 + 0.5


def test_compiler_duplicates_one_boost_and_the_empty_graph():
    from ttmi.context import ContextGraph
    twice = _graph_tables(ContextGraph([[2, 3], [2, 3]], boost=1.5))
    assert CO.fsa_run(twice, (2, 3))[2] == 2 * 1.5 * 2                     # duplicates add up
    one = _graph_tables(ContextGraph([[2, 3], [4]]))
    assert CO.fsa_run(one, (2, 3, 4))[2] == 3.0                            # boost = 1.0 for every phrase
    g = ContextGraph([]).validate(5)
    tb = _graph_tables(g)
    assert g.S == 1 and g.A == 0 and tb.arc_off.tolist() == [0, 0] and tb.fail_w.tolist() == [0.0] and tb.final_w.tolist() == [0.0]
    assert CO.fsa_run(tb, (1, 2, 3)) == (0, 0.0, 0.0)
    assert g.to("cpu") is g and g.to("cpu").tables[0] is g.tables[0]       # a device's copy is made once


def test_validate_refuses_what_breaks_the_contract():
    from ttmi.context import ContextGraph
    for bad in ([[1, 0]], [[]], [[1, -2]]):
        with pytest.raises(ValueError):
            ContextGraph(bad)
    for boost in (math.inf, math.nan, 0.0, -1.0, [1.0, 2.0]):
        with pytest.raises(ValueError):
            ContextGraph([[1, 2]], boost=boost)
    g = ContextGraph([[1, 2], [1, 4]])
    g.validate(5)
    with pytest.raises(ValueError, match=r"symbols lie in \[0, 4\)"):
        g.validate(4)                                                       # a symbol >= V
    arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w = (x.tolist() for x in g.cpu_tables())
    assert arc_sym == [1, 2, 4]
    ContextGraph.from_tables(arc_off, arc_sym, arc_next, arc_w, fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError, match="not sorted"):
        ContextGraph.from_tables(arc_off, [1, 4, 2], arc_next, arc_w, fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError, match="not sorted"):
        ContextGraph.from_tables(arc_off, [1, 2, 2], arc_next, arc_w, fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError, match="never the blank"):
        ContextGraph.from_tables(arc_off, [1, 0, 4], arc_next, arc_w, fail, fail_w, final_w).validate(5)
    for bad_fail in ([0, 1, 0, 0], [0, 0, 3, 0], [0, -1, 0, 0]):
        with pytest.raises(ValueError, match="failure link"):
            ContextGraph.from_tables(arc_off, arc_sym, arc_next, arc_w, bad_fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError, match="finite"):
        ContextGraph.from_tables(arc_off, arc_sym, arc_next, [1.0, math.inf, 1.0], fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError, match="finite"):
        ContextGraph.from_tables(arc_off, arc_sym, arc_next, arc_w, fail, [0.0, math.nan, 0.0, 0.0], final_w).validate(5)
    with pytest.raises(ValueError):
        ContextGraph.from_tables(arc_off, arc_sym, [1, 2, 9], arc_w, fail, fail_w, final_w).validate(5)
    with pytest.raises(ValueError):
        ContextGraph.from_tables([0, 1, 4, 3, 3], arc_sym, arc_next, arc_w, fail, fail_w, final_w).validate(5)


@pytest.mark.parametrize("V,W,T,seed", [(5, 8, 10, 0), (37, 4, 12, 0), (3, 32, 4, 1)])
def test_biased_oracle_with_zero_weights_is_the_unbiased_oracle(V, W, T, seed):
    logits = BO.rng_logits(seed, V)
    final, _, _ = BO.run(logits, 0, T, W)
    phrases = CO.phrases_from(final, V)
    assert phrases is not None
    zero = CO.zero_weights(CO.compile_tables(phrases, [2.0] * 4))
    plain, biased = list(BO.START) + [None] * (W - 1), CO.START + [None] * (W - 1)
    states = set()
    for t in range(T):
        rows = [logits(0, t, h.tokens) if h is not None else None for h in plain]
        plain, parent, fresh, margin, _ = BO.step(plain, rows, t, W)
        biased, b_parent, b_fresh, b_margin, counters = CO.step(biased, rows, t, W, zero)
        assert (b_parent, b_fresh, b_margin) == (parent, fresh, margin) and counters["differs"] == 0 and counters["fail_hops"] == 0
        assert [h and BO.Hyp(*h[:4]) for h in biased] == plain                   # exactly: x + 0.0 changes no value and no order
        assert all(h.bias == 0.0 for h in biased if h is not None)
        states |= {h.state for h in biased if h is not None}
    assert len(states) > 1                                                       # the automaton was walked, not left at the root


def test_a_boost_keeps_a_hotword_the_unbiased_beam_loses():
    """the point of biasing inside the search: greedy decoding (a beam of one) never sees the phrase, the biased beam of one ends on it"""
    V, T = 37, 12
    logits = BO.rng_logits(0, V)
    greedy = BO.run(logits, 0, T, 1)[0][0].tokens
    phrase = [k for k in range(1, V) if k not in greedy][:2]
    tb = CO.compile_tables([phrase], [50.0])
    beam, _, counters, _ = CO.run(logits, 0, T, 1, tb)
    (h, final_bias), = CO.final_order(beam, tb)[0]
    y = "".join(chr(65 + k) for k in h.tokens)
    assert counters["differs"] > 0 and counters["arcs"] >= 2 and "".join(chr(65 + k) for k in phrase) in y
    assert final_bias == CO.brute_bias([phrase], [50.0], h.tokens)[1] >= 100.0


def _lib():
    so = os.path.join(PKG, "ttmi", "libttmi.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    lib = ctypes.CDLL(so)
    lib.ttmi_last_error.restype = ctypes.c_char_p
    return lib


def test_beam_step_ctx_validates_its_arguments_without_gpu():
    lib = _lib()
    L = ctypes.c_long
    bufs = [(ctypes.c_double * 8)() for _ in range(8)]
    p = ctypes.cast(bufs[0], ctypes.c_void_p)
    o = [ctypes.cast(x, ctypes.c_void_p) for x in bufs[1:]]      # the _out arrays: buffers of their own

    def call(logits=p, ld=5, B=1, W=4, V=5, blank=0, ins=(p, p, p, p, p), outs=None, ld_hist=8, ld_det=8, parent=p, dtype=0, S=2, A=1,
             tables=(p, p, p, p, p, p), ctx_in=(p, p), ctx_out=None, ws=p):
        outs = o[:5] if outs is None else outs
        ctx_out = o[5:7] if ctx_out is None else ctx_out
        return lib.ttmi_beam_step_ctx(logits, dtype, L(ld), B, W, V, blank, p, p, *ins, *outs, L(ld_hist), L(ld_det), parent, p, S, A, *tables,
                                      *ctx_in, *ctx_out, ws, None)

    assert call(logits=None) < 0 and b"beam_step_ctx" in lib.ttmi_last_error() and b"null pointer" in lib.ttmi_last_error()
    assert call(parent=None) < 0 and b"null pointer" in lib.ttmi_last_error()
    for i in range(6):                                           # every table pointer
        tables = [p] * 6
        tables[i] = None
        assert call(tables=tables) < 0 and b"null pointer" in lib.ttmi_last_error(), i
    assert call(ctx_in=(None, p)) < 0 and call(ctx_in=(p, None)) < 0 and b"null pointer" in lib.ttmi_last_error()
    assert call(ctx_out=(None, o[6])) < 0 and call(ctx_out=(o[5], None)) < 0 and call(ws=None) < 0 and b"null pointer" in lib.ttmi_last_error()
    assert call(S=0) < 0 and call(A=-1) < 0
    for W in (0, 33, -1):
        assert call(W=W) < 0 and b"beam width" in lib.ttmi_last_error()
    assert call(V=1, ld=1) < 0 and b"bad arguments" in lib.ttmi_last_error()
    assert call(ld=4) < 0 and call(blank=5) < 0 and call(blank=-1) < 0 and call(ld_hist=1) < 0 and call(ld_det=0) < 0 and call(B=0) < 0
    assert call(dtype=2) < 0
    assert call(ins=(p, p, p, None, p)) < 0 and b"all four" in lib.ttmi_last_error()
    assert call(outs=[p] + o[1:5]) < 0 and b"buffers of its own" in lib.ttmi_last_error()
    assert call(ctx_out=(p, o[6])) < 0 and b"buffers of its own" in lib.ttmi_last_error()
    assert call(ctx_out=(o[5], p)) < 0 and b"buffers of its own" in lib.ttmi_last_error()
    lib.ttmi_beam_ctx_ws_bytes.restype = ctypes.c_size_t
    assert lib.ttmi_beam_ctx_ws_bytes(3, 4, 37) == 3 * 4 * 37 * 8 and lib.ttmi_beam_ctx_ws_bytes(0, 4, 37) == 0


def test_biased_beam_decoding_on_cpu_tensors_is_an_error():
    from tt.model import Transducer
    from tt.utils import AttrDict
    from ttmi.context import ContextGraph
    side = dict(n_layer=1, d_model=64, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=29, dropout=0.0))
    torch.manual_seed(0)
    model = Transducer(cfg).eval()
    g = ContextGraph([[3, 4], [5]], boost=2.0)
    with pytest.raises(ValueError, match="must live on the GPU"):
        model.beam_decode_batch(torch.zeros(2, 6, 64), [6, 4], context=g, return_bias=True)
    with pytest.raises(ValueError, match="must live on the GPU"):
        model.recognize_nbest(torch.zeros(2, 6, 64), torch.tensor([6, 4]), context=g)
    with pytest.raises(ValueError, match="ops need device tensors"):
        from ttmi import ops
        z = torch.zeros(1, 2, dtype=torch.float64)
        n = torch.zeros(1, 2, dtype=torch.int32)
        beam = (z, n, torch.zeros(1, 2, 4, dtype=torch.long), None, None)
        ops.beam_step_ctx(torch.zeros(1, 2, 29), n[:, 0], n[:, 0], beam, beam, n, n, g.tables, (n, z), (n, z), torch.zeros(8))
