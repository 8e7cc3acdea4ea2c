"""ttmi.lm.NGramLM.from_arpa: a back-off n-gram model compiled into the automaton of ttmi_beam_step_ctx, checked without a GPU against the ARPA
back-off rule restated on words: for every token sequence of up to four tokens over five symbols (the blank and four words), walking the
automaton from its start state gives the running and the final score of the sequence within 1e-5 per token (the tables hold f32 weights)."""
import itertools
import math

import pytest

import beam_ctx_oracle as CO

# a trigram model with back-off weights, an <unk>, a word (e) that is not among the symbols and a symbol (d) without a unigram
ARPA = """
\\data\\
ngram 1=7
ngram 2=8
ngram 3=5

\\1-grams:
-99.0 <s> -0.40
-1.10 </s>
-2.00 <unk>
-0.70 a -0.30
-0.90 b -0.25
-1.20 c -0.15
-1.00 e -0.20

\\2-grams:
-0.50 <s> a -0.20
-0.80 <s> b
-0.40 a b -0.35
-0.90 a e -0.10
-0.60 b a
-0.70 b c -0.05
-0.30 c </s>
-1.30 b </s>

\\3-grams:
-0.20 <s> a b
-0.35 a b c
-0.45 a b </s>
-0.55 b c a
-0.15 e a b

\\end\\
"""
SYMBOLS = {"<blank>": 0, "a": 1, "b": 2, "c": 3, "d": 4}
WORDS = {v: k for k, v in SYMBOLS.items()}
UNK = -2.00


def _grams():
    from ttmi.lm import NGramLM
    return NGramLM.parse_arpa(ARPA)


def _log10p(grams, context, word):
    """the ARPA rule: the longest listed n-gram ending in `word`, the back-off weights of the contexts left on the way (0 where a context is
    not listed); a word without a unigram scores as <unk>"""
    top = max(grams)
    ctx, acc = tuple(context[-(top - 1):]), 0.0
    while True:
        key = ctx + (word,)
        if key in grams[len(key)]:
            return acc + grams[len(key)][key][0]
        if not ctx:
            return acc + UNK
        acc += grams[len(ctx)].get(ctx, (0.0, 0.0))[1]
        ctx = ctx[1:]


def _walk(tb, start, y):
    s, bias = start, 0.0
    for k in y:
        s, d, _, _ = CO.fsa_step(tb, s, int(k))
        bias += d
    return bias, bias + float(tb.final_w[s])


@pytest.mark.parametrize("weight", [1.0, 0.4])
def test_automaton_scores_are_the_arpa_back_off_scores(weight):
    from ttmi.lm import NGramLM
    g = NGramLM.from_arpa(ARPA, SYMBOLS, weight=weight)
    assert g.validate(5) is g and g.start != 0
    tb = CO.Tables(*(x.numpy() for x in g.cpu_tables()))
    assert all(int(tb.fail[s]) < s for s in range(1, g.S))
    grams = _grams()
    c, worst = weight * math.log(10.0), 0.0
    for n in range(5):
        for y in itertools.product(range(1, 5), repeat=n):
            words, run = ["<s>"], 0.0
            for k in y:
                w = WORDS[k] if (WORDS[k],) in grams[1] else "<unk>"
                run += _log10p(grams, words, w)
                words.append(w)
            final = run + _log10p(grams, words, "</s>")
            got = _walk(tb, g.start, y)
            tol = 1e-5 * max(n, 1)
            assert abs(got[0] - c * run) <= tol and abs(got[1] - c * final) <= tol, (y, got, c * run, c * final)
            worst = max(worst, abs(got[0] - c * run), abs(got[1] - c * final))
    print("weight %.1f: %d states, %d arcs, start %d, worst error %.3e" % (weight, g.S, g.A, g.start, worst))


def test_words_outside_the_symbols_are_dropped_and_unk_falls_back():
    from ttmi.lm import NGramLM
    g = NGramLM.from_arpa(ARPA, SYMBOLS)
    assert set(g.cpu_tables()[1].tolist()) <= {1, 2, 3}          # no arc on the blank, on d (no unigram) or on anything for e
    assert abs(float(g.cpu_tables()[5][0]) - UNK * math.log(10.0)) < 1e-5
    no_unk = NGramLM.from_arpa(ARPA.replace("-2.00 <unk>\n", ""), SYMBOLS, unk_log10=-7.0)
    assert abs(float(no_unk.cpu_tables()[5][0]) - -7.0 * math.log(10.0)) < 1e-5
    from ttmi.context import ContextGraph
    assert ContextGraph([[1, 2]]).start == 0
