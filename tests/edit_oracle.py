"""Plain restatement of the edit-distance rule (include/ttmi.h, ttmi_edit_distance), for the tests of the kernel, of ttmi.metrics and of
Transducer.mwer_loss.  A helper, not a test module (like beam_oracle.py).

Among all alignments of hyp to ref the one that minimises (distance, substitutions, deletions, insertions) lexicographically.  A deletion is a
ref token without a hyp counterpart, an insertion a hyp token without a ref counterpart.

edit_counts()  dynamic programme over (distance, s, d, i) tuples, compared as tuples
brute_force()  the same minimum over EVERY alignment (every monotone path through the grid), for tiny pairs"""


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


SUB, DEL, INS = (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1)


def edit_counts(hyp, ref):
    """-> (distance, substitutions, deletions, insertions)"""
    hyp, ref = list(hyp), list(ref)
    prev = [(j, 0, j, 0) for j in range(len(ref) + 1)]                   # no hyp token yet: j deletions
    for i in range(1, len(hyp) + 1):
        h = hyp[i - 1]
        left = (i, 0, 0, i)                                              # no ref token yet: i insertions
        cur = [left]
        for j in range(1, len(ref) + 1):
            a, b = prev[j - 1], prev[j]
            if h != ref[j - 1]:
                a = (a[0] + 1, a[1] + 1, a[2], a[3])                     # substitution
            left = min(a, (b[0] + 1, b[1], b[2], b[3] + 1), (left[0] + 1, left[1], left[2] + 1, left[3]))      # ..., insertion, deletion
            cur.append(left)
        prev = cur
    return prev[len(ref)]


def brute_force(hyp, ref):
    """the minimum over all monotone paths from (0, 0) to (len(hyp), len(ref)): exponential, lengths up to 4 or so"""
    hyp, ref = list(hyp), list(ref)

    def walk(i, j, acc):
        if i == len(hyp) and j == len(ref):
            yield acc
            return
        if i < len(hyp) and j < len(ref):
            yield from walk(i + 1, j + 1, acc if hyp[i] == ref[j] else _add(acc, SUB))
        if i < len(hyp):
            yield from walk(i + 1, j, _add(acc, INS))
        if j < len(ref):
            yield from walk(i, j + 1, _add(acc, DEL))
    return min(walk(0, 0, (0, 0, 0, 0)))
