"""The device side of greedy decoding (ttmi_greedy_scan, ttmi_greedy_scan_batch, ttmi_greedy_advance) and ttmi_embed_bwd, driven directly
and compared with plain Python restatements of their contracts in include/ttmi.h: the argmax is torch.argmax's on the CPU (first maximal
index; NaN counts as the largest value), row pads are poisoned, ties sit in one lane and across lanes, utterances are ragged, and every
state word of the batched decode is compared after every advance.  The whole-model decode tests (test_model_gpu.py,
test_decode_graphs_gpu.py) only ever see random-weight logits: no ties, no rows without a finite maximum."""
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 1e30              # finite in bf16 and f32: wins every argmax it takes part in


def _padded(rows, dtype, pad=3):
    """rows f32 CPU [..., V] -> device tensor of `dtype` with a row pitch of V + pad, the pad poisoned; returns the [..., V] view"""
    V = rows.shape[-1]
    full = torch.full(rows.shape[:-1] + (V + pad,), POISON, dtype=torch.float32)
    full[..., :V] = rows
    return full.to(dtype).cuda()[..., :V]


def _argmax(row):
    """the reference argmax: torch's, on the CPU, in f32, of the values the kernel reads"""
    return int(torch.argmax(row.detach().float().cpu()))


def _scan_model(rows, blank):
    """ttmi_greedy_scan: (first row whose argmax != blank, that argmax) or (n, None)"""
    rows = rows.detach().float().cpu()
    for r in range(rows.shape[0]):
        a = _argmax(rows[r])
        if a != blank:
            return r, a
    return rows.shape[0], None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("blank", [0, 3])
@pytest.mark.parametrize("V", [1, 5, 64, 65, 4334])
def test_greedy_scan_finds_the_first_non_blank_row(V, blank, dtype):
    """all rows blank -> n << 32 (reported as (n, None)); the first non-blank row in the first, a middle and the last row (n = 3, 5, 130: the
    last row is in a partial workgroup of 4 waves) and two non-blank rows (the earlier one wins); row pitch V + 3 with a poisoned pad.
    blank = 3 with V <= 3: no column is blank, row 0 always emits."""
    from ttmi import ops
    g = torch.Generator().manual_seed(V + blank)
    for n in (1, 3, 4, 5, 130):
        base = torch.randn(n, V, generator=g)
        if blank < V:
            base[:, blank] += 50.0                                       # every row blank
        other = (blank + 1 + V // 2) % V                                 # a non-blank column (V = 1: there is none)
        mid = n // 2
        for where in ("none", "first", "middle", "last", "two"):
            rows = base.clone()
            if V > 1:
                for r in {"none": [], "first": [0], "middle": [mid], "last": [n - 1], "two": [mid, n - 1]}[where]:
                    rows[r, other] += 100.0
            dev = _padded(rows, dtype)
            want = _scan_model(dev, blank)
            if V > 1 and blank < V:
                assert want == {"none": (n, None), "first": (0, other), "middle": (mid, other), "last": (n - 1, other), "two": (mid, other)}[where]
            assert ops.greedy_scan(dev, blank) == want, (n, where)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,tied,blank,want", [
    (4334, [134, 70, 200], 0, 70),           # 70 and 134 in one lane (64 apart), 200 in another
    (4334, [4333, 4269, 13], 0, 13),
    (4334, [5, 69, 300], 5, None),           # blank among the tied ones and the lowest: the row is blank
    (4334, [70, 6, 900], 70, 6),             # blank tied, a lower index in the same lane wins
    (4334, [70, 3], 70, 3),                  # ... in another lane
    (65, [0, 64], 0, None),                  # lane 0 holds both
    (65, [64, 1], 1, None),
    (65, [64, 63], 64, 63)])
def test_greedy_scan_ties_go_to_the_lowest_index(V, tied, blank, want, dtype):
    from ttmi import ops
    rows = torch.zeros(3, V)
    rows[:, blank] = 1.0                     # rows 0 and 2 are blank
    rows[1, blank] = 0.0
    rows[1, tied] = 0.5                      # exact in bf16
    dev = _padded(rows, dtype)
    assert _argmax(dev[1]) == min(tied)
    assert ops.greedy_scan(dev, blank) == ((1, want) if want is not None else (3, None))
    assert _scan_model(dev, blank) == ((1, want) if want is not None else (3, None))


def _nonfinite_rows(V):
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(V)
    fin = torch.randn(V, generator=g)
    rows = {"all -inf": torch.full((V,), -inf), "all NaN": torch.full((V,), nan)}
    a, b, c = (V * 2) // 5, (V * 4) // 5, V - 1
    r = fin.clone(); r[[a, c]] = nan; r[0] = 9.0
    rows["NaN and finite"] = r
    r = fin.clone(); r[[b, c]] = inf; r[a] = 9.0
    rows["+inf present"] = r
    r = fin.clone(); r[[b, a]] = inf; r[c] = nan
    rows["+inf and NaN"] = r
    r = torch.full((V,), -inf); r[[b, c]] = -3.0
    rows["-inf and finite"] = r
    return rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [5, 65, 4334])
def test_greedy_scan_rows_without_a_finite_maximum(V, dtype):
    """rows that are all -inf, all NaN, NaN among finite values, +inf present: the emitted token is torch.argmax's of the same row on the
    CPU (evaluated here) and always inside [0, V).  Before the NaN-aware compare the kernels left such a row on their start index: an all
    -inf or all NaN row emitted token 0x7fffffff = 2147483647 (`best = -INF, bi = 0x7fffffff`, updated with `x > best` only), which the
    next label-encoder call embeds as a NaN row, and a NaN among finite values was skipped (the parent commit's library on an MI355X: this
    test fails for every V and type with `('all -inf', (1, 2147483647))`)."""
    from ttmi import ops
    blank = 1                                                            # (no case below has its argmax there: every row emits)
    blank_row = torch.zeros(V); blank_row[blank] = 5.0
    for name, row in _nonfinite_rows(V).items():
        rows = torch.stack([blank_row, row, blank_row])
        dev = _padded(rows, dtype)
        a = _argmax(dev[1])
        assert 0 <= a < V and a != blank
        got = ops.greedy_scan(dev, blank)
        print("V=%d %s %s: argmax %d, kernel %r" % (V, str(dtype)[6:], name, a, got))
        assert got[1] is not None and 0 <= got[1] < V, (name, got)
        assert got == (1, a), (name, got, a)
        assert ops.greedy_scan(dev[1:2], a) == (1, None), name           # the same row with its argmax as the blank: nothing to emit


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_greedy_scan_batch_rows_without_a_finite_maximum(dtype):
    """the same rows through ttmi_greedy_scan_batch + ttmi_greedy_advance: the token written into the history is in [0, V)"""
    from ttmi import ops
    V, n, blank = 65, 2, 1
    cases = _nonfinite_rows(V)
    B = len(cases)
    blank_row = torch.zeros(V); blank_row[blank] = 5.0
    logits = _padded(torch.stack([torch.stack([blank_row, r]) for r in cases.values()]), dtype)       # [B, 2, V]: frame 0 blank, frame 1 the case
    t = torch.zeros(B, dtype=torch.int32, device="cuda")
    T_len = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    need = torch.ones(B, dtype=torch.int32, device="cuda")
    done, count = torch.zeros_like(need), torch.zeros_like(need)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    key = torch.full((B,), n << 32, dtype=torch.int64, device="cuda")
    hist = torch.zeros(B, 4, dtype=torch.long, device="cuda")
    ops.greedy_scan_batch(logits, t, T_len, need, key, blank)
    ops.greedy_advance(key, n, 1, hist, t, T_len, need, done, count, flags)
    for b, name in enumerate(cases):
        a = _argmax(logits[b, 1])
        tok = int(hist[b, 1])
        assert 0 <= tok < V and tok == a and a != blank, (name, tok, a)
    assert count.tolist() == [1] * B and t.tolist() == [2] * B and flags.tolist() == [0, B]


# ---------------------------------------------------------------------------------------------------------------- the batched state machine
def _scan_batch_model(logits, t, T_len, need, key, blank):
    B, n, _ = logits.shape
    logits = logits.detach().float().cpu()
    for b in range(B):
        if not need[b]:
            continue
        for r in range(n):
            if t[b] + r >= T_len[b]:
                continue
            a = _argmax(logits[b, r])
            if a != blank:
                key[b] = min(key[b], (r << 32) | a)


def _advance_model(key, n, n_hist, hist, t, T_len, need, done, count):
    flags = [0, 0]
    for b in range(len(key)):
        k, key[b] = key[b], n << 32
        if need[b]:
            row = k >> 32
            if row < n:
                hist[b][n_hist] = k & 0xffffffff
                t[b] += row + 1
                count[b] += 1
                need[b] = 0
            else:
                t[b] += n
                if t[b] >= T_len[b]:
                    need[b], done[b] = 0, 1
        flags[0] += 1 if need[b] else 0
        flags[1] += 0 if done[b] else 1
    return flags


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,blank", [(1, 0), (5, 0), (5, 2), (70, 0)])
def test_batched_greedy_decode_state_machine(B, blank, dtype):
    """the host loop of Transducer.decode_batch in miniature (blocks of n = 4 frames, T = 12, V = 29) over seeded logits whose blank column
    is biased so that about half the frames are blank: ragged T_len (1, 3 < n, 8 and 12 = multiples of n, ...), one utterance blank
    throughout, one that emits on its last frame; the logits of the frames depend on the symbol step.  After every scan the key, after
    every advance t, need, done, count, hist, flags and the reset key are compared with the Python model.  Rows the scan must not look at
    (utterances with need == 0, frames at or beyond T_len) are poisoned with a winning non-blank symbol."""
    from ttmi import ops
    n, T, V = 4, 12, 29
    g = torch.Generator().manual_seed(B + blank)
    tables = torch.randn(2, B, T, V, generator=g)
    tables[:, :, :, blank] += 2.0
    T_list = [[12, 1, 3, 8, 5, 7, 4, 11][b % 8] for b in range(B)]
    if B == 1:
        T_list = [8]
    always_blank = 3 if B > 3 else None
    if always_blank is not None:
        tables[:, always_blank, :, blank] += 100.0
    tables[:, 0, T_list[0] - 1, (blank + 1) % V] += 100.0                # utterance 0 emits on its last frame
    poison = torch.zeros(V); poison[(blank + 5) % V] = 1000.0
    dev = "cuda"
    t = torch.zeros(B, dtype=torch.int32, device=dev)
    T_len = torch.tensor(T_list, dtype=torch.int32, device=dev)
    need = torch.ones(B, dtype=torch.int32, device=dev)
    done, count = torch.zeros_like(need), torch.zeros_like(need)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    key = torch.full((B,), n << 32, dtype=torch.int64, device=dev)
    hist = torch.zeros(B, T + 2, dtype=torch.long, device=dev)
    m = dict(t=[0] * B, need=[1] * B, done=[0] * B, count=[0] * B, key=[n << 32] * B, hist=[[0] * (T + 2) for _ in range(B)])
    n_hist, scans = 1, 0
    while True:
        for b in range(B):
            m["need"][b] = 1 - m["done"][b]
        torch.sub(1, done, out=need)
        while True:
            blk = torch.empty(B, n, V)
            for b in range(B):
                for r in range(n):
                    f = m["t"][b] + r
                    blk[b, r] = tables[n_hist % 2, b, f] if (m["need"][b] and f < T_list[b]) else poison
            logits = _padded(blk, dtype)
            ops.greedy_scan_batch(logits, t, T_len, need, key, blank)
            _scan_batch_model(logits, m["t"], T_list, m["need"], m["key"], blank)
            assert key.tolist() == m["key"], ("scan", n_hist, scans)
            ops.greedy_advance(key, n, n_hist, hist, t, T_len, need, done, count, flags)
            want_flags = _advance_model(m["key"], n, n_hist, m["hist"], m["t"], T_list, m["need"], m["done"], m["count"])
            scans += 1
            got = dict(t=t.tolist(), need=need.tolist(), done=done.tolist(), count=count.tolist(), key=key.tolist(), hist=hist.tolist())
            for name in got:
                assert got[name] == m[name], (name, n_hist, scans)
            assert flags.tolist() == want_flags, (n_hist, scans)
            if want_flags[0] == 0:
                break
        if want_flags[1] == 0:
            break
        n_hist += 1
        assert n_hist <= T + 1
    assert all(m["done"]) and all(tb >= Tb for tb, Tb in zip(m["t"], T_list))
    assert m["count"][0] >= 1 and m["hist"][0][m["count"][0]] == (blank + 1) % V      # utterance 0's last symbol is the one of its last frame
    if always_blank is not None:
        assert m["count"][always_blank] == 0
    assert n_hist == max(m["count"]) + 1 and scans >= n_hist
    for b in range(B):
        assert all(0 <= tok < V for tok in m["hist"][b]) and m["count"][b] <= T_list[b]


# ---------------------------------------------------------------------------------------------------------------- ttmi_embed_bwd
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", [1, 8, 130])
def test_embed_bwd_contract(d, pad):
    """gW += the weight gradient of torch.nn.functional.embedding (float64, CPU): duplicate ids summed (one id makes up ~70 % of the
    n = 37 rows), padding_idx skipped, ids -1 and V ignored, gW pre-filled.  n * d = 37, 296, 4810: no multiple of the 256-thread block,
    one and several blocks.  dout and the pre-fill are small integers, so the f32 atomic sums are exact in any order: torch.equal."""
    from ttmi import ops
    n, V = 37, 11
    g = torch.Generator().manual_seed(d + pad)
    tok = torch.randint(-1, V + 1, (n,), generator=g)
    tok[torch.rand(n, generator=g) < 0.7] = 4
    tok[:4] = torch.tensor([-1, V, pad, 4])
    assert (n * d) % 256 != 0 and (tok == 4).sum() > n // 2 and pad != 4
    dout = torch.randint(-4, 5, (n, d), generator=g).double()
    prefill = torch.randint(-9, 10, (V, d), generator=g).double()
    valid = (tok >= 0) & (tok < V)
    W = torch.zeros(V, d, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.embedding(tok[valid], W, padding_idx=pad) * dout[valid]).sum().backward()
    want = prefill + W.grad
    assert not W.grad[pad].any() and W.grad[4].abs().sum() > 0
    gW = prefill.float().cuda()
    out = ops.embed_bwd(tok.cuda(), dout.float().cuda(), V, pad, gW)
    assert out is gW and torch.equal(gW.cpu().double(), want)
