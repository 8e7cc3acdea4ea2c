"""The device side of decode details (ttmi_greedy_scan_batch_lp, ttmi_greedy_advance_lp), driven directly like the plain pair in
test_greedy_kernels_gpu.py (poisoned row pads with a pitch of V + 3, f32 and bf16, blank 0 and 3): the key is the plain scan's bit for bit,
the log-probabilities are torch.log_softmax's in float64 on the CPU of the values the kernel reads, skipped rows are not written, rows
without a finite log-sum-exp give NaN, and the advance is replayed beside the plain pair and against a Python restatement of its contract
in include/ttmi.h."""
import math

import pytest
import torch

from test_greedy_kernels_gpu import _argmax, _nonfinite_rows, _padded

pytestmark = pytest.mark.gpu

LP_POISON = 777.0          # what lp holds before a scan: rows the scan skips must still hold it


def _i32(values):
    return torch.tensor(values, dtype=torch.int32).cuda()


def _both_scans(logits, t, T_len, need, blank):
    """the plain scan and the _lp scan on the same inputs -> (plain key, _lp key, lp) as CPU tensors; lp starts out poisoned"""
    from ttmi import ops
    B, n, _ = logits.shape
    t, T_len, need = _i32(t), _i32(T_len), _i32(need)
    key0 = torch.full((B,), n << 32, dtype=torch.int64).cuda()
    key1 = key0.clone()
    lp = torch.full((B, n, 2), LP_POISON, dtype=torch.float32).cuda()
    ops.greedy_scan_batch(logits, t, T_len, need, key0, blank)
    ops.greedy_scan_batch_lp(logits, t, T_len, need, key1, lp, blank)
    return key0.cpu(), key1.cpu(), lp.cpu()


def _want_lp(row, blank):
    """float64 log_softmax on the CPU of the values the kernel reads -> (log P(blank), log P(argmax)); a blank outside the row: -inf"""
    x = row.detach().float().cpu().double()
    ls = torch.log_softmax(x, dim=0)
    return (float(ls[blank]) if blank < x.numel() else -math.inf), float(ls[_argmax(row)])


def _check_rows(logits, lp, t, T_len, need, blank, what):
    """every walked row within 1e-5 + 4 * 2^-23 * max|x| of the reference (the f32 error of x - (m + log sum exp(x - m)) is a few ulp of
    |x| plus about log2(V) ulp relative on the sum: below 3e-6 for |x| <= 16), every skipped row still poisoned; returns the largest error"""
    B, n, _ = logits.shape
    worst = 0.0
    for b in range(B):
        for r in range(n):
            got = lp[b, r].tolist()
            if not need[b] or t[b] + r >= T_len[b]:
                assert got == [LP_POISON, LP_POISON], (what, b, r, got)
                continue
            bound = 1e-5 + 4 * 2.0 ** -23 * float(logits[b, r].float().abs().max())
            for g, w in zip(got, _want_lp(logits[b, r], blank)):
                if math.isinf(w):
                    assert g == w, (what, b, r, got)
                else:
                    assert math.isfinite(g) and abs(g - w) <= bound, (what, b, r, g, w, bound)
                    worst = max(worst, abs(g - w))
            if _argmax(logits[b, r]) == blank:
                assert got[0] == got[1], (what, b, r, got)
    return worst


def _ragged(B, n):
    """t, T_len, need: B = 3: utterance 0 has all n frames, utterance 1's frames end inside the block (none exist for n = 1), utterance 2 has
    its symbol already (need = 0); B = 1: the utterance's frames end inside the block"""
    if B == 1:
        return [2], [2 + (n + 1) // 2], [1]
    return [2, 0, 1], [2 + n, n // 2, 1 + n], [1, 1, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("blank", [0, 3])
@pytest.mark.parametrize("V", [1, 5, 64, 65, 4334])
def test_scan_lp_key_and_log_probabilities(V, blank, dtype):
    """B in {1, 3} x n in {1, 5, 64}: randn rows scaled and clamped to |x| <= 16, the blank column raised on about half the rows so that blank
    and non-blank rows mix; then the same rows shifted by +1e4, which must stay finite (a missing max subtraction overflows exp)."""
    g = torch.Generator().manual_seed(1000 * V + blank)
    for B in (1, 3):
        for n in (1, 5, 64):
            rows = (4.0 * torch.randn(B, n, V, generator=g)).clamp_(-16.0, 16.0)
            if blank < V:
                rows[:, :, blank] += 6.0 * (torch.rand(B, n, generator=g) < 0.5)
                rows.clamp_(-16.0, 16.0)
            t, T_len, need = _ragged(B, n)
            for shift in (0.0, 1e4):
                logits = _padded(rows + shift, dtype)
                key0, key1, lp = _both_scans(logits, t, T_len, need, blank)
                assert torch.equal(key0, key1), (B, n, shift)
                worst = _check_rows(logits, lp, t, T_len, need, blank, (B, n, shift))
                print("V=%d blank=%d %s B=%d n=%d shift=%g: max |lp - ref| = %.3e" % (V, blank, str(dtype)[6:], B, n, shift, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [5, 65, 4334])
def test_scan_lp_rows_without_a_finite_log_sum_exp(V, dtype):
    """all -inf, all NaN, a NaN among finite values, +inf present, +inf and NaN: NaN in both entries, the key the plain kernel's.  -inf among
    finite values is an ordinary row (probability 0 for those entries): finite log-sum-exp, log P(blank) = -inf here (the blank is one of
    them)."""
    blank = 1
    cases = _nonfinite_rows(V)
    blank_row = torch.zeros(V); blank_row[blank] = 5.0
    logits = _padded(torch.stack([torch.stack([blank_row, r, blank_row]) for r in cases.values()]), dtype)      # [cases, 3, V]
    B = len(cases)
    key0, key1, lp = _both_scans(logits, [0] * B, [3] * B, [1] * B, blank)
    assert torch.equal(key0, key1)
    for b, name in enumerate(cases):
        assert (key1[b] >> 32) == 1 and int(key1[b] & 0xffffffff) == _argmax(logits[b, 1]), name
        if name == "-inf and finite":
            _check_rows(logits[b:b + 1], lp[b:b + 1], [0], [3], [1], blank, name)
            assert lp[b, 1, 0] == -math.inf and math.isfinite(lp[b, 1, 1])
        else:
            assert torch.isnan(lp[b, 1]).all(), (name, lp[b, 1])
            _check_rows(logits[b:b + 1, ::2], lp[b:b + 1, ::2], [0], [3], [1], blank, name)      # the finite rows around it are untouched by it


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,tied,blank", [
    (4334, [134, 70, 200], 0),               # 70 and 134 in one lane (64 apart), 200 in another
    (4334, [5, 69, 300], 5),                 # blank among the tied ones and the lowest: the row is blank, both entries equal
    (4334, [70, 3], 70),                     # blank tied, a lower index in another lane wins
    (65, [64, 63], 64)])
def test_scan_lp_ties_across_lanes(V, tied, blank, dtype):
    rows = torch.zeros(1, 3, V)
    rows[0, :, blank] = 1.0
    rows[0, 1, blank] = 0.0
    rows[0, 1, tied] = 0.5                   # exact in bf16
    logits = _padded(rows, dtype)
    key0, key1, lp = _both_scans(logits, [0], [3], [1], blank)
    assert torch.equal(key0, key1)
    _check_rows(logits, lp, [0], [3], [1], blank, tied)
    want = float(torch.log_softmax(logits[0, 1].float().cpu().double(), dim=0)[min(tied)])
    assert abs(float(lp[0, 1, 1]) - want) <= 1e-5 + 4 * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- the advance
def _advance_lp_model(key, n, lp, t, T_len, need, count, frames, tok_lp, score):
    """include/ttmi.h, ttmi_greedy_advance_lp: what the call adds to frames / tok_lp / score, from the state BEFORE it and the kernel's own lp,
    summed in row order in float64"""
    for b in range(len(key)):
        if not need[b]:
            continue
        row, t0, c = key[b] >> 32, t[b], count[b]
        if row < n:
            frames[b][c] = t0 + row
            tok_lp[b][c] = lp[b][row][1]
            for r in range(row):
                score[b] += lp[b][r][0]
            score[b] += lp[b][row][1]
        else:
            for r in range(n):
                if t0 + r < T_len[b]:
                    score[b] += lp[b][r][0]


def _replay(dtype, blank):
    """the host loop of Transducer.decode_batch in miniature, as test_batched_greedy_decode_state_machine runs it (n = 4, T = 12, V = 29, the
    blank column biased), with the plain pair and the _lp pair side by side on their own state"""
    from ttmi import ops
    B, n, T, V = 5, 4, 12, 29
    T_list = [12, 0, 3, 8, 5]                                            # ragged; utterance 1 has no frames at all
    g = torch.Generator().manual_seed(17 + blank)
    tables = torch.randn(2, B, T, V, generator=g)
    tables[:, :, :, blank] += 2.0
    tables[:, 3, :, blank] += 100.0                                      # utterance 3 is blank throughout: full and partial blocks without a symbol
    tables[:, 0, T_list[0] - 1, (blank + 1) % V] += 100.0                # utterance 0 emits on its last frame
    poison = torch.zeros(V); poison[(blank + 5) % V] = 1000.0

    def state():
        return dict(t=_i32([0] * B), need=_i32([1] * B), done=_i32([0] * B), count=_i32([0] * B), flags=_i32([0, 0]),
                    key=torch.full((B,), n << 32, dtype=torch.int64).cuda(), hist=torch.zeros(B, T + 2, dtype=torch.long).cuda())
    p, q = state(), state()
    T_len = _i32(T_list)
    ld_det = T + 1
    frames = torch.full((B, ld_det), -7, dtype=torch.int32).cuda()
    tok_lp = torch.full((B, ld_det), LP_POISON, dtype=torch.float32).cuda()
    score = torch.zeros(B, dtype=torch.float64).cuda()
    m_frames, m_lp, m_score = [[-7] * ld_det for _ in range(B)], [[LP_POISON] * ld_det for _ in range(B)], [0.0] * B
    n_hist, scans, blocks_per_symbol = 1, 0, []
    while True:
        for s in (p, q):
            torch.sub(1, s["done"], out=s["need"])
        blocks = 0
        while True:
            t_now, need_now, count_now = p["t"].tolist(), p["need"].tolist(), p["count"].tolist()
            blk = torch.empty(B, n, V)
            for b in range(B):
                for r in range(n):
                    f = t_now[b] + r
                    blk[b, r] = tables[n_hist % 2, b, f] if (need_now[b] and f < T_list[b]) else poison
            logits = _padded(blk, dtype)
            lp = torch.full((B, n, 2), LP_POISON, dtype=torch.float32).cuda()
            ops.greedy_scan_batch(logits, p["t"], T_len, p["need"], p["key"], blank)
            ops.greedy_scan_batch_lp(logits, q["t"], T_len, q["need"], q["key"], lp, blank)
            assert torch.equal(p["key"], q["key"]), ("scan", n_hist, scans)
            _advance_lp_model(q["key"].tolist(), n, lp.double().tolist(), t_now, T_list, need_now, count_now, m_frames, m_lp, m_score)
            ops.greedy_advance(p["key"], n, n_hist, p["hist"], p["t"], T_len, p["need"], p["done"], p["count"], p["flags"])
            ops.greedy_advance_lp(q["key"], n, n_hist, q["hist"], q["t"], T_len, q["need"], q["done"], q["count"], q["flags"], lp, frames, tok_lp,
                                  score)
            scans += 1
            blocks += 1
            for name in p:
                assert torch.equal(p[name], q[name]), (name, n_hist, scans)
            assert frames.tolist() == m_frames, (n_hist, scans)
            assert tok_lp.double().tolist() == m_lp, (n_hist, scans)
            for got, want in zip(score.tolist(), m_score):
                assert abs(got - want) <= 1e-12 * abs(want), (n_hist, scans, got, want)
            pending, alive = q["flags"].tolist()
            if pending == 0:
                break
        blocks_per_symbol.append(blocks)
        if alive == 0:
            break
        n_hist += 1
        assert n_hist <= T + 1
    counts = q["count"].tolist()
    assert max(blocks_per_symbol) > 1                                    # an utterance needed several blocks for one symbol
    assert counts[1] == 0 and counts[3] == 0 and m_score[1] == 0.0 and m_score[3] <= 0.0 and counts[0] >= 1
    assert m_frames[0][counts[0] - 1] == T_list[0] - 1                   # utterance 0's last symbol sits on its last frame
    for b in range(B):
        fr = m_frames[b][:counts[b]]
        assert all(a < c for a, c in zip(fr, fr[1:])) and all(0 <= f < T_list[b] for f in fr), (b, fr)
        assert m_frames[b][counts[b]:] == [-7] * (ld_det - counts[b])    # nothing written beyond the symbols emitted
        assert all(math.isfinite(v) and v <= 0.0 for v in m_lp[b][:counts[b]]) and math.isfinite(m_score[b])
    return frames.cpu(), tok_lp.cpu(), score.cpu(), q["hist"].cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("blank", [0, 2])
def test_advance_lp_state_machine(blank, dtype):
    """B = 5, ragged lengths (12, 0, 3, 8, 5), blocks of n = 4 frames.  After every scan the two keys are compared, after every advance every
    old state word (t, need, done, count, flags, key, hist) with the plain pair's and frames / tok_lp / score with the restatement of the
    contract on the kernel's own lp values: exact for frames and tok_lp, 1e-12 relative for the f64 score.  A second run gives the same bits."""
    first = _replay(dtype, blank)
    second = _replay(dtype, blank)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert first[2].dtype is torch.float64
