"""The attention row reference of tests/attn_oracle.py checks itself on the CPU: its exact form against oracle.tt_oracle (which the golden
fixtures pin), its inputs' preconditions at every GPU case, its tolerances against the reference gaps they are derived from, and - the
condition of sensitivity - that the defects the row-wise GPU test exists for (a wrong shift seam, a wrong table clamp, a wrong mask edge,
another utterance's mask, one lost key) each move a row by at least twice the loosest bound that row is held to."""
import numpy as np
import pytest
import torch

import attn_oracle as R
from oracle import tt_oracle as O

PARAMS = ("qkv_w", "o_w", "ln_g", "ln_b", "r_emb", "r_w_bias", "r_bias")


def _tt_oracle(case, m, drop):
    p = {k: case[k].numpy() for k in PARAMS}
    if drop is not None:
        p["drop_attn"] = np.asarray(drop).reshape(case["x"].shape)
    y, cache = O.rel_attn_fwd(case["x"].numpy(), p, None if m is None else np.transpose(m, (1, 2, 0)))
    dx, g = O.rel_attn_bwd(case["dy"].numpy(), cache, p)
    d = case["d"]
    return dict(y=y.reshape(-1, d), dx=dx.reshape(-1, d), g_qkv_w=g["qkv_w"], g_o_w=g["o_w"], g_ln_g=g["ln_g"], g_ln_b=g["ln_b"], g_r_emb=g["r_emb"],
                g_r_w_bias=g["r_w_bias"].reshape(-1), g_r_bias=g["r_bias"].reshape(-1))


@pytest.mark.parametrize("B,H,Dh,L,K,mask,family,p", [
    (2, 2, 64, 65, 200, "causal", "mixed", 0.0), (3, 2, 64, 129, 16, "pu_chunk_pad", "mixed", 0.1), (2, 3, 12, 33, 20, "band", "planted", 0.0),
    (3, 4, 32, 70, 64, "pu_keypad", "mixed", 0.1), (2, 2, 64, 1, 200, "none", "mixed", 0.0), (2, 4, 16, 40, 40, "holes", "planted", 0.1),
    (2, 2, 64, 130, 200, "iv", "planted", 0.0)])
def test_exact_form_equals_the_pinned_oracle(B, H, Dh, L, K, mask, family, p):
    case = R.attn_case(B, H, Dh, L, K, family, 5 + L)
    m, _ = R.mask_of(mask, L, B)
    drop = R.cpu_drop(R.Case(B, H, Dh, L, K, mask, family, 0, p, None))
    got = R.attn_ref(case, m, drop)
    for k, (e_max, _) in R.errors(got, _tt_oracle(case, m, drop)).items():
        assert e_max < 1e-12, (k, e_max)
    shifted = R.attn_ref(case, m, drop, p_shift=R.P_SHIFT)                     # exact arithmetic does not depend on where the exponentials are taken
    assert max(v[0] for v in R.errors(shifted, got).values()) < 1e-12
    n = R.unused_table_rows(L, K)
    assert not got["g_r_emb"][:n * H].any() and not got["g_r_bias"][:n * H].any()


def test_cases_cover_what_the_issue_lists():
    cs = R.CASES
    assert len(cs) == len(set(cs))
    fused = [c for c in cs if R.rounding_of(c) == "fused" and c.Dh == 64 and c.family == "mixed" and c.opt is None and c.p == 0]
    for mask in ("none", "causal"):
        assert {c.L for c in fused if c.mask == mask and c.K == 200} >= set(R.EDGE)
    assert {(c.L, c.K) for c in fused} >= {(65, 16), (513, 700), (577, 700), (449, 64), (577, 200)}
    for mask in ("band", "bytes_chunk", "holes", "iv", "iv_reach") + R.PER_UTTERANCE:
        assert {c.L for c in fused if c.mask == mask} >= set(R.SUB), mask
    assert all(c.B == 3 for c in cs if c.mask.startswith("pu_") or (c.opt and c.opt[0] == 10))
    planted = [c for c in cs if c.prec == 1 and c.family == "planted" and c.Dh == 64]
    assert {(c.L, c.mask) for c in planted} >= {(L, m) for L in R.SUB for m in ("none", "causal", "band", "iv_reach")} | {(64, "none"), (128, "none")}
    assert {c.L for c in planted if c.mask == "causal"} >= {L for L in R.EDGE if 2 <= L <= 129}
    assert {(c.L, c.mask, c.family) for c in cs if c.Dh == 32} == {(L, m, f) for L in (33, 65, 129, 200, 513) for m in ("none", "causal", "band") for f in R.FAMILIES}
    assert {(c.opt[:2], c.L, c.mask) for c in cs if c.opt} == {(o[:2], L, m) for o in R.SWITCHES for L in (129, 257, 513) for m in ("none", "band")}
    assert {(c.prec, c.L) for c in cs if c.p > 0} == {(prec, L) for prec in (0, 1) for L in (129, 257, 513)}
    for prec in (0, 2):
        assert {(c.L, c.mask, c.family) for c in cs if c.prec == prec and c.p == 0} == \
            {(L, m, f) for L in (1, 2, 65, 129, 257, 513) for m in ("none", "causal", "band", "holes", "pu_keypad") for f in R.FAMILIES}
    assert {R.rounding_of(c) for c in cs} == {None, "fused", "operands", "fast-unfused"}
    for form in ("operands", "fast-unfused"):
        assert {(c.L, c.mask) for c in cs if R.rounding_of(c) == form} == {(L, m) for L in (33, 129, 257) for m in ("none", "causal")}


def test_every_gpu_case_meets_its_preconditions():
    keys = sorted({R.input_key(c) for c in R.CASES})
    assert len(keys) >= 150
    for key in keys:
        case, m, spec = R.cached_case(*key)                                     # asserts the family's preconditions itself
        info = case["info"]
        if key[6] == "mixed":
            assert 0.5 <= info["branch"] <= 2
            assert key[3] < 16 or (0.5 <= info["ac_bd"] <= 2 and 2 <= info["n_eff"] <= key[3] / 2)
        else:
            assert key[3] < 16 or (info["n_probes"] >= 8 and info["min_partner_p"] >= R.MIN_PARTNER_P), (key, info)


def test_planted_probes_sit_on_the_seams():
    for L in (64, 65, 129, 513):
        keys = {j for _, j in R._probe_pairs(L)}
        want = {0, L - 1} | {j for t in range(1, L // 64 + 1) for j in (64 * t - 1, 64 * t) if j < L}
        assert want <= keys, (L, sorted(want - keys))
        own = [(i, j) for i, j in R._probe_pairs(L) if j - i in (1, 2)]
        assert len(own) == 8 and len({i for i, _ in own}) == 4
        rows = [t for pair in R._probe_pairs(L) for t in pair if pair[1] - pair[0] not in (1, 2)]
        assert len(rows) == len(set(rows))                                      # no row is both a source and a copy


@pytest.mark.parametrize("H,Dh,form", [(2, 64, "fused"), (4, 32, "fused"), (4, 16, "fast-unfused"), (3, 12, "operands")])
def test_rounding_forms_round(H, Dh, form):
    """each bf16 form differs from the exact one by bf16-sized amounts - neither equal to it nor off by more than roundings explain - and its
    float32 run stays close to its float64 run"""
    case, m, _ = R.cached_case(2, H, Dh, 129, 200, "causal", "mixed")
    assert R.rounding_of(R.Case(2, H, Dh, 129, 200, "causal", "mixed", 1, 0.0, None)) == form
    exact = R.attn_ref(case, m)
    e = R.errors(R.attn_ref(case, m, None, form), exact)
    for k in ("y", "dx", "g_qkv_w", "g_o_w"):
        assert 2.0 ** -12 < e[k][0] < 2.0 ** -4, (form, k, e[k])
    e32 = R.errors(R.attn_ref(case, m, None, None, torch.float32), exact)
    assert max(v[0] for v in e32.values()) < R.TOL_EXACT / 10, e32             # 1e-4 is a contract, not a fit: float32 itself is far inside it


def test_exact_cases_leave_the_contract_room():
    """prec 0 / prec 2 are held to 1e-4 on every row and element.  That is a contract only where plain float32 arithmetic sits well inside
    it - the bf16x3 mode's three-term products carry about ten times float32's error on the longer stacks: at every such case the float32
    run of the exact reference stays within a fifth of the bound of its float64 run on every row and element (measured: 8.2e-6 at worst on
    `mixed`, 1.1e-5 on `planted`).  An input that fails this is ill-conditioned, whatever a kernel makes of it: `planted` with a white dy
    was (2.7e-5; the diagonal's entry of g_r_bias a sum that cancelled 160-fold), and the bf16x3 mode then missed 1e-4 on that entry."""
    keys = sorted({(R.input_key(c), c.p) for c in R.CASES if c.prec != 1})
    assert len(keys) >= 60
    worst = {}
    for key, p in keys:
        case, m, _ = R.cached_case(*key)
        drop = R.cpu_drop(R.Case(*key, 0, p, None))
        e = R.errors(R.attn_ref(case, m, drop, None, torch.float32), R.attn_ref(case, m, drop))
        k = max(e, key=lambda n: e[n][0])
        assert e[k][0] <= R.TOL_EXACT / 5, (key, k, e[k][0])
        worst[key[6]] = max(worst.get(key[6], 0.0), e[k][0])
    print("float32 run of the exact reference, worst row or element:", worst)


_gaps = {}


def _reference_gaps():
    if not _gaps:
        by_input = {}
        for c in R.CASES:
            if c.prec == 1:
                key = (R.input_key(c), c.p)                                     # (the switches' cases share their inputs, masks and form)
                if key not in by_input:
                    by_input[key] = R.reference_gap(c)
                _gaps[c] = by_input[key]
    return _gaps


def test_tolerances_are_tied_to_the_reference():
    """TOL_MAX and TOL_Q90 are 4 x the reference's own uncertainty G over every prec-1 case, per input family and output class: re-measured
    here, so that no constant can drift from the reference it bounds."""
    gaps = _reference_gaps()
    assert set(gaps) == {c for c in R.CASES if c.prec == 1}                     # no case excluded
    g_max, g_q90 = R.gap_summary(gaps)
    for f in R.FAMILIES:
        print(f, "G_max", {k: "%.3e" % v for k, v in g_max[f].items()}, "G_q90", {k: "%.3e" % v for k, v in g_q90[f].items()})
    for f in R.FAMILIES:
        for k in R.CLASSES:
            assert 2 * g_max[f][k] <= R.TOL_MAX[f][k] <= 8 * g_max[f][k], (f, k, g_max[f][k], R.TOL_MAX[f][k])
            assert 2 * g_q90[f][k] <= R.TOL_Q90[f][k] <= 8 * g_q90[f][k], (f, k, g_q90[f][k], R.TOL_Q90[f][k])
            assert R.TOL_Q90[f][k] <= R.TOL_MAX[f][k]
    assert R.TOL_MAX["mixed"]["y"] <= 2e-2 and R.TOL_MAX["planted"]["y"] <= 2e-2   # larger: a rounding point is missing from the reference
    assert R.TOL_EXACT == 1e-4


# ------------------------------------------------------------------------------------------------------------ the condition of sensitivity
def _moved(bad, want, rows):
    """{output: worst of rowwise_err over the affected rows}"""
    e = R.row_errors(bad, want)
    return {k: float(e[k][rows[k]].max()) if k in rows else float(e[k].max()) for k in R.OUTPUTS}


def _assert_detected(what, family, moved):
    ratio = {k: v / R.TOL_MAX[family][R.CLASS_OF[k]] for k, v in moved.items()}
    best = max(ratio, key=ratio.get)
    print("%s: %s moves by %.2e = %.1f x TOL_MAX" % (what, best, moved[best], ratio[best]))
    assert ratio[best] >= 2, (what, moved)


@pytest.mark.parametrize("H,Dh,L", [(2, 64, 65), (2, 64, 257), (2, 64, 513), (4, 32, 129)])
def test_fault_1_a_row_that_shifts_its_own_upper_part_is_seen(H, Dh, L):
    case, m, _ = R.cached_case(2, H, Dh, L, 200, "none", "mixed")
    want = R.attn_ref(case, m)
    i0 = L // 3
    bad = R.attn_ref(case, m, fault=("shift_row", i0))
    rows = [b * L + i0 for b in range(2)]
    assert max(R.row_errors(bad, want)["y"][[r for r in range(2 * L) if r not in rows]]) == 0       # one query row, nothing else, in the forward pass
    _assert_detected("own row's upper shift part at L %d Dh %d" % (L, Dh), "mixed", _moved(bad, want, dict(y=rows, dx=rows)))


@pytest.mark.parametrize("L,K", [(257, 200), (513, 200), (449, 64), (65, 16)])
def test_fault_2_a_table_clamp_off_by_one_is_seen(L, K):
    case, m, _ = R.cached_case(2, 2, 64, L, K, "none", "mixed")
    want = R.attn_ref(case, m)
    _assert_detected("e(p) off by one at L %d K %d" % (L, K), "mixed", _moved(R.attn_ref(case, m, fault=("table", 1)), want, {}))


@pytest.mark.parametrize("L", [2, 3, 63, 64, 65, 127, 128, 129])
def test_fault_3_the_last_row_under_the_previous_rows_causal_mask_is_seen(L):
    assert R.Case(2, 2, 64, L, 200, "causal", "planted", 1, 0.0, None) in R.CASES
    case, m, _ = R.cached_case(2, 2, 64, L, 200, "causal", "planted")
    want = R.attn_ref(case, m)
    bad_mask = m.copy()
    bad_mask[:, L - 1] = m[:, L - 2]
    rows = [b * L + L - 1 for b in range(2)]
    _assert_detected("last row's mask at L %d" % L, "planted", _moved(R.attn_ref(case, bad_mask), want, dict(y=rows, dx=rows)))


@pytest.mark.parametrize("family", R.PER_UTTERANCE)
@pytest.mark.parametrize("L", [65, 257, 513])
def test_fault_4_another_utterances_mask_on_one_row_is_seen(L, family):
    case, m, _ = R.cached_case(3, 2, 64, L, 200, family, "mixed")
    want = R.attn_ref(case, m)
    differ = np.flatnonzero((m[0] != m[1]).any(-1))
    assert len(differ)
    r = int(differ[len(differ) // 2])
    bad_mask = m.copy()
    bad_mask[1, r] = m[0, r]
    rows = [L + r]
    _assert_detected("utterance 0's mask on row %d of utterance 1, %s at L %d" % (r, family, L), "mixed",
                     _moved(R.attn_ref(case, bad_mask), want, dict(y=rows, dx=rows)))


def test_fault_5_every_probes_lost_key_is_seen():
    """`planted`: one probe's partner key dropped in a single (b, h, i), for every probe pair, head and batch entry of every prec-1 case"""
    keys = sorted({R.input_key(c) for c in R.CASES if c.family == "planted" and c.prec == 1})
    assert len(keys) >= 40
    weakest = {}
    for n, key in enumerate(keys):
        B, H, Dh, L = key[:4]
        case, m, _ = R.cached_case(*key)
        cache = {}
        want = R.attn_ref(case, m, cache=cache)
        drops = [(b, h, i, j) for b, i, j in R.directed_probes(case, m) for h in range(H)]
        assert len(drops) >= 8 * H or L < 16
        if not drops:
            continue                                                            # (two and three rows: no room for a pair 5 rows apart)
        y = R.y_rows_without_a_key(case, cache, drops)
        ref = want["y"].reshape(B, L, -1)
        rms = float(want["y"].pow(2).mean().sqrt()) * ref.shape[-1] ** 0.5
        for (b, h, i, j), row in zip(drops, y):
            moved = float((row - ref[b, i]).norm() / max(float(ref[b, i].norm()), rms))          # ffn_oracle.rowwise_err of that row
            weakest[key] = min(weakest.get(key, moved), moved)
        if n % 9 == 0:                                                          # the short cut equals the reference run under the same mask
            b, h, i, j = drops[len(drops) // 2]
            full = np.broadcast_to((np.zeros((1, L, L), dtype=bool) if m is None else m)[:, None], (B, H, L, L)).copy()
            full[b, h, i, j] = True
            again = R.attn_ref(case, full)["y"].reshape(B, L, -1)[b, i]
            assert float((again - y[len(drops) // 2]).abs().max()) < 1e-10
    worst = min(weakest, key=weakest.get)
    print("weakest single-key drop: %.2e at %s (2 x TOL_MAX = %.2e)" % (weakest[worst], worst, 2 * R.TOL_MAX["planted"]["y"]))
    assert weakest[worst] >= 2 * R.TOL_MAX["planted"]["y"], (worst, weakest[worst])
