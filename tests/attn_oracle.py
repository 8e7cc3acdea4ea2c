"""Row-by-row reference of the relative-position attention sub-layer (tt/transformer.py RelLearnableMultiHeadAttn):

    q, k, v = x Wqkv^T;  S = ((q + u) k^T + shift(q E^T + c)) / sqrt(Dh), masked;  P = softmax(S);  O = P v;  a = drop(O Wo^T);  y = LN(x + a)

forward and every gradient of ttmi_attn_bwd, in plain torch on the CPU and without the library.  Like tests/ffn_oracle.py it can round where
the library's bf16 data flows round (`rounding`), so that a whole-row comparison is meaningful in bf16 too, and it runs in float32 as well as
float64.  The one rounding no reference can reproduce - the forward kernels round exp(s - m) to bf16 at a running maximum m that is raised
lazily - is bracketed by `p_shift`: two placements of that rounding grid are two equally valid references, and the prec-1 tolerances below
are derived from their distance and from the float32-to-float64 distance of the same form (tests/test_attn_oracle.py re-measures both).
Used by tests/test_attn_oracle.py (CPU) and tests/test_attn_rows_gpu.py."""
import collections
import functools

import numpy as np
import torch

import mask_cases as MC
from ffn_oracle import _bf16, _ln_stats, ln_bwd_rows, rowwise_err
from oracle import tt_oracle as O

OUTPUTS = ("y", "dx", "g_qkv_w", "g_o_w", "g_ln_g", "g_ln_b", "g_r_emb", "g_r_w_bias", "g_r_bias")
CLASS_OF = dict(y="y", dx="dx", g_qkv_w="weights", g_o_w="weights", g_ln_g="tables", g_ln_b="tables", g_r_emb="tables", g_r_w_bias="tables",
                g_r_bias="tables")
CLASSES = ("y", "dx", "weights", "tables")
P_SHIFT = 0.37              # the second placement of the forward kernels' bf16 rounding of exp(s - m)
MIN_PARTNER_P = 0.05        # `planted`: every unmasked probe pair's probability, every head and batch entry
BAND = (20, 3)              # mask kind 2: context_mask(L, left, right)
CHUNK = (16, 64)            # the chunk mask behind the byte and interval-table cases: chunk_mask(L, chunk, left)

# ---- tolerances.  prec 0 (exact f32) and prec 2 (bf16x3): the project's parity contract (README: within 1e-4 of the float64 oracle), applied to
# every row and element instead of the whole tensor.
TOL_EXACT = 1e-4
# prec 1, every rounding form: 4 x G per input family and output class (y | dx | the two weight gradients | table, bias and LayerNorm gradients),
# G = the larger of (this reference in float32 against the same form in float64) and (the reference at p_shift 0 against p_shift 0.37), worst row
# (G_max) and worst 90 % quantile (G_q90) over every prec-1 case of CASES.  The factor 4 is tests/ffn_oracle.py's: the kernels sum in another
# order than torch's CPU matmul and land on other bf16 round-to-nearest ties.  Per family as well as per class, because `planted` is built to be
# ill-conditioned where `mixed` is not: a row and its copy are each other's strongest keys with gradients of opposite sign, so dq = dS k cancels
# to ~ 1 / 7 of its terms (G on dx 3.2e-2 against 1.4e-2).  One bound per class over both families would hand `mixed` the bounds of `planted`.
# test_attn_oracle.py::test_tolerances_are_tied_to_the_reference re-measures G and holds 2 G <= TOL <= 8 G.  Measured:
#   mixed    G_max  y 3.71e-3 (L 513 band)     dx 1.39e-2 (L 257 causal)      weights 2.04e-2 (g_qkv_w, L 3)           tables 1.66e-1 (g_r_bias, L 2 causal)
#            G_q90  y 2.56e-3 (L 2)            dx 6.77e-3 (L 3)               weights 9.67e-3 (g_qkv_w, L 2)           tables 5.38e-2 (g_r_w_bias, L 2)
#   planted  G_max  y 3.76e-3 (L 449 causal)   dx 3.17e-2 (Dh 32, L 200 band) weights 2.05e-2 (g_qkv_w, Dh 32, L 33)   tables 2.78e-1 (g_r_bias, L 513 band)
#            G_q90  y 2.65e-3 (L 65 band)      dx 1.35e-2 (Dh 32, L 200 band) weights 1.22e-2 (g_qkv_w, Dh 32, L 33)   tables 7.58e-2 (g_r_w_bias, L 193 interval table)
# every one of them the p_shift distance (the float32 run of a form is within 1e-3 of its float64 run on the rows of y and dx).  The sequences of
# two and three rows set the gradient bounds of `mixed`: six rows of data under every sum.
G_MAX = dict(mixed=dict(y=3.71e-3, dx=1.39e-2, weights=2.04e-2, tables=1.66e-1), planted=dict(y=3.76e-3, dx=3.17e-2, weights=2.05e-2, tables=2.78e-1))
G_Q90 = dict(mixed=dict(y=2.56e-3, dx=6.77e-3, weights=9.67e-3, tables=5.38e-2), planted=dict(y=2.65e-3, dx=1.35e-2, weights=1.22e-2, tables=7.58e-2))
TOL_MAX = {f: {k: 4 * v for k, v in g.items()} for f, g in G_MAX.items()}
TOL_Q90 = {f: {k: 4 * v for k, v in g.items()} for f, g in G_Q90.items()}
FAMILIES = ("mixed", "planted")

# B, H, Dh, L, K: sizes (d = H * Dh);  mask: a name of mask_of;  family: "mixed" | "planted";  prec: 0 | 1 | 2;  p: dropout;
# opt: (key, value, default) of ttmi_set_option for the case, or None
Case = collections.namedtuple("Case", "B H Dh L K mask family prec p opt")

EDGE = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 449, 511, 512, 513, 577, 641)
SUB = (65, 129, 193, 257, 449, 513)
PER_UTTERANCE = tuple("pu_" + f for f in MC.FAMILIES)
# the remaining switches of the attention path (csrc/layers.hip ttmi_set_option), one at a time: (key, value, default)
SWITCHES = ((10, 2, 1), (14, 0, 1), (15, 1, 2), (11, 1, 0), (16, 1, 0), (8, 0, 1))


def _cases():
    out = []

    def add(L, K, mask, family, prec=1, B=2, H=2, Dh=64, p=0.0, opt=None):
        out.append(Case(B, H, Dh, L, K, mask, family, prec, p, opt))

    for L in EDGE:                                                   # prec 1 fused, Dh 64: K = 200 gives both table branches (L <= K, L > K)
        for mask in ("none", "causal"):
            add(L, 200, mask, "mixed")
    for L, K in ((65, 16), (513, 700), (577, 700), (449, 64), (577, 200)):      # the last two: L - K >= 256, no direct table folding
        if Case(2, 2, 64, L, K, "none", "mixed", 1, 0.0, None) not in out:
            add(L, K, "none", "mixed")
    add(577, 200, "band", "mixed")                                   # ((577, 200) without a mask is one of EDGE's: the route again under a band)
    for L in SUB:                                                    # every mask form; the band at 449 / 513 takes the backward's query-tile skipping
        for mask in ("band", "bytes_chunk", "holes", "iv", "iv_reach"):
            add(L, 200, mask, "mixed")
        for mask in PER_UTTERANCE:
            add(L, 200, mask, "mixed", B=3)
    for L in SUB + (64, 128):
        for mask in ("none", "causal", "band", "iv_reach"):
            if L in SUB or mask == "none":
                add(L, 200, mask, "planted")
    for L in (2, 3, 63, 64, 127, 128):                               # the last row's own key, the strongest it has under `planted`, at every tile tail up to 129
        add(L, 200, "causal", "planted")
    for L in (33, 65, 129, 200, 513):                                # Dh 32: the <32> kernels, dq / dE by the GEMM launches
        for mask in ("none", "causal", "band"):
            for family in ("mixed", "planted"):
                add(L, 200, mask, family, H=4, Dh=32)
    for opt in SWITCHES:
        for L in (129, 257, 513):
            for mask in ("none", "band"):
                add(L, 200, mask, "mixed", B=3 if opt[0] == 10 else 2, opt=opt)
    for L in (129, 257, 513):                                        # dropout on the attention output
        for prec in (0, 1):
            add(L, 200, "none", "mixed", prec=prec, p=0.1)
    for prec in (0, 2):
        for L in (1, 2, 65, 129, 257, 513):
            for mask in ("none", "causal", "band", "holes", "pu_keypad"):
                for family in ("mixed", "planted"):
                    add(L, 200, mask, family, prec=prec, B=3 if mask.startswith("pu_") else 2)
    for H, Dh in ((3, 12), (4, 16)):                                 # "operands" and "fast-unfused"
        for L in (33, 129, 257):
            for mask in ("none", "causal"):
                add(L, 200, mask, "mixed", H=H, Dh=Dh)
    assert len(out) == len(set(out))
    return out


CASES = _cases()


def case_id(c):
    return "B%d-H%dx%d-L%d-K%d-%s-%s-prec%d%s%s" % (c.B, c.H, c.Dh, c.L, c.K, c.mask, c.family, c.prec, "-p%g" % c.p if c.p else "",
                                                    "-opt%d=%d" % c.opt[:2] if c.opt else "")


def input_key(c):
    """what the inputs and the masks depend on"""
    return (c.B, c.H, c.Dh, c.L, c.K, c.mask, c.family)


def case_seed(c):
    return (c.L * 7919 + c.K * 104729 + c.H * 1299709 + c.Dh * 15485863 + c.B * 31 + (7 if c.family == "planted" else 0)) & 0x7FFFFFFF


def rounding_of(c):
    """the reference form that describes mode `prec` at this shape (csrc/layers.hip attn_fast, csrc/attn_flash.hip flash_supported)"""
    d = c.H * c.Dh
    if c.prec != 1:
        return None
    if not (d % 8 == 0 and c.Dh % 4 == 0):
        return "operands"
    return "fused" if c.Dh in (32, 64) else "fast-unfused"


# ------------------------------------------------------------------------------------------------------------------------------ masks
def mask_of(name, L, B):
    """-> (bool [B | 1, L, L], True = masked, or None;  spec) with spec what the C ABI is handed:
    (kind, left, right, tensor or None): kind 3 a uint8 array [B | 1, L | 1, L], kind 4 an int32 array [B | 1, L, 2] of (lo, hi)."""
    if name == "none":
        return None, (0, 0, 0, None)
    if name == "causal":
        return O.look_ahead_mask(L)[None], (1, 0, 0, None)
    if name == "band":
        return O.context_mask(L, *BAND)[None], (2,) + BAND + (None,)
    if name == "bytes_chunk":
        m = O.chunk_mask(L, *CHUNK)[None]
        return m, (3, 0, 0, m.astype(np.uint8))
    if name == "holes":
        m = np.ascontiguousarray(MC.per_row(MC.holes(L, 1, seed=L), 1, L))
        return m, (3, 0, 0, m.astype(np.uint8))
    if name in ("iv", "iv_reach"):
        ref = O.chunk_mask(L, *CHUNK)[:, :, None]
        lo, hi, interval = MC.row_intervals(ref, 1, L)
        assert interval
        left, right = MC.reach(lo, hi) if name == "iv_reach" else (-1, -1)
        return np.ascontiguousarray(MC.per_row(ref, 1, L)), (4, left, right, np.stack([lo, hi], -1).astype(np.int32))
    assert name.startswith("pu_"), name
    family = name[3:]
    if L >= 3:
        ref, _ = MC.build(family, L, B)
    else:                                                            # mask_cases.lengths starts at L = 3
        assert family == "keypad"
        ref = MC.key_padding(L, [L, 1, L, 1][:B])
    m = np.ascontiguousarray(MC.per_row(ref, B, L))
    if family == "keypad":
        return m, (3, 0, 0, np.ascontiguousarray(m[:, :1, :]).astype(np.uint8))
    if family in MC.INTERVAL_FAMILIES:
        lo, hi, interval = MC.row_intervals(ref, B, L)
        assert interval
        return m, (4,) + MC.reach(lo, hi) + (np.stack([lo, hi], -1).astype(np.int32),)
    return m, (3, 0, 0, m.astype(np.uint8))


# ----------------------------------------------------------------------------------------------------------------------------- inputs
def _probe_pairs(L):
    """`planted`: (source i, copy j) with x_j = x_i + small noise.  The copies sit where tiles and the shift have seams: key 0, key L - 1, the
    last key of every 64-key tile and the first key of the next, each 5 rows from its source (inside the band of BAND from one side), and for
    four query rows their own keys i + 1 and i + 2 (the zero and the first upper entry of the shifted position term)."""
    used, pairs = set(), []

    def take(i, j):
        if 0 <= i < L and 0 <= j < L and i != j and i not in used and j not in used:
            pairs.append((i, j))
            return True
        return False

    targets = [0, L - 1] + [j for t in range(1, L // 64 + 1) for j in (64 * t - 1, 64 * t)]
    seam = set(targets)
    for j in targets:
        for i in (j + 5, j - 5, j + 7, j - 7):
            if i not in seam and take(i, j):
                used.update((i, j))
                break
    for r in ([10, 26, L // 2 + 3, L - 20] if L >= 64 else [8, 14, 20, 26]):
        while r + 2 < L and any(t in used or t in seam for t in (r, r + 1, r + 2)):      # (the next free triple)
            r += 1
        if r + 2 < L:
            pairs += [(r, r + 1), (r, r + 2)]
            used.update((r, r + 1, r + 2))
    return pairs


def attn_case(B, H, Dh, L, K, family, seed):
    """float64 inputs of one case: x, dy [B, L, d] and the seven parameters; `planted` adds probes: the list of (i, j) pairs"""
    assert family in ("mixed", "planted")
    g = torch.Generator().manual_seed(seed)
    d = H * Dh

    def n(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    c = dict(B=B, H=H, Dh=Dh, L=L, K=K, d=d, family=family, seed=seed)
    c["dy"] = n(B, L, d)
    c["ln_g"] = 1 + 0.1 * n(d)
    c["ln_b"] = 0.1 * n(d)
    wv = n(H * Dh, d) / d ** 0.5
    c["o_w"] = (2.0 if family == "mixed" else 3.0) * n(d, H * Dh) / (H * Dh) ** 0.5      # the attention branch is not drowned by the residual
    if family == "mixed":
        # every row its own spread (0.7 ... 1.4) and mean: a row that took a neighbour's statistics, keys or table rows must not pass for itself
        c["x"] = n(B, L, d) * 2.0 ** (torch.rand(B, L, 1, generator=g, dtype=torch.float64) - 0.5) + 0.3 * n(B, L, 1)
        wq, wk = 1.2 * n(H * Dh, d) / d ** 0.5, 1.2 * n(H * Dh, d) / d ** 0.5
        c["r_emb"] = 1.2 * n(K, H, Dh)
        c["r_bias"] = 0.5 * n(K, H)
        c["r_w_bias"] = 0.3 * n(H, Dh)
        c["probes"] = []
    else:
        # content-dominated.  Every head's slice of a row is x_h = Q1 a + Q2 f in an orthogonal basis (Q1 | Q2) of that head, Dh / 2 columns each;
        # Wq and Wk project onto Q1 (0.95 Q1 Q1^T per head + 0.01 noise), Wv reads everything.  |a|^2 = 10 sqrt(Dh) in every row and head, so a
        # row's score with itself is ~ 9 at every Dh (~ 3 below 16 rows).  A copy j of a row i has a_j = a_i turned by ~ 27 degrees (the norm kept): the pair's
        # scores stay within 1 of a row's own, in both directions - and a part f of its own, so that its VALUE is another row's: a copy that
        # repeated its source's value could be lost without moving O.
        assert Dh % 2 == 0
        hd = Dh // 2
        r2 = (10.0 if L >= 16 else 10.0 / 3) * Dh ** 0.5            # (a handful of keys: a score of ~ 3, or the softmax is one-hot and every gradient behind it a rounding residue)
        Q = torch.stack([torch.linalg.qr(n(Dh, Dh))[0] for _ in range(H)])                  # [H, Dh, Dh]
        a = n(B, L, H, hd)
        a = a / a.norm(dim=-1, keepdim=True) * r2 ** 0.5
        f = n(B, L, H, hd) * (r2 / hd) ** 0.5
        pairs = _probe_pairs(L)
        for i, j in pairs:
            t = n(B, H, hd)
            t = t - (t * a[:, i]).sum(-1, keepdim=True) / r2 * a[:, i]
            t = a[:, i] + 0.5 * t / t.norm(dim=-1, keepdim=True) * r2 ** 0.5
            a[:, j] = t / t.norm(dim=-1, keepdim=True) * r2 ** 0.5
        c["x"] = torch.einsum("hde,blhe->blhd", Q, torch.cat([a, f], -1)).reshape(B, L, d)
        proj = torch.block_diag(*[Q[h, :, :hd] @ Q[h, :, :hd].T for h in range(H)])
        wq, wk = 0.95 * proj + 0.01 * n(d, d), 0.95 * proj + 0.01 * n(d, d)
        c["r_emb"] = 0.1 * n(K, H, Dh)
        c["r_bias"] = 0.3 * n(K, H)
        c["r_w_bias"] = 0.1 * n(H, Dh)
        c["probes"] = pairs
        # the gradient arriving at a row leans towards that row's own value (through Wo): d P_ii - delta_i then has one sign more often than
        # not, and the diagonal's entries of the position gradients are sums that do not cancel.  With white dy they cancelled 160-fold at
        # L = 513 (1539 terms of either sign), and the float32 run of the exact reference alone was 2.7e-5 off on that entry.
        a_self = (c["x"] @ wv.T) @ c["o_w"].T
        c["dy"] = c["dy"] + a_self / a_self.pow(2).mean().sqrt()
    c["qkv_w"] = torch.cat([wq, wk, wv], 0)
    return c


# -------------------------------------------------------------------------------------------------------------------------- reference
def table_index(L, K):
    """e(p) = max(0, p + K - L): the table row that serves effective position p"""
    return torch.clamp(torch.arange(L) + K - L, min=0)


def shift_index(L):
    """_rel_shift as a gather: BD[i, j] = G[row[i, j], col[i, j]] * valid[i, j] (oracle.tt_oracle.rel_shift_index)"""
    row, col, valid = O.rel_shift_index(L)
    return torch.from_numpy(row), torch.from_numpy(col), torch.from_numpy(valid)


def _full_mask(mask, B, H, L):
    """None | bool [B | 1, L, L] | bool [B, H, L, L] -> bool tensor broadcastable to [B, H, L, L], or None"""
    if mask is None:
        return None
    m = torch.as_tensor(np.asarray(mask) != 0)
    return m[:, None] if m.ndim == 3 else m


def attn_ref(case, mask=None, drop=None, rounding=None, dtype=torch.float64, p_shift=0.0, fault=None, cache=None):
    """-> dict of OUTPUTS (float64 tensors; g_r_emb as [K * H, Dh]), computed in `dtype`.
    mask: bool [B | 1, L, L] or [B, H, L, L], True = masked.  drop: the attention output's dropout multipliers [B * L * d] (0 | 1 / (1 - p)).
    rounding (read off attn_fwd_impl / attn_bwd_impl in csrc/layers.hip and the kernels they launch; "bf16" = round to nearest even, sums f32):
      None            exact arithmetic: the contract of prec 0 (f32) and prec 2 (bf16x3).  Equals oracle.tt_oracle.rel_attn_fwd / rel_attn_bwd.
      "fused"         prec 1, Dh in {32, 64}: the flash kernels (csrc/attn_flash.hip).  Forward: x and Wqkv are read in bf16 (the second bf16
                      term of a weight only where split_w says so: Wo from 4096 rows on, Wqkv never at option 13's default); q, k, v are
                      stored in bf16; q + u is formed in f32 from the bf16 q and the f32 u and rounded once; the effective table E is bf16,
                      its bias c f32; the position term c + q E^T is rounded to bf16 (the slab, or the kernels' LDS image) BEFORE the shift
                      and before the content term is added onto it; scores, maxima, exp and the softmax sum l are f32, and l sums the
                      UNROUNDED exp(s - m); exp(s - m) is rounded to bf16 as the operand of P V (see p_shift); O = (P16 V) / l is stored in
                      bf16; a = O Wo^T, the dropout, the residual and the LayerNorm are f32.
                      Backward: the LayerNorm backward is f32, dres * dropout leaves it in bf16 (dres16) for both of its products; dO is
                      stored in bf16; delta = sum(dO16 * O16) and P = exp(s - lse) are f32, recomputed from the same bf16 operands as the
                      forward; dS = P (dP - delta) scale is rounded to bf16 once and stored twice (dS and its shifted form dG); dV = P16^T dO
                      and dK = dS16^T (q + u)16 leave in bf16; dq = dS16 k + dG16 E16 is summed in f32 and rounded to bf16 once; g_r_w_bias is
                      the column sum of the f32 dS16 k; dE = dG16^T q16 and dc = colsum(dG16) are f32; g_qkv_w = dqkv16^T x16,
                      dx = dres (f32) + dqkv16 Wqkv16.
      "fast-unfused"  prec 1 with a bf16 pipeline whose head width the flash kernels do not take (Dh % 4 == 0, d % 8 == 0, Dh not in
                      {32, 64}): q, k, v, q + u, O, dres16, dO and (at the end) dq | dK | dV are stored in bf16; the position slab, the
                      scores, P, dP and dS are f32 and every product rounds its operands to bf16; g_r_w_bias and dc sum f32 values.
      "operands"      prec 1 at other shapes: f32 data flow, each product rounds both of its operands to bf16 (csrc/gemm.hip stages f32
                      tiles as bf16 under GEMM_BF16_MFMA); softmax, column sums and both LayerNorm passes are f32.
    p_shift: the exponentials are taken at rowmax + p_shift instead of rowmax.  Exact arithmetic does not depend on it; in "fused" it moves
      the grid on which exp(s - m) is rounded to bf16, as the kernels' lazily raised running maximum does.
    fault: test_attn_oracle.py's injected defects: ("shift_row", i) query row i takes the upper part of its shifted position term (j >= i + 2)
      from its own row of q E^T instead of the next row's;  ("table", 1) e(p) off by one.
    cache: dict that receives intermediates (S, P, v, O, a, dS, mean, rstd, e)."""
    assert rounding in (None, "fused", "fast-unfused", "operands")
    B, H, Dh, L, K, d = (case[k] for k in ("B", "H", "Dh", "L", "K", "d"))
    HD, BL = H * Dh, B * L
    x, dy, qkv_w, o_w, ln_g, ln_b, r_emb, u, r_bias = (case[k].to(dtype) for k in ("x", "dy", "qkv_w", "o_w", "ln_g", "ln_b", "r_emb", "r_w_bias", "r_bias"))
    op = _bf16 if rounding else (lambda t: t)                                    # a product's operands
    store = _bf16 if rounding in ("fused", "fast-unfused") else (lambda t: t)    # activations the bf16 pipelines keep in bf16
    fused = rounding == "fused"
    st_f = _bf16 if fused else (lambda t: t)                                     # what only the flash kernels round
    scale = 1.0 / Dh ** 0.5
    dm = torch.ones(BL, d, dtype=dtype) if drop is None else torch.as_tensor(drop).to(dtype).reshape(BL, d)
    m = _full_mask(mask, B, H, L)

    def heads(t):                                                                # [BL, HD] -> [B, H, L, Dh]
        return t.reshape(B, L, H, Dh).permute(0, 2, 1, 3)

    def rows(t):                                                                 # [B, H, L, Dh] -> [BL, HD]
        return t.permute(0, 2, 1, 3).reshape(BL, HD)

    x2 = x.reshape(BL, d)
    xr, wqkv = op(x2), op(qkv_w)
    wo_hi = op(o_w)
    wo = wo_hi + _bf16(o_w - wo_hi) if (store is _bf16 and BL >= 4096) else wo_hi
    qkv = store(xr @ wqkv.T)
    q, k, v = (heads(qkv[:, s * HD:(s + 1) * HD]) for s in range(3))
    qu = store(q + u[None, :, None, :])
    e = table_index(L, K)
    if fault is not None and fault[0] == "table":
        e = torch.clamp(e - fault[1], min=0)
    E = op(r_emb[e]).permute(1, 0, 2)                                            # [H, L(p), Dh]
    c = r_bias[e].T                                                              # [H, L(p)]
    G = st_f(op(q) @ E.transpose(1, 2)[None] + c[None, :, None, :])              # [B, H, L, L(p)]
    row, col, valid = shift_index(L)
    if fault is not None and fault[0] == "shift_row":
        i0 = fault[1]
        row = row.clone()
        row[i0, i0 + 2:] = i0
    flat = (row * L + col).reshape(-1)
    BD = G.reshape(B, H, L * L)[:, :, flat].reshape(B, H, L, L) * valid.to(dtype)
    S = (op(qu) @ op(k).transpose(2, 3) + BD) * scale
    if m is not None:
        S = torch.where(m, torch.full((), -float("inf"), dtype=dtype), S)
    smax = S.max(-1, keepdim=True).values + p_shift
    ex = torch.exp(S - smax)
    l = ex.sum(-1, keepdim=True)
    P = ex / l
    if fused:
        Oh = store((_bf16(ex) @ v) / l)
    else:
        Oh = store(op(P) @ op(v))
    O2 = rows(Oh)
    a = op(O2) @ wo.T
    s1 = x2 + a * dm
    mean, rstd = _ln_stats(s1)
    xh = (s1 - mean) * rstd
    y = xh * ln_g + ln_b

    dy2 = dy.reshape(BL, d)
    dres = ln_bwd_rows(dy2, s1, mean, rstd, ln_g)
    g_ln_g, g_ln_b = (dy2 * xh).sum(0), dy2.sum(0)
    da = op(store(dres * dm))                                                    # dres16
    g_o_w = da.T @ op(O2)
    dOh = heads(store(da @ wo_hi))
    dP = op(dOh) @ op(v).transpose(2, 3)
    delta = (dOh * Oh).sum(-1, keepdim=True) if fused else (dP * P).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale                                                # zero where masked (P = 0)
    dv = st_f(op(P).transpose(2, 3) @ op(dOh))
    dSr = st_f(dS)
    dk = st_f(op(dSr).transpose(2, 3) @ op(qu))
    dq_c = op(dSr) @ op(k)
    g_u = dq_c.sum((0, 2))
    dG = torch.zeros(B, H, L * L, dtype=dtype).index_add_(2, flat, (dSr * valid.to(dtype)).reshape(B, H, L * L)).reshape(B, H, L, L)
    dq = st_f(dq_c + op(dG) @ E[None])
    dE = (op(dG).transpose(2, 3) @ op(q)).sum(0)                                  # [H, L(p), Dh]
    dc = dG.sum((0, 2))                                                          # [H, L(p)]
    g_r_emb = torch.zeros(K, H, Dh, dtype=dtype).index_add_(0, e, dE.permute(1, 0, 2))
    g_r_bias = torch.zeros(K, H, dtype=dtype).index_add_(0, e, dc.T)
    dqkv = op(store(torch.cat([rows(dq), rows(dk), rows(dv)], 1)))
    g_qkv_w = dqkv.T @ xr
    dx = dres + dqkv @ wqkv
    if cache is not None:
        cache.update(S=S, P=P, v=v, O=Oh, a=a, dS=dS, mean=mean, rstd=rstd, e=e)
    out = dict(y=y, dx=dx, g_qkv_w=g_qkv_w, g_o_w=g_o_w, g_ln_g=g_ln_g, g_ln_b=g_ln_b, g_r_emb=g_r_emb.reshape(K * H, Dh), g_r_w_bias=g_u.reshape(-1),
               g_r_bias=g_r_bias.reshape(-1))
    return {n: t.to(torch.float64) for n, t in out.items()}


def unused_table_rows(L, K):
    """rows of r_emb / r_bias that no effective position maps to: the first K - L when L < K"""
    return max(K - L, 0)


# ------------------------------------------------------------------------------------------------------------------------ comparisons
def row_errors(got, want):
    """{output: rowwise_err vector}: rows of y / dx are the B L rows, g_qkv_w by its 3 H Dh rows, g_o_w by its d rows, g_r_emb as K H rows of Dh,
    the four vectors per element"""
    out = {}
    for k in OUTPUTS:
        w = np.asarray(want[k], dtype=np.float64)
        g = np.asarray(got[k], dtype=np.float64).reshape(w.shape)
        if w.ndim == 3:
            w, g = w.reshape(-1, w.shape[-1]), g.reshape(-1, w.shape[-1])
        e = rowwise_err(g, w)
        assert np.isfinite(e).all(), k
        out[k] = e
    return out


def errors(got, want):
    """{output: (max, 90 % quantile) of rowwise_err}"""
    return {k: (float(e.max()), float(np.quantile(e, 0.9))) for k, e in row_errors(got, want).items()}


def tolerances(c):
    """({class: bound on the worst row}, {class: bound on the 90 % quantile} or None) for a Case"""
    if c.prec != 1:
        return {k: TOL_EXACT for k in CLASSES}, None
    return TOL_MAX[c.family], (TOL_Q90[c.family] if rounding_of(c) == "fused" else None)


# ----------------------------------------------------------------------------------------------------------- cases, checked and cached
def preconditions(case, mask):
    """the float64 facts the input families promise (asserted: a failure is an error in the inputs) -> dict of the measured values"""
    B, H, Dh, L, d = (case[k] for k in ("B", "H", "Dh", "L", "d"))
    cache = {}
    attn_ref(case, mask, cache=cache)
    P = cache["P"]
    info = {}
    if case["family"] == "mixed":
        x2 = case["x"].reshape(B * L, d)
        info["branch"] = float((cache["a"].norm(dim=1) / x2.norm(dim=1)).median())
        assert 0.5 <= info["branch"] <= 2, ("median |a_row| / |x_row|", info["branch"])
        q, k = (case["x"].reshape(B * L, d) @ case["qkv_w"][s * d:(s + 1) * d].T for s in range(2))
        if L >= 16:
            qh, kh = (t.reshape(B, L, H, Dh).permute(0, 2, 1, 3) for t in (q, k))
            e = table_index(L, case["K"])
            ac = ((qh + case["r_w_bias"][None, :, None, :]) @ kh.transpose(2, 3)) / Dh ** 0.5
            bd = (qh @ case["r_emb"][e].permute(1, 2, 0)[None] + case["r_bias"][e].T[None, :, None, :]) / Dh ** 0.5
            info["ac_bd"] = float(ac.std() / bd.std())
            assert 0.5 <= info["ac_bd"] <= 2, ("std(AC) / std(BD)", info["ac_bd"])
            info["n_eff"] = float((1.0 / (P[:1] ** 2).sum(-1)).median())       # (utterance 0, of full length: under the per-utterance masks the padded utterances' rows keep one or two keys by construction)
            assert 2 <= info["n_eff"] <= L / 2, ("median effective number of keys", info["n_eff"])
    else:
        pairs = directed_probes(case, mask)
        if pairs:
            info["min_partner_p"] = min(float(P[b, :, i, j].min()) for b, i, j in pairs)
            assert info["min_partner_p"] >= MIN_PARTNER_P, ("a probe pair's probability", info["min_partner_p"])
        info["n_probes"] = len({(i, j) for _, i, j in pairs})
        assert L < 16 or info["n_probes"] >= 8, ("unmasked probe pairs", info["n_probes"])
    return info


def directed_probes(case, mask):
    """`planted`: (batch entry, query, key) of every probe pair, both directions, wherever the mask leaves it"""
    B, L = case["B"], case["L"]
    m = np.zeros((B, L, L), dtype=bool) if mask is None else np.broadcast_to(np.asarray(mask), (B, L, L))
    return [(b, q, k) for i, j in case["probes"] for q, k in ((i, j), (j, i)) for b in range(B) if not m[b, q, k]]


@functools.lru_cache(maxsize=8)
def cached_case(B, H, Dh, L, K, mask, family):
    """-> (inputs, mask array, mask spec), preconditions asserted"""
    case = attn_case(B, H, Dh, L, K, family, case_seed(Case(B, H, Dh, L, K, mask, family, 0, 0.0, None)))
    m, spec = mask_of(mask, L, B)
    if m is not None:
        assert (~np.broadcast_to(m, (B, L, L))).any(-1).all(), "a row without a key"
        if mask.startswith("pu_") and L >= 3:
            assert MC.every_row_keeps_a_key(MC.build(mask[3:], L, B)[0], B, L)
    case["info"] = preconditions(case, m)
    return case, m, spec


def cpu_drop(c, seed=None):
    """Bernoulli(p) multipliers 0 | 1 / (1 - p) over [B L d] from numpy: the CPU tests' stand-in for the mask the kernels draw.  None at p = 0."""
    if c.p <= 0:
        return None
    rng = np.random.default_rng(case_seed(c) if seed is None else seed)
    return torch.from_numpy((rng.random(c.B * c.L * c.H * c.Dh) >= c.p) / (1.0 - c.p))


def reference_gap(c):
    """{output: (max, q90)} of G for one prec-1 Case: per row the larger of |float32 run - float64 run| and |p_shift 0 - p_shift P_SHIFT|"""
    case, m, _ = cached_case(*input_key(c))
    r, drop = rounding_of(c), cpu_drop(c)
    base = attn_ref(case, m, drop, r)
    e32 = row_errors(attn_ref(case, m, drop, r, torch.float32), base)
    esh = row_errors(attn_ref(case, m, drop, r, p_shift=P_SHIFT), base)
    out = {}
    for k in OUTPUTS:
        e = np.maximum(e32[k], esh[k])
        out[k] = (float(e.max()), float(np.quantile(e, 0.9)))
    return out


def gap_summary(gaps, q90_forms=("fused",)):
    """{Case: {output: (max, q90)}} -> ({family: {class: G_max}}, {family: {class: G_q90}}); the quantile over the forms it is asserted for"""
    g_max = {f: {k: 0.0 for k in CLASSES} for f in FAMILIES}
    g_q90 = {f: {k: 0.0 for k in CLASSES} for f in FAMILIES}
    for c, g in gaps.items():
        for k, (mx, q) in g.items():
            g_max[c.family][CLASS_OF[k]] = max(g_max[c.family][CLASS_OF[k]], mx)
            if rounding_of(c) in q90_forms:
                g_q90[c.family][CLASS_OF[k]] = max(g_q90[c.family][CLASS_OF[k]], q)
    return g_max, g_q90


def y_rows_without_a_key(case, cache, drops):
    """exact float64 rows of y after ONE key is taken from one (b, h, i), for each (b, h, i, j) of drops, from the intermediates of an exact
    attn_ref run (cache): the softmax row is renormalised without key j, O, a and the LayerNorm of that row follow -> [len(drops), d]"""
    B, H, Dh, L, d = (case[k] for k in ("B", "H", "Dh", "L", "d"))
    out = []
    for b, h, i, j in drops:
        p = cache["P"][b, h, i].clone()
        p[j] = 0
        o = cache["O"][b, :, i].clone()                                          # [H, Dh]
        o[h] = (p / p.sum()) @ cache["v"][b, h]
        s1 = case["x"][b, i] + o.reshape(-1) @ case["o_w"].T
        mean, rstd = _ln_stats(s1[None])
        out.append(((s1[None] - mean) * rstd * case["ln_g"] + case["ln_b"])[0])
    return torch.stack(out)
