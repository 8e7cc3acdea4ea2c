"""Row-by-row reference of the position-wise FFN sub-layer (tt/transformer.py PositionwiseFF plus the layer's own dropout):

    h = LN(y);  a1 = drop_in(relu(h W1^T + b1));  f = a1 W2^T + b2;  s = y + drop_out(f);  z = drop_layer(LN(s))

with ONE (ln_g, ln_b) in both norms, forward and every gradient, in plain torch on the CPU and without the library.  It can round
where the library's two bf16 data flows round (`rounding`), so that a whole-row comparison is meaningful in bf16 too, and it can
run in float32 as well as float64: the distance between those two runs of the SAME reference is what the tolerances below are
derived from (tests/test_ffn_oracle.py re-measures it).  Used by tests/test_ffn_oracle.py (CPU) and tests/test_ffn_rows_gpu.py."""
import collections
import functools

import numpy as np
import torch

EPS = 1e-5
OUTPUTS = ("z", "dy", "g_w1", "g_b1", "g_w2", "g_b2", "g_ln_g", "g_ln_b")
MIN_PRE = 0.25      # ffn_case's precondition: no pre-activation of the ReLU closer to zero than this

# ---- tolerances.  prec 0 (exact f32) and prec 2 (bf16x3): the project's parity contract (README: within 1e-4 of the float64 oracle),
# applied to every row and column instead of the whole tensor.
TOL_EXACT = 1e-4
# prec 1 ("fast" and "operands"): 4 x the distance between this reference run in float32 and in float64 over every prec-1 case of CASES
# (masks of cpu_masks), worst row or column of any output (G_max) and worst 90 % quantile of any output (G_q90).  The factor 4: the
# kernels sum in another order than torch's CPU float32 and land on other bf16 round-to-nearest ties.
# test_ffn_oracle.py::test_tolerances_are_tied_to_the_reference re-measures both gaps and holds 2 G <= TOL <= 8 G.
TOL_MAX = 4 * 2.11e-3             # measured G_max 2.11e-3 (a row of z at 1541 x 8; next 1.09e-3, rows of z at 1541 x 136 and 1541 x 1024; "operands" 1.0e-4)
TOL_Q90 = max(4 * 2.55e-4, 1e-5)  # measured G_q90 2.55e-4 (g_b1 at 1541 x 512, Di 1024; next 2.5e-4, g_b1 at 1541 x 520; "operands" 4.4e-5); outputs no rounding flipped in: ~2e-7

Case = collections.namedtuple("Case", "rows d Di prec p grid")      # grid: ttmi_set_option(12, grid) for the case, None = default (384)


def _cases():
    out = []
    for d in (8, 136, 256, 264, 392, 512, 520, 1024):               # the bf16 pipeline's widths, every width route
        for rows in (3, 1541):                                      # 1541 = one full pass of the 384-block grid (1536 rows) + a ragged second one
            out += [Case(rows, d, 24, 0, 0.1, None), Case(rows, d, 24, 1, 0.1, None)]
    for d in (36, 37, 260, 513, 516):                               # d % 8 != 0: f32 data flow in every mode
        for rows in (3, 1541):
            out.append(Case(rows, d, 24, 0, 0.1, None))
            if d in (36, 37):
                out.append(Case(rows, d, 24, 1, 0.1, None))
    for d in (136, 512):                                            # row edges: a single row, three grid passes
        for rows in (1, 3077):
            out += [Case(rows, d, 24, 0, 0.1, None), Case(rows, d, 24, 1, 0.1, None)]
    for d in (136, 392):                                            # 3 blocks = 12 rows per pass: five passes over 50 rows, a prefetch at every boundary
        out += [Case(50, d, 24, 0, 0.1, 3), Case(50, d, 24, 1, 0.1, 3)]
    for prec in (0, 1, 2):                                          # inner width (prec 2 takes its three-term launches at 1541 x 512 x 1024)
        out += [Case(1541, 512, 1024, prec, 0.1, None), Case(1541, 64, 20, prec, 0.1, None)]
    out.append(Case(4100, 128, 24, 1, 0.1, None))                   # from 4096 rows on: second bf16 term of W2 in the forward product
    out += [Case(1541, 264, 24, 0, 0.0, None), Case(1541, 264, 24, 1, 0.0, None), Case(1541, 64, 20, 2, 0.0, None)]      # no dropout
    return out


CASES = _cases()


def case_id(c):
    return "r%d-d%d-Di%d-prec%d-p%g%s" % (c.rows, c.d, c.Di, c.prec, c.p, "" if c.grid is None else "-grid%d" % c.grid)


def case_seed(c):
    return (c.rows * 7919 + c.d * 104729 + c.Di * 1299709 + int(c.p * 10)) & 0x7FFFFFFF


def rounding_of(c):
    """the reference form that describes mode `prec` at this shape (csrc/layers.hip ffn_fast)"""
    if c.prec != 1:
        return None
    return "fast" if c.d % 8 == 0 and c.Di % 8 == 0 else "operands"


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _ln_stats(x):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + EPS)


def ln_bwd_rows(dyh, x, mean, rstd, g):
    """input gradient of LayerNorm for rows with the given statistics; dyh: gradient of the norm's output"""
    xh = (x - mean) * rstd
    dxh = dyh * g
    return rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))


def ffn_case(rows, d, Di, p, seed):
    """float64 inputs whose ReLU pre-activations all stay clear of zero (asserted: |LN(y) W1^T + b1| >= MIN_PRE), so that no rounding
    anywhere flips a gate and the sub-layer is a smooth function of its roundings; the dropout masks still gate element by element."""
    g = torch.Generator().manual_seed(seed)

    def n(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    c = dict(rows=rows, d=d, Di=Di, p=p, seed=seed)
    # every row its own mean and spread (scale 0.7 ... 1.4): statistics taken from a neighbouring row must not pass for the row's own
    c["y"] = n(rows, d) * 2.0 ** (torch.rand(rows, 1, generator=g, dtype=torch.float64) - 0.5) + n(rows, 1)
    c["dz"] = n(rows, d)
    c["w1"] = 0.2 * n(Di, d) / d ** 0.5
    sign = torch.where(torch.arange(Di) % 2 == 0, 1.0, -1.0).to(torch.float64)
    c["b1"] = sign * 1.5 * (1 + 0.1 * torch.rand(Di, generator=g, dtype=torch.float64))
    c["w2"] = n(d, Di) / Di ** 0.5
    c["b2"] = 0.1 * n(d)
    c["ln_g"] = 1 + 0.1 * n(d)
    c["ln_b"] = 0.1 * n(d)
    mean, rstd = _ln_stats(c["y"])
    pre = ((c["y"] - mean) * rstd * c["ln_g"] + c["ln_b"]) @ c["w1"].T + c["b1"]
    c["min_pre"] = float(pre.abs().min())
    assert c["min_pre"] >= MIN_PRE, "ffn_case(%d, %d, %d): a pre-activation at %.3f" % (rows, d, Di, c["min_pre"])
    return c


def cpu_masks(c, seed=None):
    """Bernoulli(p) multipliers 0 | 1/(1-p) over [rows, Di], [rows, d], [rows, d] (CoreNet.2, CoreNet.4, the layer's dropout) from
    numpy: the CPU tests' stand-in for the masks the kernels draw.  None at p = 0."""
    if c["p"] <= 0:
        return None
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    return tuple(torch.from_numpy((rng.random(s) >= c["p"]) / (1.0 - c["p"])) for s in ((c["rows"], c["Di"]), (c["rows"], c["d"]), (c["rows"], c["d"])))


def ffn_ref(case, masks=None, rounding=None, dtype=torch.float64, cache=None):
    """-> dict of OUTPUTS (float64 tensors), computed in `dtype`.  masks: (in [rows, Di], out [rows, d], layer [rows, d]) multipliers or None.
    rounding (read off ffn_fwd_impl / ffn_bwd_impl in csrc/layers.hip and the kernels they launch):
      None        exact arithmetic: the contract of prec 0 (f32) and prec 2 (bf16x3)
      "fast"      the bf16 pipeline (prec 1, d % 8 == 0 and Di % 8 == 0): h, a1 (after its dropout), dres * mask_out and da1 are stored in
                  bf16, the weights are read in bf16, sums are f32; f, dres, dh and both norms are f32.  g_b1 sums the bf16 da1.  g_b2
                  sums dres * mask_out BEFORE its rounding where the one-pass LayerNorm backward forms it (d <= 512) and the bf16 copy
                  where the general kernels do (d > 512: colsum_bf16 of dres16).  From 4096 rows on the forward product with W2 takes the second
                  bf16 term of the weight (option 13 at its default 2); the backward products never do.
      "operands"  prec 1 at other shapes: f32 data flow, each product rounds both of its operands to bf16 (csrc/gemm.hip stages f32
                  tiles as bf16 under GEMM_BF16_MFMA), f32 accumulation and f32 results; bias gradients sum the f32 values.
    cache: dict that receives the intermediates (h, a1, s, dres, dh, mean1, rstd1, mean2, rstd2)."""
    assert rounding in (None, "fast", "operands")
    rows, d, Di, p = case["rows"], case["d"], case["Di"], case["p"]
    y, dz, w1, b1, w2, b2, ln_g, ln_b = (case[k].to(dtype) for k in ("y", "dz", "w1", "b1", "w2", "b2", "ln_g", "ln_b"))
    if masks is None:
        assert p == 0, "dropout without masks"
        m_in, m_out, m_layer = torch.ones(rows, Di, dtype=dtype), torch.ones(rows, d, dtype=dtype), torch.ones(rows, d, dtype=dtype)
    else:
        m_in, m_out, m_layer = (m.to(dtype).reshape(s) for m, s in zip(masks, ((rows, Di), (rows, d), (rows, d))))
    inv_keep = 1.0 / (1.0 - p)
    rnd = _bf16 if rounding else (lambda t: t)                       # a product's operands
    store = _bf16 if rounding == "fast" else (lambda t: t)           # activations the bf16 pipeline keeps in bf16
    w1r, w2r = rnd(w1), rnd(w2)
    w2f = w2r + _bf16(w2 - w2r) if (rounding == "fast" and rows >= 4096) else w2r

    mean1, rstd1 = _ln_stats(y)
    h = store((y - mean1) * rstd1 * ln_g + ln_b)
    pre = rnd(h) @ w1r.T + b1
    assert float(pre.abs().min()) >= 0.5 * MIN_PRE, "a pre-activation within rounding of zero: the reference is not continuous here"
    a1 = store(torch.relu(pre) * m_in)
    f = rnd(a1) @ w2f.T + b2
    s = y + f * m_out
    mean2, rstd2 = _ln_stats(s)
    xh2 = (s - mean2) * rstd2
    z = (xh2 * ln_g + ln_b) * m_layer

    dzm = dz * m_layer
    dres = ln_bwd_rows(dzm, s, mean2, rstd2, ln_g)
    df = dres * m_out
    df_r = store(df)                                                 # dres16
    g_b2 = df_r.sum(0) if (rounding == "fast" and d > 512) else df.sum(0)
    df_r = rnd(df_r)
    g_w2 = df_r.T @ rnd(a1)
    da1 = store(torch.where(a1 > 0, (df_r @ w2r) * inv_keep, torch.zeros((), dtype=dtype)))
    g_b1 = da1.sum(0)
    g_w1 = rnd(da1).T @ rnd(h)
    dh = rnd(da1) @ w1r
    xh1 = (y - mean1) * rstd1
    dy = ln_bwd_rows(dh, y, mean1, rstd1, ln_g) + dres
    g_ln_g = (dzm * xh2).sum(0) + (dh * xh1).sum(0)
    g_ln_b = dzm.sum(0) + dh.sum(0)
    if cache is not None:
        cache.update(h=h, a1=a1, s=s, dres=dres, dh=dh, mean1=mean1, rstd1=rstd1, mean2=mean2, rstd2=rstd2)
    out = dict(z=z, dy=dy, g_w1=g_w1, g_b1=g_b1, g_w2=g_w2, g_b2=g_b2, g_ln_g=g_ln_g, g_ln_b=g_ln_b)
    return {k: v.to(torch.float64) for k, v in out.items()}


def rowwise_err(got, want):
    """per-row relative error of a matrix, |got_r - want_r| / max(|want_r|, rms(want) sqrt(ncols)) (the floor: rows that are zero, or nearly,
    such as an always-off unit's row of g_w1), per-element |got_c - want_c| / rms(want) of a vector.  -> numpy vector, one entry per row / element"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and want.ndim in (1, 2), (got.shape, want.shape)
    rms = float(np.sqrt(np.mean(want ** 2)))
    rms = rms if rms > 0 else 1.0
    if want.ndim == 1:
        return np.abs(got - want) / rms
    den = np.maximum(np.linalg.norm(want, axis=1), rms * np.sqrt(want.shape[1]))
    return np.linalg.norm(got - want, axis=1) / den


def errors(got, want):
    """{output: (max, 90 % quantile) of rowwise_err} over OUTPUTS; got / want: dicts of arrays or tensors"""
    out = {}
    for k in OUTPUTS:
        e = rowwise_err(np.asarray(got[k]), np.asarray(want[k]))
        assert np.isfinite(e).all(), k
        out[k] = (float(e.max()), float(np.quantile(e, 0.9)))
    return out


def tolerances(c):
    """(bound on the worst row, bound on the 90 % quantile or None) for a Case"""
    if c.prec != 1:
        return TOL_EXACT, None
    return TOL_MAX, (TOL_Q90 if rounding_of(c) == "fast" else None)


@functools.lru_cache(maxsize=4)
def cached_case(rows, d, Di, p):
    return ffn_case(rows, d, Di, p, case_seed(Case(rows, d, Di, 0, p, None)))


def reference_gaps(cases=None):
    """{Case: {output: (max, q90)}} of the float32 run of the reference against its float64 run, same rounding form, masks of cpu_masks:
    what the prec-1 tolerances are derived from"""
    out = {}
    for c in (CASES if cases is None else cases):
        if c.prec != 1:
            continue
        case = cached_case(c.rows, c.d, c.Di, c.p)
        masks = cpu_masks(case)
        r = rounding_of(c)
        out[c] = errors(ffn_ref(case, masks, r, torch.float32), ffn_ref(case, masks, r, torch.float64))
    return out


def gap_summary(gaps):
    """-> (G_max, G_q90): worst row and worst 90 % quantile over every case and output"""
    return (max(v[0] for g in gaps.values() for v in g.values()), max(v[1] for g in gaps.values() for v in g.values()))
