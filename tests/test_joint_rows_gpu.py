"""ttmi_joint_fwd / ttmi_joint_bwd / ttmi_joint_bwd_split and their chain with ttmi_rnnt_loss_fwd / _bwd / _bwd_split ROW BY ROW against the reference
of tests/joint_oracle.py, through the C ABI on buffers of the test's own: every row of the logits, of denc, ddec, g_wp and of both halves of g_wf and every
element of g_bf and g_bp is held to the bound of its precision - not a whole-tensor norm, under which one wrong frame row of denc in 1600 passes.  Every
route of joint_fwd_impl / joint_bwd_impl that the plain forms have is named in a case id and asserted reachable (joint_oracle.route_conditions): the
f32, 8-column and 4-column tanh kernels, prec 1 with J % 8 != 0, frame tails T 1, 2, 3, 17, 35, label edges U1 1, 2, 9, 65, 129, two column blocks of the
backward sums, the two-pass sum against the atomics (by option 21 and by size), the throughput and the generic input layer with and without the residual
terms, option 19, and the four shapes of the bf16x3 mode.  ctx and ws are followed by 4096 sentinel floats, logits / d logits / denc / ddec by a sentinel
row; the four parameter-gradient buffers arrive filled with a power of two near their rms (the ABI accumulates).  The pad columns [V, ldv) of the plain
forward's logits are promised nothing by include/ttmi.h (the loss never reads them) and are not asserted; those of the loss gradient are promised zero
and must be, in both planes of the pre-split form.  The exp-domain chain (ttmi_joint_fwd_exp with emis, ttmi_rnnt_loss_fwd_exp with shift_next and flag,
ttmi_rnnt_loss_bwd_exp, ttmi_joint_bwd_exp) runs under option 1 = 8 at five shapes and under the default dispatch at a sixth (joint_oracle.EXP_CASES): P, the row sums and three of their 64-column partials,
the four emis entries, srow, srow * P with its patched blank / label columns on their own, the costs and all seven gradients, with the exact zeros and bit
identities listed in the test.  Its case E2 found an out-of-bounds read in the persistent wgrad kernel.

Worst row or element measured over the cases (bound): prec 0: logits 5.7e-7, loss gradient 9.9e-6, denc 4.6e-6, ddec 1.5e-6, g_wp 3.8e-6, g_wf 5.1e-6 / 1.2e-6, g_bf 4.0e-6, g_bp 5.0e-6, costs 1.1e-7 (1e-4).  prec 2: logits 5.5e-6, loss
gradient 6.1e-5 (three-term logits at M 2048, floor 1e-2; hi + lo of the pre-split planes likewise), denc 1.6e-5, ddec 1.1e-5, g_wp 1.4e-5, g_wf 1.2e-5 / 1.2e-5, g_bf 1.2e-5, g_bp 6.2e-6,
costs 1.9e-7 (1e-4).  prec 1 "fast": logits 2.5e-3 (1.0e-2), loss gradient 7.5e-3 (3.0e-2), denc 2.8e-3 (1.1e-2), ddec 5.3e-3 (2.5e-2), g_wp 2.6e-3 (1.0e-2), g_wf 5.6e-3 (2.2e-2) / 1.9e-3
(8.0e-3), g_bf 2.3e-3 (8.0e-3), g_bp 2.1e-3 (8.8e-3), costs 2.1e-5 (8.4e-5); 90 % quantiles 1.8e-4 / 2.8e-3 / 1.3e-3 / 1.7e-3 / 1.3e-3 / 2.8e-3 / 1.4e-3 / 1.1e-3 / 1.1e-3 (4.4e-4 / 1.1e-2 /
5.2e-3 / 8.0e-3 / 6.4e-3 / 1.1e-2 / 6.0e-3 / 4.8e-3 / 4.4e-3).  "operands": logits 7.7e-4, loss gradient 3.3e-3, g_wf label half 1.4e-3, the rest under 6.2e-4.  "exp": rows of P 5.9e-3
(2.4e-2) and of srow . P 8.2e-3 (4.8e-2), row sums 7.8e-3 (3.1e-2), emis 8.0e-4 (3.2e-3), srow 1.2e-3 (4.8e-3), patched columns 4.0e-2 (6.0e-1), denc 6.5e-3 (4.8e-2), ddec 5.4e-3 (3.6e-2),
g_wp 6.4e-3 (3.6e-2), g_wf 7.1e-3 (4.4e-2) / 5.3e-3 (3.2e-2), g_bf 1.7e-3 (3.3e-2), g_bp 5.6e-3 (8.4e-2), costs 1.6e-6 (6.4e-6); 90 % quantiles: P 5.4e-5 (8.4e-3), row sums 7.9e-6 (2.7e-5), emis
2.5e-5 (1.0e-4), srow 3.2e-5 (1.1e-4), the gradients under 1.5e-3 (1.7e-2).  All read off the per-case lines the GPU run prints."""
import ctypes
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

import joint_oracle as R

pytestmark = pytest.mark.gpu

SENTINEL = -12288.0          # exact in bf16
GUARD = 4096


def _p(t):
    return c_void_p(t.data_ptr())


def _pow2_near(x):
    x = float(x)
    return 2.0 ** round(np.log2(x)) if x > 0 else 1.0


class _Run:
    """the buffers of one case and the calls on them"""

    def __init__(self, c, case):
        from ttmi import lib
        self.L = L_ = lib()
        for f in (L_.ttmi_joint_ctx_floats_prec, L_.ttmi_joint_ws_floats_prec, L_.ttmi_rnnt_workspace_bytes):
            f.restype = ctypes.c_size_t
        self.c, self.case = c, case
        dev = self.dev = torch.device("cuda")
        B, T, U1, J, V = c.B, c.T, c.U1, c.J, c.V
        self.M = M = B * T * U1
        self.t = {k: case[k].to(torch.float32).to(dev).contiguous() for k in ("enc", "dec", "wf", "bf", "wp", "bp")}
        self.dims = (c_int(B), c_int(T), c_int(U1), c_int(c.de), c_int(c.dd), c_int(J), c_int(V), c_int(c.prec))
        self.bf16 = L_.ttmi_joint_logits_dtype(c_int(c.prec), c_int(J)) == 1
        assert self.bf16 == R.joint_fast(c.prec, J)
        self.dt = torch.bfloat16 if self.bf16 else torch.float32
        # (f32 logits of the chain and of the three-term products: the pitch ttmi.ops gives them and the pre-split form asks for)
        padded = self.bf16 or c.lens is not None or (c.prec == 2 and R.x3_worth(M, V, J))
        self.ldv = (V + 63) // 64 * 64 if padded else V + c.pad
        self.n_ctx = int(L_.ttmi_joint_ctx_floats_prec(c_int(B), c_int(T), c_int(U1), c_int(J), c_int(c.prec)))
        self.n_ws = int(L_.ttmi_joint_ws_floats_prec(c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(c.prec)))
        self.ctx = torch.full((self.n_ctx + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.ws = torch.full((self.n_ws + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.logits = torch.full((M + 1, self.ldv), SENTINEL, dtype=self.dt, device=dev)
        self.stream = c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(self):
        from ttmi import check
        t = self.t
        check(self.L.ttmi_joint_fwd(_p(t["enc"]), _p(t["dec"]), _p(t["wf"]), _p(t["bf"]), _p(t["wp"]), _p(t["bp"]), *self.dims, _p(self.ctx), _p(self.ws),
                                    _p(self.logits), c_long(self.ldv), self.stream), "ttmi_joint_fwd")

    def grads(self, want):
        """fresh pre-filled gradient buffers + sentinel-rowed denc / ddec"""
        c, dev = self.c, self.dev
        g_wf = np.concatenate([want["g_wf_e"].numpy(), want["g_wf_d"].numpy()], 1)
        self.fill = dict(wf=_pow2_near(np.sqrt((g_wf ** 2).mean())), bf=_pow2_near(want["g_bf"].pow(2).mean().sqrt()),
                         wp=_pow2_near(want["g_wp"].pow(2).mean().sqrt()), bp=_pow2_near(want["g_bp"].pow(2).mean().sqrt()))
        shapes = dict(wf=(c.J, c.de + c.dd), bf=(c.J,), wp=(c.V, c.J), bp=(c.V,))
        self.g = {k: torch.full(shapes[k], self.fill[k], dtype=torch.float32, device=dev) for k in shapes}
        self.denc = torch.full((c.B * c.T + 1, c.de), SENTINEL, dtype=torch.float32, device=dev)
        self.ddec = torch.full((c.B * c.U1 + 1, c.dd), SENTINEL, dtype=torch.float32, device=dev)

    def bwd(self, dlogits, ldg, split=False):
        from ttmi import check
        t, g = self.t, self.g
        fn = self.L.ttmi_joint_bwd_split if split else self.L.ttmi_joint_bwd
        check(fn(_p(dlogits), c_long(ldg), _p(t["enc"]), _p(t["dec"]), _p(t["wf"]), _p(t["wp"]), *self.dims, _p(self.ctx), _p(self.ws), _p(self.denc),
                 _p(self.ddec), _p(g["wf"]), _p(g["bf"]), _p(g["wp"]), _p(g["bp"]), self.stream), "ttmi_joint_bwd_split" if split else "ttmi_joint_bwd")
        torch.cuda.synchronize()

    def outputs(self):
        c, g, f = self.c, self.g, self.fill
        out = dict(logits=self.logits[:self.M, :c.V], denc=self.denc[:-1], ddec=self.ddec[:-1], g_wp=g["wp"] - f["wp"], g_wf_e=g["wf"][:, :c.de] - f["wf"],
                   g_wf_d=g["wf"][:, c.de:] - f["wf"], g_bf=g["bf"] - f["bf"], g_bp=g["bp"] - f["bp"])
        return {k: v.double().cpu().numpy() for k, v in out.items()}

    def assert_guards(self):
        assert (self.ctx[self.n_ctx:] == SENTINEL).all(), "ctx written past ttmi_joint_ctx_floats_prec"
        assert (self.ws[self.n_ws:] == SENTINEL).all(), "ws written past ttmi_joint_ws_floats_prec"
        assert (self.logits[self.M].float() == SENTINEL).all(), "a logits row past the last one was written"
        assert (self.denc[-1] == SENTINEL).all() and (self.ddec[-1] == SENTINEL).all(), "a row of denc / ddec past the last one was written"


_refs = {}


def _reference(c):
    """one float64 reference per (inputs, form): prec 0 and prec 2 share the exact one"""
    key = (R.input_key(c), repr(R.form_of(c)))
    if key not in _refs:
        if len(_refs) >= 4:
            _refs.clear()                                            # cases of one key are adjacent
        _refs[key] = R.reference(c)
    return _refs[key]


def _hold(c, got, want, case, keys):
    tol_max, tol_q90 = R.tolerances(c)
    e = R.errors(got, {k: want[k].numpy() for k in keys}, case, keys, R.floor_of(c))
    print("%s (%s): " % (R.case_id(c), R.form_of(c)[0]) + "  ".join("%s %.1e/%.1e" % (k, *e[k]) for k in keys))
    for k in keys:
        cl = R.CLASS_OF[k]
        assert e[k][0] < tol_max[cl], (k, "worst row", e[k][0], tol_max[cl])
        if tol_q90 is not None:
            assert e[k][1] < tol_q90[cl], (k, "90 % quantile", e[k][1], tol_q90[cl])


def _with_option(c, body):
    from ttmi import ops
    try:
        if c.opt is not None:
            ops.set_option(c.opt[0], c.opt[1])                       # set around a complete forward + backward
        return body()
    finally:
        if c.opt is not None:
            ops.set_option(c.opt[0], c.opt[2])


def _order(c):
    return (R.input_key(c)[:7], str(c.lens), c.blank, repr(R.form_of(c)), c.prec, c.pad, c.opt or ())


@pytest.mark.parametrize("c", sorted(R.JOINT_CASES, key=_order), ids=R.case_id)
def test_joint_rows(c):
    """A: the joint alone on d logits of the test's own - every row sums to zero, one scale, pad columns zero"""
    for what, ok in R.route_conditions(c):
        assert ok, "%s: the shape does not meet the condition of '%s'" % (R.case_id(c), what)
    case = R.cached_case(*R.input_key(c))
    want = _reference(c)

    def body():
        run = _Run(c, case)
        run.fwd()
        dz = torch.zeros((run.M + 1, run.ldv), dtype=run.dt, device=run.dev)
        dz[:run.M, :c.V] = case["dz"].to(run.dt).to(run.dev)
        dz[run.M] = SENTINEL
        run.grads(want)
        run.bwd(dz, run.ldv)
        return run
    run = _with_option(c, body)
    run.assert_guards()
    _hold(c, run.outputs(), want, case, R.JOINT_OUT)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("e", R.EXP_CASES, ids=lambda e: e.route)
def test_exp_chain_rows(e):
    """C: ttmi_joint_fwd_exp with emis, ttmi_rnnt_loss_fwd_exp with shift_next and flag, ttmi_rnnt_loss_bwd_exp, ttmi_joint_bwd_exp at prec 1, lambda = 0"""
    from ttmi import check, ops
    for what, ok in R.exp_route_conditions(e):
        assert ok, "%s: the shape does not meet the condition of '%s'" % (e.route, what)
    c = R.exp_as_case(e)
    case = R.cached_exp_case(*R.exp_key(e))
    ref = R.exp_reference(e)
    want = R.exp_views(ref, case)
    B, T, U1, V, J, M = e.B, e.T, e.U1, e.V, e.J, e.B * e.T * e.U1
    valid = R.lattice_valid(case).reshape(M)
    try:
        if e.opt is not None:
            ops.set_option(e.opt[0], e.opt[1])
        run = _Run(c, case)
        run.t["bp"] = case["bp"].to(torch.float32).to(run.dev).contiguous()
        dev, L_, st, ldv = run.dev, run.L, run.stream, run.ldv
        L_.ttmi_joint_exp_padded_rows.restype = c_long
        assert L_.ttmi_joint_exp_supported(c_int(B), c_int(T), c_int(U1), c_int(J), c_int(V), c_int(1), c_long(ldv)) == 1, "the case would fall back"
        Mp = int(L_.ttmi_joint_exp_padded_rows(c_int(B), c_int(T), c_int(U1)))
        nparts = int(L_.ttmi_joint_exp_nparts(c_int(V)))
        assert Mp == (M + 63) // 64 * 64 and nparts == 4 * ((V + 255) // 256)
        P = torch.full((Mp + 1, ldv), SENTINEL, dtype=torch.bfloat16, device=dev)
        rowsum = torch.full((nparts * M + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        emis = torch.full((M + 1, 4), SENTINEL, dtype=torch.float32, device=dev)
        shift = torch.full((1,), e.shift, dtype=torch.float32, device=dev)
        shift_next = shift.clone()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        labels = _i32(case["labels"], dev) if U1 > 1 else None
        lp = _p(labels) if labels is not None else c_void_p(0)
        act, lab = _i32(case["act_lens"], dev), _i32(case["label_lens"], dev)
        t = run.t
        check(L_.ttmi_joint_fwd_exp(_p(t["enc"]), _p(t["dec"]), _p(t["wf"]), _p(t["bf"]), _p(t["wp"]), _p(t["bp"]), *run.dims, _p(run.ctx), _p(run.ws), _p(P),
                                    c_long(ldv), _p(rowsum), c_int(nparts), _p(shift), lp, c_int(e.blank), _p(emis), st), "ttmi_joint_fwd_exp")
        torch.cuda.synchronize()
        P0 = P.clone()
        lws = torch.empty(int(L_.ttmi_rnnt_workspace_bytes(c_int(B), c_int(T), c_int(U1))) // 4 + 1, dtype=torch.float32, device=dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        ones = torch.ones(B, dtype=torch.float32, device=dev)
        lens = (lp, _p(act), _p(lab), c_int(B), c_int(T), c_int(U1), c_int(V), c_int(e.blank))
        check(L_.ttmi_rnnt_loss_fwd_exp(_p(P), c_long(ldv), _p(rowsum), c_int(nparts), *lens, _p(lws), _p(costs), _p(shift), _p(shift_next), _p(emis), _p(flag), st),
              "ttmi_rnnt_loss_fwd_exp")
        srow = torch.full((M + 1,), SENTINEL, dtype=torch.float32, device=dev)
        srow16 = torch.full((Mp + 8,), SENTINEL, dtype=torch.bfloat16, device=dev)
        check(L_.ttmi_rnnt_loss_bwd_exp(_p(P), c_long(ldv), *lens, _p(lws), _p(ones), c_int(1), c_float(1.0), _p(srow), _p(srow16), st), "ttmi_rnnt_loss_bwd_exp")
        torch.cuda.synchronize()
        P1, srow_got = P.clone(), srow[:M].clone()
        assert torch.equal(_bits(srow16[:M]), _bits(srow_got.to(torch.bfloat16))), "srow16 != bf16(srow)"
        run.grads(ref)
        check(L_.ttmi_joint_bwd_exp(_p(P), c_long(ldv), _p(srow), _p(srow16), _p(t["enc"]), _p(t["dec"]), _p(t["wf"]), _p(t["wp"]), *run.dims, _p(run.ctx), _p(run.ws),
                                    _p(run.denc), _p(run.ddec), _p(run.g["wf"]), _p(run.g["bf"]), _p(run.g["wp"]), _p(run.g["bp"]), st), "ttmi_joint_bwd_exp")
        torch.cuda.synchronize()
    finally:
        if e.opt is not None:
            ops.set_option(e.opt[0], e.opt[2])

    # guards and sentinels
    run.assert_guards()
    assert (rowsum[nparts * M:] == SENTINEL).all() and (emis[M] == SENTINEL).all() and srow[M] == SENTINEL, "rowsum / emis / srow written past their ends"
    assert (P[Mp].float() == SENTINEL).all() and (srow16[Mp:].float() == SENTINEL).all(), "P / srow16 written past the padded rows"
    assert (P[M:Mp] == 0).all(), "rows [M, Mp) of P are not zero after ttmi_joint_bwd_exp"
    assert (P0[:M, V:] == 0).all() and (P1[:M, V:] == 0).all(), "pad columns of P are not exact zeros"
    assert int(flag) == 0
    vd = torch.from_numpy(valid).to(dev)
    assert (srow_got[~vd] == 0).all(), "srow is not exactly 0 on a row outside the lattice"
    assert torch.equal(_bits(P1[:M][~vd]), _bits(P0[:M][~vd])), "P was patched on a row outside the lattice"
    assert torch.equal(P[:M], P1[:M]), "ttmi_joint_bwd_exp changed a lattice row of P"
    em = emis[:M]
    last = torch.arange(M, device=dev) % U1 == U1 - 1
    assert torch.equal(em[last, 1], em[last, 0]) and torch.equal(em[last, 3], em[last, 2]), "the label entries of emis at u = U1-1 are not the blank's"

    # shift_next = max(cur, max log-sum-exp - 40) within the log-sum-exp's own bound
    lse_abs = want["lse"] + e.shift
    want_next = max(e.shift, float(lse_abs.max()) - 40.0)
    assert ("shift10" in e.route) == (want_next > e.shift), want_next
    assert abs(float(shift_next) - want_next) <= R.TOL_EXP_MAX["sums"] * float(np.sqrt((want["lse"] ** 2).mean())), (float(shift_next), want_next)

    # every row and element
    rs = rowsum[:nparts * M].view(nparts, M).double()
    got = dict(P=P0[:M, :V].double(), rowsum=rs.sum(0), emis=em.double(), srow=srow_got.double(), dlogits=srow_got.double()[:, None] * P1[:M, :V].double(),
               costs=costs.double(), denc=run.denc[:-1].double(), ddec=run.ddec[:-1].double())
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got.update({k: v for k, v in run.outputs().items() if k.startswith("g_")})
    # (the log-sum-exp of a row is no output of the ABI - it stays in the loss workspace; shift_next, srow and the costs carry it.  The entry below only fills the slot)
    got["lse"] = np.where(valid, np.log(np.maximum(got["rowsum"], 1e-300)), 0.0)
    got.update(valid=ref["valid"].numpy(), y=ref["y"].numpy(), has_label=ref["has_label"].numpy())
    got = R.exp_views(got, case)
    keys = tuple(k for k in R.EXP_OUT if k != "lse")
    err = {}
    for k in keys:
        g, w = got[k], want[k]
        ee = np.abs(g - w) / np.abs(w) if k == "costs" else (R.lattice_rows_err(g, w, case) if k == "dlogits" else R.rowwise_err(g, w))
        assert np.isfinite(ee).all(), k
        err[k] = (float(ee.max()), float(np.quantile(ee, 0.9)))
    print("%s: " % e.route + "  ".join("%s %.1e/%.1e" % (k, *err[k]) for k in keys))
    # each 64-column partial of the row sums on three parts
    frames = np.arange(T)[None, :] >= case["act_lens"][:, None]
    states = np.arange(U1)[None, :] > case["label_lens"][:, None]
    assert (got["denc"].reshape(B, T, -1)[frames] == 0).all(), "a row of denc at t >= T_b is not exactly zero"
    assert (got["ddec"].reshape(B, U1, -1)[states] == 0).all(), "a row of ddec at u > U_b is not exactly zero"
    for part in sorted({0, 1, (V - 1) // 64, nparts // 2}):      # at least three distinct ones, one in the last 256-column group
        w = ref["Pf"].numpy()[:, part * 64:min(part * 64 + 64, V)].sum(1)
        ep = R.rowwise_err(rs[part].cpu().numpy(), w) if w.any() else np.abs(rs[part].cpu().numpy())
        assert ep.max() < R.TOL_EXP_MAX["sums"], ("row-sum partial", part, ep.max())
    for k in keys:
        cl = R.EXP_CLASS_OF[k]
        bound = R.TOL_EXP_COSTS if k == "costs" else R.TOL_EXP_MAX[cl]
        assert err[k][0] < bound, (k, "worst row", err[k][0], bound)
        if k != "costs":
            assert err[k][1] < R.TOL_EXP_Q90[cl], (k, "90 % quantile", err[k][1], R.TOL_EXP_Q90[cl])


def test_exp_default_dispatch_needs_a_large_vocabulary():
    """with option 1 at its default 4 the exp-domain backward asks the persistent wgrad for V >= 1024 and 32768 padded rows (tn_v8_eligible, csrc/gemm_fast.hip):
    33 000 lattice rows at V 300 fall back to the two-call chain, so the default dispatch has no case at the small vocabularies of this file (host-side query only)"""
    from ttmi import lib
    ok = lambda V: lib().ttmi_joint_exp_supported(c_int(3), c_int(211), c_int(52), c_int(1024), c_int(V), c_int(1), c_long((V + 63) // 64 * 64))
    assert ok(300) == 0 and ok(1024) == 1


def _i32(a, dev):
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).to(dev)


@pytest.mark.parametrize("c", sorted(R.CHAIN_CASES, key=_order), ids=R.case_id)
def test_chain_rows(c):
    """B: ttmi_joint_fwd, ttmi_rnnt_loss_fwd, ttmi_rnnt_loss_bwd, ttmi_joint_bwd on ragged utterances; at prec 2, where both _ok functions agree, also
    ttmi_rnnt_loss_bwd_split + ttmi_joint_bwd_split with the planes read back as hi + lo"""
    from ttmi import check
    for what, ok in R.route_conditions(c):
        assert ok, "%s: the shape does not meet the condition of '%s'" % (R.case_id(c), what)
    case = R.cached_case(*R.input_key(c))
    want = _reference(c)
    B, T, U1, V, M = c.B, c.T, c.U1, c.V, c.B * c.T * c.U1
    keys = R.JOINT_OUT + ("costs", "dlogits")
    valid = R.lattice_valid(case)

    def zeros_outside(got, what):
        assert (got["dlogits"].reshape(B, T, U1, V)[~valid] == 0).all(), what + ": a loss-gradient row outside the lattice is not exactly zero"
        frames = np.arange(T)[None, :] >= case["act_lens"][:, None]
        states = np.arange(U1)[None, :] > case["label_lens"][:, None]
        assert (got["denc"].reshape(B, T, -1)[frames] == 0).all(), what + ": a row of denc at t >= T_b is not exactly zero"
        assert (got["ddec"].reshape(B, U1, -1)[states] == 0).all(), what + ": a row of ddec at u > U_b is not exactly zero"

    run = _Run(c, case)
    dev, L_, st = run.dev, run.L, run.stream
    labels, act, lab = _i32(case["labels"], dev), _i32(case["act_lens"], dev), _i32(case["label_lens"], dev)
    lws = torch.empty(int(L_.ttmi_rnnt_workspace_bytes(c_int(B), c_int(T), c_int(U1))) // 4 + 1, dtype=torch.float32, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    ones = torch.ones(B, dtype=torch.float32, device=dev)
    lens = (_p(labels), _p(act), _p(lab), c_int(B), c_int(T), c_int(U1), c_int(V), c_int(c.blank))
    dtc, ldv = c_int(1 if run.bf16 else 0), c_long(run.ldv)
    run.fwd()
    check(L_.ttmi_rnnt_loss_fwd(_p(run.logits), dtc, ldv, *lens, _p(lws), _p(costs), st), "ttmi_rnnt_loss_fwd")
    grad = torch.full((M + 1, run.ldv), SENTINEL, dtype=run.dt, device=dev)
    check(L_.ttmi_rnnt_loss_bwd(_p(run.logits), dtc, ldv, *lens, _p(lws), _p(ones), c_int(1), c_float(1.0), _p(grad), ldv, st), "ttmi_rnnt_loss_bwd")
    run.grads(want)
    run.bwd(grad, run.ldv)
    run.assert_guards()
    assert (grad[M].float() == SENTINEL).all(), "a loss-gradient row past the last one was written"
    assert (grad[:M, V:] == 0).all(), "pad columns of the loss gradient are not zero"
    got = run.outputs()
    got.update(costs=costs.double().cpu().numpy(), dlogits=grad[:M, :V].double().cpu().numpy())
    zeros_outside(got, "two-call chain")
    _hold(c, got, want, case, keys)

    split_ok = (c.prec == 2 and L_.ttmi_rnnt_loss_bwd_split_ok(ldv, _p(run.logits)) and
                L_.ttmi_joint_bwd_split_ok(c_int(B), c_int(T), c_int(U1), c_int(c.J), c_int(V), c_int(c.prec), ldv))
    assert bool(split_ok) == ("split-planes" in c.route), "the pre-split form is %s at this shape" % ("available" if split_ok else "not available")
    if split_ok:
        check(L_.ttmi_rnnt_loss_bwd_split(_p(run.logits), ldv, *lens, _p(lws), _p(ones), c_int(1), c_float(1.0), st), "ttmi_rnnt_loss_bwd_split")
        run.grads(want)
        run.bwd(run.logits, run.ldv, split=True)
        run.assert_guards()
        planes = run.logits[:M].view(torch.bfloat16).reshape(M, 2 * run.ldv)
        hi, lo = planes[:, :run.ldv], planes[:, run.ldv:]
        assert (hi[:, V:] == 0).all() and (lo[:, V:] == 0).all(), "pad columns of the pre-split planes are not zero"
        got2 = run.outputs()
        got2.update(costs=got["costs"], dlogits=(hi[:, :V].double() + lo[:, :V].double()).cpu().numpy(), logits=got["logits"])
        zeros_outside(got2, "pre-split chain")
        _hold(c, got2, want, case, keys)
