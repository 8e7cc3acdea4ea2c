"""Row-by-row reference of the joint network (tt/model.py JointNet in split-weight form) and of its chains with the RNN-T loss:

    PE = enc We^T, PD = dec Wd^T, h = tanh(PE[b,t] + PD[b,u] + bf), z = h Wp^T + bp           ([We | Wd] = forward_layer.weight)

forward and every gradient in plain torch, without the library, in float64 or float32: the distance between those two runs of the SAME
reference is what the prec-1 tolerances below are derived from (tests/test_joint_oracle.py re-measures it).  It can round where the
library's bf16 data flows round (`form`), and it has switches that plant the defects this code can have (`defect`), so that the CPU
tests can show that each would be seen.  The lattice is oracle.tt_oracle's; there is no third one here.
Used by tests/test_joint_oracle.py (CPU) and tests/test_joint_rows_gpu.py."""
import collections
import functools

import numpy as np
import torch

from ffn_oracle import TOL_EXACT, rowwise_err  # noqa: F401  (the comparator, its floor and its quantile conventions are the project's)
from oracle import tt_oracle as O

MAX_PRE = 4.0        # joint_case's precondition: no tanh pre-activation beyond +-4, so that 1 - h^2 >= 1.3e-3 stays above the bf16 spacing of h (2^-9 below 1)
# floor of the loss-gradient rows, as a fraction of the rms row norm of the utterance's own rows (lattice_rows_err).  Measured on the CPU: exact form, float32 run with its
# log-softmax in float32 and the lattice in float64 as in the kernels, against float64, worst row over the inputs of every chain and exp case at floor
# 1 / 1e-2 / 1e-4 / 1e-6 / 1e-8 / 1e-12: 8.9e-6 / 1.8e-5 / 1.8e-5 / 2.2e-5 / 2.2e-5 / 2.7e-5.  The gradient is multiplicative in exp(alpha + beta - ll + lp), so rows many decades
# under the rms are still resolved; what grows is the float32 error of lp = z - lse at logits near 45 (E3) and over 2000-row lattices.  The 1e-4 contract needs 2.5e-5
# (COND_EXACT): 1e-12 misses it, 1e-6 and 1e-8 hold it by a factor 1.1, 1e-4 is the smallest floor that holds it with the margin of 1e-2 (1.4) and is taken.
FLOOR_DLOGITS = 1e-4
# prec 2 where the projection runs in three bf16 terms (x3_worth): its logits carry 2^-17 per operand (rows 5.3e-6 off), and the lattice passes a logit error on to an off-path row
# once per step of the paths through it.  The reference with three-term logits (x3_chain_dlogits, float64 otherwise) against the exact one, 2048-row case, worst row at floor
# 1 / 1e-1 / 1e-2 / 1e-3 / 1e-4: 4.1e-5 / 5.6e-5 / 5.6e-5 / 8.7e-5 / 1.6e-4 (hi + lo planes: 4.6e-5 / 5.9e-5 / 5.9e-5 / 9.0e-5 / 1.6e-4): the number format itself misses 1e-4 on
# rows under 1e-3 of the rms.  1e-2 is the smallest floor at which it keeps a factor 1.7; a CPU test holds both statements.
FLOOR_DLOGITS_X3 = 1e-2
COND_EXACT = 2.5e-5  # precondition of the 1e-4 contract: the exact form in float32 is this close to float64 on every case's inputs

JOINT_OUT = ("logits", "denc", "ddec", "g_wp", "g_wf_e", "g_wf_d", "g_bf", "g_bp")
CLASS_OF = dict(logits="logits", dlogits="dlogits", denc="denc", ddec="ddec", g_wp="g_wp", g_wf_e="g_wf_e", g_wf_d="g_wf_d", g_bf="g_bf", g_bp="g_bp",
                costs="costs")

# ---- tolerances.  prec 0 (exact f32) and prec 2 (bf16x3): TOL_EXACT = 1e-4 on every row and element (the project's parity contract).
# prec 1 ("fast", "operands", "exp"): 4 x the distance G between this reference in float32 and in float64, same form, per output class, worst row
# (or element) and worst 90 % quantile over every prec-1 case of CASES; the factor 4 as in ffn_oracle.py: the kernels sum in another order
# than torch's CPU float32 and land on other bf16 round-to-nearest ties.  The exp form is measured at the case's shift and at shift + 0.37 (the
# rounding of exp(z - shift) at a shift the kernel may legitimately differ in) and the larger gap counts.
# test_joint_oracle.py::test_tolerances_are_tied_to_the_reference re-measures G and holds 2 G <= TOL <= 8 G.
# Loss-gradient rows: the floor is taken per utterance, FLOOR_DLOGITS of the rms row norm of that utterance's own rows (above).
# Measured G (worst row or element / worst 90 % quantile); the float32 run of the "fast" form takes tanh by the kernels' formula (joint_fwd_ref):
#   logits 2.5e-3 / 1.1e-4    dlogits 7.5e-3 / 2.8e-3 (U1 129)    denc 2.8e-3 / 1.3e-3    ddec 6.3e-3 / 2.0e-3 (U1 129)    g_wp 2.6e-3 / 1.6e-3
#   g_wf_e 5.6e-3 / 2.8e-3    g_wf_d 2.0e-3 / 1.5e-3    g_bf 2.0e-3 / 1.2e-3    g_bp 2.2e-3 / 1.1e-3    costs 2.1e-5 / 1.7e-5 (J 256, U1 9)
# "operands" alone: logits 7.7e-4, g_wf_d 1.4e-3, loss-gradient rows 3.3e-3, everything else under 6.2e-4.  Outputs no rounding flipped in: ~2e-7.
G_MAX = dict(logits=2.5e-3, dlogits=7.5e-3, denc=2.8e-3, ddec=6.3e-3, g_wp=2.6e-3, g_wf_e=5.6e-3, g_wf_d=2.0e-3, g_bf=2.0e-3, g_bp=2.2e-3, costs=2.1e-5)
G_Q90 = dict(logits=1.1e-4, dlogits=2.8e-3, denc=1.3e-3, ddec=2.0e-3, g_wp=1.6e-3, g_wf_e=2.8e-3, g_wf_d=1.5e-3, g_bf=1.2e-3, g_bp=1.1e-3, costs=1.7e-5)
TOL_MAX = {k: 4 * v for k, v in G_MAX.items()}
TOL_Q90 = {k: max(4 * v, 1e-5) for k, v in G_Q90.items()}

# opt: (key, value, restore) of ttmi_set_option around the case's forward + backward; pad: extra columns of the f32 logits pitch; lens: ((T_b ...), (U_b ...))
# for the chain with the loss, None = the joint alone with d logits of the test's own
Case = collections.namedtuple("Case", "route B T U1 de dd J V prec opt pad lens blank")


def _c(route, B, T, U1, de, dd, J, V, prec, opt=None, pad=0, lens=None, blank=0):
    return Case(route, B, T, U1, de, dd, J, V, prec, opt, pad, lens, blank)


def _joint_cases():
    out = []
    # tanh forward and backward in f32 (prec 0, any J), de != dd, f32 pitch ldv = V and V + 3
    out += [_c("tanh-f32-de40-dd24", 2, 3, 9, 40, 24, 36, 70, 0), _c("tanh-f32-de40-dd24-pitchV+3", 2, 3, 9, 40, 24, 36, 70, 0, pad=3)]
    # prec 1 with J % 8 != 0: f32 data flow with bf16 product operands
    out += [_c("operands-J36", 2, 17, 9, 40, 24, 36, 70, 1), _c("operands-J36-pitchV+3", 2, 17, 9, 40, 24, 36, 70, 1, pad=3)]
    # 8-column bf16 tanh kernel: 32, 64, 128, 256 threads per row; frame tails T % 4, T % 16, a lone last block; label edges; bf16 pitch at V 5, 64, 70, 300
    out += [_c("tanh8-J256-T17-U2-V64", 2, 17, 2, 16, 8, 256, 64, p) for p in (0, 1)]
    out += [_c("tanh8-J512-T35-U9-V5", 1, 35, 9, 16, 8, 512, 5, p) for p in (0, 1)]
    out += [_c("tanh8-J1024-T3-U65-V70", 2, 3, 65, 16, 8, 1024, 70, p) for p in (0, 1)]
    out += [_c("tanh8-J2048-T35-U2-V70-colblocks2", 1, 35, 2, 16, 8, 2048, 70, p) for p in (0, 1)]
    out += [_c("tanh8-J2048-T1-U9-V300-atomic-by-size", 4, 1, 9, 16, 8, 2048, 300, 1), _c("tanh8-J256-T2-U1-atomic-by-size", 16, 2, 1, 16, 8, 256, 70, 1)]
    # 4-column bf16 tanh kernel; J 1032: two column blocks of the backward sums, the second with an inactive tail
    out += [_c("tanh4-J8-T17-U9", 2, 17, 9, 16, 8, 8, 70, 1), _c("tanh4-J264-T3-U65-V300", 1, 3, 65, 16, 8, 264, 300, 1)]
    out += [_c("tanh4-J1032-T35-U2-colblocks2-tail", 2, 35, 2, 16, 8, 1032, 64, p) for p in (0, 1)]
    # the sums over frames by atomics (option 21 = 0); the label states' second term off (option 19 = 0)
    out += [_c("tanh8-J256-T17-U2-V64-opt21=0-atomics", 2, 17, 2, 16, 8, 256, 64, 1, opt=(21, 0, 1)), _c("tanh8-J256-T17-U2-V64-opt19=0", 2, 17, 2, 16, 8, 256, 64, 1, opt=(19, 0, 1))]
    # input layer: throughput kernels from B*T = 1024 on; the generic kernel at 1023, at de = 36, and without residual terms (M < din)
    out += [_c("input-fast-BT1040", 2, 520, 3, 64, 32, 256, 70, 1), _c("input-generic-BT1023", 3, 341, 3, 64, 32, 256, 70, 1)]
    out += [_c("input-generic-de36", 2, 17, 2, 36, 8, 256, 70, 1), _c("input-generic-no-residual-M<din-atomic-by-size", 1, 2, 2, 8, 8, 256, 70, 1)]
    # prec 2: below x3_worth; three-block rows in one launch and from 4096 rows on in two blocks; an f32 H split by a pass of its own (J % 4 != 0)
    out += [_c("x3-below-worth-M66", 2, 3, 11, 16, 8, 64, 70, 2), _c("x3-h3-one-launch-M2048", 2, 16, 64, 16, 8, 256, 300, 2)]
    out += [_c("x3-h3-two-blocks-M4290", 2, 33, 65, 16, 8, 256, 300, 2), _c("x3-f32-H-split-J258", 2, 16, 64, 16, 8, 258, 300, 2)]
    out += [_c("tanh8-J256-T17-U2-V64", 2, 17, 2, 16, 8, 256, 64, 2), _c("tanh-f32-de40-dd24", 2, 3, 9, 40, 24, 36, 70, 2)]
    return out


def _chain_cases():
    out = []
    for p in (0, 1, 2):
        # U_b = 0, T_b = 1 and a label equal to the blank (joint_case plants it), every utterance ragged
        out.append(_c("chain-J256-T17-U9-Ub0-Tb1-label=blank", 3, 17, 9, 16, 8, 256, 70, p, lens=((17, 1, 9), (8, 0, 5))))
        out.append(_c("chain-J1032-T35-U2-blank=V-1", 2, 35, 2, 16, 8, 1032, 64, p, lens=((35, 20), (1, 0)), blank=63))
        out.append(_c("chain-U65-two-label-slots", 2, 9, 65, 16, 8, 64, 70, p, lens=((9, 6), (64, 40))))
        out.append(_c("chain-U129-three-label-slots", 2, 5, 129, 16, 8, 64, 70, p, lens=((5, 3), (128, 70))))
    out.append(_c("chain-operands-J36", 2, 17, 9, 40, 24, 36, 70, 1, lens=((17, 11), (8, 3))))
    out.append(_c("chain-x3-split-planes-M2048", 2, 16, 64, 16, 8, 256, 300, 2, lens=((16, 9), (63, 30))))
    return out


JOINT_CASES = _joint_cases()
CHAIN_CASES = _chain_cases()
CASES = JOINT_CASES + CHAIN_CASES


def case_id(c):
    return "%s-B%d-prec%d" % (c.route, c.B, c.prec)


def input_key(c):
    return (c.B, c.T, c.U1, c.de, c.dd, c.J, c.V, c.lens, c.blank)


def al4(n):
    return (n + 3) & ~3


def al8(n):
    return (n + 7) & ~7


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the dispatch of joint_fwd_impl / joint_bwd_impl (csrc/layers.hip) and of the kernels they launch (csrc/rowops.hip), restated: the tests assert
# a case's route with these, so that a moved threshold fails loudly
def joint_fast(prec, J):
    return prec == 1 and J % 8 == 0


def joint_input_fast(c):
    if not joint_fast(c.prec, c.J) or c.de % 8 or c.dd % 8 or c.B * c.T < 1024:
        return False
    M, din = c.B * c.T * c.U1, c.de + c.dd
    need = al8(c.B * c.T * c.de) + al8(c.B * c.U1 * c.dd) + al8(c.B * c.T * c.J) + 2 * al8(c.B * c.U1 * c.J) + al8(din * c.J) + 8
    return need <= M * c.J and need + al8(din * c.J) + al8(c.B * c.U1 * c.dd) <= 2 * M * c.J


def x3_worth(M, N, K):
    return M >= 256 and N >= 64 and K >= 64 and M * N * K >= (1 << 27)


def tanh_route(c):
    if not joint_fast(c.prec, c.J):
        if c.prec == 2 and x3_worth(c.B * c.T * c.U1, c.V, c.J) and c.J % 4 == 0:
            return "x3"
        return "f32"
    return "bf16x8" if c.J in (256, 512, 1024, 2048) else "bf16x4"       # (J % 8 == 0 implies J % 4 == 0: the element-wise bf16 kernel is out of reach)


def two_pass(c):
    """the backward sums over frames: partial rows + an ordered second pass (True) or the atomic kernel"""
    opt21 = 0 if (c.opt and c.opt[0] == 21 and c.opt[1] == 0) else 1
    M = c.B * c.T * c.U1
    return bool(joint_fast(c.prec, c.J) and opt21 and c.J % 4 == 0 and 2 * c.B * cdiv(c.T, 16) * c.U1 * c.J + 16 <= M * c.J)


def form_of(c):
    """-> (form, switches) of the reference that describes the case's mode at its shape"""
    if c.prec != 1:
        return None, {}
    M, din = c.B * c.T * c.U1, c.de + c.dd
    opt19 = 0 if (c.opt and c.opt[0] == 19 and c.opt[1] == 0) else 1
    if joint_input_fast(c):
        return "fast", dict(input_fast=True, resid=True, dec_lo=bool(opt19))
    resid = M >= din
    dec_lo = bool(resid and opt19 and M * c.J >= al4(din * c.J) + c.B * c.U1 * c.dd)
    return ("fast" if c.J % 8 == 0 else "operands"), dict(input_fast=False, resid=resid, dec_lo=dec_lo)


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def joint_case(B, T, U1, de, dd, J, V, lens=None, blank=0, seed=None):
    """float64 inputs: logits of standard deviation near 2, no tanh pre-activation beyond +-MAX_PRE (asserted), d logits whose rows sum to zero at
    one scale (bf16 values, so that every mode reads the same numbers; columns are the caller's to pad).  With lens: labels with one label equal
    to the blank, ragged (T_b, U_b)."""
    seed = (B * 7919 + T * 104729 + U1 * 1299709 + J * 15485863 + V * 31 + de) & 0x7FFFFFFF if seed is None else seed
    g = torch.Generator().manual_seed(seed)

    def n(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    c = dict(B=B, T=T, U1=U1, de=de, dd=dd, J=J, V=V, blank=blank)
    # every frame and label state its own scale (0.7 ... 1.4): a neighbour's row must not pass for the row's own
    c["enc"] = n(B, T, de) * 2.0 ** (torch.rand(B, T, 1, generator=g, dtype=torch.float64) - 0.5)
    c["dec"] = n(B, U1, dd) * 2.0 ** (torch.rand(B, U1, 1, generator=g, dtype=torch.float64) - 0.5)
    c["wf"] = torch.cat([0.3 * n(J, de) / de ** 0.5, 0.3 * n(J, dd) / dd ** 0.5], 1)
    c["bf"] = 0.1 * n(J)
    pre = (c["enc"] @ c["wf"][:, :de].T)[:, :, None] + (c["dec"] @ c["wf"][:, de:].T)[:, None] + c["bf"]
    c["max_pre"] = float(pre.abs().max())
    assert c["max_pre"] <= MAX_PRE, "joint_case%r: a tanh pre-activation at %.3f" % ((B, T, U1, de, dd, J, V), c["max_pre"])
    hrms = float(torch.tanh(pre).pow(2).mean().sqrt())
    c["wp"] = n(V, J) * 2.0 / (hrms * J ** 0.5)
    c["bp"] = 0.1 * n(V)
    dz = n(B * T * U1, V)
    c["dz"] = _bf16(dz - dz.mean(1, keepdim=True))
    if lens is not None:
        rng = np.random.default_rng(seed)
        labels = rng.integers(0, V, size=(B, max(U1 - 1, 0))).astype(np.int32)
        if U1 > 1:
            labels[0, 0] = blank                                   # a label equal to the blank, inside utterance 0's lattice when U_0 > 0
        c["labels"], c["act_lens"], c["label_lens"] = labels, np.asarray(lens[0], dtype=np.int32), np.asarray(lens[1], dtype=np.int32)
        assert c["act_lens"].shape == (B,) and c["label_lens"].shape == (B,) and c["act_lens"].max() == T and (c["label_lens"] <= U1 - 1).all()
    return c


@functools.lru_cache(maxsize=4)
def cached_case(*key):
    B, T, U1, de, dd, J, V, lens, blank = key
    return joint_case(B, T, U1, de, dd, J, V, lens, blank)


def joint_fwd_ref(case, form=None, dtype=torch.float64, input_fast=False, resid=True, dec_lo=True):
    """-> dict(logits [M, V] as the mode stores them, z: the projection's unrounded accumulators + bias, H: the hidden rows as stored, h: before their
    rounding).  form (read off joint_fwd_impl):
      None        nothing rounded: the contract of prec 0 and prec 2
      "fast"      prec 1, J % 8 == 0: both input products read bf16 operands and add the second bf16 term of the weight (resid: the generic kernel has
                  room for it only when M >= de + dd) and of the label states (dec_lo: option 19, and room); PE, PD, the sum and tanh are f32; H is
                  stored in bf16; the projection reads bf16 H and bf16 Wp, accumulates in f32, adds bp and stores bf16 logits.  The throughput kernels
                  (input_fast) and the generic kernel rounding while it stages form the same numbers in the forward pass.
      "operands"  prec 1, J % 8 != 0: the same input layer, f32 H and f32 logits, the projection rounding both operands to bf16 while it stages."""
    assert form in (None, "fast", "operands")
    de = case["de"]
    enc, dec, wf, bf, wp, bp = (case[k].to(dtype) for k in ("enc", "dec", "wf", "bf", "wp", "bp"))
    B, T, U1, J, V = case["B"], case["T"], case["U1"], case["J"], case["V"]
    rnd = _bf16 if form else (lambda t: t)
    store = _bf16 if form == "fast" else (lambda t: t)
    e2, d2 = enc.reshape(B * T, -1), dec.reshape(B * U1, -1)
    PE = rnd(e2) @ rnd(wf[:, :de]).T
    PD = rnd(d2) @ rnd(wf[:, de:]).T
    if form and resid:
        wlo = _bf16(wf - _bf16(wf))
        PE = PE + rnd(e2) @ wlo[:, :de].T
        PD = PD + rnd(d2) @ wlo[:, de:].T
        if dec_lo:
            PD = PD + _bf16(d2 - _bf16(d2)) @ rnd(wf[:, de:]).T
    pre = (PE.reshape(B, T, 1, J) + bf) + PD.reshape(B, 1, U1, J)
    assert float(pre.abs().max()) <= MAX_PRE + 0.1
    # the bf16 pipeline's kernels take tanh(x) = 1 - 2 / (1 + 2^(2 x log2 e)) (fast_tanh, csrc/rowops.hip): the same function, but in float32 its error is absolute
    # (6e-8 of 1, not of h), so small h land on other bf16 values far more often than with libm's tanhf - the float32 run of this form must have that error too
    h = (1 - 2 / (1 + torch.exp2(pre * 2.8853900817779268)) if form == "fast" else torch.tanh(pre)).reshape(B * T * U1, J)
    H = store(h)
    z = rnd(H) @ rnd(wp).T + bp
    return dict(logits=store(z), z=z, H=H, h=h)


def joint_bwd_ref(case, fwd, dz, form=None, dtype=torch.float64, input_fast=False, resid=True, dec_lo=True, defect=None, dP=None, g_wp_bp=None):
    """the joint's backward for d logits `dz` [M, V] (already in the mode's storage form) -> denc, ddec, g_wp, g_wf_e, g_wf_d, g_bf, g_bp (read off joint_bwd_impl):
      "fast"      g_wp = dZ^T H16 and g_bp = column sums of dZ in f32; dP = bf16((dZ bf16(Wp)) (1 - H16^2)) from the dgrad epilogue, summed over u (dPE) and over
                  t (dPD) in f32.  Throughput input layer (input_fast): dPE, dPD rounded to bf16, g_bf = column sums of the ROUNDED dPE, ddec takes dPD's second
                  bf16 term (dec_lo: option 19); generic: the products round both operands while staging, g_bf sums the f32 dPE, no second term.
      "operands"  f32 data flow: g_bp sums f32, every product rounds both operands, dP = dH (1 - H^2) in f32; the generic input layer.
    defect: ("ddec_tail_twice", b, u) frame T-1 counted twice in one row of dPD; ("part_row_lost", b, u, k) frames 16 k .. 16 k + 15 left out of one row of dPD;
    ("g_wf_shift",) the label half of g_wf taken one column early (de - 1 against de).  dP / g_wp_bp: given by the exp-domain chain."""
    B, T, U1, J, V, de = case["B"], case["T"], case["U1"], case["J"], case["V"], case["de"]
    enc, dec, wf, wp = (case[k].to(dtype) for k in ("enc", "dec", "wf", "wp"))
    rnd = _bf16 if form else (lambda t: t)
    e2, d2 = enc.reshape(B * T, -1), dec.reshape(B * U1, -1)
    H = fwd["H"]
    if dP is None:
        dz = dz.to(dtype)
        g_bp = dz.sum(0)
        g_wp = rnd(dz).T @ rnd(H)
        dP = (rnd(dz) @ rnd(wp)) * (1 - H * H)
        if form == "fast":
            dP = _bf16(dP)
    else:
        g_wp, g_bp = g_wp_bp
    dP4 = dP.reshape(B, T, U1, J)
    dPE = dP4.sum(2).reshape(B * T, J)
    dPD = dP4.sum(1)
    if defect and defect[0] == "ddec_tail_twice":
        dPD[defect[1], defect[2]] += dP4[defect[1], T - 1, defect[2]]
    if defect and defect[0] == "part_row_lost":
        k = defect[3]
        dPD[defect[1], defect[2]] -= dP4[defect[1], 16 * k:16 * k + 16, defect[2]].sum(0)
    dPD = dPD.reshape(B * U1, J)
    We, Wd = wf[:, :de], wf[:, de:]
    if form == "fast" and input_fast:
        dPE16, dPD16 = _bf16(dPE), _bf16(dPD)
        g_bf = dPE16.sum(0)
        g_wf_e, g_wf_d = dPE16.T @ _bf16(e2), dPD16.T @ _bf16(d2)
        denc, ddec = dPE16 @ _bf16(We), dPD16 @ _bf16(Wd)
        if dec_lo:
            ddec = ddec + _bf16(dPD - dPD16) @ _bf16(Wd)
    else:
        g_bf = dPE.sum(0)
        g_wf_e, g_wf_d = rnd(dPE).T @ rnd(e2), rnd(dPD).T @ rnd(d2)
        denc, ddec = rnd(dPE) @ rnd(We), rnd(dPD) @ rnd(Wd)
    if defect and defect[0] == "g_wf_shift":
        g_wf_d = torch.cat([g_wf_e[:, -1:], g_wf_d[:, :-1]], 1)
    return dict(denc=denc, ddec=ddec, g_wp=g_wp, g_wf_e=g_wf_e, g_wf_d=g_wf_d, g_bf=g_bf, g_bp=g_bp)


def _f64(d):
    return {k: (v.to(torch.float64) if torch.is_tensor(v) else v) for k, v in d.items()}


def joint_ref(case, form=None, dtype=torch.float64, defect=None, **sw):
    """the joint alone on the case's own d logits -> dict of JOINT_OUT (float64 tensors)"""
    fwd = joint_fwd_ref(case, form, dtype, **sw)
    out = joint_bwd_ref(case, fwd, case["dz"], form, dtype, defect=defect, **sw)
    out["logits"] = fwd["logits"]
    return _f64(out)


def lattice_valid(case):
    """bool [B, T, U1]: rows inside the utterances' lattices"""
    B, T, U1 = case["B"], case["T"], case["U1"]
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    return (t < case["act_lens"][:, None, None]) & (u <= case["label_lens"][:, None, None])


def chain_ref(case, form=None, dtype=torch.float64, defect=None, **sw):
    """joint forward, oracle.tt_oracle.rnnt_loss on the logits as the mode stores them (per-utterance costs, gradient of sum_b costs[b]), the gradient
    stored in the logits' dtype, joint backward -> JOINT_OUT + costs [B] + dlogits [M, V]"""
    fwd = joint_fwd_ref(case, form, dtype, **sw)
    B, T, U1, V = case["B"], case["T"], case["U1"], case["V"]
    # (the log-softmax in `dtype`, the lattice always in float64, as the kernels carry it: a float32 lattice of 129 labels alone is 3e-4 off and would
    # measure the oracle, not the joint)
    z = fwd["logits"].reshape(B, T, U1, V).numpy()
    costs, _, grad = O.rnnt_loss(z, case["labels"], case["act_lens"], case["label_lens"], blank=case["blank"], reduction="none",
                                 lattice=lambda lpb, lpl: O.rnnt_lattice_diag(lpb.astype(np.float64), lpl.astype(np.float64)))
    dz = torch.from_numpy(np.ascontiguousarray(grad)).reshape(B * T * U1, V).to(dtype)
    if form == "fast":
        dz = _bf16(dz)
    out = joint_bwd_ref(case, fwd, dz, form, dtype, defect=defect, **sw)
    out.update(logits=fwd["logits"], dlogits=dz, costs=torch.from_numpy(np.asarray(costs, dtype=np.float64)))
    return _f64(out)


def exp_ref(case, dtype=torch.float64, shift=0.0, rounded=True, emis_fallback=False, defect=None, **sw):
    """the exp-domain chain (ttmi_joint_fwd_exp, ttmi_rnnt_loss_fwd_exp, ttmi_rnnt_loss_bwd_exp, ttmi_joint_bwd_exp; read off joint_fwd_impl, rnnt_prep_exp_kernel,
    rnnt_scale_exp_kernel, joint_bwd_impl): the "fast" forward with P = bf16(exp(z - shift)) and row sums of the unrounded values; emis 0, 1 = the blank's and
    the next label's logit from the bf16 operands, 2, 3 from the unrounded h and the f32 weight (emis_fallback: joint_emis_kernel has the rounded h only; the row
    u = U1-1 takes the blank for its label); S with the two columns' terms exchanged (the label's only for u < U_b and label != blank); log-probs from entries 2, 3;
    the lattice in float64 as the kernels carry it; srow = exp(alpha + beta - ll - log S) in f32 and bf16; blank / label entries of P patched by 1 - rb [- rl];
    H <- bf16(srow H); dP = bf16((P bf16(Wp)) (1 - H^2) srow); g_wp = P^T (srow H), g_bp = P^T srow16.  rounded=False: none of the bf16 roundings, the identity
    with the exact chain.  defect: ("emis_last_label",) the row u = U1-1 given labels[b][U1-2]'s logit for the blank's in emis; ("srow_outside", b, t) srow nonzero
    on a row t >= T_b; ("blank_patch_no_rl",) rl omitted where the label equals the blank; ("g_bp_unweighted", v) one entry of g_bp from the unweighted column sum."""
    B, T, U1, J, V, blank = case["B"], case["T"], case["U1"], case["J"], case["V"], case["blank"]
    M = B * T * U1
    r16 = _bf16 if rounded else (lambda t: t)
    fwd = joint_fwd_ref(case, "fast" if rounded else None, dtype, **sw)
    wp, bp = case["wp"].to(dtype), case["bp"].to(dtype)
    z, H, h = fwd["z"], fwd["H"], fwd["h"]
    Pf = torch.exp(z - shift)
    rowsum = Pf.sum(1)
    P = r16(Pf)
    labels = np.clip(case["labels"], 0, V - 1) if U1 > 1 else np.zeros((B, 0), dtype=np.int32)
    y = np.full((B, T, U1), blank, dtype=np.int64)
    y[:, :, :U1 - 1] = labels[:, None, :]
    if defect and defect[0] == "emis_last_label" and U1 > 1:
        y[:, :, U1 - 1] = labels[:, None, U1 - 2]
    y = torch.from_numpy(y.reshape(M))
    wb, wy = wp[blank], wp[y]
    hh = H if emis_fallback else h
    emis = torch.stack([H @ r16(wb) + bp[blank], (H * r16(wy)).sum(1) + bp[y], hh @ wb + bp[blank], (hh * wy).sum(1) + bp[y]], 1)
    valid = torch.from_numpy(lattice_valid(case).reshape(M))
    u_idx = torch.arange(M) % U1
    b_idx = torch.arange(M) // (T * U1)
    Ub = torch.from_numpy(case["label_lens"].astype(np.int64))[b_idx]
    has_label = u_idx < Ub
    S = rowsum + torch.exp(emis[:, 2] - shift) - torch.exp(emis[:, 0] - shift)
    S = S + torch.where(has_label & (y != blank), torch.exp(emis[:, 3] - shift) - torch.exp(emis[:, 1] - shift), torch.zeros((), dtype=dtype))
    lse = torch.log(S)
    lpb = (emis[:, 2] - shift - lse).to(torch.float64).reshape(B, T, U1).numpy()
    lpl = (emis[:, 3] - shift - lse).to(torch.float64).reshape(B, T, U1).numpy()
    costs = np.zeros(B)
    srow = torch.zeros(M, dtype=dtype)
    rb, rl = torch.zeros(M, dtype=dtype), torch.zeros(M, dtype=dtype)
    for b in range(B):
        Tb, U_b = int(case["act_lens"][b]), int(case["label_lens"][b])
        lb, ll_ = lpb[b, :Tb, :U_b + 1], lpl[b, :Tb, :U_b + 1].copy()
        ll_[:, U_b] = -np.inf
        alpha, beta, ll = O.rnnt_lattice(lb, ll_)
        costs[b] = -ll
        bn = np.full_like(beta, -np.inf)
        bn[:-1] = beta[1:]
        rbb = np.exp(bn - beta)
        rbb[Tb - 1, U_b] = np.exp(-beta[Tb - 1, U_b])
        rll = np.zeros_like(beta)
        rll[:, :U_b] = np.exp(beta[:, 1:] - beta[:, :U_b])
        rows = ((b * T + np.arange(Tb))[:, None] * U1 + np.arange(U_b + 1)[None, :]).reshape(-1)
        srow[rows] = (torch.from_numpy((alpha + beta - ll).reshape(-1)).to(dtype) - lse[rows]).exp()
        rb[rows], rl[rows] = torch.from_numpy(rbb.reshape(-1)).to(dtype), torch.from_numpy(rll.reshape(-1)).to(dtype)
    if defect and defect[0] == "srow_outside":
        row = (defect[1] * T + defect[2]) * U1
        assert not bool(valid[row])
        srow[row] = srow[valid].mean()
    Pp = P.clone()
    rows = torch.nonzero(valid)[:, 0]
    same = (y == blank) & has_label
    rl_in_blank = torch.zeros_like(rl) if (defect and defect[0] == "blank_patch_no_rl") else rl
    fb = 1 - rb - torch.where(same, rl_in_blank, torch.zeros((), dtype=dtype))
    Pp[rows, blank] = r16(P[rows, blank] * fb[rows])
    lab = torch.nonzero(valid & has_label & (y != blank))[:, 0]
    Pp[lab, y[lab]] = r16(P[lab, y[lab]] * (1 - rl[lab]))
    srow16 = r16(srow)
    dlogits = srow[:, None] * Pp
    dP = (Pp @ r16(wp)) * (1 - H * H) * srow[:, None]
    Hs = r16(srow[:, None] * H)
    g_wp = Pp.T @ Hs
    g_bp = Pp.T @ srow16
    if defect and defect[0] == "g_bp_unweighted":
        g_bp[defect[1]] = Pp[:, defect[1]].sum()
    out = joint_bwd_ref(case, fwd, None, "fast" if rounded else None, dtype, dP=r16(dP), g_wp_bp=(g_wp, g_bp), **sw)
    out.update(logits=fwd["logits"], P=P, Pf=Pf, P_patched=Pp, rowsum=rowsum, emis=emis, lse=lse, srow=srow, srow16=srow16, dlogits=dlogits,
               costs=torch.from_numpy(costs), valid=valid, y=y, has_label=has_label)
    return _f64(out)


def lattice_rows_err(got, want, case, floor=None):
    """rowwise_err's measure of loss-gradient rows with the floor taken per utterance: |got_r - want_r| / max(|want_r|, floor x the rms row norm of that
    utterance's rows inside its lattice), floor = FLOOR_DLOGITS (1 is rowwise_err itself) -> one vector over all rows inside the lattices"""
    floor = FLOOR_DLOGITS if floor is None else floor
    B, T, U1 = case["B"], case["T"], case["U1"]
    valid = lattice_valid(case).reshape(B, T * U1)
    got, want = np.asarray(got, dtype=np.float64).reshape(B, T * U1, -1), np.asarray(want, dtype=np.float64).reshape(B, T * U1, -1)
    out = []
    for b in range(B):
        g, w = got[b][valid[b]], want[b][valid[b]]
        rms = float(np.sqrt(np.mean(w ** 2))) or 1.0
        out.append(np.linalg.norm(g - w, axis=1) / np.maximum(np.linalg.norm(w, axis=1), floor * rms * np.sqrt(w.shape[1])))
    return np.concatenate(out)


def floor_of(c):
    """the floor of the loss-gradient rows for a Case"""
    return FLOOR_DLOGITS_X3 if (c.prec == 2 and x3_worth(c.B * c.T * c.U1, c.V, c.J)) else FLOOR_DLOGITS


def x3_chain_dlogits(case):
    """the loss gradient (float64) of the exact chain fed logits of the three-term form hi . hi + lo . hi + hi . lo -> (as the two-call chain leaves it, as hi + lo planes)"""
    fwd = joint_fwd_ref(case)
    H, wp = fwd["H"], case["wp"]
    Hh, Wh = _bf16(H), _bf16(wp)
    z3 = Hh @ Wh.T + _bf16(H - Hh) @ Wh.T + Hh @ _bf16(wp - Wh).T + case["bp"]
    B, T, U1, V = case["B"], case["T"], case["U1"], case["V"]
    _, _, grad = O.rnnt_loss(z3.reshape(B, T, U1, V).numpy(), case["labels"], case["act_lens"], case["label_lens"], blank=case["blank"], reduction="none")
    g = torch.from_numpy(np.ascontiguousarray(grad)).reshape(-1, V)
    return g, _bf16(g) + _bf16(g - _bf16(g))


def errors(got, want, case=None, keys=JOINT_OUT, floor=None):
    """{output: (max, 90 % quantile) of the row / element errors}.  costs: relative per utterance; dlogits: lattice_rows_err"""
    out = {}
    for k in keys:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        if k == "costs":
            e = np.abs(g - w) / np.abs(w)
        elif k == "dlogits":
            e = lattice_rows_err(g, w, case, floor)
        else:
            e = rowwise_err(g, w)
        assert np.isfinite(e).all(), k
        out[k] = (float(e.max()), float(np.quantile(e, 0.9)))
    return out


def tolerances(c):
    """({class: bound on the worst row / element}, {class: bound on the 90 % quantile} or None) for a Case"""
    if c.prec != 1:
        return {k: TOL_EXACT for k in TOL_MAX}, None
    return TOL_MAX, TOL_Q90


def reference(c, dtype=torch.float64, defect=None):
    case = cached_case(*input_key(c))
    form, sw = form_of(c)
    return (joint_ref if c.lens is None else chain_ref)(case, form, dtype, defect=defect, **sw)


def out_keys(c):
    return JOINT_OUT if c.lens is None else JOINT_OUT + ("costs", "dlogits")


def reference_gaps(cases=None):
    """{Case: {output: (max, q90)}} of the float32 run of the reference against its float64 run in the same form, over the prec-1 cases"""
    out = {}
    for c in (CASES if cases is None else cases):
        if c.prec != 1:
            continue
        case = cached_case(*input_key(c))
        out[c] = errors(reference(c, torch.float32), reference(c, torch.float64), case, out_keys(c))
    return out


def gap_summary(gaps):
    """-> (G_max, G_q90): {class: worst row, worst 90 % quantile} over every case and output"""
    gm, gq = {k: 0.0 for k in TOL_MAX}, {k: 0.0 for k in TOL_MAX}
    for g in gaps.values():
        for k, (m, q) in g.items():
            cl = CLASS_OF[k]
            gm[cl], gq[cl] = max(gm[cl], m), max(gq[cl], q)
    return gm, gq


def route_conditions(c):
    """[(what the case id claims, does the shape meet the condition as csrc/layers.hip / csrc/rowops.hip state it)]: every word of a case's route
    name is checked here, so that a case cannot quietly move to another route when a threshold changes"""
    M, din, r = c.B * c.T * c.U1, c.de + c.dd, c.route
    form, sw = form_of(c)
    default = c._replace(opt=None)
    out = [("logits dtype", (form == "fast") == joint_fast(c.prec, c.J))]
    if "tanh-f32" in r or c.prec == 0:
        out.append(("f32 tanh kernels", tanh_route(c) == "f32"))
    if r.startswith("tanh8") and c.prec == 1:
        out.append(("8-column bf16 tanh kernel", tanh_route(c) == "bf16x8" and c.J // 8 in (32, 64, 128, 256)))
    if r.startswith("tanh4") and c.prec == 1:
        out.append(("4-column bf16 tanh kernel", tanh_route(c) == "bf16x4"))
    if "operands" in r:
        out.append(("prec 1 with J % 8 != 0", c.prec == 1 and c.J % 8 != 0 and form == "operands"))
    if "colblocks2" in r:
        out.append(("two column blocks of the backward sums", cdiv(c.J, 1024) == 2 if c.prec == 1 else cdiv(c.J, 256) > 1))
    if "colblocks2-tail" in r:
        out.append(("an inactive tail in the last column block", c.J % 1024 != 0 and (c.J % 1024) // 4 < 256))
    if "atomic-by-size" in r:
        out.append(("2 part + 16 > M J: the atomic kernel by itself", c.prec == 1 and c.opt is None and not two_pass(c) and c.T <= 2))
    elif c.prec == 1 and form == "fast" and "opt21=0" not in r:
        out.append(("two-pass sum", two_pass(c)))
    if "opt21=0" in r:
        out.append(("option 21 = 0 takes the atomics where the default would not", not two_pass(c) and two_pass(default)))
    if "opt19=0" in r:
        out.append(("option 19 = 0 removes a term that exists", not sw["dec_lo"] and form_of(default)[1]["dec_lo"]))
    if "input-fast" in r:
        out.append(("throughput input layer", joint_input_fast(c) and c.B * c.T >= 1024))
    if "input-generic" in r:
        out.append(("generic input layer", not joint_input_fast(c)))
    if "BT1023" in r:
        out.append(("one frame short of the throughput kernels", c.B * c.T == 1023 and joint_input_fast(c._replace(T=c.T + 1))))
    if "de36" in r:
        out.append(("de % 8 != 0", c.de % 8 != 0 and joint_input_fast(c._replace(de=40, B=64)) and not joint_input_fast(c._replace(B=64))))
    if "no-residual" in r:
        out.append(("M < din: no residual terms", M < din and not sw["resid"]))
    elif c.prec == 1:
        out.append(("residual terms", sw["resid"]))
    if "x3-below-worth" in r:
        out.append(("below x3_worth", c.prec == 2 and not x3_worth(M, c.V, c.J)))
    if "x3-h3-one-launch" in r:
        out.append(("three-block rows, one launch", c.prec == 2 and tanh_route(c) == "x3" and M < 4096))
    if "x3-h3-two-blocks" in r:
        out.append(("three-block rows, two blocks", c.prec == 2 and tanh_route(c) == "x3" and M >= 4096))
    if "x3-f32-H-split" in r:
        out.append(("split of an f32 H", c.prec == 2 and x3_worth(M, c.V, c.J) and c.J % 4 != 0 and tanh_route(c) == "f32"))
    if "split-planes" in r:
        out.append(("pre-split planes", c.prec == 2 and x3_worth(M, c.V, c.J)))
    if "de40-dd24" in r:
        out.append(("de != dd", c.de != c.dd))
    if "pitchV+3" in r:
        out.append(("f32 pitch V + 3", c.pad == 3 and not joint_fast(c.prec, c.J)))
    return out


# ---- C: the exp-domain chain at prec 1.  Option 1 = 8 takes the persistent kernels wherever they can run (from 1985 lattice rows, J % 256 == 0, J >= 1024,
# V >= 256: gemm_fast_joint_exp_ok); bias: added to the projection bias, shift: the device scalar subtracted before exp
ExpCase = collections.namedtuple("ExpCase", "route B T U1 de dd J V lens blank opt shift bias")
EXP_CASES = [
    # 8 frames per block with a tail of 3, 2144 rows (pad rows up to 2176), ragged, a label equal to the blank
    ExpCase("E1-tt8-tail3-padrows-label=blank", 2, 67, 16, 16, 8, 1024, 300, ((67, 61), (15, 11)), 0, (1, 8, 4), 0.0, 0.0),
    # 4 frames per block (T < 64), 256 threads per row, V % 8 == 1: the element-wise column tail; an utterance with U_b = 0
    ExpCase("E2-tt4-J2048-V257", 3, 23, 31, 16, 8, 2048, 257, ((23, 20, 9), (30, 12, 0)), 0, (1, 8, 4), 0.0, 0.0),
    # J outside the 8-column kernel's list: 4-column tanh + joint_emis_kernel; ldv == V; logits near 45 under a shift of 10, so that shift_next moves
    ExpCase("E3-J1280-emis-kernel-ldv=V-shift10", 2, 35, 30, 16, 8, 1280, 512, ((35, 30), (29, 20)), 511, (1, 8, 4), 10.0, 45.0),
    # the emis partials exceed 60 KB of LDS (4 frames x 250 labels x 4 waves x 16 bytes = 64 000): joint_emis_kernel; four label slots in the lattice
    ExpCase("E4-U250-emis-lds-fallback", 1, 9, 250, 16, 8, 2048, 300, ((9,), (200,)), 0, (1, 8, 4), 0.0, 0.0),
    # U1 == 1, labels NULL
    ExpCase("E5-U1=1-labels-null", 2, 1003, 1, 16, 8, 1024, 300, ((1003, 700), (0, 0)), 0, (1, 8, 4), 0.0, 0.0),
]
# the default dispatch (option 1 left at 4): the persistent wgrad then asks for V >= 1024 and 32 768 padded rows (tn_v8_eligible), so the case is large - 32 916 rows x 1024 x
# 1024, 3 s per reference on the CPU.  Bias + 7 under a shift of 7.5, blank = V-1
EXP_CASES += [ExpCase("E6-default-dispatch-32916rows-V1024-shift7.5", 3, 211, 52, 16, 8, 1024, 1024, ((211, 180, 97), (51, 30, 12)), 1023, None, 7.5, 7.0)]
EXP_OUT = ("P", "rowsum", "emis0", "emis1", "emis2", "emis3", "lse", "srow", "dlogits", "dz_blank", "dz_label", "costs", "denc", "ddec", "g_wp", "g_wf_e", "g_wf_d", "g_bf", "g_bp")
EXP_CLASS_OF = dict(CLASS_OF, P="P", dlogits="dlogits", rowsum="sums", lse="sums", emis0="emis", emis1="emis", emis2="emis", emis3="emis", srow="srow",
                    dz_blank="dzcol", dz_label="dzcol")
P_SHIFT = 0.37
# Measured G of the exp form (float32 against float64, and shift against shift + 0.37, the larger), worst row or element / worst 90 % quantile over EXP_CASES.
# The shift sets nearly all of them: another placement of bf16's grid under exp(z - shift) moves every row of P by up to 2^-9 and with it everything
# downstream; the float32 run alone is at 1e-3 (rows of P: a flipped bit of H or of P) and 2e-7 where nothing flipped.
#   P 5.9e-3 / 2.1e-3    dlogits 1.2e-2 / 5.2e-3    sums 7.8e-3 / 6.7e-6 (row sums at E6; lse 6.4e-5)    emis 8.0e-4 / 2.5e-5    srow 1.2e-3 / 2.7e-5
#   dzcol 1.5e-1 / 5.3e-3 (the patched label entries at E6)    denc 1.2e-2 / 5.6e-3    ddec 9.1e-3 / 5.5e-3    g_wp 9.0e-3 / 4.5e-3
#   g_wf_e 1.1e-2 / 5.6e-3    g_wf_d 8.1e-3 / 4.6e-3    g_bf 8.3e-3 / 4.4e-3    g_bp 2.1e-2 / 4.2e-3 (U1 250)    costs 1.6e-6 / 1.5e-6
G_EXP_MAX = dict(P=5.9e-3, dlogits=1.2e-2, sums=7.8e-3, emis=8.0e-4, srow=1.2e-3, dzcol=1.5e-1, denc=1.2e-2, ddec=9.1e-3, g_wp=9.0e-3, g_wf_e=1.1e-2, g_wf_d=8.1e-3, g_bf=8.3e-3,
                 g_bp=2.1e-2, costs=1.6e-6)
G_EXP_Q90 = dict(P=2.1e-3, dlogits=5.2e-3, sums=6.7e-6, emis=2.5e-5, srow=2.7e-5, dzcol=5.3e-3, denc=5.6e-3, ddec=5.5e-3, g_wp=4.5e-3, g_wf_e=5.6e-3, g_wf_d=4.6e-3, g_bf=4.4e-3,
                 g_bp=4.2e-3, costs=1.5e-6)
TOL_EXP_MAX = {k: 4 * v for k, v in G_EXP_MAX.items()}
TOL_EXP_Q90 = {k: max(4 * v, 1e-5) for k, v in G_EXP_Q90.items()}
COSTS_ASSERTED_ELSEWHERE = 8e-5      # tests/test_fused_loss_gpu.py test_exp_domain_vs_oracle: the costs' bound here must come out below it, or this one holds
TOL_EXP_COSTS = min(TOL_EXP_MAX["costs"], COSTS_ASSERTED_ELSEWHERE)


def exp_as_case(e):
    return Case(e.route, e.B, e.T, e.U1, e.de, e.dd, e.J, e.V, 1, None, 0, e.lens, e.blank)


def exp_key(e):
    return (e.B, e.T, e.U1, e.de, e.dd, e.J, e.V, e.lens, e.blank, e.bias)


@functools.lru_cache(maxsize=2)
def cached_exp_case(*key):
    B, T, U1, de, dd, J, V, lens, blank, bias = key
    case = joint_case(B, T, U1, de, dd, J, V, lens, blank)
    case["bp"] = case["bp"] + bias
    return case


def emis_route(e):
    """joint_tanh_fwd_emis (csrc/rowops.hip) -> (frames per block of the 8-column kernel or None, does joint_emis_kernel form the entries)"""
    tt = 8 if e.T >= 64 else 4
    part_bytes = tt * e.U1 * (e.J // 8 // 64 if e.J // 8 >= 64 else 1) * 4 * 4
    if e.J in (256, 512, 1024, 2048) and part_bytes <= 60 * 1024:
        return tt, False
    return None, True


def exp_supported(e, cus=256):
    """gemm_fast_joint_exp_ok restated: under option 1 = 8, and (e.opt None) under the default 4 on a device of `cus` compute units"""
    M, ldv = e.B * e.T * e.U1, (e.V + 63) // 64 * 64
    Mp = (M + 63) // 64 * 64
    if e.opt is None:
        nt = lambda m, n, k: m >= 1024 and n >= 256 and k >= 128 and k % 64 == 0 and cdiv(m, 256) * cdiv(n, 128) >= cus * 3 // 4
        return bool(e.J % 8 == 0 and nt(M, e.V, e.J) and nt(M, e.J, ldv) and e.J % 256 == 0 and e.J // 256 >= 4 and Mp >= 32768 and e.V >= 1024)
    nt = lambda m, n, k: m >= 1024 and n >= 256 and k >= 128 and k % 64 == 0
    return bool(e.J % 8 == 0 and nt(M, e.V, e.J) and nt(M, e.J, ldv) and e.J % 256 == 0 and e.J // 256 >= 4 and Mp >= 2048 and e.V >= 256)


def exp_route_conditions(e):
    M, r = e.B * e.T * e.U1, e.route
    tt, fallback = emis_route(e)
    out = [("the persistent kernels take the case under option 1 = 8", exp_supported(e) and e.opt == (1, 8, 4))]
    if "default-dispatch" in r:
        out = [("the default dispatch takes the case", e.opt is None and exp_supported(e) and not exp_supported(e._replace(V=960)) and tt == 8 and not fallback and e.blank == e.V - 1)]
    if "tt8" in r:
        out.append(("8 frames per block", tt == 8 and not fallback))
    if "tail3" in r:
        out.append(("a tail of 3 frames", e.T % 8 == 3))
    if "padrows" in r:
        out.append(("row count no multiple of 64", M % 64 != 0))
    if "tt4" in r:
        out.append(("4 frames per block", tt == 4 and not fallback and e.T % 4 != 0))
    if "J2048" in r:
        out.append(("256 threads per row", e.J // 8 == 256))
    if "V257" in r:
        out.append(("V % 8 == 1", e.V % 8 == 1))
    if "emis-kernel" in r:
        out.append(("J outside the 8-column kernel's list", fallback and e.J not in (256, 512, 1024, 2048) and e.J % 4 == 0))
    if "ldv=V" in r:
        out.append(("ldv == V", e.V % 64 == 0))
    if "emis-lds-fallback" in r:
        out.append(("emis partials over 60 KB", fallback and e.J in (256, 512, 1024, 2048)))
    if "U250" in r:
        out.append(("four label slots", cdiv(e.U1, 64) == 4))
    if "U1=1" in r:
        out.append(("U1 == 1", e.U1 == 1))
    if "label=blank" in r:
        out.append(("a label equal to the blank inside the lattice", e.lens[1][0] > 0))
    return out


def exp_reference(e, dtype=torch.float64, shift=None, defect=None):
    case = cached_exp_case(*exp_key(e))
    _, sw = form_of(exp_as_case(e))
    return exp_ref(case, dtype, e.shift if shift is None else shift, True, emis_route(e)[1], defect, **sw)


def exp_views(out, case, scale=1.0):
    """the outputs of exp_ref (or of the kernels) as the matrices and vectors EXP_OUT names; scale: e^(shift difference) that brings P, its sums and
    1 / srow of a run at another shift to this one's"""
    valid, y, has_label = (np.asarray(out[k]).astype(bool) if k != "y" else np.asarray(out[k]).astype(np.int64) for k in ("valid", "y", "has_label"))
    a = {k: np.asarray(out[k], dtype=np.float64) for k in ("P", "rowsum", "emis", "lse", "srow", "dlogits", "costs", "denc", "ddec", "g_wp", "g_wf_e", "g_wf_d", "g_bf", "g_bp")}
    v = dict(a)
    v["P"], v["rowsum"], v["srow"], v["lse"] = a["P"] * scale, a["rowsum"] * scale, a["srow"] / scale, a["lse"][valid] + np.log(scale)
    for i in range(4):
        v["emis%d" % i] = a["emis"][:, i]
    v["dz_blank"] = a["dlogits"][valid, case["blank"]]
    lab = valid & has_label
    v["dz_label"] = a["dlogits"][lab, y[lab]] if lab.any() else np.zeros(1)
    return v


def exp_errors(got, want, case):
    out = {}
    for k in EXP_OUT:
        g, w = got[k], want[k]
        e = np.abs(g - w) / np.abs(w) if k == "costs" else (lattice_rows_err(g, w, case) if k == "dlogits" else rowwise_err(g, w))
        assert np.isfinite(e).all(), k
        out[k] = (float(e.max()), float(np.quantile(e, 0.9)))
    return out


def exp_gaps(cases=None):
    """{ExpCase: {output: (max, q90)}}: the larger of the float32 run against the float64 run and of the float64 run at shift + P_SHIFT against the one at shift"""
    out = {}
    for e in (EXP_CASES if cases is None else cases):
        case = cached_exp_case(*exp_key(e))
        base = exp_views(exp_reference(e), case)
        e32 = exp_errors(exp_views(exp_reference(e, torch.float32), case), base, case)
        esh = exp_errors(exp_views(exp_reference(e, shift=e.shift + P_SHIFT), case, float(np.exp(P_SHIFT))), base, case)
        out[e] = {k: (max(e32[k][0], esh[k][0]), max(e32[k][1], esh[k][1])) for k in EXP_OUT}
    return out


def exp_gap_summary(gaps):
    gm, gq = {k: 0.0 for k in TOL_EXP_MAX}, {k: 0.0 for k in TOL_EXP_MAX}
    for g in gaps.values():
        for k, (m, q) in g.items():
            cl = EXP_CLASS_OF[k]
            gm[cl], gq[cl] = max(gm[cl], m), max(gq[cl], q)
    return gm, gq
