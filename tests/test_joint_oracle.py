"""The reference of tests/joint_oracle.py checked against the project's oracle and torch autograd, its exp-domain form against the exact chain, the
preconditions of its inputs, the tolerances tied to its own float32 / float64 distance, every case's route, and seven planted defects (each must move a
row or an element by at least twice its bound, so that tests/test_joint_rows_gpu.py would fail on it).  CPU only."""
import numpy as np
import pytest
import torch

import joint_oracle as R
from oracle import tt_oracle as O


def _small(lens=((9, 6), (4, 2)), blank=3, U1=5):
    return R.joint_case(2, 9, U1, 16, 8, 64, 70, lens=lens, blank=blank)


def _sd(case):
    return {"joint.forward_layer.weight": case["wf"].numpy(), "joint.forward_layer.bias": case["bf"].numpy(),
            "joint.project_layer.weight": case["wp"].numpy(), "joint.project_layer.bias": case["bp"].numpy()}


def _oracle_joint(case, dz):
    sd, grads = _sd(case), {}
    z, cache = O.joint_fwd(case["enc"].numpy(), case["dec"].numpy(), sd)
    denc, ddec = O.joint_bwd(dz.reshape(z.shape), cache, sd, grads)
    de = case["de"]
    g_wf = grads["joint.forward_layer.weight"]
    return dict(logits=z.reshape(-1, z.shape[-1]), denc=denc.reshape(-1, de), ddec=ddec.reshape(-1, case["dd"]), g_wp=grads["joint.project_layer.weight"],
                g_wf_e=g_wf[:, :de], g_wf_d=g_wf[:, de:], g_bf=grads["joint.forward_layer.bias"], g_bp=grads["joint.project_layer.bias"])


def test_exact_reference_equals_the_oracle():
    case = _small()
    got = R.joint_ref(case)
    want = _oracle_joint(case, case["dz"].numpy())
    for k in R.JOINT_OUT:
        assert np.abs(got[k].numpy() - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    # with the lattice: the costs and the loss gradient of oracle.tt_oracle.rnnt_loss on the oracle's own logits, and the joint's gradients of that
    z4 = want["logits"].reshape(2, 9, 5, 70)
    costs, _, grad = O.rnnt_loss(z4, case["labels"], case["act_lens"], case["label_lens"], blank=case["blank"], reduction="none")
    chain = R.chain_ref(case)
    assert np.abs(chain["costs"].numpy() - costs).max() <= 1e-12 * np.abs(costs).max()
    assert np.abs(chain["dlogits"].numpy() - grad.reshape(-1, 70)).max() <= 1e-12
    want = _oracle_joint(case, grad)
    for k in R.JOINT_OUT:
        assert np.abs(chain[k].numpy() - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k


def test_exact_reference_equals_autograd():
    case = _small()
    t = {k: case[k].clone().requires_grad_(True) for k in ("enc", "dec", "wf", "bf", "wp", "bp")}
    de = case["de"]
    pre = (t["enc"] @ t["wf"][:, :de].T)[:, :, None] + (t["dec"] @ t["wf"][:, de:].T)[:, None] + t["bf"]
    z = torch.tanh(pre).reshape(-1, case["J"]) @ t["wp"].T + t["bp"]
    (z * case["dz"]).sum().backward()
    got = R.joint_ref(case)
    want = dict(logits=z.detach(), denc=t["enc"].grad.reshape(-1, de), ddec=t["dec"].grad.reshape(-1, case["dd"]), g_wp=t["wp"].grad, g_wf_e=t["wf"].grad[:, :de],
                g_wf_d=t["wf"].grad[:, de:], g_bf=t["bf"].grad, g_bp=t["bp"].grad)
    for k in R.JOINT_OUT:
        assert float((got[k] - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), k


@pytest.mark.parametrize("lens,blank,U1", [(((9, 6), (4, 2)), 0, 5), (((9, 6), (4, 0)), 3, 5), (((9, 6), (4, 2)), 69, 5), (((9, 3), (0, 0)), 0, 1)],
                         ids=["label=blank", "blank3-Ub0", "blank=V-1", "U1=1"])
@pytest.mark.parametrize("shift", [0.0, 1.5])
def test_exp_form_with_nothing_rounded_is_the_exact_chain(lens, blank, U1, shift):
    """srow * P with its patched blank / label entries IS d logits, and the row sums with the two columns exchanged give the same costs: to 1e-10, with a
    label equal to the blank (joint_case plants labels[0][0] = blank), a nonzero blank and U1 == 1"""
    case = _small(lens, blank, U1)
    if U1 > 1:
        assert case["labels"][0, 0] == blank and case["label_lens"][0] > 0
    exact = R.chain_ref(case)
    got = R.exp_ref(case, shift=shift, rounded=False)
    assert float((got["costs"] - exact["costs"]).abs().max()) <= 1e-10 * float(exact["costs"].abs().max())
    assert float((got["dlogits"] - exact["dlogits"]).abs().max()) <= 1e-10
    for k in R.JOINT_OUT:
        assert float((got[k] - exact[k]).abs().max()) <= 1e-10 * max(1.0, float(exact[k].abs().max())), k
    outside = ~got["valid"].bool()
    assert float(got["srow"][outside].abs().max() if outside.any() else 0.0) == 0.0


def _all_inputs():
    seen = {}
    for c in R.CASES:
        seen.setdefault(R.input_key(c), (c, R.cached_case))
    for e in R.EXP_CASES:
        seen.setdefault(R.exp_key(e), (R.exp_as_case(e), R.cached_exp_case))
    return seen


def test_input_preconditions_and_conditioning():
    """no tanh pre-activation beyond +-4 (asserted by the builder: building is the test), logits of standard deviation near 2, and the exact form in float32
    within 2.5e-5 of float64 on every case's inputs: the precondition of the 1e-4 contract"""
    worst = 0.0
    for key, (c, build) in _all_inputs().items():
        case = build(*key)
        assert case["max_pre"] <= R.MAX_PRE
        ref = (R.joint_ref if c.lens is None else R.chain_ref)
        keys = R.out_keys(c)
        a, b = ref(case), ref(case, dtype=torch.float32)
        std = float((a["logits"] - a["logits"].mean()).std())
        assert 1.5 < std < 2.5, (key, std)
        e = R.errors(b, a, case, keys)
        worst = max(worst, max(v[0] for v in e.values()))
        assert worst < R.COND_EXACT, (key, e)
    print("exact form, float32 against float64, worst row or element: %.1e" % worst)


def test_every_route_of_the_table_is_named_and_reached():
    for c in R.CASES:
        for what, ok in R.route_conditions(c):
            assert ok, (R.case_id(c), what)
    for e in R.EXP_CASES:
        for what, ok in R.exp_route_conditions(e):
            assert ok, (e.route, what)
    ids = " ".join(R.case_id(c) for c in R.CASES)
    for word in ("tanh-f32", "tanh8-J256", "tanh8-J512", "tanh8-J1024", "tanh8-J2048", "tanh4-J8", "tanh4-J264", "tanh4-J1032", "operands-J36", "colblocks2", "opt21=0",
                 "atomic-by-size", "input-fast", "input-generic-BT1023", "de36", "no-residual", "de40-dd24", "opt19=0", "x3-below-worth", "x3-h3-one-launch",
                 "x3-h3-two-blocks", "x3-f32-H-split", "pitchV+3", "split-planes", "Ub0", "Tb1", "label=blank", "blank=V-1", "U65", "U129"):
        assert word in ids, word
    assert {c.T for c in R.JOINT_CASES} >= {1, 2, 3, 17, 35} and {c.U1 for c in R.CASES} >= {1, 2, 9, 65, 129} and {c.V for c in R.JOINT_CASES} >= {5, 64, 70, 300}
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)


def _tied(G, TOL, floor=None):
    for k in TOL:
        if floor is not None and TOL[k] == floor and 4 * G[k] <= floor:
            continue
        assert 2 * G[k] <= TOL[k] <= 8 * G[k], (k, G[k], TOL[k])


def test_tolerances_are_tied_to_the_reference():
    """2 G <= TOL <= 8 G per output class with G re-measured here: the float32 run of the reference against its float64 run in the same form over every
    prec-1 case, for the exp form also against the run at shift + 0.37"""
    gm, gq = R.gap_summary(R.reference_gaps())
    print("G_MAX", {k: "%.2g" % v for k, v in gm.items()}, "G_Q90", {k: "%.2g" % v for k, v in gq.items()})
    _tied(gm, R.TOL_MAX)
    _tied(gq, R.TOL_Q90, 1e-5)
    gm, gq = R.exp_gap_summary(R.exp_gaps())
    print("G_EXP_MAX", {k: "%.2g" % v for k, v in gm.items()}, "G_EXP_Q90", {k: "%.2g" % v for k, v in gq.items()})
    _tied(gm, R.TOL_EXP_MAX)
    _tied(gq, R.TOL_EXP_Q90, 1e-5)
    assert R.TOL_EXP_COSTS == R.TOL_EXP_MAX["costs"] < R.COSTS_ASSERTED_ELSEWHERE


def test_three_term_logits_set_the_floor_of_prec_2():
    """the bf16x3 number format alone (reference with three-term logits, float64 otherwise) keeps every loss-gradient row within 1e-4 at FLOOR_DLOGITS_X3 and
    does not at FLOOR_DLOGITS: why prec 2 has a floor of its own where its projection runs in three terms"""
    c = next(c for c in R.CHAIN_CASES if "split-planes" in c.route)
    assert R.floor_of(c) == R.FLOOR_DLOGITS_X3 and R.floor_of(c._replace(prec=0)) == R.FLOOR_DLOGITS
    case = R.cached_case(*R.input_key(c))
    want = R.chain_ref(case)["dlogits"].numpy()
    for g in R.x3_chain_dlogits(case):
        assert R.lattice_rows_err(g.numpy(), want, case, R.FLOOR_DLOGITS_X3).max() < 0.6 * R.TOL_EXACT
        assert R.lattice_rows_err(g.numpy(), want, case, R.FLOOR_DLOGITS).max() > R.TOL_EXACT


def _case(route, prec=1):
    return next(c for c in R.CASES if c.route == route and c.prec == prec)


def _moved(bad, good, case, keys, tol, class_of):
    """the largest (error of a row or element) / (its bound) over the outputs"""
    e = R.errors(bad, good, case, keys)
    return max(e[k][0] / tol[class_of[k]] for k in keys)


@pytest.mark.parametrize("route,defect", [
    ("tanh8-J256-T17-U2-V64", ("ddec_tail_twice", 1, 1)),                  # 1: the last frame of a ragged 16-frame block summed from the clamped address
    ("tanh4-J1032-T35-U2-colblocks2-tail", ("ddec_tail_twice", 0, 0)),      #    ... of a block of 3 frames
    ("tanh8-J256-T17-U2-V64", ("g_wf_shift",)),                             # 3: the label half of g_wf one column early
    ("tanh4-J1032-T35-U2-colblocks2-tail", ("part_row_lost", 1, 1, 1)),     # 6: one 16-frame partial row of one label state left out
    ("chain-J256-T17-U9-Ub0-Tb1-label=blank", ("part_row_lost", 0, 3, 0)),
], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_planted_defects_of_the_joint_are_seen(route, defect):
    for prec in (0, 1):
        c = _case(route, prec)
        case = R.cached_case(*R.input_key(c))
        good, bad = R.reference(c), R.reference(c, defect=defect)
        assert _moved(bad, good, case, R.out_keys(c), R.tolerances(c)[0], R.CLASS_OF) >= 2.0, (prec, defect)


@pytest.mark.parametrize("defect", [("emis_last_label",), ("srow_outside", 1, 66), ("blank_patch_no_rl",), ("g_bp_unweighted", 17)], ids=lambda d: d[0])
def test_planted_defects_of_the_exp_chain_are_seen(defect):
    """2: the row u = U1-1 given labels[b][U1-2]'s logit for the blank's in emis; 4: srow nonzero on a row t >= T_b; 5: the blank patch without rl where the label
    equals the blank; 7: one vocabulary row's share of g_bp from the unweighted column sum - on E1 (ragged 61 of 67 frames, labels[0][0] = blank)"""
    e = R.EXP_CASES[0]
    case = R.cached_exp_case(*R.exp_key(e))
    assert e.lens[0][1] <= 66 < e.T and case["labels"][0, 0] == e.blank
    good, bad = R.exp_views(R.exp_reference(e), case), R.exp_views(R.exp_reference(e, defect=defect), case)
    err = R.exp_errors(bad, good, case)
    assert max(err[k][0] / R.TOL_EXP_MAX[R.EXP_CLASS_OF[k]] for k in R.EXP_OUT if k != "costs") >= 2.0, (defect, err)
