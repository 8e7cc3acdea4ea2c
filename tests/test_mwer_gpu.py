"""Per-utterance weights on the fused joint + loss, and Transducer.mwer_loss (minimum word error rate training on the N-best list), against
compositions of the ops that existed before them: the two-call form with MATERIALISED logits and torch autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err
from edit_oracle import edit_counts
from test_fused_loss_gpu import _run, _training_sized
from test_model_gpu import build

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["tiny_klong", "tiny_kshort"])
def gm(request):
    z, sd = load_golden(request.param)
    return z, sd, build(sd)


def _grads(model, inp):
    return inp.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _same_gradients(got, want, tol):
    assert rel_err(got[0].cpu().numpy(), want[0].cpu().numpy()) < tol
    assert set(got[1]) == set(want[1])
    for n in want[1]:
        assert rel_err(got[1][n].cpu().numpy(), want[1][n].cpu().numpy()) < tol, n


# ------------------------------------------------------------------ 1. utterance_weights against the two-call form
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_utterance_weights_vs_two_call_form(gm, prec, chunk, reduction, monkeypatch):
    z, sd, model = gm
    from warprnnt_pytorch import RNNTLoss
    monkeypatch.setenv("TTMI_PRECISION", prec)
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    tgt = torch.tensor(z["targets"], device="cuda")
    al, ll = torch.tensor(z["ragged/act_lens"], device="cuda"), torch.tensor(z["ragged/label_lens"], device="cuda")
    tol = 1e-5 if prec == "fp32" else 1e-2                   # tests/test_fused_loss_gpu.py: fused against two-call
    for w in ([0.0, -0.75], [2.5, 0.0], [1.75, -0.5]):       # a zero, a negative and a non-unit entry, in either position
        for dtype in (torch.float32, torch.float64):
            wt = torch.tensor(w, dtype=dtype, device="cuda")
            model.zero_grad()
            inp = torch.tensor(z["inputs"], device="cuda", requires_grad=True)
            costs = RNNTLoss(reduction="none", check_lengths=False)(model(inp, tgt), tgt.int(), al, ll)
            want = (costs * wt.float()).sum() / (2.0 if reduction == "mean" else 1.0)
            want.backward()
            ref = _grads(model, inp)
            model.zero_grad()
            inp = torch.tensor(z["inputs"], device="cuda", requires_grad=True)
            got = model.loss(inp, al, tgt, ll, reduction=reduction, chunk=chunk, check_lengths=False, utterance_weights=wt)
            assert got.shape == (1,) and got.dtype is torch.float32
            assert abs(float(got.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
            got.backward()
            _same_gradients(_grads(model, inp), ref, tol)
            assert wt.grad is None


def test_utterance_weights_contract(gm):
    z, sd, model = gm
    inp, tgt = torch.tensor(z["inputs"], device="cuda"), torch.tensor(z["targets"], device="cuda")
    al, ll = torch.tensor(z["ragged/act_lens"], device="cuda"), torch.tensor(z["ragged/label_lens"], device="cuda")
    ones = torch.ones(2, device="cuda")
    with pytest.raises(ValueError):
        model.loss(inp, al, tgt, ll, reduction="none", check_lengths=False, utterance_weights=ones)
    with pytest.raises(ValueError):
        model.loss(inp, al, tgt, ll, check_lengths=False, utterance_weights=ones.cpu())
    with pytest.raises(ValueError):
        model.loss(inp, al, tgt, ll, check_lengths=False, utterance_weights=torch.ones(3, device="cuda"))
    with pytest.raises(ValueError):
        model.loss(inp, al, tgt, ll, check_lengths=False, utterance_weights=torch.ones(2, dtype=torch.int32, device="cuda"))
    # w = 1: the bits of the call without weights, value and gradients
    res = []
    for w in (None, ones):
        model.zero_grad()
        x = inp.clone().requires_grad_(True)
        loss = model.loss(x, al, tgt, ll, reduction="mean", chunk=2, check_lengths=False, utterance_weights=w)
        loss.backward()
        res.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert rel_err(res[1][1].cpu().numpy(), res[0][1].cpu().numpy()) < 1e-6       # (the weight gradients' atomic sums: not bit-stable run to run)


# ------------------------------------------------------------------ 2. utterance_weights on the exp-domain form
def test_utterance_weights_exp_domain(monkeypatch):
    """B = 8, T = 200, U = 20 in one chunk, the second call after seeding: the exp-domain kernels with per-utterance weights are as close to the
    fp32 pipeline with the same weights as the plain bf16 form is (the bound of test_exp_domain_fast_path, measured the same way)"""
    import ttmi.ops as ops
    model, x, y, al, ll = _training_sized(monkeypatch, "fp32")
    w = torch.tensor([1.0, 0.0, -0.5, 2.0, 0.25, 1.5, -1.25, 0.75], device="cuda")
    ref = _run(model, x, y, al, ll, chunk=8, utterance_weights=w)
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    plain = _run(model, x, y, al, ll, chunk=8, utterance_weights=w)
    calls = []
    orig = ops.joint_fwd_exp
    monkeypatch.setattr(ops, "joint_fwd_exp", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    seed = _run(model, x, y, al, ll, chunk=8, exp_domain=True, utterance_weights=w)
    assert not calls and seed[0] == plain[0]
    fast = _run(model, x, y, al, ll, chunk=8, exp_domain=True, utterance_weights=w)
    assert calls, "the exp-domain kernels did not run"
    e_plain, e_fast = rel_err(plain[1], ref[1]), rel_err(fast[1], ref[1])
    print("weighted loss fp32 %.4f  bf16 %.4f  exp-domain %.4f;  gradient error vs fp32: bf16 %.2e, exp-domain %.2e" % (ref[0], plain[0], fast[0], e_plain, e_fast))
    assert e_fast < max(1.5 * e_plain, 5e-3)


# ------------------------------------------------------------------ 3. mwer_loss with given hypotheses against a composition of existing ops
def _hypotheses(z):
    tgt, ll = z["targets"], z["ragged/label_lens"]
    t0, t1 = [int(v) for v in tgt[0, :ll[0]]], [int(v) for v in tgt[1, :ll[1]]]
    other = lambda t: t % 47 + 1                              # another symbol of [1, 48)
    h0 = [t0, [], t0[:3] + [other(t0[3])] + t0[3:] + [other(t0[0])], t0[:2] + [other(t0[2])] + t0[3:]]      # itself, empty, longer, one token differs
    h1 = [t1[:1] + [other(t1[1])] + t1[2:], t1, [t1[0]]]
    return [h0, h1], [t0, t1]


def _yardstick(model, z, hyps, refs, rnnt_weight):
    """the definition, on materialised logits, in torch float64 with autograd: -> value, costs, errors, per-row weights, gradients"""
    from warprnnt_pytorch import RNNTLoss
    B = len(hyps)
    rows = [(b, h) for b, hs in enumerate(hyps) for h in hs]
    n_hyp = len(rows)
    if rnnt_weight > 0:
        rows += [(b, refs[b]) for b in range(B)]
    U = max([1] + [len(h) for _, h in rows[:n_hyp]] + ([z["targets"].shape[1]] if rnnt_weight > 0 else []))
    labels = torch.tensor([h + [0] * (U - len(h)) for _, h in rows], device="cuda")
    ll = torch.tensor([len(h) for _, h in rows], dtype=torch.int32, device="cuda")
    row_utt = torch.tensor([b for b, _ in rows], device="cuda")
    al = torch.tensor(z["ragged/act_lens"], device="cuda")[row_utt].contiguous()
    W = torch.tensor([edit_counts(h, refs[b])[0] for b, h in rows], dtype=torch.float64, device="cuda")
    model.zero_grad()
    inp = torch.tensor(z["inputs"], device="cuda", requires_grad=True)
    enc = model.encoder(inp, model._audio_mask(inp))
    dec = model._label_states(F.pad(labels, pad=[1, 0, 0, 0], value=0))
    logits = model.joint(enc.index_select(0, row_utt), dec)
    costs = RNNTLoss(reduction="none", check_lengths=False)(logits, labels.int(), al, ll)
    costs.retain_grad()
    c = costs.double()
    value = 0.0
    for b in range(B):
        sel = [k for k in range(n_hyp) if rows[k][0] == b]
        P = torch.softmax(-c[sel], dim=0)
        value = value + (P * W[sel]).sum() / B
    if rnnt_weight > 0:
        value = value + rnnt_weight * c[n_hyp:].mean()
    value.backward()
    return float(value.detach()), costs.detach().clone(), W.int(), costs.grad.double(), _grads(model, inp), row_utt[:n_hyp]


@pytest.mark.parametrize("rnnt_weight", [0.0, 0.5])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mwer_loss_vs_composition_of_existing_ops(gm, prec, rnnt_weight, monkeypatch):
    """the rows run as ONE chunk here: the library picks its GEMM kernels by row count, so only then do the fused op and the materialising
    two-call form run the same kernels on the same shapes - the condition under which their per-utterance costs are the same bits.  Chunks of 3
    rows (a ragged last chunk) follow in fp32 under the bounds that a different summation order inside the joint's products allows."""
    z, sd, model = gm
    monkeypatch.setenv("TTMI_PRECISION", prec)
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    hyps, refs = _hypotheses(z)
    want_value, want_costs, want_W, want_w, want_grads, row_utt = _yardstick(model, z, hyps, refs, rnnt_weight)
    tgt = torch.tensor(z["targets"], device="cuda")
    tgt[1, 4:] = 17                                          # pads behind the transcript are not tokens
    al, ll = torch.tensor(z["ragged/act_lens"], device="cuda"), torch.tensor(z["ragged/label_lens"], device="cuda")
    model.zero_grad()
    inp = torch.tensor(z["inputs"], device="cuda", requires_grad=True)
    loss, det = model.mwer_loss(inp, al, tgt, ll, hypotheses=hyps, rnnt_weight=rnnt_weight, details=True)
    assert loss.shape == (1,) and det.hypotheses == hyps
    assert det.costs.dtype is torch.float32 and torch.equal(det.costs, want_costs)
    assert det.errors.dtype is torch.int32 and torch.equal(det.errors, want_W)
    assert det.posteriors.dtype is torch.float64 and det.expected_errors.shape == (2,) and det.expected_errors.dtype is torch.float64
    print("value %.12f (yardstick %.12f), expected errors %s" % (float(loss.detach()), want_value, det.expected_errors.tolist()))
    assert abs(float(loss.detach()) - want_value) <= 1e-9 * abs(want_value)
    loss.backward()
    _same_gradients(_grads(model, inp), want_grads, 1e-5 if prec == "fp32" else 1e-2)
    if rnnt_weight == 0.0:
        from ttmi.metrics import mwer_weights
        w = mwer_weights(det.costs, det.errors, row_utt, 2).weights
        assert (w - want_w).abs().max() <= 1e-6 * want_w.abs().max()          # (autograd hands the weights on through the f32 costs)
        for b in range(2):
            assert abs(float(w[row_utt == b].sum())) < 1e-12
            assert abs(float(det.posteriors[row_utt == b].sum()) - 1.0) < 1e-12
    if prec == "fp32":
        # chunks of 3 + 3 + 1 (+ 2) rows: other GEMM kernels by row count, so the f32 costs may move by a few ulp (2^-23 each; 1e-6 allows 8)
        # and with them P_i by 2 x 170 x 1e-6 relative (costs of about 170 nats): the value within 5e-4
        with torch.no_grad():
            v3, d3 = model.mwer_loss(inp, al, tgt, ll, hypotheses=hyps, rnnt_weight=rnnt_weight, chunk=3, details=True)
        assert torch.equal(d3.errors, want_W)
        assert ((d3.costs - want_costs).abs() <= 1e-6 * want_costs.abs()).all()
        assert abs(float(v3) - want_value) <= 5e-4 * abs(want_value)


# ------------------------------------------------------------------ 4. the search path
def test_mwer_loss_search_path(gm):
    z, sd, model = gm
    inp = torch.tensor(z["inputs"], device="cuda")
    tgt = torch.tensor(z["targets"], device="cuda")
    al = torch.tensor([40, 1], dtype=torch.int32, device="cuda")          # an utterance of one frame
    ll = torch.tensor(z["ragged/label_lens"], device="cuda")
    model.eval()
    nbest = model.recognize_nbest(inp, al, beam_width=4)
    want = [[list(h.tokens) for h in res] for res in nbest]
    assert all(1 <= len(hs) <= 4 for hs in want) and all(len(h) <= 1 for h in want[1])
    for training in (True, False):
        model.train(training)
        a, det = model.mwer_loss(inp, al, tgt, ll, beam_width=4, details=True)
        assert model.training is training
        assert det.hypotheses == want
        b = model.mwer_loss(inp, al, tgt, ll, hypotheses=want)
        assert torch.equal(a, b)
    two, det2 = model.mwer_loss(inp, al, tgt, ll, beam_width=4, nbest=2, details=True)
    assert det2.hypotheses == [hs[:2] for hs in want]
    # an exception inside the search leaves the mode as it was
    model.train()
    with pytest.raises(ValueError):
        model.mwer_loss(inp, al, tgt, ll, beam_width=99)
    assert model.training
    model.eval()


# ------------------------------------------------------------------ 5. edges
def test_mwer_loss_edges(gm):
    z, sd, model = gm
    tgt = torch.tensor(z["targets"], device="cuda")
    al, ll = torch.tensor(z["ragged/act_lens"], device="cuda"), torch.tensor(z["ragged/label_lens"], device="cuda")
    # every hypothesis of the batch is empty: all deletions, one hypothesis per utterance, nothing to learn
    model.zero_grad()
    inp = torch.tensor(z["inputs"], device="cuda", requires_grad=True)
    loss, det = model.mwer_loss(inp, al, tgt, ll, hypotheses=[[[]], [[]]], details=True)
    assert float(loss.detach()) == float(ll.double().mean()) and det.errors.tolist() == ll.tolist() and det.posteriors.tolist() == [1.0, 1.0]
    loss.backward()
    assert inp.grad is None or not inp.grad.any()
    assert all(p.grad is None or not p.grad.any() for p in model.parameters())
    # one hypothesis next to four
    hyps, refs = _hypotheses(z)
    hyps = [hyps[0], [hyps[1][0]]]
    model.zero_grad()
    loss, det = model.mwer_loss(inp, al, tgt, ll, hypotheses=hyps, details=True)
    assert float(det.posteriors[4]) == 1.0 and float(det.expected_errors[1]) == float(edit_counts(hyps[1][0], refs[1])[0])
    want = sum(float(det.posteriors[k]) * edit_counts(hyps[0][k], refs[0])[0] for k in range(4))
    assert abs(float(det.expected_errors[0]) - want) < 1e-9
    assert abs(float(loss.detach()) - float(det.expected_errors.mean())) < 1e-12
    loss.backward()
    assert torch.isfinite(inp.grad).all()
    # no graph, no second pass
    with torch.no_grad():
        again = model.mwer_loss(inp, al, tgt, ll, hypotheses=hyps)
    assert torch.equal(again, loss.detach()) and not again.requires_grad
    good = _hypotheses(z)[0]
    with pytest.raises(ValueError):
        model.mwer_loss(inp, al, tgt, ll, hypotheses=[good[0] + [good[0][0]], good[1]])        # a duplicate within an utterance
    with pytest.raises(ValueError):
        model.mwer_loss(inp, al, tgt, ll, hypotheses=[good[0], []])                            # an utterance without a hypothesis
    with pytest.raises(ValueError):
        model.mwer_loss(inp, al, tgt, ll, hypotheses=[good[0], [[1, 48]]])                     # a token outside [0, V)
    with pytest.raises(ValueError):
        model.mwer_loss(inp, al, tgt, ll, hypotheses=[good[0], [[-1]]])
    with pytest.raises(ValueError):
        model.mwer_loss(inp.detach().cpu(), al, tgt, ll, hypotheses=good)                      # CPU inputs


# ------------------------------------------------------------------ 6. the logits never exist whole
def test_mwer_loss_never_holds_the_logits(monkeypatch):
    """B = 4 with four hypotheses each at T = 200, U = 20, V = 4334 (bf16 pipeline), chunks of 2 rows: the step's peak memory above its
    baseline stays below the [16, T, U + 1, 4352] bf16 logits that any materialising implementation has to hold"""
    model, x, y, al, ll = _training_sized(monkeypatch, "bf16")
    B, T, U = 4, 200, 20
    x, y, al, ll = x[:B].contiguous(), y[:B].contiguous(), al[:B].contiguous(), ll[:B].contiguous()
    g = torch.Generator().manual_seed(9)
    hyps = [[torch.randint(1, 4334, (U - k,), generator=g).tolist() for k in range(4)] for _ in range(B)]
    model.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = model.mwer_loss(x, al, y, ll, hypotheses=hyps, rnnt_weight=0.0, chunk=2)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    logits_bytes = 16 * T * (U + 1) * 4352 * 2
    print("mwer_loss peak above baseline: %.0f MB (whole logits: %.0f MB)" % (peak / 2 ** 20, logits_bytes / 2 ** 20))
    assert torch.isfinite(loss).all() and all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert peak < logits_bytes
