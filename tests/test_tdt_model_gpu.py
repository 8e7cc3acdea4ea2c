"""A token-and-duration model (config.tdt_durations) through the Python layers, on the tiny two-layer Transducer of tests/test_mono_model_gpu.py
with tdt_durations = [1, 2, 3]: Transducer.loss against model(inputs, targets) + TDTLoss (the project's 1e-4, as the monotonic forms are held
to each other), both against the float64 oracle (tests/tdt_oracle.py) chained through torch autograd on float64 copies of the joint network,
and recognize / decode_batch against the oracle decoder on the model's own f32 joint rows."""
import numpy as np
import pytest
import torch

import tdt_oracle as O
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
B, T, U, D, V = 3, 12, 5, 64, 29
DUR = [1, 2, 3]
ACT, LAB = [12, 10, 7], [5, 3, 0]


def _model(seed=9, **extra):
    from tt.model import Transducer
    from tt.utils import AttrDict
    side = dict(n_layer=2, d_model=D, n_head=2, d_head=32, d_inner=96)
    cfg = AttrDict(dict(enc=dict(side, max_input_length=16), dec=dict(side, max_target_length=8),
                        joint=dict(input_size=128, inner_size=48), vocab_size=V, dropout=0.0, **extra))
    torch.manual_seed(seed)
    return Transducer(cfg).cuda().eval()


def _tdt_model(**extra):
    return _model(tdt_durations=DUR, **extra)


def _batch():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, D, generator=g).cuda()
    y = torch.randint(1, V, (B, U), generator=g).cuda()
    return x, y, torch.tensor(ACT, dtype=torch.int32, device="cuda"), torch.tensor(LAB, dtype=torch.int32, device="cuda")


def _grads(model, xi):
    return torch.cat([xi.grad.reshape(-1)] + [p.grad.reshape(-1) for p in model.parameters()]).double().cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_loss_equals_the_two_call_form(prec, monkeypatch):
    """Transducer.loss (chunk default and chunk = 1) against model(inputs, targets) + TDTLoss, on materialised logits and on the handle of the
    bf16 pipeline (which TDTLoss materialises)"""
    import tt.model as TM
    from ttmi.tdt import TDTLoss
    monkeypatch.setenv("TTMI_PRECISION", prec)
    model = _tdt_model()
    assert model.tdt_durations == (1, 2, 3) and model.joint.project_layer.out_features == V + 3
    x, y, al, ll = _batch()
    crit = TDTLoss(DUR, check_lengths=False)
    res = []
    for form in ("materialised", "deferred", "fused", "fused_chunk1"):
        monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1" if form == "deferred" else "0")
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        if form.startswith("fused"):
            loss = model.loss(xi, al, y, ll, check_lengths=False, **({"chunk": 1} if form.endswith("1") else {}))
        else:
            lg = model(xi, y)
            assert isinstance(lg, TM.DeferredLogits) == (form == "deferred") and lg.shape[-1] == V + 3
            loss = crit(lg, y.int(), al, ll)
        (loss * 4.0).sum().backward()
        res.append((loss.detach().double().cpu().numpy(), _grads(model, xi)))
    for name, (loss, grads) in zip(("deferred", "fused", "fused chunk 1"), res[1:]):
        print("%s %s: loss %.7f against %.7f, gradient rel err %.2e" % (prec, name, loss[0], res[0][0][0], rel_err(grads, res[0][1])))
        # bf16, chunk = 1: one-utterance chunks run other GEMM variants of the joint, whose bf16 partial products round differently - the
        # bound tests/test_fused_loss_gpu.py has for that case (1e-2); the lattice kernels see one utterance at a time either way
        assert loss.shape == (1,) and rel_err(loss, res[0][0]) < TOL, name
        if prec == "bf16" and name == "fused chunk 1":
            assert rel_err(grads, res[0][1]) < 1e-2, name
        else:
            assert rel_err(grads, res[0][1]) < TOL, name                               # the form equality: 1e-4
    assert np.isfinite(res[0][1]).all() and np.abs(res[0][1]).max() > 0


def _oracle_through_the_joint(model, enc, dec, y):
    """float64 torch copy of the joint on the model's states, the oracle's cost and d cost / d logits chained into states and parameters"""
    j = model.joint
    e64, d64, wf, bf, wp, bp = (t.detach().double().cpu().requires_grad_(True)
                                for t in (enc, dec, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias))
    h = torch.tanh((e64 @ wf[:, :D].t())[:, :, None, :] + (d64 @ wf[:, D:].t())[:, None, :, :] + bf)
    z = h @ wp.t() + bp
    want_c, want_g = O.tdt_loss(z.detach().numpy(), y.cpu().numpy(), ACT, LAB, tuple(DUR))
    z.backward(torch.tensor(want_g / B))
    return want_c, (e64, d64, wf, bf, wp, bp)


def test_gradients_against_the_oracle_through_the_joint(monkeypatch):
    """fp32 mode, both forms: TDTLoss on the joint's logits, and Transducer.loss's chunk form driven on the same states"""
    import tt.model as TM
    from ttmi import ops
    from ttmi.tdt import TDTLoss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _tdt_model()
    x, y, al, ll = _batch()
    with torch.no_grad():
        enc, dec = model._encode(x, y)
    j = model.joint
    want_c, want = _oracle_through_the_joint(model, enc, dec, y)
    for form in ("two_call", "fused"):
        e, d = enc.clone().requires_grad_(True), dec.clone().requires_grad_(True)
        model.zero_grad()
        if form == "two_call":
            loss = TDTLoss(DUR, check_lengths=False)(j(e, d), y.int(), al, ll)
        else:
            loss = TM._JointLossFn.apply(e, d, j.forward_layer.weight, j.forward_layer.bias, j.project_layer.weight, j.project_layer.bias,
                                         y.int().contiguous(), al, ll, TM.default_precision(), 2, "mean", None, True, 0, 0.0, None,
                                         ops.TDTLattice(DUR))
        loss.backward()
        got = [e.grad, d.grad, j.forward_layer.weight.grad, j.forward_layer.bias.grad, j.project_layer.weight.grad, j.project_layer.bias.grad]
        print("%s: loss %.7f, oracle %.7f" % (form, float(loss.detach()), want_c.mean()))
        assert abs(float(loss.detach()) - want_c.mean()) <= TOL * want_c.mean()
        for name, a, b in zip(("enc", "dec", "wf", "bf", "wp", "bp"), got, want):
            print("  d %s rel err %.2e" % (name, rel_err(a.cpu().numpy(), b.grad.numpy())))
            assert rel_err(a.cpu().numpy(), b.grad.numpy()) < TOL, (form, name)
    assert float(j.project_layer.weight.grad[V:].abs().max()) > 0                    # the duration rows learn


def test_utterance_weights_reduction_none_and_ctc_weight(monkeypatch):
    from ttmi.tdt import TDTLoss
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "0")
    model = _tdt_model()
    x, y, al, ll = _batch()
    w = torch.tensor([1.75, 0.0, -0.5], device="cuda")
    model.zero_grad()
    xi = x.clone().requires_grad_(True)
    costs = TDTLoss(DUR, reduction="none", check_lengths=False)(model(xi, y), y.int(), al, ll)
    assert costs.shape == (B,)
    (costs * w).sum().backward()
    ref = _grads(model, xi)
    with torch.no_grad():
        none = model.loss(x, al, y, ll, reduction="none", check_lengths=False)
    assert none.shape == (B,) and rel_err(none.cpu().numpy(), costs.detach().cpu().numpy()) < TOL
    for chunk in (1, 2):
        model.zero_grad()
        xi = x.clone().requires_grad_(True)
        got = model.loss(xi, al, y, ll, reduction="sum", chunk=chunk, check_lengths=False, utterance_weights=w)
        want = float((costs.detach() * w).sum())
        assert got.shape == (1,) and abs(float(got) - want) <= TOL * abs(want)
        got.backward()
        assert rel_err(_grads(model, xi), ref) < TOL, chunk
    head = _model(seed=3, tdt_durations=DUR, ctc_weight=0.3)
    with torch.no_grad():
        both = float(head.loss(x, al, y, ll, check_lengths=False))
        plain = float(head.loss(x, al, y, ll, check_lengths=False, ctc_weight=0))
        ctc = float(head.ctc_loss(x, al, y, ll))
    assert abs((both - plain) - 0.3 * ctc) <= TOL * 0.3 * ctc
    # under check_lengths an utterance with more labels than frames is refused; with the check off it costs +inf
    full_al, full_ll = torch.tensor([12, 12, 4], dtype=torch.int32, device="cuda"), torch.tensor([5, 5, 5], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="TDT.*more labels than frames"):
        model.loss(x, full_al, y, full_ll)
    with pytest.raises(ValueError, match="TDT.*more labels than frames"):
        TDTLoss(DUR)(model(x, y), y.int(), full_al, full_ll)
    with torch.no_grad():
        c = model.loss(x, full_al, y, full_ll, reduction="none", check_lengths=False)
    assert torch.isposinf(c[2]) and torch.isfinite(c[:2]).all()


def _oracle_decode(model, enc, lengths):
    """the oracle decoder on the model's own f32 joint rows: one label-encoder and one joint call per decision"""
    out = []
    for b in range(enc.shape[0]):
        def rows(t, tokens):
            hist = torch.tensor([[0] + tokens], dtype=torch.long, device=enc.device)
            return model.joint(enc[b, t], model.decoder(hist)[0, -1]).double().cpu().numpy()
        out.append(O.greedy_decode(rows, int(lengths[b]), tuple(DUR), V))
    return out


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_recognize_equals_the_oracle_decoder(graphs, monkeypatch):
    from ttmi.tdt import TDTDecodeResult
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    model = _tdt_model(decode_batch_graphs=graphs)
    with torch.no_grad():
        model.joint.project_layer.bias[0] -= 1.0                                     # fewer blanks: tokens from a random-weight model
    g = torch.Generator().manual_seed(5)
    for lengths in ([12, 9, 12, 5], [11]):
        x = torch.randn(len(lengths), T, D, generator=g).cuda()
        al = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            enc = model.encoder(x, None)
            want = _oracle_decode(model, enc, lengths)
        got = model.recognize(x, al, details=True)
        plain = model.recognize(x, al)
        blocks = model.decode_batch(enc, al, block=2, details=True)                  # jumps of 3 frames leave a block of 2
        for b in range(len(lengths)):
            r = got[b]
            print("B %d utt %d: tokens %s frames %s durations %s score %.6f (oracle %.6f)"
                  % (len(lengths), b, r.tokens, r.frames, r.durations, r.score, want[b][4]))
            assert isinstance(r, TDTDecodeResult)
            assert (r.tokens, r.frames, r.durations) == (want[b][0], want[b][1], want[b][3])
            assert np.allclose(r.logprobs, want[b][2], rtol=1e-4, atol=1e-5) and abs(r.score - want[b][4]) <= TOL * abs(want[b][4])
            assert plain[b] == r.tokens
            assert (blocks[b].tokens, blocks[b].frames, blocks[b].durations) == (r.tokens, r.frames, r.durations)
        assert any(r.tokens for r in got)
    assert model.decode(enc[0], 11) == got[0].tokens and model.decode(enc[0], 11, details=True).frames == got[0].frames
    assert model.decode(enc[0], 11, block=2) == got[0].tokens                         # decode hands its block on


def test_a_model_without_the_key_is_unchanged(monkeypatch):
    monkeypatch.setenv("TTMI_PRECISION", "fp32")
    from tt.model import DecodeResult
    plain, empty = _model(), _model(tdt_durations=[])
    assert plain.tdt_durations is None and empty.tdt_durations is None
    assert list(plain.state_dict()) == list(empty.state_dict()) == list(_tdt_model().state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), empty.state_dict().values()))
    x, y, al, ll = _batch()
    a, b = plain.recognize(x, al, details=True), empty.recognize(x, al, details=True)
    assert all(isinstance(r, DecodeResult) for r in a + b) and plain.recognize(x, al) == [r.tokens for r in a]
    assert [(r.tokens, r.frames) for r in a] == [(r.tokens, r.frames) for r in b]
    assert all(abs(p.score - q.score) <= 1e-6 * abs(p.score) for p, q in zip(a, b))
    with torch.no_grad():
        assert torch.equal(plain.loss(x, al, y, ll, check_lengths=False), empty.loss(x, al, y, ll, check_lengths=False))


def test_every_entry_point_that_is_not_built_raises(monkeypatch):
    from warprnnt_pytorch import RNNTLoss, rnnt_align
    from ttmi.beam import BeamSearch
    from ttmi.streaming import StreamingRecognizer
    monkeypatch.setenv("TTMI_PRECISION", "bf16")
    monkeypatch.setenv("TTMI_DEFERRED_LOGITS", "1")
    model = _tdt_model()
    x, y, al, ll = _batch()
    with torch.no_grad():
        enc = model.encoder(x, None)
        handle = model(x, y)
    calls = [lambda: model.loss(x, al, y, ll, topology="monotonic"), lambda: model.loss(x, al, y, ll, exp_domain=True),
             lambda: model.loss(x, al, y, ll, fastemit_lambda=0.01),
             lambda: model.loss(x, al, y, ll, distill=torch.zeros(B, T, U + 1, 3, device="cuda"), distill_weight=0.5),
             lambda: model.lattice_posteriors(x, al, y, ll), lambda: model.mwer_loss(x, al, y, ll), lambda: model.align(x, al, y, ll),
             lambda: model.align(x, al, y, ll, stats=True), lambda: model.align_monotonic(x, al, y, ll),
             lambda: model.beam_decode_batch(enc, al), lambda: model.recognize_nbest(x, al), lambda: model.recognize_nbest(x, al, ctc_weight=0.3),
             lambda: model.beam_search_state(B), lambda: model.beam_search(enc[0], 12), lambda: model.recognize_beam_search(x, al),
             lambda: BeamSearch(model, B), lambda: StreamingRecognizer(model), lambda: StreamingRecognizer(model, beam_width=4),
             lambda: RNNTLoss(check_lengths=False)(handle, y.int(), al, ll), lambda: rnnt_align(handle, y.int(), al, ll, check_lengths=False)]
    for call in calls:
        with pytest.raises(ValueError, match="TDT.*not built"):
            call()
