"""CPU: the fp64 restatements of tests/model_refs.py against what the reference project itself recorded - the logits and every
gradient of its GRU S2VT (tests/golden/gru_tiny.npz) and of its Att_Baseline (att_tiny.npz) - and the hand-written GRU layer and
BPTT against torch's fp64 autograd of nn.GRU.  tests/test_gpu_model_variants.py compares the HIP paths with these restatements at
sizes the reference never recorded, so they are validated here first."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_refs as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RECORD = 2e-6        # the recorded values are fp32 results of the reference's fp32 run: a few ulps of max|ref|


def _against_fixture(g, logits, P, what):
    errs = {"logits": float(np.abs(logits.detach().numpy() - g["logits"]).max() / np.abs(g["logits"]).max())}
    assert errs["logits"] <= FP32_RECORD, (what, errs)
    for k, p in P.items():
        ref = g["grad/" + k].astype(np.float64)
        assert p.grad is not None, k
        got = p.grad.numpy()
        if np.abs(ref).max() == 0.0:
            assert np.abs(got).max() == 0.0, k
            errs[k] = 0.0
            continue
        errs[k] = float(np.abs(got - ref).max() / np.abs(ref).max())
        assert errs[k] <= FP32_RECORD, (what, k, errs[k])
    print("%s: max error / max|ref| %.3g (%s)" % (what, max(errs.values()), max(errs, key=errs.get)))


def test_gru_model64_reproduces_the_reference_fixture():
    """gru_model64 + reference_criterion64 on gru_tiny: logits and all 13 gradients within 2e-6 of max|ref| (measured: logits
    1.5e-7, gradients at most 4.4e-7, word_rnn.weight_ih_l0)."""
    g = np.load(os.path.join(GOLD, "gru_tiny.npz"))
    B, L, Fd, H, E, V = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    P = R.leaves64(synth.make_gru_state_dict(V, Fd, H, E, seed=seed).items())
    feats, caps, mask = synth.make_batch(B, L, Fd, V, seed=1234 + seed)
    logits = R.gru_model64(P, feats, caps[:, :-1])
    loss = R.reference_criterion64(logits, caps, mask)
    loss.backward()
    assert len(P) == 13 and abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    _against_fixture(g, logits, P, "gru_tiny")


def test_att_model64_reproduces_the_reference_fixture():
    """att_model64 + reference_criterion64 on att_tiny (the recorded parameters): logits and all 22 gradients within 2e-6 of
    max|ref| (measured: logits 1.3e-7, gradients at most 4.2e-7, encoder.bias_ih_l0_reverse), the three attention layers' five
    gradient tensors exactly zero."""
    g = np.load(os.path.join(GOLD, "att_tiny.npz"))
    B, L, Fd, H, E, V = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    P = R.leaves64((str(k), torch.from_numpy(g["param/" + str(k)])) for k in g["keys"])
    feats, caps, mask = synth.make_batch(B, L, Fd, V, seed=900 + seed)
    logits = R.att_model64(P, feats, caps[:, :-1])
    loss = R.reference_criterion64(logits, caps, mask)
    loss.backward()
    assert len(P) == 22 and abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    for k in P:
        if k.startswith("att_"):
            assert float(P[k].grad.abs().max()) == 0.0 and float(np.abs(g["grad/" + k]).max()) == 0.0, k
    _against_fixture(g, logits, P, "att_tiny")


def test_reference_criterion64_is_the_unmasked_mean():
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(3, 4, 11, generator=g, dtype=torch.float64)
    caps = torch.randint(0, 11, (3, 5), generator=g)
    mask = (torch.rand(3, 5, generator=g) > 0.4).float()
    mask[0, 1] = 1.0
    ref = torch.nn.functional.cross_entropy(logits.reshape(-1, 11), caps[:, 1:].reshape(-1))
    assert abs(float(R.reference_criterion64(logits, caps, mask)) - float(ref)) < 1e-14


@pytest.mark.parametrize("T,B,H,n_gx,dh_first", [(5, 3, 7, 5, 0), (5, 3, 7, 2, 2), (4, 2, 6, 0, 3), (1, 4, 5, 1, 0)])
def test_gru_layer64_and_bptt64_against_autograd(T, B, H, n_gx, dh_first):
    """gru_layer64 is nn.GRU in fp64 (its input weight the identity, so the gate input is the layer's input), and gru_bptt64 from
    its h_all and stash gives autograd's gradient of the gate input and of h W_hh^T + b_hh: 1e-12 relative."""
    g = torch.Generator().manual_seed(T * 100 + H)
    k = H ** -0.5
    rnd = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)
    w_hh, b_hh, b_ih = rnd(3 * H, H) * k, rnd(3 * H) * k, rnd(3 * H) * k
    gx = rnd(n_gx * B, 3 * H).requires_grad_()
    dh_out = rnd((T - dh_first) * B, H)
    h_all, stash = R.gru_layer64(gx.detach(), n_gx, b_ih, w_hh, b_hh, T, B)
    # torch's nn.GRU over the same gate inputs: x = the gate input, W_ih = I, b_ih = 0; the later steps get b_ih as their input
    gi = torch.cat([gx, b_ih.expand((T - n_gx) * B, -1)]).view(T, B, 3 * H)
    cell = torch.nn.GRU(3 * H, H).double()
    zero_b = torch.zeros(3 * H, dtype=torch.float64)
    bh, wh = b_hh.clone().requires_grad_(), w_hh.clone().requires_grad_()
    out, _ = torch.func.functional_call(cell, {"weight_ih_l0": torch.eye(3 * H, dtype=torch.float64), "weight_hh_l0": wh,
                                               "bias_ih_l0": zero_b, "bias_hh_l0": bh}, (gi,))
    gi.retain_grad()
    (out.reshape(T * B, H)[dh_first * B:] * dh_out).sum().backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert rel(h_all, out.detach().reshape(T * B, H)) <= 1e-12
    dgx, dgh = R.gru_bptt64(w_hh, dh_out, dh_first, h_all, stash, T, B)
    assert rel(dgx, gi.grad.reshape(T * B, 3 * H)) <= 1e-12
    assert rel(dgh.sum(0), bh.grad) <= 1e-12                          # db_hh = the column sums of dgh
    if T > 1:
        assert rel(dgh[B:].t() @ h_all[:-B], wh.grad) <= 1e-12        # dW_hh = sum_t dgh_t^T h_{t-1}
    else:
        assert float(wh.grad.abs().max()) == 0.0
    if n_gx:
        assert rel(dgx[:n_gx * B], gx.grad) <= 1e-12
    z, _ = R.gru_bptt64(w_hh, None, 0, h_all, stash, T, B)
    assert float(z.abs().max()) == 0.0
