"""GPU: S2VT(rnn_type='gru') on the GRU timestep kernels (csrc/gru.hip) - the step kernels against an fp64 torch GRU cell, train
mode / greedy decode / ten Adam steps against outputs of the reference itself (tests/golden/gru_*.npz, tools/make_gru_golden.py),
determinism, error paths, checkpoints and the train.py entry point."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _setup(name):
    import S2VTModel
    from s2vt_video_caption_amd import synth
    g = np.load(os.path.join(GOLD, name + ".npz"))
    B, L, F, H, E, V = (int(x) for x in g["dims"])
    seed = int(g["seed"])
    sd = synth.make_gru_state_dict(V, F, H, E, seed=seed)
    feats, caps, mask = synth.make_batch(B, L, F, V, seed=1234 + seed)
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, rnn_type="gru")
    m.load_state_dict(sd)
    return g, sd, m.to(DEV), feats.to(DEV), caps.to(DEV), mask.to(DEV)


# ------------------------------------------------------------------------------------------------------- step kernels
def _cell64(x_gate, h, w_hh, b_hh):
    """nn.GRU step in fp64 from the gate input x_gate [B,3H]: (h', r, z, n, ghn)."""
    H = w_hh.shape[1]
    gh = h @ w_hh.t() + b_hh
    r = torch.sigmoid(x_gate[:, :H] + gh[:, :H])
    z = torch.sigmoid(x_gate[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(x_gate[:, 2 * H:] + r * gh[:, 2 * H:])
    return n + z * (h - n), r, z, n, gh[:, 2 * H:]


def _close(got, ref, what):
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= 1e-5 * max(ref.abs().max().item(), 1e-30), (what, err, ref.abs().max().item())


@pytest.mark.parametrize("B", [4, 10, 16, 17, 33, 64])
@pytest.mark.parametrize("H", [30, 32, 36, 512, 1000])      # H = 36: 2 K chunks for 8 waves
def test_gru_step_kernels_against_fp64_cell(lib, B, H):
    """Forward (zero state / given state, with and without the token segment) and the BPTT step against the fp64 cell and
    its autograd.  H = 30 with E = 26 (rows not a multiple of 4 floats) runs the scalar-load kernels, the other sizes the
    16-byte-load ones."""
    from s2vt_video_caption_amd import capi, ops
    g = torch.Generator().manual_seed(100 * B + H)
    E, V = (40 if H % 4 == 0 else 26), 97
    k = H ** -0.5
    w_hh = ((torch.rand(3 * H, H, generator=g) * 2 - 1) * k)
    b_hh = ((torch.rand(3 * H, generator=g) * 2 - 1) * k)
    b_ih = ((torch.rand(3 * H, generator=g) * 2 - 1) * k)
    w_ih = ((torch.rand(3 * H, E + H, generator=g) * 2 - 1) * k)
    gx = torch.randn(B, 3 * H, generator=g)
    h0 = torch.randn(B, H, generator=g).tanh()
    emb = torch.randn(V, E, generator=g)
    tok = torch.randint(0, V, (B,), generator=g)
    d = {n: t.to(DEV) for n, t in dict(w_hh=w_hh, b_hh=b_hh, b_ih=b_ih, w_ih=w_ih, gx=gx, h0=h0, emb=emb).items()}
    W, Bh = w_hh.double(), b_hh.double()
    # zero state and zero input (b_ih alone), stash
    h, st = ops.gru_step_fwd(None, d["b_ih"], d["w_hh"], d["b_hh"], None, want_stash=True, B=B)
    hr, r, z, n, ghn = _cell64(b_ih.double().expand(B, -1), torch.zeros(B, H, dtype=torch.float64), W, Bh)
    _close(h, hr, "h zero state")
    _close(st, torch.cat([r, z, n, ghn], 1), "stash zero state")
    # given state
    h, st = ops.gru_step_fwd(d["gx"], None, d["w_hh"], d["b_hh"], d["h0"], want_stash=True)
    hr, r, z, n, ghn = _cell64(gx.double(), h0.double(), W, Bh)
    _close(h, hr, "h")
    _close(st, torch.cat([r, z, n, ghn], 1), "stash")
    # token segment: int32 tokens, the constant token, the packed word of the argmax step
    xt = gx.double() + emb.double()[tok] @ w_ih.double()[:, :E].t()
    h = ops.gru_step_fwd_token(d["gx"], d["w_hh"], d["b_hh"], d["h0"], d["emb"], d["w_ih"], tok=tok.int().to(DEV))
    _close(h, _cell64(xt, h0.double(), W, Bh)[0], "h token")
    h = ops.gru_step_fwd_token(d["gx"], d["w_hh"], d["b_hh"], None, d["emb"], d["w_ih"], tok_const=3)
    xt3 = gx.double() + emb.double()[3] @ w_ih.double()[:, :E].t()
    _close(h, _cell64(xt3, torch.zeros(B, H, dtype=torch.float64), W, Bh)[0], "h sos, zero state")
    packed = (torch.randint(0, 1 << 30, (B,), generator=g) << 32) | (0xFFFFFFFF - tok)
    h = ops.gru_step_fwd_token(d["gx"], d["w_hh"], d["b_hh"], d["h0"], d["emb"], d["w_ih"], tok_packed=packed.to(DEV))
    _close(h, _cell64(xt, h0.double(), W, Bh)[0], "h packed token")
    capi.check_async_error()
    # guards: a constant token outside the vocabulary is refused at once; an id of the int32 array is read as token 0 and
    # reported by the next check
    with pytest.raises(IndexError):
        ops.gru_step_fwd_token(d["gx"], d["w_hh"], d["b_hh"], d["h0"], d["emb"], d["w_ih"], tok_const=V)
    bad = tok.clone()
    bad[B - 1] = V + 3
    tok0 = tok.clone()
    tok0[B - 1] = 0
    h = ops.gru_step_fwd_token(d["gx"], d["w_hh"], d["b_hh"], d["h0"], d["emb"], d["w_ih"], tok=bad.int().to(DEV))
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()
    xt0 = gx.double() + emb.double()[tok0] @ w_ih.double()[:, :E].t()
    _close(h, _cell64(xt0, h0.double(), W, Bh)[0], "h, bad id read as token 0")
    # BPTT of step t (state h0 -> h1) with a successor step t+1 (h1 -> h2): autograd of the fp64 cells
    gx2 = torch.randn(B, 3 * H, generator=g)
    dh_out1, dh_out2 = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    hp = h0.double().requires_grad_()
    x1g = gx.double().requires_grad_()
    Wg = W.clone().requires_grad_()
    h1, r1, z1, n1, ghn1 = _cell64(x1g, hp, Wg, Bh)
    h1k = h1.detach().requires_grad_()
    x2g = gx2.double().requires_grad_()
    h2, r2, z2, n2, ghn2 = _cell64(x2g, h1k, W, Bh)
    (h2 * dh_out2.double()).sum().backward()
    dgx2_ref = x2g.grad
    dh1_ref = h1k.grad + dh_out1.double()
    (h1 * dh1_ref).sum().backward()
    st1 = torch.cat([r1, z1, n1, ghn1], 1).detach().float().to(DEV)
    st2 = torch.cat([r2, z2, n2, ghn2], 1).detach().float().to(DEV)
    dh = torch.empty(B, H, device=DEV)
    dgx2, dgh2 = ops.gru_step_bwd(None, None, None, dh_out2.to(DEV), st2, h1.detach().float().to(DEV), dh)
    _close(dgx2, dgx2_ref, "dgx last step")
    _close(dh, dh_out2.double(), "dh last step")
    wt = d["w_hh"].t().contiguous()
    dgx1, dgh1 = ops.gru_step_bwd(dgh2, wt, st2, dh_out1.to(DEV), st1, d["h0"], dh)
    _close(dh, dh1_ref, "dh")
    _close(dgx1, x1g.grad, "dgx")
    _close(dgh1[:, :2 * H], x1g.grad[:, :2 * H], "dgh r,z")
    _close(dgh1[:, 2 * H:], x1g.grad[:, 2 * H:] * r1.detach(), "dgh n")


# --------------------------------------------------------------------------------------------------- model parity
def _train_once(m, feats, caps, mask):
    import utils
    m.zero_grad(set_to_none=True)
    m.train()
    logits = m(feats, targets=caps[:, :-1], mode="train")
    loss = utils.MaskCriterion()(logits, caps, mask)
    loss.backward()
    return loss, logits


@pytest.mark.parametrize("name", ["gru_tiny", "gru_ref", "gru_c2"])
def test_gru_train_step_against_reference(lib, name):
    """Loss within 1e-4, logits slice and every gradient within the bounds of test_gpu_parity._c2_body (norm, sum, leading
    entries; all of it at the tiny size)."""
    from s2vt_video_caption_amd import functional as _F
    g, _, m, feats, caps, mask = _setup(name)
    loss, logits = _train_once(m, feats, caps, mask)
    assert _F._fusable_train_node(logits) is None          # MaskCriterion takes its materialised-gradient route here
    assert abs(float(loss) - float(g["loss"])) < 1e-4, (float(loss), float(g["loss"]))
    lg = logits.detach().cpu()
    assert np.abs(lg[:, ::13, :64].numpy() - g["logits_rows"]).max() < 5e-5
    if "logits" in g.files:
        assert np.abs(lg.numpy() - g["logits"]).max() < 5e-5
    for k, p in m.named_parameters():
        got = p.grad.detach().cpu()
        gn = float(g["gradnorm/" + k])
        assert abs(float(got.double().norm()) - gn) <= 5e-4 * gn + 1e-7, k
        assert abs(float(got.double().sum()) - float(g["gradsum/" + k])) <= 2e-4 * gn * got.numel() ** 0.5 + 1e-7, k
        ref = g["gradhead/" + k]
        assert np.abs(got.reshape(-1)[:32].numpy() - ref).max() <= 2e-6 + 5e-4 * np.abs(ref).max(), k
        if "grad/" + k in g.files:
            full = g["grad/" + k]
            assert np.abs(got.numpy() - full).max() <= 2e-6 + 2e-4 * np.abs(full).max(), k


@pytest.mark.parametrize("name", ["gru_tiny", "gru_ref", "gru_c2", "gru_ragged"])
def test_gru_greedy_ids_against_reference(lib, name):
    """mode='test': bit-exact ids on every row whose fp64 top-2 margin is >= 1e-5 at every step (the fixture's count)."""
    g, _, m, feats, _, _ = _setup(name)
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test").cpu().numpy()
    ref, marg = g["greedy_ids"], g["greedy_margin"]
    assert ids.shape == ref.shape and ids.dtype == np.int64
    robust = (marg >= 1e-5).all(1)
    assert int(robust.sum()) == int(g["n_robust_rows"])
    np.testing.assert_array_equal(ids[robust], ref[robust])


def test_gru_ten_adam_steps_at_config2(lib):
    """BASELINE configs[1]: ten torch.optim.Adam steps (lr 1e-3) on one batch - the loss within 1e-4 of the reference at every
    step, the final parameter norms within 1e-4 relative."""
    import utils
    g, _, m, feats, caps, mask = _setup("gru_c2")
    gl = np.load(os.path.join(GOLD, "gru_c2long.npz"))
    opt = torch.optim.Adam(m.parameters(), lr=float(gl["lr"]))
    losses = []
    for _ in range(int(gl["n_steps"])):
        opt.zero_grad()
        m.train()
        loss = utils.MaskCriterion()(m(feats, targets=caps[:, :-1], mode="train"), caps, mask)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.abs(np.array(losses) - gl["losses"]).max() < 1e-4, (losses, gl["losses"])
    for k, v in m.state_dict().items():
        ref = float(gl["finalnorm/" + k])
        assert abs(float(v.double().norm()) - ref) <= 1e-4 * ref, k


def test_gru_backward_is_deterministic(lib):
    _, _, m, feats, caps, mask = _setup("gru_ref")
    grads = []
    for _ in range(2):
        _train_once(m, feats, caps, mask)
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_gru_error_paths(lib):
    import utils
    from s2vt_video_caption_amd import capi
    _, _, m, feats, caps, mask = _setup("gru_tiny")
    bad = caps.clone()
    bad[1, 2] = m.vocab_size + 5                      # a word id outside the vocabulary (embedding input and criterion target)
    with pytest.raises(IndexError):
        loss = utils.MaskCriterion()(m(feats, targets=bad[:, :-1], mode="train"), bad, mask)
        torch.cuda.synchronize()
        capi.check_async_error()
    bad = caps.clone()
    bad[0, 0] = -1                                    # the first embedding input only
    with pytest.raises(IndexError):
        m(feats, targets=bad[:, :-1], mode="train")
        torch.cuda.synchronize()
        capi.check_async_error()
    loss = utils.MaskCriterion()(m(feats, targets=caps[:, :-1], mode="train"), caps, mask)   # and the next call is clean
    torch.cuda.synchronize()
    capi.check_async_error()
    assert np.isfinite(float(loss))
    with pytest.raises(NotImplementedError, match="GRU"):
        m(feats, mode="beam_search")


def test_gru_checkpoint_from_cpu_torch_loads_and_decodes(lib, tmp_path):
    """A state_dict written by CPU torch from a CPU S2VT(rnn_type='gru') loads into the drop-in and decodes the reference's ids."""
    import S2VTModel
    g, sd, _, feats, _, _ = _setup("gru_tiny")
    B, L, F, H, E, V = (int(x) for x in g["dims"])
    cpu = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, rnn_type="gru")
    cpu.load_state_dict(sd)
    torch.save(cpu.state_dict(), tmp_path / "gru.pth")
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, rnn_type="gru")
    m.load_state_dict(torch.load(tmp_path / "gru.pth"))
    with torch.no_grad():
        ids = m.to(DEV).eval()(feats, mode="test").cpu().numpy()
    np.testing.assert_array_equal(ids, g["greedy_ids"])


def _make_toy(root, L, F, V=30, n=(12, 6, 4), seed=0):
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "feats"), exist_ok=True)
    caps, ids = {}, []
    for i in range(sum(n)):
        vid = "vid%02d" % i
        ids.append(vid)
        np.save(os.path.join(root, "feats", vid + ".npy"), rng.randn(L, F).astype(np.float32))
        caps[vid] = [[3] + [int(x) for x in rng.randint(5, V, size=rng.randint(2, 6))] + [4] for _ in range(rng.randint(2, 4))]
    w2i = {"<pad>": 0, "<unk>": 1, "<sos>": 3, "<eos>": 4}
    for i in range(V):
        if i not in (0, 1, 3, 4):
            w2i["w%d" % i] = i
    data = {"word2ix": w2i, "ix2word": {str(v): k for k, v in w2i.items()}, "captions": caps,
            "splits": {"train": ids[:n[0]], "valid": ids[n[0]:n[0] + n[1]], "test": ids[n[0] + n[1]:]}}
    with open(os.path.join(root, "captions.json"), "w") as f:
        json.dump(data, f)


def test_train_entry_point_with_gru(lib, tmp_path):
    """train.py --rnn-type gru on a tiny synthetic split: two epochs, a full-module GRU checkpoint that eval.generate decodes."""
    sys.path.insert(0, ROOT)
    import eval as s2vt_eval
    import train
    L, F = 8, 24
    _make_toy(str(tmp_path), L, F)
    ck = tmp_path / "ck"
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(L), "--dim-hidden", "32", "--dim-embed", "24", "--feat-dim", str(F),
                       "--batch-size", "4", "--epochs", "2", "--lr", "5e-3", "--save-path", str(ck), "--no-shuffle",
                       "--seed", "7", "--rnn-type", "gru"])
    got = train.run(opt)
    assert len(got["train_loss"]) == 2 and all(np.isfinite(got["train_loss"]))
    final = ck / (got["start_time"] + "final.pth")
    m = torch.load(final, weights_only=False)
    assert isinstance(m.vid_rnn, torch.nn.GRU) and isinstance(m.word_rnn, torch.nn.GRU)
    out = s2vt_eval.generate(str(final), str(tmp_path / "captions.json"), str(tmp_path / "feats"), batch_size=3, mode="test")
    assert len(out) == 4
