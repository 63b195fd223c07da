"""GPU: stacked LSTM S2VT (num_layers > 1) on the layer-wavefront chain kernels (csrc/lstm_stack.hip) - the chain entry points
against an fp64 torch LSTM and its autograd, train mode (with and without inter-layer dropout masks) and greedy decode against
an fp64 composite of single-layer nn.LSTMs, the layer-by-layer device path, determinism, error paths, checkpoints and the
train.py entry point."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _close(got, ref, what, rel=1e-5):
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= rel * max(ref.abs().max().item(), 1e-30), (what, err, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------- chain kernels
def _cell64(pre, c_prev):
    H = pre.shape[1] // 4
    i, f, g, o = pre[:, :H].sigmoid(), pre[:, H:2 * H].sigmoid(), pre[:, 2 * H:3 * H].tanh(), pre[:, 3 * H:].sigmoid()
    c = f * c_prev + i * g
    return o * c.tanh(), c, torch.cat([i, f, g, o], 1)


def _rand(g, *shape, k=1.0):
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * k


@pytest.mark.parametrize("B", [4, 10, 17, 33, 64])
@pytest.mark.parametrize("H", [30, 32, 36, 512, 1000])      # H = 36: 2 K chunks for 8 waves; B = 33: ragged 32-row tile
def test_chain_kernels_against_fp64(lib, B, H):
    """A chain of 2-5 layers over T = 7 steps: gate-input rows over a sub-range of steps, initial states, dropout masks on the
    inner layers and an external dense input on layer 0; forward h / c / stash and backward dG against fp64 torch and its
    autograd, and the input gradients dG^0 W_in^0 and dG^0_0 W_hh^0 formed from dG.  H = 30 runs the scalar-load kernels; the
    chain of 5 (H = 32) holds diagonals longer than one launch, and at B = 64 its masked layers run on the 32-row tile."""
    from s2vt_video_caption_amd import ops
    n = {30: 3, 32: 5, 36: 3, 512: 4, 1000: 2}[H]          # 5 layers: diagonals split over two launches; masks on layers 1 and 3
    T, t0, ng = 7, 2, 3
    g = torch.Generator().manual_seed(B * 1000 + H)
    k = H ** -0.5
    x_in = _rand(g, T * B, H).requires_grad_()
    lay64 = []
    for j in range(n):
        lay64.append(dict(w_hh=_rand(g, 4 * H, H, k=k), w_in=_rand(g, 4 * H, H, k=k), bias=_rand(g, 4 * H, k=k).requires_grad_(),
                          gx=_rand(g, ng * B, 4 * H) if j % 2 == 0 else None,
                          h0=_rand(g, B, H, k=0.5) if j != 1 else None, c0=_rand(g, B, H) if j != 1 else None,
                          mask=(torch.rand(T * B, H, generator=g) > 0.3).double() / 0.7 if j < n - 1 and j % 2 else None))
    lay64[0]["h0"].requires_grad_()
    dh_ext = _rand(g, (T - 1) * B, H)
    # fp64 reference with autograd on the pre-activations
    pres, outs = [], []
    x = x_in
    for j, l in enumerate(lay64):
        h, c = (l["h0"] if l["h0"] is not None else torch.zeros(B, H, dtype=torch.float64)), \
               (l["c0"] if l["c0"] is not None else torch.zeros(B, H, dtype=torch.float64))
        hs, cs, sts, pj = [], [], [], []
        for t in range(T):
            pre = l["bias"] + x[t * B:(t + 1) * B] @ l["w_in"].t() + h @ l["w_hh"].t()
            if l["gx"] is not None and t0 <= t < t0 + ng:
                pre = pre - l["bias"] + l["gx"][(t - t0) * B:(t - t0 + 1) * B]
            pre.retain_grad()
            pj.append(pre)
            h, c, st = _cell64(pre, c)
            hs.append(h); cs.append(c); sts.append(st)
        hall = torch.cat(hs)
        outs.append((hall, torch.cat(cs), torch.cat(sts)))
        pres.append(pj)
        x = hall * l["mask"] if l["mask"] is not None else hall
    (outs[-1][0][B:] * dh_ext).sum().backward()

    f32 = lambda t: None if t is None else t.detach().float().to(DEV).contiguous()
    layers = []
    for j, l in enumerate(lay64):
        d = dict(w_hh=f32(l["w_hh"]), bias=f32(l["bias"]), h0=f32(l["h0"]), c0=f32(l["c0"]), mask=f32(l["mask"]),
                 w_in=f32(l["w_in"]), x_in=f32(x_in) if j == 0 else None,
                 h=torch.empty(T * B, H, device=DEV), c=torch.empty(T * B, H, device=DEV),
                 stash=torch.empty(T * B, 4 * H, device=DEV), hm=torch.empty(T * B, H, device=DEV) if l["mask"] is not None else None)
        if l["gx"] is not None:
            d.update(gx=f32(l["gx"]), gx_t0=t0, n_gx=ng)
        layers.append(d)
    ops.lstm_chain_fwd(T, B, H, layers)
    for j in range(n):
        _close(layers[j]["h"], outs[j][0], "h%d" % j)
        _close(layers[j]["c"], outs[j][1], "c%d" % j)
        _close(layers[j]["stash"], outs[j][2], "stash%d" % j)
        if lay64[j]["mask"] is not None:
            _close(layers[j]["hm"], outs[j][0] * lay64[j]["mask"], "hm%d" % j)
    layers[0].update(x_in=None, w_in=None)          # no backward through an external input
    layers[-1].update(dh_ext=f32(dh_ext), dh_t0=1)
    for d in layers:
        d["dg"] = torch.empty(T * B, 4 * H, device=DEV)
    ops.lstm_chain_bwd(T, B, H, layers)
    for j in range(n):
        _close(layers[j]["dg"], torch.cat([p.grad for p in pres[j]]), "dG%d" % j, rel=2e-5)
    _close(layers[0]["dg"] @ f32(lay64[0]["w_in"]), x_in.grad, "dx", rel=2e-5)
    _close(layers[0]["dg"][:B] @ f32(lay64[0]["w_hh"]), lay64[0]["h0"].grad, "dh0", rel=2e-5)


def test_chain_token_segment_against_fp64(lib):
    """One decode step of a 3-layer word chain (T = 1): initial states, the vid half as the external input and the token segment
    (constant token, then the packed argmax word) against fp64."""
    from s2vt_video_caption_amd import ops
    B, H, E, V, n = 10, 64, 40, 23, 3
    g = torch.Generator().manual_seed(7)
    k = H ** -0.5
    emb = _rand(g, V, E)
    w0 = _rand(g, 4 * H, E + H, k=k)
    ws = [(_rand(g, 4 * H, H, k=k), _rand(g, 4 * H, H, k=k), _rand(g, 4 * H, k=k), _rand(g, B, H, k=0.5), _rand(g, B, H))
          for _ in range(n)]
    xv = _rand(g, B, H)
    toks = torch.randint(0, V, (B,), generator=g)
    packed = (0xFFFFFFFF - toks).long() | (torch.randint(0, 2 ** 30, (B,), generator=g) << 32)
    for tok_const, tok_packed in ((5, None), (0, packed)):
        tk = toks if tok_packed is not None else torch.full((B,), tok_const)
        x, ref = None, []
        for j, (w_hh, w_in, b, h0, c0) in enumerate(ws):
            if j == 0:
                pre = b + emb[tk] @ w0[:, :E].t() + xv @ w0[:, E:].t() + h0 @ w_hh.t()
            else:
                pre = b + x @ w_in.t() + h0 @ w_hh.t()
            x, c, _ = _cell64(pre, c0)
            ref.append((x, c))
        f32 = lambda t: t.float().to(DEV).contiguous()
        w0d = f32(w0)
        layers = []
        for j, (w_hh, w_in, b, h0, c0) in enumerate(ws):
            d = dict(w_hh=f32(w_hh), bias=f32(b), h0=f32(h0), c0=f32(c0), h=torch.empty(B, H, device=DEV), c=torch.empty(B, H, device=DEV))
            if j == 0:
                d.update(x_in=f32(xv), w_in=w0d[:, E:], emb=f32(emb), w_e=w0d, E=E, V=V, tok_const=tok_const,
                         tok_packed=tok_packed.to(DEV) if tok_packed is not None else None)
            else:
                d.update(w_in=f32(w_in))
            layers.append(d)
        ops.lstm_chain_fwd(1, B, H, layers)
        for j in range(n):
            _close(layers[j]["h"], ref[j][0], "h%d" % j)
            _close(layers[j]["c"], ref[j][1], "c%d" % j)


# ------------------------------------------------------------------------------------------------------- model level
def _model(N, B, L, F, H, E, V, p=0.0, seed=0):
    import S2VTModel
    from s2vt_video_caption_amd import synth
    torch.manual_seed(seed)
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, num_layers=N, rnn_dropout=p)
    feats, caps, _ = synth.make_batch(B, L, F, V, seed=1234 + seed)
    return m.to(DEV), feats.to(DEV), caps.to(DEV)


def _ref64(m, feats, caps_in, rnn_masks=None, out_mask=None):
    """fp64 composite of single-layer nn.LSTMs on CPU with the model's weights (S2VTModel.py:48-81), masks applied between the
    layers of each nn.LSTM.  Returns (logits, {name: parameter leaf})."""
    P = {k: v.detach().double().cpu().requires_grad_() for k, v in m.named_parameters()}
    B, L, _ = feats.shape
    H, E, N = m.dim_hid, m.dim_embed, m.vid_rnn.num_layers
    T = 2 * L - 1
    masks = [None if mk is None else mk.double().cpu().view(T, B, H).transpose(0, 1) for mk in (rnn_masks or [None] * (2 * N - 2))]

    def lstm(prefix, x, ms):
        for k in range(N):
            cell = torch.nn.LSTM(x.shape[2], H, batch_first=True).double()
            out, _ = torch.func.functional_call(cell, {
                "weight_ih_l0": P["%s.weight_ih_l%d" % (prefix, k)], "weight_hh_l0": P["%s.weight_hh_l%d" % (prefix, k)],
                "bias_ih_l0": P["%s.bias_ih_l%d" % (prefix, k)], "bias_hh_l0": P["%s.bias_hh_l%d" % (prefix, k)]}, (x,))
            x = out * ms[k] if k < N - 1 and ms[k] is not None else out
        return x

    x = feats.double().cpu() @ P["feat_linear.weight"].t() + P["feat_linear.bias"]
    x = torch.cat([x, torch.zeros(B, L - 1, H, dtype=torch.float64)], 1)
    v = lstm("vid_rnn", x, masks[:N - 1])
    emb = P["embedding.weight"][caps_in.cpu()]
    w_in = torch.cat([torch.cat([torch.zeros(B, L, E, dtype=torch.float64), emb], 1), v], 2)
    w = lstm("word_rnn", w_in, masks[N - 1:])
    res = w[:, L:]
    if out_mask is not None:
        res = res * out_mask.double().cpu()
    return res @ P["out_linear.weight"].t() + P["out_linear.bias"], P


def _check_train(m, feats, caps, rnn_masks=None, out_mask=None, logits=None):
    from s2vt_video_caption_amd import stack_functional as S
    g = torch.Generator().manual_seed(3)
    if logits is None:
        logits = S.train_forward(m, feats, caps[:, :-1], out_mask=out_mask, rnn_masks=rnn_masks)
    R = torch.randn(*logits.shape, generator=g)
    m.zero_grad()
    (logits * R.to(DEV)).sum().backward()
    ref, P = _ref64(m, feats, caps[:, :-1], rnn_masks, out_mask)
    (ref * R.double()).sum().backward()
    _close(logits.detach(), ref.detach(), "logits", rel=2e-5)
    for name, p in m.named_parameters():
        _close(p.grad, P[name].grad, name, rel=1e-4)


# (the mode-3 cases keep the ids they had before the GEMM mode became a parameter)
@pytest.mark.parametrize("N,gemm_mode", [pytest.param(2, 3, id="2"), pytest.param(3, 3, id="3"),
                                         pytest.param(2, 0, id="2-gemm0"), pytest.param(3, 0, id="3-gemm0")])
@pytest.mark.parametrize("B,H", [(5, 30), (16, 64), (64, 128)])
def test_stacked_train_against_fp64_composite(lib, N, B, H, gemm_mode):
    """S2VT.forward(mode='train') of a stacked model: logits and every parameter gradient (all _l1 / _l2 tensors included)
    against an fp64 composite of single-layer nn.LSTMs, with the projections on the plane GEMMs (mode 3) and on s2vt_gemm_f32
    (mode 0)."""
    m, feats, caps = _model(N, B, 6, 48, H, H - 8, 37)
    prev = lib.s2vt_set_gemm_mode(gemm_mode)
    try:
        logits = m(feats, targets=caps[:, :-1], mode="train")
        _check_train(m, feats, caps, logits=logits)
    finally:
        lib.s2vt_set_gemm_mode(prev)


def test_stacked_train_with_injected_masks(lib):
    """Inter-layer dropout masks (p = 0.3) and an out_drop mask given to train_forward: outputs and gradients against the fp64
    composite with the same masks."""
    N, B, L, H = 3, 8, 6, 64
    m, feats, caps = _model(N, B, L, 48, H, 56, 37, p=0.3)
    g = torch.Generator().manual_seed(11)
    T = 2 * L - 1
    masks = [((torch.rand(T * B, H, generator=g) > 0.3).float() / 0.7).to(DEV) for _ in range(2 * (N - 1))]
    out_mask = ((torch.rand(B, L - 1, H, generator=g) > 0.2).float() / 0.8).to(DEV)
    _check_train(m, feats, caps, rnn_masks=masks, out_mask=out_mask)


def test_forward_draws_masks_and_eval_disables_them(lib):
    """In training, forward draws {0, 1/(1-p)} masks with the right keep fraction; in eval a p > 0 model equals p = 0 bit for bit."""
    from s2vt_video_caption_amd import stack_functional as S
    N, B, L, H, p = 2, 16, 8, 64, 0.3
    m, feats, caps = _model(N, B, L, 48, H, 56, 37, p=p)
    masks = S.draw_rnn_masks(m.train(), 2 * L - 1, B, DEV)
    assert len(masks) == 2 * (N - 1)
    for mk in masks:
        vals = torch.unique(mk).cpu()
        assert all(abs(v - 0.0) < 1e-7 or abs(v - 1 / (1 - p)) < 1e-6 for v in vals.tolist()), vals
        keep = (mk > 0).double().mean().item()
        sigma = (p * (1 - p) / mk.numel()) ** 0.5
        assert abs(keep - (1 - p)) < 4 * sigma, keep
    m.eval()
    assert S.draw_rnn_masks(m, 2 * L - 1, B, DEV) is None
    m0, _, _ = _model(N, B, L, 48, H, 56, 37, p=0.0)
    m0.load_state_dict(m.state_dict())
    m0.eval()
    with torch.no_grad():
        a = m(feats, targets=caps[:, :-1], mode="train")
        b = m0(feats, targets=caps[:, :-1], mode="train")
        assert torch.equal(a, b)
        assert torch.equal(m(feats, mode="test"), m0(feats, mode="test"))


def _greedy64(m, feats):
    """fp64 greedy decode of the composite (S2VTModel.py:82-110): ids [B, L-1] and per-step top-2 margins."""
    P = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    B, L, _ = feats.shape
    H, E, N = m.dim_hid, m.dim_embed, m.vid_rnn.num_layers

    def step(prefix, x, st):
        new = []
        for k in range(N):
            h, c = st[k]
            pre = x @ P["%s.weight_ih_l%d" % (prefix, k)].t() + P["%s.bias_ih_l%d" % (prefix, k)] + \
                h @ P["%s.weight_hh_l%d" % (prefix, k)].t() + P["%s.bias_hh_l%d" % (prefix, k)]
            h, c, _ = _cell64(pre, c)
            new.append((h, c))
            x = h
        return x, new

    z = torch.zeros(B, H, dtype=torch.float64)
    x = feats.double().cpu() @ P["feat_linear.weight"].t() + P["feat_linear.bias"]
    sv = [(z, z)] * N
    sw = [(z, z)] * N
    for t in range(L):
        v, sv = step("vid_rnn", x[:, t], sv)
        _, sw = step("word_rnn", torch.cat([torch.zeros(B, E, dtype=torch.float64), v], 1), sw)
    tok = torch.full((B,), m.sos_ix, dtype=torch.long)
    ids, margins = [], []
    for i in range(L - 1):
        v, sv = step("vid_rnn", torch.zeros(B, H, dtype=torch.float64), sv)
        o, sw = step("word_rnn", torch.cat([P["embedding.weight"][tok], v], 1), sw)
        logit = o @ P["out_linear.weight"].t() + P["out_linear.bias"]
        top2 = logit.topk(2, 1).values
        margins.append(top2[:, 0] - top2[:, 1])
        tok = logit.argmax(1)
        ids.append(tok)
    return torch.stack(ids, 1), torch.stack(margins, 1)


@pytest.mark.parametrize("N,B,H", [(2, 4, 32), (2, 10, 30), (3, 16, 64), (2, 64, 128)])
def test_stacked_greedy_ids_against_fp64(lib, N, B, H):
    """Greedy ids of a stacked model bit-exact against the fp64 composite on every row whose top-2 margins stay robust."""
    m, feats, _ = _model(N, B, 8, 48, H, H + 4, 41, seed=N + B)
    with torch.no_grad():
        ids = m.eval()(feats, mode="test").cpu()
    ref, marg = _greedy64(m, feats)
    robust = (marg > 1e-4).all(1)
    assert robust.sum() >= B // 2
    assert torch.equal(ids[robust], ref[robust])


def test_wavefront_agrees_with_layerwise_at_config2_dims(lib):
    """The wavefront path and the layer-by-layer path on the one-layer kernels (reference_layerwise) at configs[1] dims
    (B = 64, H = E = 1000, L = 80), N = 2: logits and gradients within fp32 tolerance."""
    from s2vt_video_caption_amd import stack_functional as S
    m, feats, caps = _model(2, 64, 80, 4096, 1000, 1000, 12000)
    g = torch.Generator().manual_seed(5)
    R = torch.randn(64, 79, 12000, generator=g).to(DEV)
    out = {}
    for name, fn in (("wave", S.train_forward), ("layer", S.reference_layerwise)):
        m.zero_grad()
        lg = fn(m, feats, caps[:, :-1])
        (lg * R).sum().backward()
        out[name] = (lg.detach(), {k: p.grad.clone() for k, p in m.named_parameters()})
    _close(out["wave"][0], out["layer"][0], "logits", rel=1e-5)
    for k in out["wave"][1]:
        _close(out["wave"][1][k], out["layer"][1][k], k, rel=1e-4)


def test_one_layer_chain_meets_the_c2_fixture(lib):
    """stack_functional.train_forward on a ONE-layer model at BASELINE configs[1] (a chain of two, called directly) against the
    reference's c2 fixture: loss within 1e-4, logits slice and every gradient within the bounds of test_gpu_parity._c2_body."""
    import S2VTModel
    import utils
    from s2vt_video_caption_amd import stack_functional as S
    from s2vt_video_caption_amd import synth
    g = np.load(os.path.join(GOLD, "c2.npz"))
    d = synth.CONFIGS["c2"]
    seed, scale = int(g["seed"]), float(g["out_scale"])
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=scale)
    feats, caps, mask = (t.to(DEV) for t in synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed))
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(sd)
    m.to(DEV).train()
    logits = S.train_forward(m, feats, caps[:, :-1])
    loss = utils.MaskCriterion()(logits, caps, mask)
    loss.backward()
    assert abs(float(loss) - float(g["losses"][0])) < 1e-4, (float(loss), float(g["losses"][0]))
    assert np.abs(logits.detach().cpu()[:, ::13, :64].numpy() - g["logits_rows"]).max() < 5e-5 * scale
    for k, p in m.named_parameters():
        got = p.grad.detach().cpu()
        gn = float(g["gradnorm/" + k])
        assert abs(float(got.double().norm()) - gn) <= 5e-4 * gn + 1e-7, k
        assert abs(float(got.double().sum()) - float(g["gradsum/" + k])) <= 2e-4 * gn * got.numel() ** 0.5 + 1e-7, k
        ref = g["gradhead/" + k]
        assert np.abs(got.reshape(-1)[:32].numpy() - ref).max() <= 2e-6 + 5e-4 * np.abs(ref).max(), k


# ------------------------------------------------------------------------------------------- against the reference itself
def _gsetup(name):
    """fixture of tools/make_stack_golden.py (outputs of the reference's own stacked S2VT) and the model it was made from"""
    import S2VTModel
    from s2vt_video_caption_amd import synth
    g = np.load(os.path.join(GOLD, name + ".npz"))
    B, L, F, H, E, V = (int(x) for x in g["dims"])
    N, seed = int(g["num_layers"]), int(g["seed"])
    sd = synth.make_state_dict(V, F, H, E, seed=seed, num_layers=N)
    feats, caps, mask = synth.make_batch(B, L, F, V, seed=1234 + seed)
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, num_layers=N)
    m.load_state_dict(sd)
    return g, m.to(DEV), feats.to(DEV), caps.to(DEV), mask.to(DEV)


@pytest.mark.parametrize("name", ["stack_tiny", "stack3_tiny", "stack_ref", "stack_c2"])
def test_stacked_train_step_against_reference(lib, name):
    """Loss within 1e-4, logits slice and every gradient (all _l1 / _l2 tensors included) within the bounds of
    test_gru_train_step_against_reference (norm, sum, leading entries; all of it at the tiny sizes)."""
    import utils
    g, m, feats, caps, mask = _gsetup(name)
    m.train()
    logits = m(feats, targets=caps[:, :-1], mode="train")
    loss = utils.MaskCriterion()(logits, caps, mask)
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 1e-4, (float(loss), float(g["loss"]))
    lg = logits.detach().cpu()
    assert np.abs(lg[:, ::13, :64].numpy() - g["logits_rows"]).max() < 5e-5
    if "logits" in g.files:
        assert np.abs(lg.numpy() - g["logits"]).max() < 5e-5
    names = [k for k, _ in m.named_parameters()]
    assert any("_l1" in k for k in names)
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


@pytest.mark.parametrize("name", ["stack_tiny", "stack_ref", "stack_c2", "stack_ragged"])
def test_stacked_greedy_ids_against_reference(lib, name):
    """mode='test': bit-exact ids on every row whose fp64 top-2 margin is >= 1e-5 at every step (the fixture's count)."""
    g, m, feats, _, _ = _gsetup(name)
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test").cpu().numpy()
    ref, marg = g["greedy_ids"], g["greedy_margin"]
    assert ids.shape == ref.shape and ids.dtype == np.int64
    robust = (marg >= 1e-5).all(1)
    assert int(robust.sum()) == int(g["n_robust_rows"])
    np.testing.assert_array_equal(ids[robust], ref[robust])


def test_stacked_ten_adam_steps_at_config2(lib):
    """BASELINE configs[1], N = 2: ten torch.optim.Adam steps (lr 1e-3) on one batch - the loss within 1e-4 of the reference at
    every step, the final parameter norms within 1e-4 relative."""
    import utils
    g, m, feats, caps, mask = _gsetup("stack_c2")
    opt = torch.optim.Adam(m.parameters(), lr=float(g["long_lr"]))
    losses = []
    for _ in range(len(g["long_losses"])):
        opt.zero_grad()
        m.train()
        loss = utils.MaskCriterion()(m(feats, targets=caps[:, :-1], mode="train"), caps, mask)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.abs(np.array(losses) - g["long_losses"]).max() < 1e-4, (losses, g["long_losses"])
    for k, v in m.state_dict().items():
        ref = float(g["finalnorm/" + k])
        assert abs(float(v.double().norm()) - ref) <= 1e-4 * ref, k


def test_stacked_backward_is_deterministic(lib):
    m, feats, caps = _model(2, 16, 8, 48, 64, 56, 37)
    grads = []
    for _ in range(2):
        m.zero_grad()
        m(feats, targets=caps[:, :-1], mode="train").square().sum().backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_stacked_error_paths(lib):
    import S2VTModel
    from s2vt_video_caption_amd import capi
    m, feats, caps = _model(2, 4, 6, 48, 32, 32, 37)
    bad = caps[:, :-1].clone()
    bad[1, 2] = 37
    m(feats, targets=bad, mode="train")
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()
    m(feats, targets=caps[:, :-1], mode="train")
    torch.cuda.synchronize()
    capi.check_async_error()
    with pytest.raises(NotImplementedError, match="BeamSearchNode"):
        m(feats, mode="beam_search")
    for kw in (dict(num_layers=2, rnn_type="gru"), dict(bidirectional=True), dict(num_layers=2, bidirectional=True)):
        mm = S2VTModel.S2VT(37, 48, 6, dim_hid=32, dim_embed=32, **kw).to(DEV)
        with pytest.raises(NotImplementedError):
            mm(feats, targets=caps[:, :-1], mode="train")
    with pytest.raises(NotImplementedError):
        m._hip_params()


def test_stacked_checkpoint_from_cpu_torch_loads_and_decodes(lib, tmp_path):
    """A state_dict of a CPU model (nn.LSTM layout with _l1 keys) loads into a fresh model and decodes."""
    import S2VTModel
    torch.manual_seed(1)
    cpu = S2VTModel.S2VT(37, 48, 6, dim_hid=32, dim_embed=32, num_layers=2)
    path = str(tmp_path / "s.pth")
    torch.save(cpu.state_dict(), path)
    m = S2VTModel.S2VT(37, 48, 6, dim_hid=32, dim_embed=32, num_layers=2)
    m.load_state_dict(torch.load(path))
    m.to(DEV).eval()
    feats = torch.randn(3, 6, 48).to(DEV)
    with torch.no_grad():
        ids = m(feats, mode="test").cpu()
    ref, marg = _greedy64(m, feats)
    assert ids.shape == (3, 5) and ids.dtype == torch.int64
    robust = (marg > 1e-4).all(1)
    assert robust.any()
    assert torch.equal(ids[robust], ref[robust])


def test_train_entry_point_with_stacked_lstm(lib, tmp_path):
    """train.py --num-layers 2 --rnn-dropout 0.2 on a tiny synthetic split: one epoch, a stacked checkpoint that decodes."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train
    from test_gpu_gru import _make_toy
    L, F = 8, 24
    _make_toy(str(tmp_path), L, F)
    ck = tmp_path / "ck"
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(L), "--dim-hidden", "32", "--dim-embed", "24", "--feat-dim", str(F),
                       "--batch-size", "4", "--epochs", "1", "--lr", "5e-3", "--save-path", str(ck), "--no-shuffle",
                       "--seed", "7", "--num-layers", "2", "--rnn-dropout", "0.2"])
    got = train.run(opt)
    assert len(got["train_loss"]) == 1 and all(np.isfinite(got["train_loss"]))
    m = torch.load(ck / (got["start_time"] + "final.pth"), weights_only=False)
    assert m.vid_rnn.num_layers == 2 and m.word_rnn.num_layers == 2 and m.vid_rnn.dropout == 0.2
    with torch.no_grad():
        ids = m.eval()(torch.randn(3, L, F, device=DEV), mode="test")
    assert ids.shape == (3, L - 1)
