"""GPU tests of the sampled decode (mode='sample') and of utils.RewardCriterion.

The reference of every check is float64 on the CPU: the numpy restatement of the noise (sampling.py) and a teacher-forced replay of
the network ALONG THE DEVICE'S OWN IDS (oracle forward_train in float64; tools/make_gru_golden's arithmetic for the GRU).  A draw
is right when its float64 score is within eps of the float64 maximum - at every row and step, no row left out."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops, sampling, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_gru_golden as gru_gen  # noqa: E402
import test_sampling_host as hs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set(lib, name, value):
    return lib.s2vt_set_option(name.encode(), value)


def _step_inputs(B, H, V, seed):
    """h like an LSTM output, out_linear like the synthetic recipe (U(-1/sqrt(H), 1/sqrt(H)))"""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(H)
    h = torch.tanh(torch.randn(B, H, generator=g))
    w = (torch.rand(V, H, generator=g) * 2 - 1) * k
    b = (torch.rand(V, generator=g) * 2 - 1) * k
    return h, w, b


# ------------------------------------------------------------------ the noise itself
@pytest.mark.parametrize("planes", [False, True])
def test_device_noise_matches_restatement(lib, planes):
    """w_out = 0, b_out = 0 at index n and -1e30 elsewhere: the packed score IS g of element n"""
    B, H, V, seed, step, row0 = 5, 32, 23, 0x1234567890ABCDEF, 3, 7
    h = torch.randn(B, H, device=DEV)
    w = torch.zeros(V, H, device=DEV)
    want = sampling.gumbel_noise(seed, step, np.arange(row0, row0 + B), V)
    worst = 0.0
    for n in range(V):
        b = torch.full((V,), -1e30, device=DEV)
        b[n] = 0.0
        ids, packed = ops.decode_step_sample(h, w, b, temperature=0.7, seed=seed, step=step, row0=row0, planes=planes, return_packed=True)
        assert (ids.cpu() == n).all()
        got = ops.packed_score(packed).cpu().double().numpy()
        worst = max(worst, np.abs(got - want[:, n]).max())
    print("max |g_device - g_float64| = %.3g (tol %.3g)" % (worst, hs.NOISE_TOL))
    assert worst <= hs.NOISE_TOL
    # zero weights, zero bias, temperature 1: the packed score is the row's maximum noise, at its index
    ids, packed = ops.decode_step_sample(h, w, torch.zeros(V, device=DEV), seed=seed, step=step, row0=row0, planes=planes,
                                         return_packed=True)
    assert np.array_equal(ids.cpu().numpy(), want.argmax(1))
    assert np.abs(ops.packed_score(packed).cpu().double().numpy() - want.max(1)).max() <= hs.NOISE_TOL


def test_noise_extremes_on_device(lib):
    """the ends of the range: the accurate log keeps the bound where u is next to 0 and next to 1 (host-side check of the map the
    device shares is test_sampling_host; here: no NaN / inf ever wins over a large vocabulary)"""
    B, H, V = 64, 32, 12001
    h = torch.zeros(B, H, device=DEV)
    w = torch.zeros(V, H, device=DEV)
    ids, packed = ops.decode_step_sample(h, w, None, seed=9, step=0, return_packed=True)
    want = sampling.gumbel_noise(9, 0, B, V)
    sc = ops.packed_score(packed).cpu().double().numpy()
    assert np.isfinite(sc).all() and np.abs(sc - want.max(1)).max() <= hs.NOISE_TOL
    assert np.array_equal(ids.cpu().numpy(), want.argmax(1))


# ------------------------------------------------------------------ exactness of a draw: the step kernels
@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("B", [4, 10, 64, 128])
@pytest.mark.parametrize("H", [32, 512, 1000])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_step_kernel_draw_is_exact(lib, planes, B, H, temperature):
    V, seed, step = 301, 4242 + B + H, 5
    h, w, b = _step_inputs(B, H, V, seed)
    ids = ops.decode_step_sample(h.to(DEV), w.to(DEV), b.to(DEV), temperature=temperature, seed=seed, step=step, planes=planes).cpu().numpy()
    score = (h.double() @ w.double().t() + b.double()).numpy() / temperature + sampling.gumbel_noise(seed, step, B, V)
    assert ids.min() >= 0 and ids.max() < V                      # vocabulary padding rows never win
    chosen = score[np.arange(B), ids]
    gap = score.max(1) - chosen
    print("B=%d H=%d planes=%d: max float64 gap of the chosen index %.3g (eps %.3g)" % (B, H, planes, gap.max(), hs.eps_for(temperature)))
    assert (gap <= hs.eps_for(temperature)).all()
    # it is a sample: not the arg-max of the logits on every row
    if B >= 64:
        assert (ids != (score - sampling.gumbel_noise(seed, step, B, V)).argmax(1)).any()


# ------------------------------------------------------------------ the whole decode
def _model(d, sd, **kw):
    import S2VTModel
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _check_along_ids(sd, feats, ids, seed, temperature, V):
    score = hs.scores_along_ids_fp64(sd, feats, ids.cpu(), seed, temperature)
    idn = ids.cpu().numpy()
    assert idn.min() >= 0 and idn.max() < V
    chosen = np.take_along_axis(score, idn[:, :, None], 2)[:, :, 0]
    gap = score.max(2) - chosen
    print("max float64 gap of the chosen index %.3g (eps %.3g)" % (gap.max(), hs.eps_for(temperature)))
    assert (gap <= hs.eps_for(temperature)).all()


@pytest.mark.parametrize("B,fused", [(4, 1), (10, 1), (64, 1), (128, 1), (128, 0), (40, 1)])
@pytest.mark.parametrize("H", [32, 512, 1000])
def test_whole_decode_draw_is_exact(lib, B, fused, H):
    """step-kernel path (B < 24), plane path with the fused 'arg-max of step t + recurrent GEMM of step t+1' launch, the two-chain
    schedule (decode_fused = 0: row0 = 64 for the second half) and a padded batch"""
    d = dict(B=B, L=6, F=64, H=H, E=40, V=301)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21)
    feats, _, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=22)
    m = _model(d, sd)
    prev = _set(lib, "decode_fused", fused)
    try:
        for temperature, seed in ((1.0, 77), (0.5, (1 << 40) + 5)):
            ids = m(feats.to(DEV), mode="sample", temperature=temperature, seed=seed)
            assert ids.dtype == torch.int64 and tuple(ids.shape) == (B, d["L"] - 1)
            _check_along_ids(sd, feats, ids, seed, temperature, d["V"])
    finally:
        _set(lib, "decode_fused", prev)
    capi.check_async_error()


def test_layout_independence(lib):
    d, sd, feats = hs.layout_fixture()
    seed = d["sample_seed"]
    m = _model(d, sd)
    ref_ids, marg = hs.replay_sample_fp64(sd, feats, seed)
    robust = (marg >= hs.eps_for(1.0)).all(1)
    assert robust.mean() >= 0.9
    extra, _, _ = synth.make_batch(30, d["L"], d["F"], d["V"], seed=99)
    big = torch.cat([feats, extra], 0)                          # B = 40: padded to 64 rows on the plane path, first 10 rows equal
    outs = {"B10": m(feats.to(DEV), mode="sample", seed=seed).cpu()}
    for fused in (0, 1):
        prev = _set(lib, "decode_fused", fused)
        try:
            outs["B40/fused%d" % fused] = m(big.to(DEV), mode="sample", seed=seed).cpu()[:10]
        finally:
            _set(lib, "decode_fused", prev)
    for name, ids in outs.items():
        assert torch.equal(ids[robust], ref_ids[robust]), name


def test_determinism_and_seeding(lib):
    d = synth.CONFIGS["mid64"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=31)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=32)
    m = _model(d, sd)
    x = feats.to(DEV)
    a = m(x, mode="sample", seed=5)
    assert torch.equal(a, m(x, mode="sample", seed=5))
    assert not torch.equal(a, m(x, mode="sample", seed=6))
    torch.manual_seed(123)
    b = m(x, mode="sample")
    c = m(x, mode="sample")
    torch.manual_seed(123)
    assert torch.equal(b, m(x, mode="sample")) and not torch.equal(b, c)
    # a greedy call in between fills / reuses the same weight-image cache
    g = m(x, mode="test")
    assert torch.equal(a, m(x, mode="sample", seed=5)) and torch.equal(g, m(x, mode="test"))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            m(x, mode="sample", temperature=bad)
    # temperature -> small (0.01): the greedy caption.  score = logit / t + g with g in [-2.82, 16.64]: a step is decided by its
    # logits wherever its float64 top-2 margin / t exceeds the noise range (19.5); a row follows the greedy caption up to its
    # first step that is not.  The fixture's out_linear is widened (synth's out_scale) so that these decided prefixes are more
    # than half of all steps - asserted, so the comparison cannot become vacuous
    t = 0.01
    from oracle import s2vt_oracle as orc
    sd_w = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=31, out_scale=400.0)
    mw = _model(d, sd_w)
    gi, gm = orc.greedy_decode(sd_w, feats, dtype=torch.float64, return_margins=True)
    decided = gm.numpy() / t > 19.5
    first = np.where(decided.all(1), decided.shape[1], (~decided).argmax(1))          # length of the decided prefix per row
    cold = mw(x, mode="sample", temperature=t, seed=5).cpu()
    print("decided prefixes: %.1f %% of all steps; whole rows %d of %d" % (100.0 * first.sum() / decided.size,
                                                                            (first == decided.shape[1]).sum(), len(first)))
    assert first.sum() >= 0.5 * decided.size
    for r in range(len(first)):
        assert torch.equal(cold[r, :first[r]], gi[r, :first[r]]), r


# ------------------------------------------------------------------ distribution on the device
def test_device_distribution(lib):
    """64 rows x the fixed seeds, one step, the fixed logit vector of the CPU test as the bias (h = 0): same chi-square bound, and
    the device counts equal the restatement's except on draws within eps"""
    V = hs.DIST_V
    h = torch.zeros(64, 32, device=DEV)
    w = torch.zeros(V, 32, device=DEV)
    b = torch.tensor(hs.DIST_LOGITS, dtype=torch.float32, device=DEV)
    p = np.exp(hs.DIST_LOGITS - hs.DIST_LOGITS.max())
    p /= p.sum()
    for planes in (False, True):
        counts = np.zeros(V)
        differ = 0
        for s in hs.SEEDS:
            ids = ops.decode_step_sample(h, w, b, seed=s, step=0, planes=planes).cpu().numpy()
            counts += np.bincount(ids, minlength=V)
            sc = b.cpu().double().numpy()[None, :] + sampling.gumbel_noise(s, 0, 64, V)
            own = sc.argmax(1)
            gap = sc.max(1) - sc[np.arange(64), ids]
            assert (gap <= hs.eps_for(1.0)).all()
            differ += int((own != ids).sum())
        stat = hs.chi_square(counts, p)
        print("planes=%d: chi2 = %.2f (bound %.2f); %d of %d draws differ from the restatement (all within eps)" %
              (planes, stat, hs.CHI2_BOUND, differ, 64 * len(hs.SEEDS)))
        assert stat < hs.CHI2_BOUND


def test_model_first_step_distribution(lib):
    """64 identical clips: the first decode step of mode='sample' draws from the softmax of one logit vector"""
    d = dict(B=64, L=4, F=64, H=32, E=24, V=hs.DIST_V)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=41, out_scale=4.0)
    one, _, _ = synth.make_batch(1, d["L"], d["F"], d["V"], seed=42)
    feats = one.expand(64, -1, -1).contiguous()
    m = _model(d, sd)
    from oracle import s2vt_oracle as orc
    prefix = torch.full((1, d["L"] - 1), 3, dtype=torch.long)
    with torch.no_grad():
        logit = orc.forward_train(sd, one, prefix, dtype=torch.float64)[0, 0].numpy()
    p = np.exp(logit - logit.max())
    p /= p.sum()
    counts = np.zeros(d["V"])
    for s in hs.SEEDS:
        counts += np.bincount(m(feats.to(DEV), mode="sample", seed=s)[:, 0].cpu().numpy(), minlength=d["V"])
    stat = hs.chi_square(counts, p)
    print("chi2 = %.2f (bound %.2f)" % (stat, hs.CHI2_BOUND))
    assert stat < hs.CHI2_BOUND


# ------------------------------------------------------------------ GRU / stacked / Att_Baseline
def test_gru_sample_is_exact(lib):
    d, sd, feats, _, _ = gru_gen.setup("gru_tiny")
    m = _model(d, sd, rnn_type="gru")
    seed, temperature = 314, 1.0
    ids = m(feats.to(DEV), mode="sample", seed=seed).cpu()
    assert torch.equal(ids, m(feats.to(DEV), mode="sample", seed=seed).cpu())
    # float64 replay along the device's ids (the arithmetic of make_gru_golden.replay_fp64, keeping the logits)
    p = {k: v.double() for k, v in sd.items()}
    B, L, H, E, V = feats.shape[0], d["L"], d["H"], d["E"], d["V"]
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    pad = torch.cat([x, torch.zeros(B, L - 1, H, dtype=torch.float64)], 1)
    v = [p["vid_rnn." + k] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    w = [p["word_rnn." + k] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    out1, _ = gru_gen._gru_seq(pad, torch.zeros(B, H, dtype=torch.float64), *v)
    _, hh = gru_gen._gru_seq(torch.cat([torch.zeros(B, L, E, dtype=torch.float64), out1[:, :L]], 2), torch.zeros(B, H, dtype=torch.float64), *w)
    tok = torch.full((B,), 3, dtype=torch.long)
    for i in range(L - 1):
        if i:
            tok = ids[:, i - 1]
        _, hh = gru_gen._gru_seq(torch.cat([p["embedding.weight"][tok], out1[:, L + i]], 1).unsqueeze(1), hh, *w)
        score = (hh @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy() / temperature + sampling.gumbel_noise(seed, i, B, V)
        gap = score.max(1) - score[np.arange(B), ids[:, i].numpy()]
        assert (gap <= hs.eps_for(temperature)).all(), i
    assert ids.max() < V


def _assert_draws_exact(score, ids, temperature, step):
    gap = score.max(1) - score[np.arange(score.shape[0]), ids]
    assert (gap <= hs.eps_for(temperature)).all(), (step, gap.max())
    return gap.max()


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_stacked_sample_is_exact(lib, temperature):
    """num_layers = 2: float64 replay along the device's ids (the arithmetic of make_stack_golden.replay_fp64, keeping the logits)"""
    import make_stack_golden as stack_gen
    d, sd, feats, _, _ = stack_gen.setup("stack_tiny")
    N, B, L, H, E, V = d["N"], feats.shape[0], d["L"], d["H"], d["E"], d["V"]
    m = _model(d, sd, num_layers=N)
    seed = 2718
    ids = m(feats.to(DEV), mode="sample", seed=seed, temperature=temperature).cpu()
    assert tuple(ids.shape) == (B, L - 1) and ids.dtype == torch.int64 and 0 <= int(ids.min()) and int(ids.max()) < V
    assert torch.equal(ids, m(feats.to(DEV), mode="sample", seed=seed, temperature=temperature).cpu())
    assert not torch.equal(ids, m(feats.to(DEV), mode="sample", seed=seed + 1, temperature=temperature).cpu())
    p = {k: v.double() for k, v in sd.items()}
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    z = torch.zeros(B, H, dtype=torch.float64)
    sv, sw = [(z, z)] * N, [(z, z)] * N
    for t in range(L):
        v, sv = stack_gen._lstm_stack_step(x[:, t], sv, p, "vid_rnn", N)
        _, sw = stack_gen._lstm_stack_step(torch.cat([torch.zeros(B, E, dtype=torch.float64), v], 1), sw, p, "word_rnn", N)
    tok = torch.full((B,), 3, dtype=torch.long)
    worst = 0.0
    for i in range(L - 1):
        if i:
            tok = ids[:, i - 1]
        v, sv = stack_gen._lstm_stack_step(z, sv, p, "vid_rnn", N)
        o, sw = stack_gen._lstm_stack_step(torch.cat([p["embedding.weight"][tok], v], 1), sw, p, "word_rnn", N)
        score = (o @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy() / temperature + sampling.gumbel_noise(seed, i, B, V)
        worst = max(worst, _assert_draws_exact(score, ids[:, i].numpy(), temperature, i))
    print("stacked: max float64 gap of the chosen index %.3g (eps %.3g)" % (worst, hs.eps_for(temperature)))
    capi.check_async_error()


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_att_baseline_sample_is_exact(lib, temperature):
    """Att_Baseline: float64 replay along the device's ids with torch's own nn.LSTM / nn.Linear in float64 on the CPU over a copy
    of the module's parameters (the network as the reference computes it: every attention weight is 1, the context is the sum of
    the bidirectional encoder's outputs).  L steps, the first input is <sos>, decode step i uses the noise of step i."""
    import copy
    import attention_baseline
    d = dict(B=5, L=8, F=64, H=32, E=24, V=50)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=6)
    torch.manual_seed(0)
    att = attention_baseline.Att_Baseline(d["V"], d["F"], length=d["L"], dim_hid=d["H"], dim_embed=d["E"])
    with torch.no_grad():
        att.out_linear.weight.mul_(4.0)                                    # logits wide enough for the draws to depend on them
    m64 = copy.deepcopy(att).double().eval()
    att = att.to(DEV).eval()
    seed = 1618
    ids = att(feats.to(DEV), mode="sample", seed=seed, temperature=temperature).cpu()
    B, L, V = d["B"], d["L"], d["V"]
    assert tuple(ids.shape) == (B, L) and ids.dtype == torch.int64 and 0 <= int(ids.min()) and int(ids.max()) < V
    assert torch.equal(ids, att(feats.to(DEV), mode="sample", seed=seed, temperature=temperature).cpu())
    assert not torch.equal(ids, att(feats.to(DEV), mode="sample", seed=seed + 1, temperature=temperature).cpu())
    worst = 0.0
    with torch.no_grad():
        enc, _ = m64.encoder(m64.feat_linear(feats.double()))              # [B, L, 2H]
        ctxv = enc.sum(1)
        state = None
        tok = torch.full((B,), int(att.sos_ix), dtype=torch.long)
        for i in range(L):
            if i:
                tok = ids[:, i - 1]
            out, state = m64.decoder(torch.cat([m64.embedding(tok), ctxv], 1).unsqueeze(1), state)
            score = m64.out_linear(out[:, 0]).numpy() / temperature + sampling.gumbel_noise(seed, i, B, V)
            worst = max(worst, _assert_draws_exact(score, ids[:, i].numpy(), temperature, i))
    print("Att_Baseline: max float64 gap of the chosen index %.3g (eps %.3g)" % (worst, hs.eps_for(temperature)))
    capi.check_async_error()


# ------------------------------------------------------------------ RewardCriterion
def _reward_case(B, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, L - 1, V, generator=g) * 2
    target = torch.randint(0, V, (B, L), generator=g)
    weight = torch.randn(B, L, generator=g)
    weight[:, L // 2 + 1:] = 0.0                   # zero after "<eos>"
    if B > 1:
        weight[1] = 0.0                            # a row without any weight
    return logits, target, weight


@pytest.mark.parametrize("B,L,V", [(1, 5, 50), (7, 9, 301), (64, 12, 1000), (2, 4, 16388), (3, 5, 1027)])
def test_reward_criterion_matches_float64_autograd(lib, B, L, V):
    import utils
    logits, target, weight = _reward_case(B, L, V, 50 + B)
    x = logits.to(DEV).requires_grad_(True)
    loss = utils.RewardCriterion()(x, target.to(DEV), weight.to(DEV))
    (loss * 1.7).backward()                        # (a grad_output other than 1, as test_mean_ce_fwd_bwd: the gout factor)
    x64 = logits.double().requires_grad_(True)
    w = weight[:, 1:].double()
    norm = max(int((w != 0).sum()), 1)
    ref = -(w * torch.log_softmax(x64, 2).gather(2, target[:, 1:, None]).squeeze(2)).sum() / norm
    (ref * 1.7).backward()
    # The relative tolerance of tests/test_gpu_kernels.py::test_mean_ce_fwd_bwd (2e-6 on the loss, 1e-7 + 2e-6 x the gradient's
    # scale), applied to the magnitudes that enter here: the weights have both signs, so the sum cancels and fp32 rounding goes
    # with sum |w_i CE_i| / norm, not with the result; the gradient's scale is max |w| / norm where the mean CE's is 1 / rows
    ce = -torch.log_softmax(x64.detach(), 2).gather(2, target[:, 1:, None]).squeeze(2)
    mag = float((w.abs() * ce).sum() / norm)
    print("loss %.8f ref %.8f (terms %.3f)" % (float(loss), float(ref), mag))
    assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, mag)
    err = (x.grad.cpu().double() - x64.grad).abs().max().item()
    print("max |dlogits - ref| = %.3g" % err)
    assert err <= 1e-7 + 2e-6 * float(w.abs().max()) / norm
    assert (x.grad.cpu()[weight[:, 1:] == 0] == 0).all()
    # deterministic: a second backward is bit-equal
    x2 = logits.to(DEV).requires_grad_(True)
    loss2 = utils.RewardCriterion()(x2, target.to(DEV), weight.to(DEV))
    (loss2 * 1.7).backward()
    assert torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)
    capi.check_async_error()


def test_reward_criterion_all_zero_weight_and_bad_target(lib):
    import utils
    logits, target, weight = _reward_case(3, 6, 40, 1)
    x = logits.to(DEV).requires_grad_(True)
    loss = utils.RewardCriterion()(x, target.to(DEV), torch.zeros_like(weight).to(DEV))
    loss.backward()
    assert float(loss) == 0.0 and not x.grad.any()
    capi.check_async_error()
    bad = target.clone()
    bad[2, 3] = 40
    utils.RewardCriterion()(logits.to(DEV), bad.to(DEV), weight.to(DEV))
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()


def test_bad_id_of_the_second_of_two_flagged_entry_points_is_reported_once(lib):
    """Two per-op entry points that share the device's flag words (PostedFlags), back to back: the mean CE with good targets,
    then s2vt_tokens_time_major with one bad id.  The first call's record is clean, the second's is not: one IndexError."""
    from s2vt_video_caption_amd import functional as F
    capi.check_async_error()
    logits, target, _ = _reward_case(3, 6, 40, 2)
    loss = F.mean_cross_entropy(logits.to(DEV), target.to(DEV))
    bad = target.clone()
    bad[1, 2] = 40
    tok = ops.tokens_time_major(bad.to(DEV), 5, 40)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and int(tok.max()) < 40           # (the bad id is clamped)
    with pytest.raises(IndexError):
        capi.check_async_error()
    capi.check_async_error()


def test_reward_criterion_trains_the_model_on_sampled_ids(lib):
    """the self-critical step's device side: sample, teacher-force the sampled ids, weighted loss, backward - finite gradients"""
    import utils
    d = synth.CONFIGS["tiny"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=42)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=42)
    m = _model(d, sd).train()
    x = feats.to(DEV)
    with torch.no_grad():
        ids = m(x, mode="sample", seed=3)
    caps = torch.cat([torch.full((d["B"], 1), 3, dtype=torch.long, device=DEV), ids], 1)
    weight = torch.zeros(d["B"], d["L"], device=DEV)
    weight[:, 1:4] = torch.tensor([0.5, -0.25, 1.0], device=DEV)[:, None]
    loss = utils.RewardCriterion()(m(x, targets=caps[:, :-1], mode="train"), caps, weight)
    loss.backward()
    assert torch.isfinite(loss)
    for n, q in m.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), n
    assert m.out_linear.weight.grad.abs().sum() > 0
    capi.check_async_error()


# ------------------------------------------------------------------ train.py --self-critical
@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_self_critical_epoch_end_to_end(tmp_path, rnn_type):
    """one epoch of train.py --self-critical on the toy split of the entry-point tests: finite loss, rewards recorded, the split of
    a step reported, the checkpoint loads and decodes.  No claim about caption quality."""
    sys.path.insert(0, ROOT)
    import train
    import test_train_eval_parity as toy
    toy.make_toy(str(tmp_path))
    ck = tmp_path / "ck"
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(toy.L), "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F),
                       "--batch-size", str(toy.BS), "--epochs", "1", "--lr", "1e-3", "--save-path", str(ck), "--no-shuffle",
                       "--seed", "7", "--rnn-type", rnn_type, "--self-critical", "--sc-temperature", "1.0"])
    got = train.run(opt)
    assert len(got["train_loss"]) == 1 and np.isfinite(got["train_loss"][0]) and np.isfinite(got["valid_loss"][0])
    sp = got["sc_split_ms"]
    assert sp["steps"] == 3 and all(sp[k] > 0 for k in ("sample", "greedy", "scoring", "train"))
    print("self-critical step split (ms per step):", {k: round(v / sp["steps"], 2) for k, v in sp.items() if k != "steps"})
    assert len(got["reward_sample"]) == 3 and all(np.isfinite(got["reward_sample"])) and all(r >= 0 for r in got["reward_greedy"])
    m = torch.load(ck / (got["start_time"] + "final.pth"), weights_only=False).to(DEV).eval()
    import dataloader
    ds = dataloader.VideoDataset(str(tmp_path / "captions.json"), str(tmp_path / "feats"), max_len=toy.L, mode="test")
    feats = torch.stack([ds[i][0] for i in range(len(ds))]).to(DEV)
    ids = m(feats, mode="test")
    assert tuple(ids.shape) == (len(ds), toy.L - 1) and int(ids.max()) < 30
    assert torch.isfinite(torch.cat([q.reshape(-1) for q in m.parameters()])).all()
