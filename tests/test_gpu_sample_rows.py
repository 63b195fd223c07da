"""GPU tests of K sampled captions per clip on one encode (S2VT.sample, csrc/api_sample_rows.hip) and of the grouped self-critical
weights (s2vt_sc_weights_group).

The reference of a draw is float64 on the CPU, as in test_gpu_sampling.py: the numpy restatement of the noise and a teacher-forced
replay of the network along the device's own ids, on the clips repeated K times - row b*K + k is batch row b*K + k of that batch.
A draw is right when its float64 score is within eps of the float64 maximum - at every row and step, no row left out."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops, synth
from s2vt_video_caption_amd import functional as F
from s2vt_video_caption_amd.self_critical import advantage_weights, group_advantages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sampling_host as hs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOS, EOS = 3, 4


def _model(d, sd, **kw):
    import S2VTModel
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ 1. every draw is exact
@pytest.mark.parametrize("B,K", [(3, 2), (10, 5), (40, 3), (64, 2)])
@pytest.mark.parametrize("H", [32, 1000])
def test_every_draw_is_exact(lib, B, K, H):
    """fp32 step path inside one tile (R = 6) and with a ragged row count (R = 50: the clip gather is not the identity); the plane
    path with B padded to 64 in the encode while the rows pad to 128 (R = 120) and without padding (R = 128); H = 1000: the k
    padding of the h_t plane image"""
    d = dict(B=B, L=6, F=64, H=H, E=40, V=301)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21)
    feats, _, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=22)
    m = _model(d, sd)
    rep = feats.repeat_interleave(K, 0)
    for temperature, seed in ((1.0, 77), (0.5, (1 << 40) + 5)):
        ids = m.sample(feats.to(DEV), K, temperature=temperature, seed=seed)
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (B, K, d["L"] - 1) and ids.is_cuda
        flat = ids.view(B * K, -1).cpu()
        score = hs.scores_along_ids_fp64(sd, rep, flat, seed, temperature)
        idn = flat.numpy()
        assert idn.min() >= 0 and idn.max() < d["V"]
        gap = score.max(2) - np.take_along_axis(score, idn[:, :, None], 2)[:, :, 0]
        print("B=%d K=%d H=%d t=%g: max float64 gap of the chosen index %.3g (eps %.3g)" % (B, K, H, temperature, gap.max(),
                                                                                              hs.eps_for(temperature)))
        assert (gap <= hs.eps_for(temperature)).all()
    capi.check_async_error()


# ------------------------------------------------------------------ 2. the draws of the repeated batch
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("seed", [2024, 77])
def test_same_draws_as_the_repeated_batch(lib, K, seed):
    d, sd, feats = hs.layout_fixture()
    B = d["B"]
    m = _model(d, sd)
    rep = feats.repeat_interleave(K, 0)
    ref_ids, marg = hs.replay_sample_fp64(sd, rep, seed)
    print("K=%d seed=%d: smallest float64 top-2 margin %.3g (eps %.3g)" % (K, seed, marg.min(), hs.eps_for(1.0)))
    assert (marg >= hs.eps_for(1.0)).all()                       # every row is decided: none is left out below
    got = m.sample(feats.to(DEV), K, seed=seed)
    assert tuple(got.shape) == (B, K, d["L"] - 1)
    flat = got.view(B * K, -1).cpu()
    assert torch.equal(flat, ref_ids)
    assert torch.equal(flat, m(rep.to(DEV), mode="sample", seed=seed).cpu())
    rows = got.cpu()
    for b in range(B):                                           # the K rows of a clip are K different draws
        assert len({tuple(r.tolist()) for r in rows[b]}) == K, b
    # K = 1 is mode='sample' with a middle axis of 1
    assert torch.equal(m.sample(feats.to(DEV), 1, seed=seed)[:, 0].cpu(), m(feats.to(DEV), mode="sample", seed=seed).cpu())
    capi.check_async_error()


# ------------------------------------------------------------------ 3. determinism, seeding, the decode cache
def test_determinism_seeding_and_cache(lib):
    d = synth.CONFIGS["mid64"]
    K = 2
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=31)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=32)
    x = feats.to(DEV)
    fresh = _model(d, sd)
    greedy = fresh(x, mode="test").cpu()                          # what a fresh model decodes
    m = _model(d, sd)
    assert F._DECODE_CACHES.get(m) is None
    a = m.sample(x, K, seed=5)
    entry = F._DECODE_CACHES.get(m)
    assert entry is not None and entry[2]                         # the first call on fresh weights filled the decode cache
    assert torch.equal(greedy, m(x, mode="test").cpu())           # ... with every image a greedy decode reads
    assert F._DECODE_CACHES.get(m)[1] is entry[1]
    assert torch.equal(a, m.sample(x, K, seed=5))
    assert not torch.equal(a, m.sample(x, K, seed=6))
    torch.manual_seed(123)
    b = m.sample(x, K)
    c = m.sample(x, K)
    torch.manual_seed(123)
    assert torch.equal(b, m.sample(x, K)) and not torch.equal(b, c)
    # plane path against the fp32 path: in gemm mode 0 the call takes no cache and draws on the fp32-input MFMA path; the two may
    # differ only where two float64 scores along the plane path's ids are closer than the paths' logit rounding
    assert capi.decode_plan(capi.Dims(d["B"], d["L"], d["F"], d["H"], d["E"], d["V"]))[1] == 1      # (a was the plane path's)
    prev = lib.s2vt_set_gemm_mode(0)
    try:
        f32 = m.sample(x, K, seed=5)
    finally:
        lib.s2vt_set_gemm_mode(prev)
    rep = feats.repeat_interleave(K, 0)
    flat = a.view(d["B"] * K, -1).cpu()
    score = hs.scores_along_ids_fp64(sd, rep, flat, 5)
    top = np.sort(score, axis=2)
    decided = ((top[:, :, -1] - top[:, :, -2]) >= hs.eps_for(1.0)).all(1)
    print("rows decided at every step: %d of %d" % (decided.sum(), len(decided)))
    # (a top-2 gap below eps = 1.4e-5 has a probability of about eps per step - the gap's density near 0 is of order 1 - so about
    # 23 * eps = 3e-4 per row: the bound only keeps the comparison from becoming vacuous)
    assert decided.mean() >= 0.9
    assert torch.equal(f32.view(d["B"] * K, -1).cpu()[decided], flat[decided])
    capi.check_async_error()


# ------------------------------------------------------------------ 4. GRU and stacked models
@pytest.mark.parametrize("kind", ["gru", "stacked"])
def test_gru_and_stacked_sample_rows(lib, kind):
    if kind == "gru":
        import make_gru_golden as gen
        d, sd, feats, _, _ = gen.setup("gru_tiny")
        m = _model(d, sd, rnn_type="gru")
    else:
        import make_stack_golden as gen
        d, sd, feats, _, _ = gen.setup("stack_tiny")
        m = _model(d, sd, num_layers=d["N"])
    B, K, s = feats.shape[0], 3, 314
    got = m.sample(feats.to(DEV), K, seed=s)
    assert tuple(got.shape) == (B, K, d["L"] - 1) and got.dtype == torch.int64
    assert torch.equal(got.view(K * B, -1), m(feats.repeat_interleave(K, 0).to(DEV), mode="sample", seed=s))
    capi.check_async_error()


# ------------------------------------------------------------------ 5. the grouped weights
@pytest.mark.parametrize("B,K,T", [(1, 2, 5), (7, 5, 9), (64, 3, 30)])
def test_grouped_weights_equal_the_host(lib, B, K, T):
    rng = np.random.RandomState(100 * B + K)
    R = B * K
    sampled = torch.tensor(rng.randint(5, 30, size=(R, T)), dtype=torch.long)
    sampled[0, 0] = EOS                                    # <eos> first
    sampled[1, T // 2] = EOS                               # in the middle
    sampled[1, T - 1] = EOS                                # twice: the first counts
    for r in range(2, R, 3):
        sampled[r, rng.randint(0, T)] = EOS                # rows 3, 4, 6, 7, ...: no <eos>
    assert (sampled == EOS).any(1).sum() < R or R <= 2
    r_s = rng.rand(B, K) * 3
    r_s[B - 1, :] = 0.1 + 0.2                              # one clip with equal rewards (a value whose K-term sum rounds)
    if B > 1:
        r_s[0, 0], r_s[0, 1] = 0.1 + 0.2, 0.3              # a difference that only float64 resolves before the one rounding to fp32
    r_g = rng.rand(B) * 3
    dev_s = sampled.to(DEV)
    t_s = torch.tensor(r_s.reshape(-1), device=DEV)
    sos_col = torch.full((R, 1), SOS, dtype=torch.long)
    for greedy in (None, r_g):
        adv, base = group_advantages(r_s, greedy)
        want_w = advantage_weights(sampled, adv.reshape(-1), EOS)
        caps, weight, baseline = ops.sc_weights_group(dev_s, t_s, None if greedy is None else torch.tensor(greedy, device=DEV), K, SOS,
                                                      EOS, return_baseline=True)
        torch.cuda.synchronize()
        assert caps.dtype == torch.int64 and weight.dtype == torch.float32 and baseline.dtype == torch.float64
        assert tuple(caps.shape) == tuple(weight.shape) == (R, T + 1) and tuple(baseline.shape) == (R,)
        assert torch.equal(caps.cpu(), torch.cat([sos_col, sampled], 1))
        assert np.array_equal(baseline.cpu().numpy(), base.reshape(-1))
        assert torch.equal(weight.cpu(), want_w)
        two = ops.sc_weights_group(dev_s, t_s, None if greedy is None else torch.tensor(greedy, device=DEV), K, SOS, EOS)
        assert len(two) == 2 and torch.equal(two[1], weight)
        if greedy is None:
            assert (weight.cpu()[(B - 1) * K:] == 0).all()                                       # the equal group: exactly zero
            assert B == 1 or (want_w[:K, 1:2] != 0).all()
    # K = 1 with a greedy reward is s2vt_sc_weights
    t_g = torch.tensor(np.repeat(r_g, K), device=DEV)
    c1, w1 = ops.sc_weights_group(dev_s, t_s, t_g, 1, SOS, EOS)
    c0, w0 = ops.sc_weights(dev_s, t_s, t_g, SOS, EOS)
    assert torch.equal(c1, c0) and torch.equal(w1, w0)
    with pytest.raises(ValueError):
        ops.sc_weights_group(dev_s, t_s, None, 1, SOS, EOS)
    with pytest.raises(capi.S2VTHipError):
        ops.sc_weights_group(dev_s, t_s.float(), None, K, SOS, EOS)
    capi.check_async_error()


# ------------------------------------------------------------------ 6. train.py --self-critical --sc-samples K --sc-baseline mean
@pytest.mark.parametrize("where", ["host", "device"])
def test_self_critical_epoch_with_grouped_baseline(tmp_path, where):
    """one epoch (3 steps) on the toy split of the entry-point tests: K = 3 samples per clip, each compared with the mean of the other
    two - no greedy decode runs; the defaults still run the greedy baseline.  No claim about caption quality."""
    sys.path.insert(0, ROOT)
    import dataloader
    import train
    import S2VTModel
    import test_train_eval_parity as toy
    toy.make_toy(str(tmp_path))

    def run(name, extra):
        opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                           "--train-length", str(toy.L), "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F),
                           "--batch-size", str(toy.BS), "--epochs", "1", "--lr", "1e-3", "--save-path", str(tmp_path / name),
                           "--no-shuffle", "--seed", "7", "--self-critical", "--sc-reward", where] + extra)
        return train.run(opt)

    h = run("ck_mean", ["--sc-samples", "3", "--sc-baseline", "mean"])
    assert len(h["train_loss"]) == 1 and np.isfinite(h["train_loss"][0]) and np.isfinite(h["valid_loss"][0])
    assert len(h["reward_sample"]) == 3 and all(np.isfinite(h["reward_sample"]))
    assert len(h["reward_baseline"]) == 3 and all(np.isfinite(h["reward_baseline"]))
    assert h["reward_greedy"] == []
    sp = h["sc_split_ms"]
    assert sorted(sp) == ["greedy", "sample", "scoring", "steps", "train"]
    assert sp["steps"] == 3 and sp["greedy"] == 0 and all(sp[k] > 0 for k in ("sample", "scoring", "train"))
    print(where, "K = 3, mean baseline: step split (ms per step):", {k: round(v / sp["steps"], 2) for k, v in sp.items() if k != "steps"})
    trained = torch.load(tmp_path / "ck_mean" / (h["start_time"] + "final.pth"), weights_only=False)
    word2ix = dataloader.VideoDataset(str(tmp_path / "captions.json"), str(tmp_path / "feats"), max_len=toy.L).word2ix
    torch.manual_seed(0)                                   # train.run's seeded default init
    init = S2VTModel.S2VT(len(word2ix), toy.F, length=toy.L, dim_hid=toy.H, dim_embed=toy.E, sos_ix=word2ix['<sos>'],
                          eos_ix=word2ix['<eos>'])
    w = trained.out_linear.weight.detach().cpu()
    assert torch.isfinite(w).all() and not torch.equal(w, init.out_linear.weight.detach())
    # the defaults: today's step, a greedy decode per step
    h1 = run("ck_default", ["--sc-samples", "1"])
    assert len(h1["reward_greedy"]) == 3 and len(h1["reward_sample"]) == 3 and h1["sc_split_ms"]["greedy"] > 0
    assert h1["reward_baseline"] == h1["reward_greedy"]
    capi.check_async_error()
