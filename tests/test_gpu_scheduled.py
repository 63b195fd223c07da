"""GPU tests of scheduled sampling (S2VT.forward(mode='train', ss_prob > 0)).

The references are float64 on the CPU and the numpy coin (sampling.ss_coin), never the code under test: the words a pass fed
(`used`) must follow the coin rule exactly, and every choice of the model (`draws`) must be within the sampled decode's eps of the
float64 maximum of a teacher-forced replay ALONG `used` - at every row and step."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, functional, gru_functional, ops, sampling, stack_functional, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_gru_golden as gru_gen  # noqa: E402
import make_stack_golden as stack_gen  # noqa: E402
import test_sampling_host as hs  # noqa: E402
from oracle import s2vt_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, F, E, V = 6, 64, 40, 301
T = L - 1
SOS = 3


def _set(lib, name, value):
    return lib.s2vt_set_option(name.encode(), value)


def _model(H, sd, **kw):
    import S2VTModel
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _batch(B, seed=22):
    feats, caps, mask = synth.make_batch(B, L, F, V, seed=seed)
    return feats, caps, mask


def _assert_rule(used, draws, targets, p, seed):
    """used follows the coin rule exactly; both outcomes of the coin occur"""
    used, draws, targets = used.cpu().numpy(), draws.cpu().numpy(), targets.cpu().numpy()
    assert np.array_equal(used[:, 0], targets[:, 0])
    assert np.array_equal(used, sampling.ss_used(targets, draws, p, seed))
    own = np.stack([sampling.ss_coin(seed, j, targets.shape[0]) < np.float32(p) for j in range(1, targets.shape[1])], 1)
    assert own.any() and not own.all()
    assert draws.min() >= 0 and draws.max() < V


def _assert_draws(score, draws, temperature):
    """score float64 [B, T, V] along `used`: every draw within eps of its row's maximum"""
    dn = draws.cpu().numpy()
    gap = score.max(2) - np.take_along_axis(score, dn[:, :, None], 2)[:, :, 0]
    eps = hs.eps_for(1.0 if temperature is None else temperature)
    print("max float64 gap of the chosen index %.3g (eps %.3g)" % (gap.max(), eps))
    assert (gap <= eps).all()


def _noise(seed, B, temperature):
    if temperature is None:
        return 0.0
    return np.stack([sampling.gumbel_noise(seed, j, B, V) for j in range(T)], 1)


# ------------------------------------------------------------------ 1. the coin, bit-exact
@pytest.mark.parametrize("B", [1, 5, 64, 130])
def test_coin_is_bit_exact(lib, B):
    g = torch.Generator().manual_seed(B)
    targets = torch.randint(0, V, (B, 9), generator=g)
    draws = torch.randint(0, V, (B,), generator=g) + 1000           # disjoint from the targets' ids: the source of a word is visible
    for p in (0.0, 0.25, 1.0):
        for seed in (12345, (1 << 40) + 17):
            for step in (1, 7):
                for row0 in (0, 64):
                    got = ops.ss_mix(draws.to(DEV), targets.to(DEV), p, seed, step, row0=row0).cpu().numpy()
                    own = sampling.ss_coin(seed, step, np.arange(row0, row0 + B)) < np.float32(p)
                    want = np.where(own, draws.numpy(), targets[:, step].numpy())
                    assert np.array_equal(got, want), (p, seed, step, row0)
    # step 0 has no previous draw
    assert torch.equal(ops.ss_mix(draws.to(DEV), targets.to(DEV), 1.0, 5, 0).cpu(), targets[:, 0])


# ------------------------------------------------------------------ 2. the whole pass, exact along its own inputs
@pytest.mark.parametrize("B,fused", [(4, 1), (10, 1), (64, 1), (128, 1), (128, 0), (40, 1)])
@pytest.mark.parametrize("H", [32, 1000])
def test_whole_pass_is_exact_along_its_inputs(lib, B, fused, H):
    """step-kernel path (gate GEMVs at B = 4), the fused plane schedule, the two-chain schedule (row0 = 64) and a padded batch"""
    sd = synth.make_state_dict(V, F, H, E, seed=21)
    feats, caps, _ = _batch(B)
    targets = caps[:, :-1]
    m = _model(H, sd)
    p = 0.5
    prev = _set(lib, "decode_fused", fused)
    try:
        for temperature, seed in ((None, 77), (0.5, (1 << 40) + 5)):
            used, draws = functional.scheduled_inputs(feats.to(DEV), targets.to(DEV), m._hip_params(), p, temperature=temperature,
                                                      seed=seed, owner=m, return_draws=True)
            assert used.dtype == draws.dtype == torch.int64 and tuple(used.shape) == tuple(draws.shape) == (B, T)
            _assert_rule(used, draws, targets, p, seed)
            with torch.no_grad():
                logits = orc.forward_train(sd, feats, used.cpu(), dtype=torch.float64).numpy()
            score = logits if temperature is None else logits / temperature + _noise(seed, B, temperature)
            _assert_draws(score, draws, temperature)
    finally:
        _set(lib, "decode_fused", prev)
    capi.check_async_error()


# ------------------------------------------------------------------ 3. the ends of the range are the existing modes
@pytest.mark.parametrize("B", [10, 64])
def test_ends_of_the_range_agree_with_the_existing_modes(lib, B):
    H = 32
    sd = synth.make_state_dict(V, F, H, E, seed=21)
    feats, caps, _ = _batch(B)
    targets = caps[:, :-1].clone()
    targets[:, 0] = SOS
    m = _model(H, sd)
    x, tg = feats.to(DEV), targets.to(DEV)
    used, draws = functional.scheduled_inputs(x, tg, m._hip_params(), 1.0, seed=9, owner=m, return_draws=True)
    assert torch.equal(draws, m(x, mode="test")) and torch.equal(used[:, 1:], draws[:, :-1]) and torch.equal(used[:, 0], tg[:, 0])
    t, s = 0.5, (1 << 33) + 3
    used, draws = functional.scheduled_inputs(x, tg, m._hip_params(), 1.0, temperature=t, seed=s, owner=m, return_draws=True)
    assert torch.equal(draws, m(x, mode="sample", temperature=t, seed=s)) and torch.equal(used[:, 1:], draws[:, :-1])
    for temperature in (None, 0.5):
        assert torch.equal(functional.scheduled_inputs(x, tg, m._hip_params(), 0.0, temperature=temperature, seed=4, owner=m), tg)
    capi.check_async_error()


# ------------------------------------------------------------------ 4. the train step on `used` is the plain train step
def _step(m, x, targets, caps, mask, **kw):
    import utils
    m.zero_grad(set_to_none=True)
    logits = m(x, targets=targets, mode="train", **kw)
    utils.MaskCriterion()(logits, caps, mask).backward()
    return logits.detach().clone(), {n: q.grad.detach().clone() for n, q in m.named_parameters()}


@pytest.mark.parametrize("B", [7, 64])
def test_train_step_on_used_is_the_plain_train_step(lib, B):
    H = 32
    sd = synth.make_state_dict(V, F, H, E, seed=21)
    feats, caps, mask = _batch(B)
    m = _model(H, sd).train()
    x, cp, mk = feats.to(DEV), caps.to(DEV), mask.to(DEV)
    tg = cp[:, :-1]
    seed = 31
    la, ga = _step(m, x, tg, cp, mk, ss_prob=0.5, seed=seed)
    used = functional.scheduled_inputs(x, tg, m._hip_params(), 0.5, seed=seed, owner=m)
    assert not torch.equal(used, tg)
    lb, gb = _step(m, x, used, cp, mk)
    assert torch.equal(la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    l0, g0 = _step(m, x, tg, cp, mk)
    l1, g1 = _step(m, x, tg, cp, mk, ss_prob=0.0)
    assert torch.equal(l0, l1) and not torch.equal(l0, la)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    capi.check_async_error()


# ------------------------------------------------------------------ 5. seeding
def test_seeding(lib):
    B, H = 10, 32
    sd = synth.make_state_dict(V, F, H, E, seed=21)
    feats, caps, _ = _batch(B)
    m = _model(H, sd)
    x, tg = feats.to(DEV), caps[:, :-1].to(DEV)

    def run(seed):
        return functional.scheduled_inputs(x, tg, m._hip_params(), 0.5, temperature=1.0, seed=seed, owner=m)
    a = run(5)
    assert torch.equal(a, run(5)) and not torch.equal(a, run(6))
    torch.manual_seed(123)
    b, c = run(None), run(None)
    torch.manual_seed(123)
    assert torch.equal(b, run(None)) and not torch.equal(b, c)


# ------------------------------------------------------------------ 6. a bad ground-truth id
def test_bad_forced_id_raises_index_error(lib):
    B, H, p = 5, 32, 0.5
    sd = synth.make_state_dict(V, F, H, E, seed=21)
    feats, caps, _ = _batch(B)
    m = _model(H, sd)
    x = feats.to(DEV)
    seed, row, col = next((s, 2, 3) for s in range(100) if sampling.ss_coin(s, 3, B)[2] >= np.float32(p))   # (2, 3) is fed from targets
    bad = caps[:, :-1].clone()
    bad[row, col] = V
    capi.check_async_error()
    used = functional.scheduled_inputs(x, bad.to(DEV), m._hip_params(), p, seed=seed, owner=m)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()
    assert int(used[row, col]) == V                         # (recorded as given; the kernel read token 0)
    functional.scheduled_inputs(x, caps[:, :-1].to(DEV), m._hip_params(), p, seed=seed, owner=m)
    torch.cuda.synchronize()
    capi.check_async_error()


# ------------------------------------------------------------------ 7. GRU and stacked LSTM
def _gru_logits_fp64(sd, feats, used, H):
    """tools/make_gru_golden's arithmetic, teacher-forced along `used`: float64 logits [B, T, V]"""
    p = {k: v.double() for k, v in sd.items()}
    B = feats.shape[0]
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    pad = torch.cat([x, torch.zeros(B, L - 1, H, dtype=torch.float64)], 1)
    v = [p["vid_rnn." + k] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    w = [p["word_rnn." + k] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    out1, _ = gru_gen._gru_seq(pad, torch.zeros(B, H, dtype=torch.float64), *v)
    _, hh = gru_gen._gru_seq(torch.cat([torch.zeros(B, L, E, dtype=torch.float64), out1[:, :L]], 2), torch.zeros(B, H, dtype=torch.float64), *w)
    out = []
    for i in range(T):
        _, hh = gru_gen._gru_seq(torch.cat([p["embedding.weight"][used[:, i]], out1[:, L + i]], 1).unsqueeze(1), hh, *w)
        out.append(hh @ p["out_linear.weight"].t() + p["out_linear.bias"])
    return torch.stack(out, 1).numpy()


def _stack_logits_fp64(sd, feats, used, H, N):
    """tools/make_stack_golden's arithmetic, teacher-forced along `used`: float64 logits [B, T, V]"""
    p = {k: v.double() for k, v in sd.items()}
    B = feats.shape[0]
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    z = torch.zeros(B, H, dtype=torch.float64)
    sv, sw = [(z, z)] * N, [(z, z)] * N
    for t in range(L):
        v, sv = stack_gen._lstm_stack_step(x[:, t], sv, p, "vid_rnn", N)
        _, sw = stack_gen._lstm_stack_step(torch.cat([torch.zeros(B, E, dtype=torch.float64), v], 1), sw, p, "word_rnn", N)
    out = []
    for i in range(T):
        v, sv = stack_gen._lstm_stack_step(z, sv, p, "vid_rnn", N)
        o, sw = stack_gen._lstm_stack_step(torch.cat([p["embedding.weight"][used[:, i]], v], 1), sw, p, "word_rnn", N)
        out.append(o @ p["out_linear.weight"].t() + p["out_linear.bias"])
    return torch.stack(out, 1).numpy()


@pytest.mark.parametrize("B", [10, 64])
@pytest.mark.parametrize("kind", ["gru", "stack"])
def test_gru_and_stacked_pass_is_exact_along_its_inputs(lib, kind, B):
    H, p = 32, 0.5
    feats, caps, mask = _batch(B)
    targets = caps[:, :-1]
    if kind == "gru":
        sd = synth.make_gru_state_dict(V, F, H, E, seed=5)
        m, mod = _model(H, sd, rnn_type="gru"), gru_functional
    else:
        sd = synth.make_state_dict(V, F, H, E, seed=21, num_layers=2)
        m, mod = _model(H, sd, num_layers=2, rnn_dropout=0.3).train(), stack_functional       # (no dropout mask may be drawn)
    for temperature, seed in ((None, 77), (0.5, (1 << 40) + 5)):
        used, draws = mod.scheduled_inputs(m, feats.to(DEV), targets.to(DEV), p, temperature=temperature, seed=seed, return_draws=True)
        assert tuple(used.shape) == tuple(draws.shape) == (B, T)
        _assert_rule(used, draws, targets, p, seed)
        logits = _gru_logits_fp64(sd, feats, used.cpu(), H) if kind == "gru" else _stack_logits_fp64(sd, feats, used.cpu(), H, 2)
        score = logits if temperature is None else logits / temperature + _noise(seed, B, temperature)
        _assert_draws(score, draws, temperature)
    # through forward(): the train step runs on the words of the pass with the same seed
    import utils
    m.eval()
    x, cp, mk = feats.to(DEV), caps.to(DEV), mask.to(DEV)
    used = mod.scheduled_inputs(m, x, cp[:, :-1], p, seed=11)
    la = m(x, targets=cp[:, :-1], mode="train", ss_prob=p, seed=11)
    assert torch.equal(la, m(x, targets=used, mode="train")) and not torch.equal(used, cp[:, :-1])
    utils.MaskCriterion()(la, cp, mk).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())
    torch.cuda.synchronize()
    capi.check_async_error()


@pytest.mark.parametrize("kind", ["gru", "stack"])
def test_gru_and_stacked_bad_forced_id(lib, kind):
    B, H, p = 5, 32, 0.5
    feats, caps, _ = _batch(B)
    if kind == "gru":
        m, mod = _model(H, synth.make_gru_state_dict(V, F, H, E, seed=5), rnn_type="gru"), gru_functional
    else:
        m, mod = _model(H, synth.make_state_dict(V, F, H, E, seed=21, num_layers=2), num_layers=2), stack_functional
    seed = next(s for s in range(100) if sampling.ss_coin(s, 3, B)[2] >= np.float32(p))
    bad = caps[:, :-1].clone()
    bad[2, 3] = V
    capi.check_async_error()
    with pytest.raises(IndexError):
        mod.scheduled_inputs(m, feats.to(DEV), bad.to(DEV), p, seed=seed)
        torch.cuda.synchronize()
        capi.check_async_error()
    mod.scheduled_inputs(m, feats.to(DEV), caps[:, :-1].to(DEV), p, seed=seed)
    torch.cuda.synchronize()
    capi.check_async_error()


# ------------------------------------------------------------------ 8. train.py end to end
@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_scheduled_sampling_epochs_end_to_end(tmp_path, capsys, rnn_type):
    """three tiny epochs of train.py with the ramp 0, 0.25, 0.5 on the toy split of the entry-point tests: finite losses, the
    printed probability follows the ramp, the checkpoint loads and decodes"""
    import train
    import test_train_eval_parity as toy
    toy.make_toy(str(tmp_path))
    ck = tmp_path / "ck"
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(toy.L), "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F),
                       "--batch-size", str(toy.BS), "--epochs", "3", "--lr", "1e-3", "--save-path", str(ck), "--no-shuffle",
                       "--seed", "7", "--rnn-type", rnn_type, "--scheduled-sampling-start", "0", "--scheduled-sampling-increase-every", "1",
                       "--scheduled-sampling-increase-prob", "0.25", "--scheduled-sampling-max-prob", "0.5"])
    got = train.run(opt)
    assert got["ss_prob"] == [0.0, 0.25, 0.5]
    assert len(got["train_loss"]) == 3 and np.isfinite(got["train_loss"]).all() and np.isfinite(got["valid_loss"]).all()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    assert [float(ln.rsplit("ss_prob: ", 1)[1]) for ln in lines] == [0.0, 0.25, 0.5]
    m = torch.load(ck / (got["start_time"] + "final.pth"), weights_only=False).to(DEV).eval()
    import dataloader
    ds = dataloader.VideoDataset(str(tmp_path / "captions.json"), str(tmp_path / "feats"), max_len=toy.L, mode="test")
    feats = torch.stack([ds[i][0] for i in range(len(ds))]).to(DEV)
    ids = m(feats, mode="test")
    assert tuple(ids.shape) == (len(ds), toy.L - 1) and int(ids.max()) < 30
    assert torch.isfinite(torch.cat([q.reshape(-1) for q in m.parameters()])).all()
