"""GPU tests of the truncated draw (csrc/truncate.hip: top-k / nucleus ahead of the Gumbel-max draw) from the row kernel up to
S2VT.sample_truncated (n_samples = 1: mode='sample' with truncation), the GRU / stacked / Att_Baseline step loops, train.py and eval.py.

The reference of every check is float64 on the CPU: sampling.truncation_mask (the definition restated in numpy), the restated noise,
and - for whole decodes - a teacher-forced float64 replay ALONG THE DEVICE'S OWN IDS.  Where fp32 cannot decide an element (a
nucleus cut-off within the rounding of the sums, a score within the logits' rounding of the k-th largest) the reference brackets:
the device's kept set must lie between S_lo and S_hi (test_truncated_host.bracket, where the bracket's width is derived)."""
import json
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
import model_refs as refs  # noqa: E402
import test_sampling_host as hs  # noqa: E402
import test_truncated_host as ht  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _draw(logits, **kw):
    ids, kept = ops.truncated_draw(logits, return_kept=True, **kw)
    return ids.cpu().numpy(), kept.cpu().numpy()


# ------------------------------------------------------------------ 1. exact top-k on tie-laden exact inputs
# every RegRow width and both sides of its boundary (16 / 32 / 48 / 64 elements per thread), LdsRow, V no multiple of 4 or 256
@pytest.mark.parametrize("V", [23, 301, 4096, 4097, 8193, 12289, 16385])
def test_top_k_is_exact_on_ties(lib, V):
    """logits = randint(-40, 40) / 8 and temperature 1 or 0.5: the scores are exact in fp32 and full of equal values, so `kept` is
    #{s >= k-th largest} exactly and the draw is the float64 arg-max of s + g over that set up to the noise's rounding"""
    seed, step, R = 9000 + V, 2, 70
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-40, 40, (R, V), generator=g).float() / 8
    xd = x.to(DEV)
    noise = sampling.gumbel_noise(seed, step, R, V)
    worst = 0.0
    for t in (1.0, 0.5):
        s = x.double().numpy() / t
        desc = -np.sort(-s, axis=1)
        for k in sorted({1, 2, 5, 20, 255, 256, 257, V - 1, V} & set(range(1, V + 1))):
            want = (s >= desc[:, k - 1:k]).sum(1)
            mask = sampling.truncation_mask(s, k, 1.0)
            assert np.array_equal(mask.sum(1), want)
            for rows in (1, 5, 70):
                ids, kept = _draw(xd[:rows], temperature=t, top_k=k, seed=seed, step=step)
                assert np.array_equal(kept, want[:rows]), (t, k, rows)
                worst = max(worst, ht.check_draws(s[:rows] + noise[:rows], ids, mask[:rows], mask[:rows], hs.NOISE_TOL))
    print("V=%d: kept exact; largest float64 gap of a draw %.3g (tol %.3g)" % (V, worst, hs.NOISE_TOL))
    capi.check_async_error()


# ------------------------------------------------------------------ 2. k = 1
@pytest.mark.parametrize("V", [23, 4097, 16385])
def test_top_1_is_the_argmax(lib, V):
    """equal maxima all stay under the tie rule of the definition (kept = their number) and the noise decides among them; a row with
    ONE maximum draws it for any seed and temperature - the arg-max of the row"""
    g = torch.Generator().manual_seed(77 + V)
    x = torch.randint(-40, 40, (5, V), generator=g).float() / 8
    want = x.double().numpy().argmax(1)                                  # (numpy: the first of equal values)
    for seed in (0, 5, (1 << 50) + 3):
        for t in (1.0, 0.5, 3.0):
            ids, kept, packed = ops.truncated_draw(x.to(DEV), temperature=t, top_k=1, seed=seed, step=seed % 7, return_kept=True,
                                                   return_packed=True)
            sel = sampling.truncation_mask(x.double().numpy() / t, 1, 1.0)
            score = x.double().numpy() / t + sampling.gumbel_noise(seed, seed % 7, 5, V)
            assert np.array_equal(kept.cpu().numpy(), sel.sum(1))
            ht.check_draws(score, ids.cpu().numpy(), sel, sel, hs.NOISE_TOL)
    # one maximum per row (a bump on the first of the equal maxima): the arg-max, whatever the seed and the temperature
    y = x.clone()
    y[np.arange(5), want] += 0.125
    for seed in (0, 5, (1 << 50) + 3):
        for t in (1.0, 0.5, 3.0):
            ids, kept = _draw(y.to(DEV), temperature=t, top_k=1, seed=seed, step=1)
            assert np.array_equal(ids, want) and (kept == 1).all()
    capi.check_async_error()


# ------------------------------------------------------------------ 3. nucleus
@pytest.mark.parametrize("V", ht.NUCLEUS_V)
def test_nucleus_lands_inside_the_float64_bracket(lib, V):
    x = ht.nucleus_logits(V)
    t, seed, step = ht.NUCLEUS_T, 4242 + V, 3
    s = x.double().numpy() / t
    cases = []
    for p in ht.NUCLEUS_P:                                               # the CPU precondition first: before the device is touched
        lo, hi = ht.bracket(s, 0, p, ht.DELTA)
        assert int((lo.sum(1) != hi.sum(1)).sum()) <= 2, p
        cases.append((p, lo, hi))
    score = s + sampling.gumbel_noise(seed, step, 64, V)
    xd = x.to(DEV)
    for p, lo, hi in cases:
        ids, kept = _draw(xd, temperature=t, top_p=p, seed=seed, step=step)
        n_lo, n_hi = lo.sum(1), hi.sum(1)
        print("V=%d p=%.1f: kept %d..%d (reference %d..%d)" % (V, p, kept.min(), kept.max(), n_lo.min(), n_hi.max()))
        assert ((n_lo <= kept) & (kept <= n_hi)).all(), (p, np.nonzero((kept < n_lo) | (kept > n_hi))[0])
        ht.check_draws(score, ids, lo, hi, hs.NOISE_TOL)
    capi.check_async_error()


# ------------------------------------------------------------------ 4. both together
def test_top_k_then_top_p_renormalises(lib):
    V, t, k, p, seed, step = 301, 0.125, 5, 0.9, 31, 1
    x = ht.step_logits(64, 32, V, 555)
    s = x.double().numpy() / t
    lo, hi = ht.bracket(s, k, p, ht.DELTA)
    only_p = sampling.truncation_mask(s, 0, p)
    only_k = sampling.truncation_mask(s, k, 1.0)
    both = sampling.truncation_mask(s, k, p)
    differs = (both != only_p).any(1) & (both != only_k).any(1)
    assert differs.any() and int((lo.sum(1) != hi.sum(1)).sum()) <= 2    # (CPU: the case shows the renormalisation)
    ids, kept = _draw(x.to(DEV), temperature=t, top_k=k, top_p=p, seed=seed, step=step)
    assert ((lo.sum(1) <= kept) & (kept <= hi.sum(1))).all()
    assert (kept[differs] != only_p.sum(1)[differs]).any() or (kept[differs] != only_k.sum(1)[differs]).any()
    ht.check_draws(s + sampling.gumbel_noise(seed, step, 64, V), ids, lo, hi, hs.NOISE_TOL)
    capi.check_async_error()


# ------------------------------------------------------------------ 5. no truncation: today's draw
@pytest.mark.parametrize("B", [4, 64])
@pytest.mark.parametrize("H", [32, 512])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_nothing_truncated_is_the_heads_draw(lib, B, H, temperature):
    from test_gpu_sampling import _step_inputs
    V, seed, step = 301, 4242 + B + H, 5
    h, w, b = _step_inputs(B, H, V, seed)
    hd, wd, bd = h.to(DEV), w.to(DEV), b.to(DEV)
    ids, kept = _draw(ops.gemm(hd, wd, bd), temperature=temperature, top_k=0, top_p=1.0, seed=seed, step=step)
    assert (kept == V).all()
    score = (h.double() @ w.double().t() + b.double()).numpy() / temperature + sampling.gumbel_noise(seed, step, B, V)
    gap = score.max(1) - score[np.arange(B), ids]
    print("B=%d H=%d: max float64 gap of the chosen index %.3g (eps %.3g)" % (B, H, gap.max(), hs.eps_for(temperature)))
    assert (gap <= hs.eps_for(temperature)).all()                        # test_step_kernel_draw_is_exact's check
    head = ops.decode_step_sample(hd, wd, bd, temperature=temperature, seed=seed, step=step).cpu().numpy()
    top = np.sort(score, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 2 * hs.eps_for(temperature)
    assert clear.mean() >= 0.9 and np.array_equal(ids[clear], head[clear])
    capi.check_async_error()


def test_top20_entry_point_is_the_fan_out(lib):
    """the beam searches' fan-out kernel through its own entry point (what tools/bench_sample_trunc.py times the draw against)"""
    x = ht.step_logits(7, 32, 301, 99)
    ix, lp = ops.top20_logprob(x.to(DEV))
    want_lp, want_ix = torch.log_softmax(x.double(), 1).topk(20, dim=1)
    order = want_ix.argsort(1)                                           # ascending token order
    assert torch.equal(ix.cpu().long(), want_ix.gather(1, order))
    assert (lp.cpu().double() - want_lp.gather(1, order)).abs().max() <= 2e-6 * 8
    capi.check_async_error()


# ------------------------------------------------------------------ 6. distribution
@pytest.mark.parametrize("top_k,top_p", ht.DIST_TRUNC)
def test_truncated_distribution(lib, top_k, top_p):
    V = hs.DIST_V
    x32 = torch.tensor(hs.DIST_LOGITS, dtype=torch.float32)
    s = x32.double().numpy()[None, :].repeat(64, 0)
    mask = sampling.truncation_mask(s, top_k, top_p)
    assert int(mask[0].sum()) == ht.DIST_KEPT
    # the restatement's draws and which of them are comparable: top-2 margin inside the kept set above twice the noise's rounding
    want, comparable = [], []
    for sd in hs.SEEDS:
        sc = np.where(mask, s + sampling.gumbel_noise(sd, 0, 64, V), -np.inf)
        want.append(sc.argmax(1))
        top = np.sort(sc, axis=1)
        comparable.append(top[:, -1] - top[:, -2] > 2 * hs.NOISE_TOL)
    want, comparable = np.array(want), np.array(comparable)
    assert int((~comparable).sum()) <= 2                                 # (CPU, before the device is touched)
    xd = x32.to(DEV)[None, :].repeat(64, 1).contiguous()
    got = np.array([_draw(xd, top_k=top_k, top_p=top_p, seed=sd, step=0)[0] for sd in hs.SEEDS])
    assert mask[0][got].all()                                            # no draw outside the kept set
    assert np.array_equal(got[comparable], want[comparable])
    assert np.array_equal(np.bincount(got[comparable], minlength=V), np.bincount(want[comparable], minlength=V))
    p = np.where(mask[0], np.exp(s[0] - s[0].max()), 0.0)
    p /= p.sum()
    counts = np.bincount(got.reshape(-1), minlength=V).astype(np.float64)
    stat = hs.chi_square(counts[mask[0]], p[mask[0]])
    print("top_k=%d top_p=%.1f: chi2 = %.2f over %d kept (bound %.2f)" % (top_k, top_p, stat, ht.DIST_KEPT, ht.CHI2_BOUND_KEPT))
    assert stat < ht.CHI2_BOUND_KEPT
    capi.check_async_error()


# ------------------------------------------------------------------ 7. the whole decode, one-layer LSTM
DIMS = dict(L=6, F=64, E=40, V=301)
TRUNCS = (dict(top_k=5), dict(top_p=0.7), dict(top_k=5, top_p=0.7))


def _one(m, x, **kw):
    """mode='sample' with truncation: S2VT.sample_truncated's single sample per clip, [B, L-1]"""
    return m.sample_truncated(x, 1, **kw)[:, 0]


def _model(d, sd, **kw):
    import S2VTModel
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _check_steps(score, noise, ids, temperature, top_k=0, top_p=1.0):
    """score, noise float64 [rows, steps, V] along the device's ids: at every (row, step) the id is in S_hi and within eps of the
    best of S_lo.  The logits of the device and of the replay differ by up to MARGIN: a score by MARGIN / t against the k-th largest,
    the masses by the factor exp(+-MARGIN / t) each way - delta_model = DELTA + 2 MARGIN / t."""
    worst = 0.0
    for j in range(score.shape[1]):
        lo, hi = ht.bracket(score[:, j] - noise[:, j], top_k, top_p, ht.DELTA + 2 * hs.MARGIN / temperature, hs.MARGIN / temperature)
        worst = max(worst, ht.check_draws(score[:, j], ids[:, j], lo, hi, hs.eps_for(temperature)))
    return worst


def _replay(sd, feats, ids, seed, temperature, rows=None):
    B, L, _ = feats.shape
    V = sd["out_linear.weight"].shape[0]
    rows = np.arange(B) if rows is None else rows
    score = hs.scores_along_ids_fp64(sd, feats, ids.cpu(), seed, temperature, rows=rows)
    noise = np.stack([sampling.gumbel_noise(seed, t, rows, V) for t in range(L - 1)], 1)
    return score, noise


@pytest.mark.parametrize("B", [4, 40, 64, 128])                          # step path without a cache, a padded plane batch, 64, 128
@pytest.mark.parametrize("H", [32, 512])
def test_whole_decode_stays_inside_the_truncation(lib, B, H):
    d = dict(DIMS, B=B, H=H)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21)
    feats, _, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=22)
    m, x = _model(d, sd), feats.to(DEV)
    t, seed = 1.0, 77
    plain = m.sample(x, 1, temperature=t, seed=seed)
    assert torch.equal(plain, m.sample_truncated(x, 1, temperature=t, seed=seed, top_k=0, top_p=1.0))
    assert torch.equal(plain, m.sample_truncated(x, 1, temperature=t, seed=seed))
    assert torch.equal(plain, m.sample_truncated(x, 1, temperature=t, seed=seed, top_k=d["V"]))
    for kw in TRUNCS:
        ids = _one(m, x, temperature=t, seed=seed, **kw)
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (B, d["L"] - 1)
        idn = ids.cpu().numpy()
        assert idn.min() >= 0 and idn.max() < d["V"]
        score, noise = _replay(sd, feats, ids, seed, t)
        worst = _check_steps(score, noise, idn, t, **kw)
        print("B=%d H=%d %s: max float64 gap %.3g (eps %.3g)" % (B, H, kw, worst, hs.eps_for(t)))
        assert torch.equal(ids, _one(m, x, temperature=t, seed=seed, **kw))
        assert not torch.equal(ids, _one(m, x, temperature=t, seed=seed + 1, **kw))
    if B in (4, 40):
        K = 3
        assert torch.equal(m.sample(x, K, temperature=t, seed=seed), m.sample_truncated(x, K, temperature=t, seed=seed, top_k=0, top_p=1.0))
        for kw in TRUNCS:
            ids = m.sample_truncated(x, K, temperature=t, seed=seed, **kw)
            assert tuple(ids.shape) == (B, K, d["L"] - 1)
            flat = ids.view(B * K, -1)
            score, noise = _replay(sd, feats.repeat_interleave(K, 0), flat, seed, t)
            _check_steps(score, noise, flat.cpu().numpy(), t, **kw)
            assert torch.equal(ids, m.sample_truncated(x, K, temperature=t, seed=seed, **kw))
    # top_k = 1: the greedy caption, up to a row's first step whose float64 greedy margin is below MARGIN
    from oracle import s2vt_oracle as orc
    gi, gm = orc.greedy_decode(sd, feats, dtype=torch.float64, return_margins=True)
    decided = gm.numpy() >= hs.MARGIN
    first = np.where(decided.all(1), decided.shape[1], (~decided).argmax(1))
    one = _one(m, x, temperature=t, seed=seed, top_k=1).cpu()
    greedy = m(x, mode="test").cpu()
    assert first.sum() >= 0.9 * decided.size
    for r in range(B):
        assert torch.equal(one[r, :first[r]], gi[r, :first[r]]) and torch.equal(one[r, :first[r]], greedy[r, :first[r]]), r
    capi.check_async_error()


# ------------------------------------------------------------------ 8. GRU, stacked LSTM, Att_Baseline
def _along(logits64, seed, temperature, rows, V):
    noise = np.stack([sampling.gumbel_noise(seed, j, rows, V) for j in range(logits64.shape[1])], 1)
    return logits64 / temperature + noise, noise


def test_gru_truncated_sample(lib):
    import make_gru_golden as gru_gen
    d, sd, feats, _, _ = gru_gen.setup("gru_tiny")
    m = _model(d, sd, rnn_type="gru")
    seed, t, B, V = 314, 1.0, feats.shape[0], d["V"]
    ids = _one(m, feats.to(DEV), seed=seed, top_k=5).cpu()
    assert torch.equal(ids, _one(m, feats.to(DEV), seed=seed, top_k=5).cpu())
    assert torch.equal(m(feats.to(DEV), mode="sample", seed=seed), _one(m, feats.to(DEV), seed=seed, top_k=0, top_p=1.0))
    caps_in = torch.cat([torch.full((B, 1), 3, dtype=torch.long), ids[:, :-1]], 1)
    with torch.no_grad():
        logits = refs.gru_model64({k: refs.d64(v) for k, v in sd.items()}, feats, caps_in).numpy()
    score, noise = _along(logits, seed, t, B, V)
    _check_steps(score, noise, ids.numpy(), t, top_k=5)
    k3 = m.sample_truncated(feats.to(DEV), 3, seed=seed, top_k=5)
    assert torch.equal(k3.view(B * 3, -1), _one(m, feats.to(DEV).repeat_interleave(3, 0), seed=seed, top_k=5))
    capi.check_async_error()


def test_stacked_truncated_sample(lib):
    import make_stack_golden as stack_gen
    d, sd, feats, _, _ = stack_gen.setup("stack_tiny")
    N, B, L, H, E, V = d["N"], feats.shape[0], d["L"], d["H"], d["E"], d["V"]
    m = _model(d, sd, num_layers=N)
    seed, t = 2718, 1.0
    ids = _one(m, feats.to(DEV), seed=seed, top_k=5).cpu()
    assert torch.equal(ids, _one(m, feats.to(DEV), seed=seed, top_k=5).cpu())
    # float64 replay along the device's ids (the arithmetic of make_stack_golden.replay_fp64, keeping the logits)
    p = {k: v.double() for k, v in sd.items()}
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    z = torch.zeros(B, H, dtype=torch.float64)
    sv, sw = [(z, z)] * N, [(z, z)] * N
    for j in range(L):
        v, sv = stack_gen._lstm_stack_step(x[:, j], sv, p, "vid_rnn", N)
        _, sw = stack_gen._lstm_stack_step(torch.cat([torch.zeros(B, E, dtype=torch.float64), v], 1), sw, p, "word_rnn", N)
    tok = torch.full((B,), 3, dtype=torch.long)
    logits = []
    for i in range(L - 1):
        if i:
            tok = ids[:, i - 1]
        v, sv = stack_gen._lstm_stack_step(z, sv, p, "vid_rnn", N)
        o, sw = stack_gen._lstm_stack_step(torch.cat([p["embedding.weight"][tok], v], 1), sw, p, "word_rnn", N)
        logits.append((o @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy())
    score, noise = _along(np.stack(logits, 1), seed, t, B, V)
    _check_steps(score, noise, ids.numpy(), t, top_k=5)
    capi.check_async_error()


def test_att_baseline_truncated_sample(lib):
    import attention_baseline
    d = dict(B=5, L=8, F=64, H=32, E=24, V=50)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=6)
    torch.manual_seed(0)
    att = attention_baseline.Att_Baseline(d["V"], d["F"], length=d["L"], dim_hid=d["H"], dim_embed=d["E"])
    with torch.no_grad():
        att.out_linear.weight.mul_(4.0)                                  # logits wide enough for the draws to depend on them
    P = {k: refs.d64(v) for k, v in att.state_dict().items()}
    att = att.to(DEV).eval()
    seed, t, B, L, V = 1618, 1.0, d["B"], d["L"], d["V"]
    ids = att(feats.to(DEV), mode="sample", seed=seed, top_k=5).cpu()
    assert tuple(ids.shape) == (B, L) and torch.equal(ids, att(feats.to(DEV), mode="sample", seed=seed, top_k=5).cpu())
    assert torch.equal(att(feats.to(DEV), mode="sample", seed=seed), att(feats.to(DEV), mode="sample", seed=seed, top_k=0, top_p=1.0))
    # the composite teacher-forces L - 1 steps: the first L - 1 of the L draws are checked along the ids
    caps_in = torch.cat([torch.full((B, 1), int(att.sos_ix), dtype=torch.long), ids[:, :L - 2]], 1)
    with torch.no_grad():
        logits = refs.att_model64(P, feats, caps_in).numpy()
    score, noise = _along(logits, seed, t, B, V)
    _check_steps(score, noise, ids[:, :L - 1].numpy(), t, top_k=5)
    capi.check_async_error()


# ------------------------------------------------------------------ 9. train.py and eval.py
def test_self_critical_and_eval_with_truncation(tmp_path):
    sys.path.insert(0, ROOT)
    import eval as s2vt_eval
    import train
    import test_train_eval_parity as toy
    toy.make_toy(str(tmp_path))
    ck = tmp_path / "ck"
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(toy.L), "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F),
                       "--batch-size", "6", "--epochs", "1", "--lr", "1e-3", "--save-path", str(ck), "--no-shuffle", "--seed", "7",
                       "--self-critical", "--sc-samples", "2", "--sc-top-k", "5"])           # 12 training clips: two steps
    got = train.run(opt)
    assert got["sc_split_ms"]["steps"] == 2 and len(got["train_loss"]) == 1 and np.isfinite(got["train_loss"][0])
    assert len(got["reward_sample"]) == 2 and all(np.isfinite(got["reward_sample"]))
    capi.check_async_error()
    out = tmp_path / "pred.json"
    s2vt_eval.main(["--model-path", str(ck / (got["start_time"] + "final.pth")), "--caption-file", str(tmp_path / "captions.json"),
                    "--feats-path", str(tmp_path / "feats"), "--batch-size", "3", "--sample", "2", "--top-k", "5", "--out", str(out)])
    with open(str(out) + ".samples.json", encoding="utf-8") as f:
        samples = json.load(f)
    with open(out, encoding="utf-8") as f:
        preds = json.load(f)
    assert set(samples) == set(preds) and len(samples) == 4
    assert all(isinstance(c, list) and len(c) == 2 and all(isinstance(w, str) and "<eos>" not in w for w in c) for c in samples.values())
    capi.check_async_error()
