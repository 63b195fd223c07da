"""Host-side checks of the sampled decode (mode='sample') and of the reward-weighted loss's surface: the numpy restatement of the
noise (sampling.py) against known answers and a second implementation, the C ABI's argument checks (no device needed: every
rejection happens before the first device call), and the fixtures the GPU tests of test_gpu_sampling.py rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, sampling, synth
from oracle import s2vt_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- shared with test_gpu_sampling.py
SEEDS = tuple(range(101, 133))                   # 32 call seeds x 64 rows = 2048 draws of the distribution checks
DIST_V = 23
DIST_LOGITS = np.linspace(-2.0, 2.0, DIST_V)     # fixed logit vector of the distribution checks (p from 0.3 % to 17 %)
# chi2.ppf(1 - 1e-6, 22): the bound of the distribution checks.  scipy.stats.chi2.ppf(1 - 1e-6, 22) = 68.85576868064251; the
# hard-coded value is used where scipy is absent (the survival function of chi2 with 22 degrees of freedom at 68.8558 is 1e-6)
try:
    from scipy.stats import chi2 as _chi2
    CHI2_BOUND = float(_chi2.ppf(1 - 1e-6, DIST_V - 1))
except ImportError:                              # pragma: no cover
    CHI2_BOUND = 68.85576868064251
# Device noise against the float64 restatement: 2 ulp of fp32 at the top of the range (g <= 16.64 lies in [16, 32): ulp = 2^-19 =
# 1.9e-6) - one for the rounding of the accurate logf, one for what the relative error of -log(u) contributes
NOISE_TOL = 4e-6
MARGIN = 1e-5                                    # tools/make_gru_golden.MARGIN: what the greedy tests grant the kernels' logits
LAYOUT = dict(B=10, L=8, F=64, H=32, E=24, V=50, seed=11, sample_seed=2024)     # fixture of the layout-independence test


def eps_for(temperature):
    return MARGIN / temperature + NOISE_TOL


def chi_square(counts, p):
    n = counts.sum()
    return float((((counts - n * p) ** 2) / (n * p)).sum())


def dist_counts(logits, seeds, rows, step=0, temperature=1.0):
    """(counts [V] of arg-max(logit / t + g) over seeds x rows, top-2 score margins [len(seeds), rows]) of the numpy restatement"""
    V = logits.shape[0]
    counts = np.zeros(V)
    margins = []
    for s in seeds:
        sc = logits[None, :] / temperature + sampling.gumbel_noise(s, step, rows, V)
        counts += np.bincount(sc.argmax(1), minlength=V)
        top = np.sort(sc, axis=1)
        margins.append(top[:, -1] - top[:, -2])
    return counts, np.array(margins)


def replay_sample_fp64(sd, feats, seed, temperature=1.0, rows=None, sos_ix=3):
    """mode='sample' in float64 on the CPU with the restated noise: (ids [B, L-1], top-2 score margins [B, L-1]).  Step t's logits
    are the teacher-forced logits of the prefix drawn so far (oracle forward_train in float64)."""
    B, L, _ = feats.shape
    V = sd["out_linear.weight"].shape[0]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    prefix = torch.full((B, L - 1), 0, dtype=torch.long)
    prefix[:, 0] = sos_ix
    ids = torch.zeros(B, L - 1, dtype=torch.long)
    marg = np.zeros((B, L - 1))
    for t in range(L - 1):
        with torch.no_grad():
            logits = orc.forward_train(sd, feats, prefix, dtype=torch.float64)[:, t].numpy()
        sc = logits / temperature + sampling.gumbel_noise(seed, t, rows, V)
        ids[:, t] = torch.from_numpy(sc.argmax(1))
        top = np.sort(sc, axis=1)
        marg[:, t] = top[:, -1] - top[:, -2]
        if t + 1 < L - 1:
            prefix[:, t + 1] = ids[:, t]
    return ids, marg


def scores_along_ids_fp64(sd, feats, ids, seed, temperature=1.0, rows=None, sos_ix=3):
    """float64 scores [B, L-1, V] of a sampled decode ALONG THE GIVEN ids (teacher-forced replay + restated noise)"""
    B, L, _ = feats.shape
    V = sd["out_linear.weight"].shape[0]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    prefix = torch.cat([torch.full((B, 1), sos_ix, dtype=torch.long), ids[:, :-1].cpu()], 1)
    with torch.no_grad():
        logits = orc.forward_train(sd, feats, prefix, dtype=torch.float64).numpy()
    g = np.stack([sampling.gumbel_noise(seed, t, rows, V) for t in range(L - 1)], 1)
    return logits / temperature + g


def layout_fixture():
    d = LAYOUT
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=d["seed"])
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=d["seed"])
    return d, sd, feats


# ---- Philox known answers
def _philox_python_ints(counter, key):
    """a second, deliberately different implementation: Python integers, the round written out from the Random123 definition"""
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) % 2 ** 32, (k[1] + 0xBB67AE85) % 2 ** 32]
        hi0, lo0 = divmod(0xD2511F53 * c[0], 2 ** 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c[2], 2 ** 32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
    return c


# Random123 kat_vectors, philox4x32-10: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,expected", KAT)
def test_philox_known_answers(counter, key, expected):
    got = sampling.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert [int(x) for x in got] == list(expected)
    assert _philox_python_ints(counter, key) == list(expected)       # the typed vectors against the second implementation


def test_philox_matches_second_implementation_on_random_inputs():
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(64, 2), dtype=np.uint64).astype(np.uint32)
    got = sampling.philox4x32_10(ctr, key)
    for i in range(64):
        assert [int(x) for x in got[i]] == _philox_python_ints(ctr[i], key[i])


def test_gumbel_noise_mapping_and_range():
    g = sampling.gumbel_noise(5, 3, [0, 7], 10)
    # element (row 7, v = 6): counter (1, 7, 3, tag), word 2
    x = _philox_python_ints((1, 7, 3, sampling.STREAM_TAG), (5, 0))[2]
    u = ((x >> 9) + 0.5) * 2.0 ** -23
    assert g[1, 6] == pytest.approx(-np.log(-np.log(u)), rel=1e-12)
    # rows are independent of the batch they sit in; V does not shift elements
    assert np.array_equal(sampling.gumbel_noise(5, 3, 8, 10)[7], g[1])
    assert np.array_equal(sampling.gumbel_noise(5, 3, [7], 23)[0, :10], g[1])
    # a 64-bit seed uses both key words
    assert not np.array_equal(sampling.gumbel_noise(5 + (1 << 32), 3, [7], 10)[0], g[1])
    lo, hi = sampling.gumbel_from_bits(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert -2.82 < lo < -2.81 and 16.63 < hi < 16.64
    u = sampling.uniform_from_bits(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert 0.0 < u[0] and u[1] < 1.0 and np.all(u.astype(np.float32).astype(np.float64) == u)      # exact in fp32


def test_restatement_distribution_chi_square():
    """arg-max(logit + gumbel_noise) over the GPU test's seeds and rows follows softmax(logit): deterministic"""
    p = np.exp(DIST_LOGITS - DIST_LOGITS.max())
    p /= p.sum()
    counts, _ = dist_counts(DIST_LOGITS, SEEDS, 64)
    assert counts.sum() == 64 * len(SEEDS)
    stat = chi_square(counts, p)
    print("chi2 = %.2f (bound %.2f), N = %d" % (stat, CHI2_BOUND, counts.sum()))
    assert stat < CHI2_BOUND
    # and it is not the arg-max: a sharper temperature moves the counts towards the mode
    cold, _ = dist_counts(DIST_LOGITS, SEEDS[:4], 64, temperature=0.01)
    assert cold[DIST_V - 1] == 4 * 64


def test_layout_fixture_is_margin_robust_in_float64():
    """the layout-independence test asserts equal ids on rows whose float64 margin is >= eps at every step and that these are at
    least 90 % of the rows: the fixture meets that in the float64 replay alone"""
    d, sd, feats = layout_fixture()
    ids, marg = replay_sample_fp64(sd, feats, d["sample_seed"])
    robust = (marg >= eps_for(1.0)).all(1)
    assert robust.mean() >= 0.9
    assert ids.min() >= 0 and ids.max() < d["V"]
    assert len(np.unique(ids.numpy())) > 5                           # a sample, not one token


# ---- surface
NEW_SYMBOLS = ("s2vt_decode_step_sample", "s2vt_decode_step_sample_x3_workspace_bytes", "s2vt_decode_step_sample_x3",
               "s2vt_sample_decode", "s2vt_sample_decode_cached", "s2vt_weighted_ce_forward", "s2vt_weighted_ce_backward")


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.s2vt_abi_version() == 9 == capi.ABI_VERSION
    assert "0x47554D42" in header and sampling.STREAM_TAG == 0x47554D42      # the mapping is stated in the header
    philox = open(os.path.join(ROOT, "s2vt-video-caption_amd", "csrc", "philox.h")).read()
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert const in philox


def _last_error(lib):
    return lib.s2vt_last_error().decode()


@pytest.mark.parametrize("temperature", [0.0, -1.0, float("nan"), float("inf"), 1e-40])      # (1e-40: subnormal, 1 / t = inf)
def test_bad_temperature_is_rejected_on_the_host(lib, temperature):
    """non-null (never dereferenced) pointers: the temperature check comes before any device call"""
    fake = ctypes.c_void_p(4096)
    d = capi.Dims(2, 4, 8, 8, 8, 16)
    ps = capi.Params()
    for f in capi.PARAM_FIELDS:
        setattr(ps, f, 4096)
    calls = {
        "s2vt_decode_step_sample": lambda: lib.s2vt_decode_step_sample(2, 8, 16, fake, fake, fake, temperature, 1, 0, 0, fake, None),
        "s2vt_decode_step_sample_x3": lambda: lib.s2vt_decode_step_sample_x3(2, 8, 16, fake, fake, fake, temperature, 1, 0, 0, fake, fake,
                                                                            1 << 30, None),
        "s2vt_sample_decode": lambda: lib.s2vt_sample_decode(ctypes.byref(d), ctypes.byref(ps), fake, 3, temperature, 1, fake, fake,
                                                             1 << 30, None),
        "s2vt_sample_decode_cached": lambda: lib.s2vt_sample_decode_cached(ctypes.byref(d), ctypes.byref(ps), fake, 3, temperature, 1,
                                                                           fake, fake, 1 << 30, fake, 1 << 30, 0, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = _last_error(lib)
        assert msg.startswith(name + ":") and "temperature" in msg, msg


def test_null_pointers_are_rejected_on_the_host(lib):
    fake = ctypes.c_void_p(4096)
    d = capi.Dims(2, 4, 8, 8, 8, 16)
    ps = capi.Params()
    assert lib.s2vt_decode_step_sample(2, 8, 16, None, fake, fake, 1.0, 1, 0, 0, fake, None) == -1
    assert _last_error(lib).startswith("s2vt_decode_step_sample:")
    assert lib.s2vt_decode_step_sample(2, 8, 16, fake, fake, fake, 1.0, 1, 0, 0, None, None) == -1
    assert lib.s2vt_decode_step_sample(2, 8, 16, fake, fake, fake, 1.0, 1, -1, 0, fake, None) == -1
    assert lib.s2vt_decode_step_sample_x3(2, 8, 16, fake, fake, fake, 1.0, 1, 0, 0, fake, None, 0, None) == -1
    assert _last_error(lib).startswith("s2vt_decode_step_sample_x3:")
    assert lib.s2vt_decode_step_sample_x3(2, 8, 16, fake, fake, fake, 1.0, 1, 0, 0, fake, fake, 16, None) == -1
    assert "workspace" in _last_error(lib)
    assert lib.s2vt_sample_decode(ctypes.byref(d), ctypes.byref(ps), fake, 3, 1.0, 1, None, fake, 1 << 30, None) == -1
    assert _last_error(lib).startswith("s2vt_sample_decode:")
    assert lib.s2vt_sample_decode(None, ctypes.byref(ps), fake, 3, 1.0, 1, fake, fake, 1 << 30, None) == -1
    assert lib.s2vt_sample_decode_cached(ctypes.byref(d), ctypes.byref(ps), fake, 3, 1.0, 1, fake, fake, 1 << 30, None, 0, 0, None) == -1
    assert _last_error(lib).startswith("s2vt_sample_decode_cached:")
    assert lib.s2vt_weighted_ce_forward(2, 3, 16, None, fake, 4, fake, 4, fake, fake, fake, None) == -1
    assert _last_error(lib).startswith("s2vt_weighted_ce_forward:")
    assert lib.s2vt_weighted_ce_forward(2, 3, 16, fake, fake, 4, fake, 3, fake, fake, fake, None) == -1      # weight_ld < L
    assert lib.s2vt_weighted_ce_backward(2, 3, 16, fake, fake, 4, fake, 4, fake, fake, fake, None, None) == -1
    assert _last_error(lib).startswith("s2vt_weighted_ce_backward:")
    assert lib.s2vt_decode_step_sample_x3_workspace_bytes(64, 32, 100) == lib.s2vt_decode_step_argmax_x3_workspace_bytes(64, 32, 100)


def test_python_surface_checks_arguments():
    import inspect
    import S2VTModel
    import attention_baseline
    import utils
    sig = inspect.signature(S2VTModel.S2VT.forward)
    assert list(sig.parameters)[-2:] == ["temperature", "seed"]
    assert sig.parameters["temperature"].default == 1.0 and sig.parameters["seed"].default is None
    sig = inspect.signature(attention_baseline.Att_Baseline.forward)
    assert sig.parameters["temperature"].default == 1.0 and sig.parameters["seed"].default is None
    assert hasattr(utils, "RewardCriterion")
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sampling.check_sample_args(bad, 1)
    with pytest.raises(ValueError):
        sampling.check_sample_args(1.0, -1)
    torch.manual_seed(77)
    a = sampling.check_sample_args(1.0, None)[1]
    b = sampling.check_sample_args(1.0, None)[1]
    torch.manual_seed(77)
    assert sampling.check_sample_args(1.0, None)[1] == a and a != b and 0 <= a < 2 ** 63
    assert sampling.check_sample_args(0.5, 9) == (0.5, 9)


def test_train_parses_self_critical():
    import train
    opt = train.parse(["--self-critical"])
    assert opt.self_critical is True and opt.sc_temperature == 1.0
    assert train.parse(["--self-critical", "--sc-temperature", "0.7"]).sc_temperature == 0.7
    assert train.parse([]).self_critical is False


def test_advantage_weights_and_rewarder():
    from s2vt_video_caption_amd.self_critical import CiderRewarder, advantage_weights
    w = advantage_weights(torch.tensor([[5, 6, 4, 9, 9], [5, 6, 7, 8, 9]]), [0.5, -1.0], eos_ix=4)
    assert w.tolist() == [[0.0, 0.5, 0.5, 0.5, 0.0, 0.0], [0.0, -1.0, -1.0, -1.0, -1.0, -1.0]]
    caps = {"a": [[3, 5, 6, 7, 4], [3, 5, 6, 8, 4]], "b": [[3, 9, 10, 4]]}
    r = CiderRewarder(caps, ["a", "b"], sos_ix=3, eos_ix=4)
    exact, partial, none = r.rewards(["a", "a", "a"], [[5, 6, 7, 4, 9], [5, 6, 4, 0, 0], [11, 12, 4, 0, 0]])
    assert exact > partial > none == 0.0


def test_rewarder_equals_caption_metrics_cider_on_the_training_split():
    """CiderRewarder.score is caption_metrics.cider's per-id value when the corpus is the split the rewarder was built from"""
    import caption_metrics
    from s2vt_video_caption_amd.self_critical import CiderRewarder
    rng = np.random.RandomState(3)
    vids = ["v%02d" % i for i in range(9)]
    caps = {v: [[3] + [int(x) for x in rng.randint(5, 14, size=rng.randint(2, 7))] + [4] for _ in range(rng.randint(1, 4))] for v in vids}
    cand = {v: [int(x) for x in rng.randint(5, 14, size=rng.randint(1, 7))] + [4, 0, 0] for v in vids}
    cand[vids[0]] = caps[vids[0]][0][1:]                                   # one exact match
    text = lambda ids: " ".join(str(t) for t in ids)                       # noqa: E731
    gts = {v: [text(c[1:-1]) for c in caps[v]] for v in vids}
    res = {v: [text(cand[v][:cand[v].index(4)])] for v in vids}
    _, per_id = caption_metrics.cider(gts, res)
    r = CiderRewarder(caps, vids, sos_ix=3, eos_ix=4)
    got = r.rewards(sorted(vids), [cand[v] for v in sorted(vids)])
    assert np.allclose(got, per_id, rtol=1e-12, atol=0) and got.max() > 1.0
