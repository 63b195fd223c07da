"""GPU tests of the device-resident self-critical reward: s2vt_cider_rewards / s2vt_sc_weights through self_critical.DeviceCiderRewarder,
ops and train.py --sc-reward device.

References: the reference scorer's own recorded CIDEr values (tests/golden/metrics.json) and the host scorer CiderRewarder, at the
bounds tests/test_caption_metrics.py applies to the host code on that fixture (rtol 1e-10, atol 1e-12).  The bound is derivable:
the device only performs IEEE + * / sqrt min on float64 factors the host precomputed, the sums run over at most 4 * 79
non-negative terms (no cancellation), so the worst relative error is a few hundred ulp, about 1e-13.  Every row is compared."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder, advantage_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cider_reward_host as hc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOS, EOS = hc.SOS, hc.EOS
RTOL, ATOL = 1e-10, 1e-12
B, T = 64, 79


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    print("rows %d  max abs err %.3e  max rel err %.3e  max score %.4f" % (
        len(want), err.max(), (err / np.maximum(np.abs(want), 1e-300))[want != 0].max() if (want != 0).any() else 0.0, want.max()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ the reference scorer's recorded numbers
@pytest.mark.parametrize("name", ["corpus48", "corpus5", "single"])
def test_rewards_match_the_reference_scorers_recorded_cider(lib, name):
    with open(os.path.join(ROOT, "tests", "golden", "metrics.json")) as f:
        c = json.load(f)[name]
    vids = sorted(c["gts"])
    words = sorted({w for v in vids for s in c["gts"][v] + c["res"][v] for w in s.split()})
    ix = {w: 5 + i for i, w in enumerate(words)}
    caps = {v: [[SOS] + [ix[w] for w in s.split()] + [EOS] for s in c["gts"][v]] for v in vids}
    cand = [[ix[w] for w in c["res"][v][0].split()] + [EOS] for v in vids]
    width = max(len(r) for r in cand) + 2
    ids = torch.tensor([(r + [0] * width)[:width] for r in cand], dtype=torch.long, device=DEV)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV, vocab_size=5 + len(words))
    got = d.rewards(vids, ids)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (len(vids),)
    capi.check_async_error()
    got = got.cpu().numpy()
    assert len(got) == len(c["cider_each"])
    _close(got, c["cider_each"])
    if name == "single":
        assert got.tolist() == [0.0]
    else:
        assert got.max() > 1.0


# ------------------------------------------------------------------ random sweep against the host scorer
def _sweep_batch(seed, lo, hi):
    """(clips, caps, video id per row, id rows [B][T]): 1..20 references per clip, the edge cases of the host test, random rows and
    rows cut from the clip's own references (so that a large vocabulary also scores above 0)"""
    vids, caps, rng = hc.edge_corpus(seed, n_clips=12, lo=lo, hi=hi, max_refs=20, ref_words=(2, 13))
    rows = hc.edge_candidates(vids, caps, lo, hi, T)
    while len(rows) < B:
        v = vids[rng.randint(len(vids))]
        kind = rng.randint(4)
        if kind == 0:                                     # random words, <eos> somewhere (or nowhere), pads behind it
            n = rng.randint(1, T + 1)
            row = [int(x) for x in rng.randint(lo, hi, size=n)] + [EOS] + [0] * T
        elif kind == 1:                                   # a reference of the clip with one word replaced and one pad inserted
            ref = list(caps[v][rng.randint(len(caps[v]))][1:-1])
            ref[rng.randint(len(ref))] = int(rng.randint(lo, hi))
            ref.insert(rng.randint(len(ref) + 1), 0)
            row = ref + [EOS] + [int(x) for x in rng.randint(lo, hi, size=T)]        # what follows <eos> is not read
        elif kind == 2:                                   # two references back to back, no <eos>: a long candidate with repeats
            a, b2 = caps[v][0][1:-1], caps[v][-1][1:-1]
            row = (a + b2) * T
        else:                                             # a leading <sos>, then an exact reference
            row = caps[v][rng.randint(len(caps[v]))]
        rows.append((v, (row + [0] * T)[:T]))
    return vids, caps, [v for v, _ in rows], [r for _, r in rows]


@pytest.mark.parametrize("lo,hi", [(5, 14), (5, 12000)])
@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_rewards_match_the_host_scorer_on_random_batches(lib, seed, lo, hi):
    vids, caps, row_vids, rows = _sweep_batch(seed, lo, hi)
    assert len(rows) == B and all(len(r) == T for r in rows)
    assert all(1 <= len(caps[v]) <= 20 for v in vids) and max(len(caps[v]) for v in vids) > 5
    host = CiderRewarder(caps, vids, SOS, EOS)
    want = host.rewards(row_vids, rows)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV, vocab_size=hi + 4)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    got = d.rewards(row_vids, ids)
    wide = torch.full((B, T + 9), 7, dtype=torch.long, device=DEV)                  # the same rows as a strided view
    wide[:, 5:5 + T] = ids
    view = wide[:, 5:5 + T]
    assert not view.is_contiguous() and view.stride() == (T + 9, 1)
    got_view = d.rewards(row_vids, view)
    capi.check_async_error()
    _close(got.cpu().numpy(), want)
    _close(got_view.cpu().numpy(), want)
    assert torch.equal(got, got_view)
    assert (want > 0).sum() >= B // 4 and want.max() > 1.0 and (want == 0).sum() >= 3


# ------------------------------------------------------------------ determinism
def test_rewards_are_bit_identical_across_calls_and_batch_compositions(lib):
    vids, caps, row_vids, rows = _sweep_batch(31, 5, 14)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    a = d.rewards(row_vids, ids)
    b2 = d.rewards(row_vids, ids)
    assert torch.equal(a, b2)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).tolist()
    c = d.rewards([row_vids[i] for i in perm], ids[perm])
    assert torch.equal(c, a[perm])
    for i in (0, 1, 9, 17, 40, 63):                                                  # a row alone = the row inside the batch of 64
        one = d.rewards([row_vids[i]], ids[i:i + 1])
        assert tuple(one.shape) == (1,) and torch.equal(one, a[i:i + 1]), i
    capi.check_async_error()
    assert (a > 0).sum() > 10


def test_long_rows_up_to_the_lds_limit(lib):
    """T = 256 and T = CIDER_MAX_T: the n-gram list fills the LDS layout; beyond it the call is refused with a message"""
    vids, caps, rng = hc.edge_corpus(41, n_clips=6, max_refs=5)
    host = CiderRewarder(caps, vids, SOS, EOS)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV)
    for width in (256, capi.CIDER_MAX_T):
        rows = [[int(x) for x in rng.randint(5, 14, size=width)] for _ in vids]     # no <eos>: width words each
        rows[1][width // 2] = EOS
        got = d.rewards(vids, torch.tensor(rows, dtype=torch.long, device=DEV))
        capi.check_async_error()
        _close(got.cpu().numpy(), host.rewards(vids, rows))
    with pytest.raises(ValueError, match="LDS"):
        d.rewards(vids, torch.zeros(len(vids), capi.CIDER_MAX_T + 1, dtype=torch.long, device=DEV))


# ------------------------------------------------------------------ s2vt_sc_weights
def test_sc_weights_equal_the_host_construction(lib):
    rng = np.random.RandomState(5)
    Tw = 11
    sampled = torch.tensor(rng.randint(5, 30, size=(8, Tw)), dtype=torch.long)
    sampled[0, 0] = EOS                                   # <eos> first
    sampled[1, Tw - 1] = EOS                              # <eos> last
    sampled[2, 3] = EOS
    sampled[2, 7] = EOS                                   # two: the first counts
    sampled[3, 5] = EOS                                   # rows 4..7: no <eos>
    r_s = rng.rand(8) * 3
    r_g = rng.rand(8) * 3
    r_s[6], r_g[6] = 0.25, 2.75                           # negative advantages as well: rows 6 and 7
    r_s[7], r_g[7] = min(r_s[7], r_g[7]), max(r_s[7], r_g[7]) + 0.5
    r_g[4] = r_s[4]                                       # advantage exactly 0
    r_s[5], r_g[5] = 0.1 + 0.2, 0.3                       # a difference that only float64 resolves before the one rounding to fp32
    assert (r_s - r_g > 0).any() and (r_s - r_g < 0).any()
    caps, weight = ops.sc_weights(sampled.to(DEV), torch.tensor(r_s, device=DEV), torch.tensor(r_g, device=DEV), SOS, EOS)
    torch.cuda.synchronize()
    assert caps.dtype == torch.int64 and weight.dtype == torch.float32 and tuple(caps.shape) == tuple(weight.shape) == (8, Tw + 1)
    assert torch.equal(caps.cpu(), torch.cat([torch.full((8, 1), SOS, dtype=torch.long), sampled], 1))
    want = advantage_weights(sampled, r_s - r_g, EOS)
    assert torch.equal(weight.cpu(), want)
    assert want[0].tolist()[:3] == [0.0, float(np.float32(r_s[0] - r_g[0])), 0.0] and (want[1, 1:] != 0).all() and (want[4] == 0).all()
    with pytest.raises(capi.S2VTHipError):
        ops.sc_weights(sampled.to(DEV), torch.tensor(r_s, device=DEV).float(), torch.tensor(r_g, device=DEV), SOS, EOS)


# ------------------------------------------------------------------ out-of-range token: an error flag, not a fault
def test_out_of_range_token_raises_indexerror_and_the_next_call_is_clean(lib):
    vids, caps, row_vids, rows = _sweep_batch(51, 5, 14)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    clean = d.rewards(row_vids, ids)
    capi.check_async_error()
    first_eos = [r.index(EOS) if EOS in r else T for r in rows]
    for bad_value in (65536, -1, 2 ** 40):
        row = next(i for i in range(B) if first_eos[i] >= 3)
        bad = ids.clone()
        bad[row, 1] = bad_value                            # before the row's first <eos>: the scorer reads it
        got = d.rewards(row_vids, bad)
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
        keep = torch.arange(B, device=DEV) != row
        assert torch.equal(got[keep], clean[keep]) and bool(torch.isfinite(got).all())       # the other rows are untouched
        again = d.rewards(row_vids, ids)
        torch.cuda.synchronize()
        capi.check_async_error()
        assert torch.equal(again, clean)
    row = next(i for i in range(B) if first_eos[i] < T - 1)
    behind = ids.clone()
    behind[row, first_eos[row] + 1] = 70000                # behind the first <eos>: never read, no error
    got = d.rewards(row_vids, behind)
    torch.cuda.synchronize()
    capi.check_async_error()
    assert torch.equal(got, clean)
    with pytest.raises(KeyError):
        d.rewards(["no such clip"] + row_vids[1:], ids)


# ------------------------------------------------------------------ train.py --self-critical --sc-reward device
@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_self_critical_epoch_host_and_device_rewards_agree(tmp_path, rnn_type):
    """the toy recipe of test_gpu_sampling.test_self_critical_epoch_end_to_end, once per rewarder: same seeds, so the first step
    samples the same ids and its two mean rewards agree to 1e-10 (later steps follow weights that differ through the fp32 rounding of
    the advantage and are not compared)"""
    sys.path.insert(0, ROOT)
    import train
    import test_train_eval_parity as toy
    toy.make_toy(str(tmp_path))
    got = {}
    for where in ("host", "device"):
        opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                           "--train-length", str(toy.L), "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F),
                           "--batch-size", str(toy.BS), "--epochs", "1", "--lr", "1e-3", "--save-path", str(tmp_path / ("ck_" + where)),
                           "--no-shuffle", "--seed", "7", "--rnn-type", rnn_type, "--self-critical", "--sc-temperature", "1.0",
                           "--sc-reward", where])
        got[where] = h = train.run(opt)
        assert len(h["train_loss"]) == 1 and np.isfinite(h["train_loss"][0]) and np.isfinite(h["valid_loss"][0])
        sp = h["sc_split_ms"]
        assert sorted(sp) == ["greedy", "sample", "scoring", "steps", "train"]
        assert sp["steps"] == 3 and all(sp[k] > 0 for k in ("sample", "greedy", "scoring", "train"))
        print(where, "self-critical step split (ms per step):", {k: round(v / sp["steps"], 2) for k, v in sp.items() if k != "steps"})
        assert len(h["reward_sample"]) == 3 and all(np.isfinite(h["reward_sample"])) and all(r >= 0 for r in h["reward_greedy"])
    print("first step rewards:", {k: (v["reward_sample"][0], v["reward_greedy"][0]) for k, v in got.items()})
    assert abs(got["host"]["reward_sample"][0] - got["device"]["reward_sample"][0]) <= 1e-10
    assert abs(got["host"]["reward_greedy"][0] - got["device"]["reward_greedy"][0]) <= 1e-10
