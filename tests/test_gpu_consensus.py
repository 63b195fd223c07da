"""GPU tests of consensus (MBR) caption selection: s2vt_cider_consensus through ops.cider_consensus, DeviceCiderRewarder.consensus,
consensus.select and eval.py --consensus.

Reference: the host oracle CiderRewarder.consensus (caption_metrics.cider_of_vectors of every candidate against the clip's other
candidates), every element at rtol 1e-10, atol 1e-12 - the bound tests/test_gpu_cider_reward.py derives for the same arithmetic: the
device only performs IEEE + * / sqrt min on float64 factors the host precomputed, sums of non-negative terms (no cancellation) over at
most 4 T terms per pair and K - 1 pairs - at T = 512, K = 64 about 2100 roundings of 1.1e-16 each, 2.4e-13 relative in the worst
case.  The candidates, their seeds
and the oracle's values are tests/test_consensus_host.py's (computed once per process)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, consensus, synth
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cider_reward_host as hc  # noqa: E402
import test_consensus_host as ch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOS, EOS = ch.SOS, ch.EOS
RTOL, ATOL = ch.RTOL, ch.ATOL
_REW = {}


def rewarders():
    """(host, device) rewarders over the corpus of the host tests, the table uploaded once per process"""
    if not _REW:
        vids, caps, host, _ = ch.corpus()
        _REW["r"] = (host, DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV), caps)
    return _REW["r"]


def _close(got, want):
    """every element: -inf where the oracle has -inf, the bound elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), ~fin)
    err = np.abs(got[fin] - want[fin])
    print("elements %d (%d finite)  max abs err %.3e  max rel err %.3e  max utility %.4f" % (
        want.size, fin.sum(), err.max() if fin.any() else 0.0,
        (err / np.maximum(np.abs(want[fin]), 1e-300))[want[fin] != 0].max() if (want[fin] != 0).any() else 0.0, want[fin].max() if fin.any() else 0.0))
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL)


def _check_selection(rows, best_d, util_d, want_best, want, valid=None):
    """best is the first maximum of the RETURNED utility (exactly, on the device); the chosen candidate is within twice the bound of
    the oracle's maximum; on clear clips it has the oracle's words"""
    masked = util_d if valid is None else torch.where(valid, util_d, torch.full_like(util_d, float("-inf")))
    assert best_d.dtype == torch.int64 and torch.equal(best_d, masked.argmax(1))
    best = best_d.cpu().numpy()
    clear = ch.clear_clips(rows, want_best, want, None if valid is None else valid.cpu().numpy())
    for b in range(len(rows)):
        fin = np.isfinite(want[b])
        if not fin.any():
            assert best[b] == 0
            continue
        top = want[b][fin].max()
        assert fin[best[b]] and top - want[b][best[b]] <= 2 * (ATOL + RTOL * abs(top)), b
        if clear[b]:
            assert ch.words_of(rows[b][best[b]]) == ch.words_of(rows[b][want_best[b]]), b
    return clear


# ------------------------------------------------------------------ values and selection
@pytest.mark.parametrize("shape", sorted(ch.SWEEP))
def test_utility_and_choice_match_the_oracle(lib, shape):
    host, dev, _ = rewarders()
    rows, want_best, want = ch.sweep_case(shape)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    best, util = dev.consensus(ids)
    assert util.dtype == torch.float64 and util.is_cuda and tuple(util.shape) == shape[:2] and tuple(best.shape) == shape[:1]
    capi.check_async_error()
    _close(util.cpu().numpy(), want)
    clear = _check_selection(rows, best, util, want_best, want)
    print(shape, "clear clips %d of %d" % (clear.sum(), shape[0]))
    assert 2 * clear.sum() >= shape[0]
    chosen, b2, u2 = consensus.select(dev, ids)
    assert torch.equal(b2, best) and torch.equal(u2, util) and torch.equal(chosen, ids[torch.arange(shape[0], device=DEV), best])


# ------------------------------------------------------------------ the mask
def test_masked_candidates(lib):
    host, dev, caps = rewarders()
    B, K, T = 9, 6, 12
    rows = ch.candidates(5, B, K, T, caps)
    valid = np.random.RandomState(5).rand(B, K) < 0.6
    valid[0], valid[1] = [False, False, False, True, False, False], False        # a single valid candidate; none
    valid[2], valid[3, 0] = True, False
    assert (valid.sum(1) >= 2).sum() >= 5
    want_best, want = host.consensus(rows, valid)
    ids, vd = torch.tensor(rows, dtype=torch.long, device=DEV), torch.tensor(valid, device=DEV)
    best, util = dev.consensus(ids, vd)
    capi.check_async_error()
    _close(util.cpu().numpy(), want)
    _check_selection(rows, best, util, want_best, want, vd)
    assert best[0] == 3 and util[0, 3] == 0.0 and best[1] == 0 and bool(torch.isneginf(util[1]).all())
    b8, u8 = dev.consensus(ids, vd.to(torch.uint8))
    assert torch.equal(b8, best) and torch.equal(u8, util)
    # consensus.select: scores that are not finite are the mask; [B, G, n, T] is [B, G * n, T]
    scores = torch.where(vd, torch.randn(B, K, device=DEV), torch.tensor(float("-inf"), device=DEV))
    scores[3, 0] = float("nan")
    chosen, bs, us = consensus.select(dev, ids.view(B, 2, 3, T), scores.view(B, 2, 3))
    assert torch.equal(bs, best) and torch.equal(us, util) and torch.equal(chosen, ids[torch.arange(B, device=DEV), best])
    ch_h, bh, uh = consensus.select(host, ids, scores)                               # the host path, results back on the device
    assert uh.is_cuda and np.array_equal(bh.cpu().numpy(), want_best) and np.array_equal(uh.cpu().numpy(), want)
    with pytest.raises(capi.S2VTHipError):
        dev.consensus(ids, vd[:, :5])
    with pytest.raises(capi.S2VTHipError):
        dev.consensus(ids, vd.cpu())


# ------------------------------------------------------------------ determinism
def test_bits_do_not_depend_on_the_call_the_batch_or_the_row_stride(lib):
    host, dev, _ = rewarders()
    shape = (70, 7, 79)
    B, K, T = shape
    rows, _, _ = ch.sweep_case(shape)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    valid = torch.tensor(np.random.RandomState(9).rand(B, K) < 0.8, device=DEV)
    for v in (None, valid):
        best, util = dev.consensus(ids, v)
        b2, u2 = dev.consensus(ids, v)
        assert torch.equal(best, b2) and torch.equal(util.view(torch.int64), u2.view(torch.int64))
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(DEV)
        bp, up = dev.consensus(ids[perm], None if v is None else v[perm])
        assert torch.equal(bp, best[perm]) and torch.equal(up.view(torch.int64), util[perm].view(torch.int64))
        for b in (0, 1, 33, 69):                                                       # a clip alone = the clip inside the batch of 70
            b1, u1 = dev.consensus(ids[b:b + 1], None if v is None else v[b:b + 1])
            assert torch.equal(b1, best[b:b + 1]) and torch.equal(u1.view(torch.int64), util[b:b + 1].view(torch.int64)), b
        wide = torch.full((B, K, T + 9), 7, dtype=torch.long, device=DEV)              # the same rows as a row-strided view
        wide[:, :, 5:5 + T] = ids
        view = wide[:, :, 5:5 + T]
        assert not view.is_contiguous() and view.stride() == (K * (T + 9), T + 9, 1)
        bv, uv = dev.consensus(view, v)
        assert torch.equal(bv, best) and torch.equal(uv.view(torch.int64), util.view(torch.int64))
    capi.check_async_error()
    tr = ids.transpose(1, 2).contiguous().transpose(1, 2)                              # last stride K: a contiguous copy is taken
    assert tr.stride(2) != 1
    bt, ut = dev.consensus(tr, valid)
    assert torch.equal(bt, best) and torch.equal(ut.view(torch.int64), util.view(torch.int64))


# ------------------------------------------------------------------ out-of-range token: an error flag, not a fault
def test_out_of_range_token_raises_indexerror_and_the_next_call_is_clean(lib):
    host, dev, _ = rewarders()
    rows, _, _ = ch.sweep_case((5, 5, 3))
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    clean_b, clean_u = dev.consensus(ids)
    capi.check_async_error()
    clip, k = next((b, k) for b in range(5) for k in range(5) if EOS not in rows[b][k][:2])
    for bad_value in (70000, -1):
        bad = ids.clone()
        bad[clip, k, 1] = bad_value                        # before the row's first <eos>: the scorer reads it
        got_b, got_u = dev.consensus(bad)
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
        keep = torch.arange(5, device=DEV) != clip
        assert torch.equal(got_u[keep].view(torch.int64), clean_u[keep].view(torch.int64)) and torch.equal(got_b[keep], clean_b[keep])
        assert bool(torch.isfinite(got_u).all())
        # the row was scored without the token
        fixed = [[list(r) for r in c] for c in rows]
        fixed[clip][k][1] = 0
        _close(got_u.cpu().numpy()[clip], host.consensus(fixed)[1][clip])
        again_b, again_u = dev.consensus(ids)
        torch.cuda.synchronize()
        capi.check_async_error()
        assert torch.equal(again_u.view(torch.int64), clean_u.view(torch.int64)) and torch.equal(again_b, clean_b)
    masked = torch.ones(5, 5, dtype=torch.bool, device=DEV)
    masked[clip, k] = False                                # a candidate that is not valid is not read: no error
    bad = ids.clone()
    bad[clip, k, 1] = 70000
    dev.consensus(bad, masked)
    torch.cuda.synchronize()
    capi.check_async_error()
    with pytest.raises(capi.S2VTHipError):                 # a host tensor: there is no CPU fallback
        dev.consensus(ids.cpu())
    with pytest.raises(ValueError):
        dev.consensus(torch.zeros(2, capi.CONSENSUS_MAX_K + 1, 4, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match="LDS"):
        dev.consensus(torch.zeros(2, 3, capi.CIDER_MAX_T + 1, dtype=torch.long, device=DEV))


# ------------------------------------------------------------------ the shared candidate phase leaves s2vt_cider_rewards alone
def test_cider_rewards_bits_are_unchanged_around_a_consensus_call(lib):
    vids, caps, rng = hc.edge_corpus(21, n_clips=12, max_refs=6, ref_words=(2, 13))
    T = 24
    cases = hc.edge_candidates(vids, caps, 5, 14, T)
    cases += [(v, ([int(x) for x in rng.randint(5, 14, size=rng.randint(1, 20))] + [EOS] + [0] * T)[:T]) for v in vids]
    row_vids, rows = [v for v, _ in cases], [r for _, r in cases]
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    before = d.rewards(row_vids, ids)
    best, util = d.consensus(ids[:20].view(4, 5, T))
    after = d.rewards(row_vids, ids)
    capi.check_async_error()
    assert torch.equal(before.view(torch.int64), after.view(torch.int64))
    np.testing.assert_allclose(before.cpu().numpy(), CiderRewarder(caps, vids, SOS, EOS).rewards(row_vids, rows), rtol=RTOL, atol=ATOL)
    assert (before > 0).sum() >= 6 and bool(torch.isfinite(util).all())


# ------------------------------------------------------------------ end to end: the model's own candidates
def test_select_on_sampled_beam_and_group_candidates(lib):
    import S2VTModel
    d = synth.CONFIGS["tiny"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=42, out_scale=4.0)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=42)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    vids, caps, _ = hc.random_corpus(7, n_clips=9, lo=5, hi=d["V"])
    host, dev = CiderRewarder(caps, vids, SOS, EOS), DeviceCiderRewarder(caps, vids, SOS, EOS, device=DEV, vocab_size=d["V"])
    x = feats.to(DEV)
    with torch.no_grad():
        sampled = m.sample(x, n_samples=5, seed=1)
        nb, _, nb_scores = m(x, mode='beam', beam_width=5, n_best=5, max_beam_depth=8)
        gr, _, gr_scores = m.beam_diverse(x, beam_width=6, num_groups=3, max_beam_depth=8)
    assert tuple(sampled.shape) == (d["B"], 5, d["L"] - 1) and tuple(nb.shape) == (d["B"], 5, 8) and tuple(gr.shape) == (d["B"], 3, 1, 8)
    for cands, scores in ((sampled, None), (nb, nb_scores), (gr, gr_scores)):
        chosen, best, util = consensus.select(dev, cands, scores)
        capi.check_async_error()
        flat = cands.reshape(d["B"], -1, cands.shape[-1])
        K = flat.shape[1]
        assert tuple(chosen.shape) == (d["B"], flat.shape[2]) and tuple(util.shape) == (d["B"], K) and chosen.is_cuda and util.is_cuda
        assert all(torch.equal(chosen[b], flat[b, best[b]]) for b in range(d["B"]))         # rows of the candidates
        ch_h, best_h, util_h = consensus.select(host, cands, scores)                         # the host path on the same ids
        want = util_h.cpu().numpy()
        _close(util.cpu().numpy(), want)
        valid = None if scores is None else torch.isfinite(scores).reshape(d["B"], -1)
        _check_selection(flat.cpu().tolist(), best, util, best_h.cpu().numpy(), want, valid)
        assert np.isfinite(want).any(1).all() and want.max() > 0


_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""


def test_eval_writes_the_consensus_choice_and_leaves_the_predictions(lib, tmp_path):
    """three runs in ONE child process (the tool brings its own feed thread and copy stream): --sample 5 with and without --consensus,
    and --beam 4 --n-best 3 --consensus"""
    import subprocess
    import S2VTModel
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path), V=64)
    V = len(data["word2ix"])
    m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
    m.load_state_dict(synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=38, out_scale=16.0))
    torch.save(m, tmp_path / "model.pth")
    common = ["--model-path", str(tmp_path / "model.pth"), "--caption-file", str(tmp_path / "captions.json"), "--feats-path",
              str(tmp_path / "feats"), "--batch-size", "3"]
    runs = [common + ["--sample", "5", "--sample-seed", "3", "--out", str(tmp_path / "plain.json")],
            common + ["--sample", "5", "--sample-seed", "3", "--consensus", "--out", str(tmp_path / "cons.json")],
            common + ["--beam", "4", "--beam-mode", "cumulative", "--n-best", "3", "--consensus", "--out", str(tmp_path / "beam.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    read = lambda n: open(str(tmp_path / n), "rb").read()                # noqa: E731
    load = lambda n: json.loads(read(n))                                  # noqa: E731
    assert read("plain.json") == read("cons.json") and read("plain.json.samples.json") == read("cons.json.samples.json")
    assert not os.path.exists(str(tmp_path / "plain.json.consensus.json"))
    cons, samples = load("cons.json.consensus.json"), load("cons.json.samples.json")
    assert set(cons) == set(data["splits"]["test"]) == set(load("cons.json"))
    for vid, e in cons.items():
        assert set(e) == {"chosen", "utility", "captions"} and e["captions"] == samples[vid] and len(e["utility"]) == 5
        assert e["chosen"] == e["utility"].index(max(e["utility"])) and min(e["utility"]) >= 0
    beam, bc, nbest = load("beam.json"), load("beam.json.consensus.json"), load("beam.json.nbest.json")
    for vid, e in bc.items():
        assert e["captions"] == nbest[vid] and beam[vid] == e["captions"][e["chosen"]] and len(e["utility"]) == 3
        finite = [u for u in e["utility"] if u is not None]
        assert finite and e["utility"][e["chosen"]] == max(finite)
