"""GPU tests of the sentence BLEU-4 reward beside CIDEr: s2vt_mixed_rewards / s2vt_mixed_consensus through ops,
self_critical.DeviceMixedRewarder, consensus.select and train.py --sc-bleu-weight.

What is compared bit for bit, and why it can be: BLEU-4 is integer counting followed by one fixed fp64 chain of + * / sqrt on one
thread with the brevity penalty read from the host's table, so out_bleu equals the host oracle (MixedRewarder.bleu) and the numpy walk
(bleu_walk / bleu_consensus_walk) exactly.  The CIDEr part comes from the code s2vt_cider_rewards / s2vt_cider_consensus run, so it
equals THEIR bits exactly; and the mix is two products and one add, so out equals w_c * out_cider + w_b * out_bleu computed in numpy
from the parts, exactly.  Against the HOST CIDEr (CiderRewarder, table_walk, consensus_walk) the CIDEr part - and with it the mix - is
held to the project's host/device bound of tests/test_gpu_cider_reward.py (rtol 1e-10, atol 1e-12), not to equality: the numpy walks add
a candidate's terms in entry order, the kernels lane-strided with a butterfly, on the parent commit as well (the tests print the
measured difference, a few 1e-16 relative)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, consensus, ops
from s2vt_video_caption_amd.self_critical import DeviceCiderRewarder, DeviceMixedRewarder, MixedRewarder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bleu_reward_host as hb  # noqa: E402
import test_cider_reward_host as hc  # noqa: E402
import test_consensus_host as ch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOS, EOS = hc.SOS, hc.EOS
RTOL, ATOL = 1e-10, 1e-12
WC, WB = hb.WC, hb.WB
B = 37
LO, HI, TOP = 5, 14, 65535


def bits(t):
    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------ the corpus, the batches and their oracle, built once
_STATE = {}


def world():
    """(vids, caps, host MixedRewarder, DeviceMixedRewarder on the card): six clips, the first three with 1, 3 and 40 references -
    more references than the workgroup has wavefronts -, ids LO .. HI and, in two references, 60000 and 65535"""
    if "world" not in _STATE:
        vids, caps, rng = hc.edge_corpus(7, n_clips=6, lo=LO, hi=HI, max_refs=3, ref_words=(3, 9))
        words = lambda n: [int(x) for x in rng.randint(LO, HI + 1, size=n)]          # noqa: E731
        caps[vids[0]] = [[SOS, HI] + words(5) + [EOS]]
        caps[vids[1]] = [[SOS, HI] + words(4) + [EOS], [SOS, 60000, TOP, TOP, 6, EOS], [SOS] + words(7) + [EOS]]
        caps[vids[2]] = [[SOS, HI] + words(rng.randint(2, 12)) + [EOS] for _ in range(40)]
        assert [len(caps[v]) for v in vids[:3]] == [1, 3, 40]
        host = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
        dev = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB, device=DEV, vocab_size=TOP + 1)
        _STATE["world"] = (vids, caps, host, dev)
    return _STATE["world"]


def batch(T):
    """(clip per row, B id rows of T tokens, host cider, host bleu) for one width, computed once: rows without <eos>, <eos> at 0, a
    leading <sos>, pads inside, repeated words, ids up to 65535, references of the clip (exact, one word replaced, two back to back)"""
    if T not in _STATE:
        vids, caps, host, _ = world()
        rng = np.random.RandomState(100 + T)
        pad = lambda row: (list(row) + [0] * T)[:T]                                  # noqa: E731
        ref = lambda v, i=0: caps[v][i % len(caps[v])][1:-1]                          # noqa: E731
        rows = [
            (vids[0], pad([EOS, 5, 6])),                                             # <eos> at position 0
            (vids[1], pad(ref(vids[1], 1) * T)),                                     # no <eos>: the whole row counts; 65535 twice per period
            (vids[1], pad([SOS] + ref(vids[1], 1) + [EOS])),                         # a leading <sos>; an exact reference with 60000, 65535
            (vids[2], pad([LO, SOS, LO + 1, EOS])),                                  # ... dropped at position 0 only
            (vids[2], pad([0, ref(vids[2], 3)[0], 0, 0] + ref(vids[2], 3)[1:] + [0, EOS, LO])),      # pads inside
            (vids[0], pad([HI] * T)),                                                # one word repeated through the row, no <eos>
            (vids[2], pad([7] * 9 + [EOS])),                                         # repeated words: the clipping is active
            (vids[1], pad([TOP, TOP, TOP, TOP, EOS])),                               # 65535 in every field of a key
            (vids[3], pad([HI, EOS])),                                               # one word
            (vids[4], pad([HI, LO, EOS])),                                           # two
            (vids[5], pad([HI, LO, LO + 1, EOS])),                                   # three
            (vids[0], pad(ref(vids[0]) + [EOS])),                                    # the clip's only reference
        ]
        while len(rows) < B:
            v = vids[len(rows) % len(vids)]
            kind = len(rows) % 4
            if kind == 0:
                row = [int(x) for x in rng.randint(LO, HI + 1, size=rng.randint(1, T + 1))] + [EOS]
            elif kind == 1:
                row = list(ref(v, rng.randint(40)))
                row[rng.randint(len(row))] = int(rng.randint(LO, HI + 1))
                row.insert(rng.randint(len(row) + 1), 0)
                row = row + [EOS] + [int(x) for x in rng.randint(LO, HI, size=T)]    # what follows <eos> is not read
            elif kind == 2:
                row = (ref(v, 0) + ref(v, 1)) * T                                    # long, with repeats, no <eos>
            else:
                row = [SOS] + ref(v, rng.randint(40)) + [EOS]
            rows.append((v, pad(row)))
        row_vids, ids = [v for v, _ in rows], [r for _, r in rows]
        _STATE[T] = (row_vids, ids) + host.parts(row_vids, ids)
    return _STATE[T]


def _close(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    rel = (err / np.maximum(np.abs(want), 1e-300))[want != 0]
    print("%s: rows %d  max abs err %.3e  max rel err %.3e  bit-equal %d" % (name, want.size, err.max(), rel.max() if rel.size else 0.0,
                                                                              int((got == want).sum())))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ the rewards kernel against the oracle
@pytest.mark.parametrize("T", [1, 5, 31, 130, 512])
def test_mixed_rewards_against_the_oracle(lib, T):
    """T = 130 crosses the 64-lane strip chunk and a 512-entry sort, 512 is the LDS limit"""
    vids, caps, host, dev = world()
    row_vids, rows, cider, bleu = batch(T)
    assert len(rows) == B and all(len(r) == T for r in rows)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    tb, bt = dev._tables(ids)
    clip_rows = torch.tensor([dev.row_of[v] for v in row_vids], dtype=torch.int32, device=DEV)
    out, oc, ob = ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, WC, WB, return_parts=True)
    plain = ops.cider_rewards(tb, clip_rows, ids, SOS, EOS)
    wide = torch.full((B, T + 9), 7, dtype=torch.long, device=DEV)                   # the same rows as a strided view: ld > T
    wide[:, 5:5 + T] = ids
    view = wide[:, 5:5 + T]
    assert view.stride() == (T + 9, 1)
    out_v, oc_v, ob_v = ops.mixed_rewards(tb, bt, clip_rows, view, SOS, EOS, WC, WB, return_parts=True)
    only = ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, WC, WB)               # the parts are optional outputs
    capi.check_async_error()
    assert all(t.dtype == torch.float64 and t.is_cuda and tuple(t.shape) == (B,) for t in (out, oc, ob, only))
    o, c, b = out.cpu().numpy(), oc.cpu().numpy(), ob.cpu().numpy()
    print("T %d  bleu max %.4f  rows with bleu > 1e-3: %d  cider max %.4f" % (T, bleu.max(), int((bleu > 1e-3).sum()), cider.max()))
    assert (b == bleu).all()                                                         # BLEU-4: the oracle's bits
    assert (b == np.array([dev.bleu_walk(v, r) for v, r in zip(row_vids, rows)])).all()
    assert torch.equal(bits(oc), bits(plain))                                        # CIDEr: s2vt_cider_rewards' bits
    assert (o == WC * c + WB * b).all()                                              # the mix of the parts
    for a, a_v in ((out, out_v), (oc, oc_v), (ob, ob_v), (out, only)):
        assert torch.equal(bits(a), bits(a_v))
    _close("cider against the host", c, cider)
    _close("mix against the host", o, WC * cider + WB * bleu)
    assert b[0] == 0.0 and o[0] == 0.0
    if T >= 5:
        assert b.max() > 0.9 and (b > 1e-3).sum() >= 5


def test_a_row_alone_two_calls_and_the_unit_weights(lib):
    vids, caps, host, dev = world()
    row_vids, rows, cider, bleu = batch(31)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    a = dev.rewards(row_vids, ids)
    pa = dev.last_parts
    again = dev.rewards(row_vids, ids)
    assert torch.equal(bits(a), bits(again))
    pc, pb = dev.parts(row_vids, ids)
    assert torch.equal(bits(pc), bits(pa[0])) and torch.equal(bits(pb), bits(pa[1]))
    for i in (0, 1, 5, 6, 11, 20, 36):                                               # a row alone = the row inside the batch
        one = dev.rewards([row_vids[i]], ids[i:i + 1])
        assert tuple(one.shape) == (1,) and torch.equal(bits(one), bits(a[i:i + 1])), i
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).tolist()
    assert torch.equal(bits(dev.rewards([row_vids[i] for i in perm], ids[perm])), bits(a[perm]))
    tb, bt = dev._tables(ids)
    clip_rows = torch.tensor([dev.row_of[v] for v in row_vids], dtype=torch.int32, device=DEV)
    plain = ops.cider_rewards(tb, clip_rows, ids, SOS, EOS)
    assert torch.equal(bits(ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, 1.0, 0.0)), bits(plain))    # weights (1, 0)
    assert torch.equal(bits(ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, 0.0, 1.0)), bits(pb))
    capi.check_async_error()
    assert (a > 0).sum() > 10


# ------------------------------------------------------------------ the consensus entry
@pytest.mark.parametrize("shape", [(3, 1, 7), (4, 2, 7), (6, 5, 7), (2, 64, 7), (3, 5, 130), (2, 2, 130)])
def test_mixed_consensus_against_the_walks_and_the_oracle(lib, shape):
    Bc, K, T = shape
    vids, caps, _, _ = ch.corpus()
    key = ("consensus",) + shape
    if key not in _STATE:
        host = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
        rows = ch.candidates(17 + K + T, Bc, K, T, caps)
        rng = np.random.RandomState(K + T)
        masks = [None, rng.rand(Bc, K) < 0.6, np.zeros((Bc, K), dtype=bool), np.eye(K, dtype=bool)[rng.randint(K, size=Bc)]]
        _STATE[key] = (rows, masks, [host.consensus(rows, m) for m in masks])
    rows, masks, oracle = _STATE[key]
    dev = _STATE.setdefault("consensus_dev", DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB, device=DEV))
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    tb, bt = dev._tables(ids)
    for m, (want_best, want_util) in zip(masks, oracle):                             # all, some, none and exactly one valid
        valid = None if m is None else torch.tensor(m, device=DEV)
        best, util = dev.consensus(ids, valid)
        cbest, cutil = ops.cider_consensus(tb, ids, SOS, EOS, valid)
        b2, u2 = ops.mixed_consensus(tb, bt, ids, SOS, EOS, WC, WB, valid)
        capi.check_async_error()
        assert best.dtype == torch.int64 and util.dtype == torch.float64 and tuple(util.shape) == (Bc, K)
        assert torch.equal(best, b2) and torch.equal(bits(util), bits(u2))
        u, cu = util.cpu().numpy(), cutil.cpu().numpy()
        v = np.ones((Bc, K), dtype=bool) if m is None else m
        walk_c = np.stack([dev.consensus_walk(rows[b], v[b])[1] for b in range(Bc)])
        walk_b = np.stack([dev.bleu_consensus_walk(rows[b], v[b]) for b in range(Bc)])
        others = v & (v.sum(1, keepdims=True) > 1)
        assert (np.isneginf(u) == ~v).all() and (u[v & ~others] == 0.0).all()
        assert (u[others] == (WC * cu + WB * walk_b)[others]).all()                   # s2vt_cider_consensus' bits and the BLEU walk's, mixed
        if others.any():
            _close("utility against the walks", u[others], (WC * walk_c + WB * walk_b)[others])
            _close("utility against the host", u[others], want_util[others])
        masked = torch.where(torch.tensor(v, device=DEV), util, torch.full_like(util, -float("inf")))
        assert torch.equal(best, torch.where(torch.tensor(v.any(1), device=DEV), masked.argmax(1), torch.zeros_like(best)))
        clear = ch.clear_clips(rows, want_best, want_util, None if m is None else m.tolist())
        got_best = best.cpu().numpy()
        assert all(ch.words_of(rows[b][got_best[b]]) == ch.words_of(rows[b][want_best[b]]) for b in np.nonzero(clear)[0])
    ones = ops.mixed_consensus(tb, bt, ids, SOS, EOS, 1.0, 0.0)                      # weights (1, 0): s2vt_cider_consensus' bits
    plain = ops.cider_consensus(tb, ids, SOS, EOS)
    assert torch.equal(ones[0], plain[0]) and torch.equal(bits(ones[1]), bits(plain[1]))


def test_select_on_groups_with_scores_that_are_not_finite(lib):
    vids, caps, _, _ = ch.corpus()
    host = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    dev = _STATE.setdefault("consensus_dev", DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB, device=DEV))
    Bc, G, n, T = 4, 2, 3, 9
    rows = torch.tensor(ch.candidates(5, Bc, G * n, T, caps)).view(Bc, G, n, T)
    scores = torch.zeros(Bc, G, n)
    scores[0, 1, 2], scores[1, 0, 0], scores[2] = float("-inf"), float("nan"), float("inf")
    chosen, best, util = consensus.select(dev, rows.to(DEV), scores.to(DEV))
    capi.check_async_error()
    hc_, hb_, hu = consensus.select(host, rows, scores)
    assert chosen.is_cuda and tuple(chosen.shape) == (Bc, T) and tuple(util.shape) == (Bc, G * n)
    u = util.cpu().numpy()
    assert (np.isneginf(u) == ~torch.isfinite(scores).view(Bc, -1).numpy()).all() and np.isneginf(u[2]).all() and best[2] == 0
    fin = np.isfinite(u)
    _close("select against the host", u[fin], hu.numpy()[fin])
    flat = rows.view(Bc, -1, T)
    assert all(torch.equal(chosen[b].cpu(), flat[b, best[b]]) for b in range(Bc))


# ------------------------------------------------------------------ error paths
def test_error_paths(lib):
    vids, caps, host, dev = world()
    row_vids, rows, cider, bleu = batch(31)
    ids = torch.tensor(rows, dtype=torch.long, device=DEV)
    tb, bt = dev._tables(ids)
    clip_rows = torch.tensor([dev.row_of[v] for v in row_vids], dtype=torch.int32, device=DEV)
    clean = ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, WC, WB, return_parts=True)
    capi.check_async_error()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    out = torch.empty(B, dtype=torch.float64, device=DEV)
    long_ids = torch.zeros(B, capi.CIDER_MAX_T + 1, dtype=torch.long, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.s2vt_mixed_rewards(ctypes.byref(tb), ctypes.byref(bt), ptr(clip_rows), ptr(long_ids), B, capi.CIDER_MAX_T + 1,
                                  capi.CIDER_MAX_T + 1, SOS, EOS, WC, WB, ptr(out), None, None, stream) == -1       # S2VT_ERR_ARG
    assert "LDS" in lib.s2vt_last_error().decode()
    assert lib.s2vt_mixed_rewards(ctypes.byref(tb), None, ptr(clip_rows), ptr(ids), B, 31, 31, SOS, EOS, WC, WB, ptr(out), None, None,
                                  stream) == -1                                      # a null table
    with pytest.raises(ValueError, match="LDS"):
        ops.mixed_rewards(tb, bt, clip_rows, long_ids, SOS, EOS, WC, WB)
    for bad in ((float("nan"), 0.5), (1.0, float("inf"))):                          # before the library is called
        with pytest.raises(ValueError, match="finite"):
            ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, *bad)
        with pytest.raises(ValueError, match="finite"):
            ops.mixed_consensus(tb, bt, ids.view(1, B, 31), SOS, EOS, *bad)
    # a token of 70000 before the row's first <eos>: IndexError at the next check, the other rows untouched, the next call clean
    first_eos = [r.index(EOS) if EOS in r else 31 for r in rows]
    row = next(i for i in range(B) if first_eos[i] >= 3)
    bad = ids.clone()
    bad[row, 1] = 70000
    got = ops.mixed_rewards(tb, bt, clip_rows, bad, SOS, EOS, WC, WB, return_parts=True)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()
    keep = torch.arange(B, device=DEV) != row
    assert all(torch.equal(bits(g[keep]), bits(c[keep])) and bool(torch.isfinite(g).all()) for g, c in zip(got, clean))
    again = ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, WC, WB, return_parts=True)
    torch.cuda.synchronize()
    capi.check_async_error()
    assert all(torch.equal(bits(g), bits(c)) for g, c in zip(again, clean))
    # a clip row out of range scores 0.0 in all three outputs and is reported
    wrong = clip_rows.clone()
    wrong[4], wrong[9] = len(vids), -1
    got = ops.mixed_rewards(tb, bt, wrong, ids, SOS, EOS, WC, WB, return_parts=True)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        capi.check_async_error()
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[4] = keep[9] = False
    for g, c in zip(got, clean):
        assert g[4] == 0.0 and g[9] == 0.0 and torch.equal(bits(g[keep]), bits(c[keep]))
    again = ops.mixed_rewards(tb, bt, clip_rows, ids, SOS, EOS, WC, WB)
    torch.cuda.synchronize()
    capi.check_async_error()
    assert torch.equal(bits(again), bits(clean[0]))
    with pytest.raises(KeyError):
        dev.rewards(["no such clip"] + row_vids[1:], ids)


# ------------------------------------------------------------------ train.py --sc-bleu-weight
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import train
import test_train_eval_parity as toy
tmp = sys.argv[2]
toy.make_toy(tmp, n_train=8)
seen = []
make = train.make_self_critical_step
def spy(model, optimizer, reward_criterion, rewarder, *a, **kw):
    seen.append(type(rewarder).__name__)
    return make(model, optimizer, reward_criterion, rewarder, *a, **kw)
train.make_self_critical_step = spy
out = {}
for name, extra in (("host", ["--sc-reward", "host", "--sc-bleu-weight", "0.5"]), ("device", ["--sc-reward", "device", "--sc-bleu-weight", "0.5"]),
                    ("default", ["--sc-reward", "device"])):
    opt = train.parse(["--caption-file", tmp + "/captions.json", "--feats-path", tmp + "/feats", "--train-length", str(toy.L),
                       "--dim-hidden", str(toy.H), "--dim-embed", str(toy.E), "--feat-dim", str(toy.F), "--batch-size", str(toy.BS),
                       "--epochs", "1", "--lr", "1e-3", "--save-path", tmp + "/ck_" + name, "--no-shuffle", "--seed", "7", "--self-critical",
                       "--sc-temperature", "1.0", "--sc-samples", "2", "--sc-baseline", "mean"] + extra)
    h = train.run(opt)
    out[name] = {k: h.get(k) for k in ("train_loss", "reward_sample", "reward_baseline", "reward_greedy", "reward_cider", "reward_bleu")}
    out[name]["steps"] = h["sc_split_ms"]["steps"]
out["types"] = seen
print("RESULT " + json.dumps(out))
"""


def test_two_self_critical_steps_host_and_device_mixed_rewards_agree(tmp_path):
    """two --self-critical --sc-bleu-weight 0.5 --sc-samples 2 --sc-baseline mean steps at the toy dims, in a child process, once per
    rewarder: same seeds and the same sampled ids, so the rewards' history agrees to rtol 1e-10 (the CIDEr part's bound)"""
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    got = json.loads(next(l for l in text.splitlines() if l.startswith("RESULT "))[7:])
    print(got)
    assert got["types"] == ["MixedRewarder", "DeviceMixedRewarder", "DeviceCiderRewarder"]
    host, dev, plain = got["host"], got["device"], got["default"]
    assert host["steps"] == dev["steps"] == 2 and len(host["reward_sample"]) == len(dev["reward_sample"]) == 2
    assert len(host["reward_bleu"]) == len(dev["reward_bleu"]) == 1 == len(host["reward_cider"]) == len(dev["reward_cider"])
    for k in ("reward_sample", "reward_bleu", "reward_cider"):
        assert np.isfinite(host[k]).all() and np.isfinite(dev[k]).all()
        np.testing.assert_allclose(dev[k], host[k], rtol=1e-10, atol=0)
    assert host["reward_bleu"][0] > 0 and host["reward_greedy"] == [] and np.isfinite(dev["train_loss"]).all()
    # the defaults: today's rewarder, no new history
    assert plain["reward_cider"] is None and plain["reward_bleu"] is None and len(plain["reward_sample"]) == 2
