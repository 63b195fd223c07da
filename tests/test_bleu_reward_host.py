"""Host-side checks of the sentence BLEU-4 reward beside CIDEr (train.py --sc-bleu-weight, eval.py --consensus-bleu-weight): the oracle
self_critical.MixedRewarder against caption_metrics.bleu (the restated reference scorer, pinned by tests/test_caption_metrics.py),
DeviceMixedRewarder's flat BLEU table and its numpy walks (what s2vt_mixed_rewards / s2vt_mixed_consensus run on the card,
tests/test_gpu_bleu_reward.py) against the oracle bit for bit, the mix, consensus under the mixed utility and the flags.  No device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from caption_metrics import bleu, ngrams
from s2vt_video_caption_amd import capi, consensus
from s2vt_video_caption_amd.self_critical import (CiderRewarder, DeviceCiderRewarder, DeviceMixedRewarder, MixedRewarder, pack_key,
                                                  sentence_bleu4, strip_caption, unpack_key)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cider_reward_host as hc  # noqa: E402
import test_consensus_host as ch  # noqa: E402

SOS, EOS = hc.SOS, hc.EOS
NEW_SYMBOLS = ("s2vt_mixed_rewards", "s2vt_mixed_consensus_workspace_bytes", "s2vt_mixed_consensus")
WC, WB = 0.75, 0.5


# ---- shared with test_gpu_bleu_reward.py
def crafted_corpus():
    """clips for the crafted rows: `near` has a reference on each side of a 4-word row at equal distance (3 and 5 words), `twice`
    one reference holding word 7 twice, `same` one reference to be matched exactly"""
    caps = {"near": [[SOS, 5, 6, 7, EOS], [SOS, 5, 6, 7, 8, 9, EOS]], "twice": [[SOS, 7, 8, 7, 9, EOS]],
            "same": [[SOS, 5, 6, 7, 8, 9, 10, EOS], [SOS, 11, 12, EOS]]}
    return sorted(caps), caps


def crafted_rows(T=12):
    pad = lambda row: (row + [0] * T)[:T]                        # noqa: E731
    return [
        ("same", pad([EOS, 5, 6])),                              # an empty row: exactly 0.0
        ("same", pad([5, EOS])),                                 # 1 word: guess_k = 0 for k = 2, 3, 4
        ("same", pad([5, 6, EOS])),                              # 2 words
        ("same", pad([5, 6, 7, EOS])),                           # 3 words
        ("same", pad([5, 6, 7, 8, 9, 10, EOS])),                 # equal to a reference: c = rl, bp just below 1 (the epsilons)
        ("twice", pad([7, 7, 7, 7, EOS])),                       # `a a a a` against a reference holding `a` twice: clipping
        ("near", pad([5, 6, 7, 8, EOS])),                        # references of 3 and 5 words, the row has 4: the shorter one wins
        ("near", pad([SOS, 5, 0, 6, 7, EOS, 8])),                # a leading <sos>, a pad inside, words behind <eos>
    ]


def as_strings(caps, vid, row):
    """(gts, res) of caption_metrics.bleu for one id row: the same ids rendered as strings"""
    text = lambda words: " ".join("w%d" % w for w in words)      # noqa: E731
    return {vid: [text(strip_caption(c, SOS, EOS)) for c in caps[vid]]}, {vid: [text(strip_caption(row, SOS, EOS))]}


def random_rows(vids, caps, rng, lo, hi, n, T=24):
    """rows as the CIDEr sweeps draw them: random words, and references of the clip with one word replaced (so that BLEU is not tiny)"""
    rows = []
    for i in range(n):
        v = vids[rng.randint(len(vids))]
        if i % 2:
            ref = list(caps[v][rng.randint(len(caps[v]))][1:-1])
            ref[rng.randint(len(ref))] = int(rng.randint(lo, hi))
            row = ref + [EOS]
        else:
            row = [int(x) for x in rng.randint(lo, hi, size=rng.randint(1, 12))] + [EOS]
        rows.append((v, (row + [0] * T)[:T]))
    return rows


# ------------------------------------------------------------------ the C surface
def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.s2vt_abi_version() == 9 == capi.ABI_VERSION
    body = re.search(r"typedef struct s2vt_bleu_table \{(.*?)\} s2vt_bleu_table;", header, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.replace("*", " "))]
    assert fields == [f[0] for f in capi.BleuTable._fields_]
    assert ctypes.sizeof(capi.BleuTable) == 6 * 8 + 8 + 3 * 4 + 4
    assert ctypes.sizeof(capi.CiderTable) == 9 * 8 + 8 + 8 + 3 * 4 + 4          # untouched
    for B, K, T in ((3, 5, 79), (1, 1, 1), (2, 64, 512), (0, 5, 7), (2, 65, 7), (2, 5, 513)):
        assert lib.s2vt_mixed_consensus_workspace_bytes(B, K, T) == lib.s2vt_cider_consensus_workspace_bytes(B, K, T)


def test_bad_arguments_are_rejected_on_the_host(lib):
    """non-null (never dereferenced) pointers: every rejection comes before the first device call"""
    fake = ctypes.c_void_p(4096)
    tb, bt = capi.CiderTable(), capi.BleuTable()
    for f, _ in capi.CiderTable._fields_[:9]:
        setattr(tb, f, 4096)
    for f, _ in capi.BleuTable._fields_[:6]:
        setattr(bt, f, 4096)
    tb.n_idf, tb.n_clips, tb.n_refs, tb.n_pen = 1, 1, 1, 1
    bt.n_keys, bt.n_clips, bt.n_refs, bt.n_rl = 1, 1, 1, capi.CIDER_MAX_T + 1
    err = lambda: lib.s2vt_last_error().decode()                 # noqa: E731
    rewards = lambda t, b, T=8, ld=8, wc=1.0, wb=0.5: lib.s2vt_mixed_rewards(                        # noqa: E731
        t, b, fake, fake, 2, T, ld, SOS, EOS, wc, wb, fake, None, None, None)
    assert rewards(None, ctypes.byref(bt)) == -1 and err().startswith("s2vt_mixed_rewards:")
    assert rewards(ctypes.byref(tb), None) == -1                                                     # a null BLEU table
    assert rewards(ctypes.byref(tb), ctypes.byref(bt), T=8, ld=7) == -1
    assert rewards(ctypes.byref(tb), ctypes.byref(bt), T=capi.CIDER_MAX_T + 1, ld=1024) == -1
    assert str(capi.CIDER_MAX_T) in err() and "LDS" in err()
    assert rewards(ctypes.byref(tb), ctypes.byref(bt), wb=float("nan")) == -1 and "finite" in err()
    assert rewards(ctypes.byref(tb), ctypes.byref(bt), wc=float("inf")) == -1
    bt.bp = None
    assert rewards(ctypes.byref(tb), ctypes.byref(bt)) == -1 and "table" in err()
    cons = lambda b, wb=0.5: lib.s2vt_mixed_consensus(ctypes.byref(tb), b, fake, 2, 3, 8, 8, SOS, EOS, None, 1.0, wb, fake, fake,   # noqa: E731
                                                      fake, 1 << 30, None)
    assert cons(ctypes.byref(bt)) == -1 and err().startswith("s2vt_mixed_consensus:") and "bp" in err()
    assert cons(None) == -1
    bt.bp = 4096
    assert cons(ctypes.byref(bt), wb=float("-inf")) == -1 and "finite" in err()
    bt.n_clips = 2                                                                                   # another corpus than the CIDEr table's
    assert rewards(ctypes.byref(tb), ctypes.byref(bt)) == -1 and "table" in err()


# ------------------------------------------------------------------ the oracle against the restated reference scorer
def test_crafted_rows_equal_caption_metrics_bleu():
    vids, caps = crafted_corpus()
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    got = []
    for vid, row in crafted_rows():
        gts, res = as_strings(caps, vid, row)
        want = bleu(gts, res)[1][3][0]
        got.append(m.bleu(vid, row))
        print(vid, strip_caption(row, SOS, EOS), got[-1], want)
        np.testing.assert_allclose(got[-1], want, rtol=1e-12, atol=0)
    assert got[0] == 0.0                                         # the empty row, exactly
    assert all(0.0 < g < 0.05 for g in got[1:4])                 # 1..3 words: the high orders have guess 0 and match 0
    assert 1.0 - 1e-6 < got[4] < 1.0                             # c = rl: just below 1
    # clipping: 4 unigram guesses, 2 of them matched; no such bigram in the reference
    assert got[5] == sentence_bleu4([7, 7, 7, 7], [[7, 8, 7, 9]]) and 0.0 < got[5] < 1e-6
    # the shorter of the two equally close references wins: every n-gram is matched (by the longer one) and c = 4 > rl = 3 leaves no
    # brevity penalty; rl = 5 would give exp(1 - 5/4)
    assert got[6] > 0.999 and 0.77 < sentence_bleu4([5, 6, 7, 8], [[5, 6, 7, 8, 9]]) < 0.78
    assert got[7] == m.bleu("near", [5, 6, 7, EOS])


@pytest.mark.parametrize("seed,lo,hi", [(3, 5, 14), (11, 5, 14), (12, 5, 12000)])
def test_oracle_and_walk_on_random_corpora(seed, lo, hi):
    """MixedRewarder.bleu = caption_metrics.bleu's per-id BLEU_4 to rtol 1e-12 (sqrt(sqrt(.)) against ** 0.25: measured <= 2.3e-16
    relative, the margin covers a libm whose pow is a few ulp off); bleu_walk = the oracle bit for bit"""
    vids, caps, rng = hc.edge_corpus(seed, lo=lo, hi=hi)
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    d = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB)
    cases = hc.edge_candidates(vids, caps, lo, hi, 24) + random_rows(vids, caps, rng, lo, hi, 40)
    got = np.array([m.bleu(v, r) for v, r in cases])
    want = []
    for v, r in cases:
        gts, res = as_strings(caps, v, r)
        want.append(bleu(gts, res)[1][3][0])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    walk = np.array([d.bleu_walk(v, r) for v, r in cases])
    assert walk.dtype == np.float64 and (walk == got).all()
    assert got[0] == 0.0 and got.max() > 0.5 and (got > 1e-3).sum() >= 5


def test_crafted_rows_walk_bitwise():
    vids, caps = crafted_corpus()
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    d = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB)
    for vid, row in crafted_rows():
        assert d.bleu_walk(vid, row) == m.bleu(vid, row), (vid, row)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_bleu_table_invariants(seed):
    vids, caps, _ = hc.edge_corpus(seed)
    d = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB)
    plain = DeviceCiderRewarder(caps, vids, SOS, EOS)
    h = d.host
    for k, a in plain.host.items():                              # the CIDEr table is what it was
        assert h[k].dtype == a.dtype and np.array_equal(h[k], a), k
    assert sorted(set(h) - set(plain.host)) == ["bleu_key_off", "bleu_keys", "bleu_max", "bleu_ref_words", "bp"]
    off = h["bleu_key_off"]
    assert off.dtype == np.int32 and h["bleu_max"].dtype == np.int32 and h["bleu_keys"].dtype == np.uint64
    assert len(off) == len(vids) + 1 and off[0] == 0 and off[-1] == len(h["bleu_keys"]) == len(h["bleu_max"]) and np.all(np.diff(off) > 0)
    assert h["bleu_max"].min() >= 1 and h["bleu_max"].max() >= 2
    r = 0
    for c, v in enumerate(vids):
        keys = h["bleu_keys"][off[c]:off[c + 1]].astype(object)
        assert np.all(np.diff(keys) > 0)                         # strictly ascending: unique and sorted
        counts = [ngrams(strip_caption(cap, SOS, EOS), 4) for cap in caps[v]]
        union = set(g for cnt in counts for g in cnt)
        assert {unpack_key(k) for k in keys} == union
        for k, mx in zip(keys, h["bleu_max"][off[c]:off[c + 1]]):
            assert mx == max(cnt.get(unpack_key(k), 0) for cnt in counts)
        for cap in caps[v]:
            assert h["bleu_ref_words"][r] == len(strip_caption(cap, SOS, EOS))
            r += 1
    assert r == len(h["bleu_ref_words"]) == h["clip_ref_off"][-1]
    assert (h["bleu_ref_words"] != h["ref_len"]).any()           # words, not CIDEr's bigram count
    bp = h["bp"]
    assert bp.dtype == np.float64 and bp.shape == (capi.CIDER_MAX_T + 1, max(int(h["bleu_ref_words"].max()), capi.CIDER_MAX_T) + 1)
    assert (bp[0] == 0.0).all() and bp[5, 3] == 1.0 and 1.0 - 1e-6 < bp[5, 5] < 1.0 and bp[3, 5] == np.exp(1.0 - 1.0 / ((3 + 1e-15) / (5 + 1e-9)))
    assert pack_key((5,)) in h["bleu_keys"]


def test_constructor_errors():
    vids, caps, _ = hc.random_corpus(3)
    for bad in ((float("nan"), 0.5), (1.0, float("inf")), ("x", 0.5), (None, 1.0)):
        with pytest.raises(ValueError):
            MixedRewarder(caps, vids, SOS, EOS, *bad)
        with pytest.raises(ValueError):
            DeviceMixedRewarder(caps, vids, SOS, EOS, *bad)
    with pytest.raises(ValueError):
        DeviceMixedRewarder(caps, vids, SOS, EOS, 1.0, 0.5, n=3)
    d = DeviceMixedRewarder(caps, vids, SOS, EOS, 1.0, 0.5)
    assert isinstance(d, DeviceCiderRewarder) and isinstance(MixedRewarder(caps, vids, SOS, EOS), CiderRewarder)
    with pytest.raises(capi.S2VTHipError):                       # a host tensor: there is no CPU fallback
        d.rewards([vids[0]], torch.tensor([[5, 6, EOS]]))
    with pytest.raises(capi.S2VTHipError):
        d.consensus(torch.tensor([[[5, 6, EOS], [5, 7, EOS]]]))


# ------------------------------------------------------------------ the mix
def test_rewards_are_the_mix_of_the_parts_bitwise():
    vids, caps, rng = hc.edge_corpus(3)
    rows = hc.edge_candidates(vids, caps, 5, 14, 24) + random_rows(vids, caps, rng, 5, 14, 20)
    row_vids, ids = [v for v, _ in rows], [r for _, r in rows]
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    cider, bl = m.parts(row_vids, ids)
    got = m.rewards(row_vids, torch.tensor(ids))
    assert got.dtype == np.float64 and (got == WC * cider + WB * bl).all()
    assert (m.last_parts[0] == cider).all() and (m.last_parts[1] == bl).all()
    assert all(m.score(v, r) == g for v, r, g in zip(row_vids, ids, got))
    plain = CiderRewarder(caps, vids, SOS, EOS).rewards(row_vids, ids)
    assert (cider == plain).all()
    assert (MixedRewarder(caps, vids, SOS, EOS, 1.0, 0.0).rewards(row_vids, ids) == plain).all()          # weights (1, 0): CIDEr's bits
    assert (MixedRewarder(caps, vids, SOS, EOS).rewards(row_vids, ids) == plain).all()                    # the defaults
    assert (MixedRewarder(caps, vids, SOS, EOS, 0.0, 1.0).rewards(row_vids, ids) == bl).all()
    assert (bl > 0).sum() > 10 and (cider > 0).sum() > 10


# ------------------------------------------------------------------ consensus under the mixed utility
def _direct_consensus(m, rows, valid):
    """the definition, literally"""
    _, cider = CiderRewarder.consensus(m, rows, valid)
    B, K = len(rows), len(rows[0])
    valid = np.ones((B, K), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    util, best = np.full((B, K), -np.inf), np.zeros(B, dtype=np.int64)
    for b in range(B):
        words = [strip_caption(r, SOS, EOS) for r in rows[b]]
        top = None
        for i in range(K):
            if not valid[b, i]:
                continue
            others = [words[j] for j in range(K) if j != i and valid[b, j]]
            util[b, i] = WC * cider[b, i] + WB * sentence_bleu4(words[i], others) if others else 0.0
            if top is None or util[b, i] > util[b, top]:
                top = i
        best[b] = 0 if top is None else top
    return best, util


@pytest.mark.parametrize("seed,B,K,T", [(1, 4, 5, 7), (2, 3, 7, 20), (3, 2, 2, 5), (4, 2, 1, 6)])
def test_consensus_oracle_masks_and_walk(seed, B, K, T):
    vids, caps, _, _ = ch.corpus()
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    d = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB)
    rows = ch.candidates(seed, B, K, T, caps)
    rng = np.random.RandomState(seed)
    masks = [None, rng.rand(B, K) < 0.6, np.zeros((B, K), dtype=bool), np.eye(K, dtype=bool)[rng.randint(K, size=B)]]
    for valid in masks:                                          # all, some, none and exactly one valid
        best, util = m.consensus(rows, valid)
        wb, wu = _direct_consensus(m, rows, valid)
        assert (best == wb).all() and (util == wu).all()
        v = np.ones((B, K), dtype=bool) if valid is None else valid
        assert (np.isneginf(util) == ~v).all()
        alone = v & (v.sum(1, keepdims=True) == 1)
        assert (util[alone] == 0.0).all()
        for b in range(B):                                       # the kernels' walks, bit for bit
            cw = d.consensus_walk(rows[b], v[b])[1]
            bw = d.bleu_consensus_walk(rows[b], v[b])
            assert bw.dtype == np.float64 and (np.isneginf(bw) == ~v[b]).all()
            others = v[b].sum() - 1
            want = [sentence_bleu4(strip_caption(rows[b][i], SOS, EOS),
                                   [strip_caption(rows[b][j], SOS, EOS) for j in range(K) if j != i and v[b, j]]) if others > 0 else 0.0
                    for i in range(K) if v[b, i]]
            assert bw[v[b]].tolist() == want
            np.testing.assert_allclose((WC * cw + WB * bw)[v[b]] if others > 0 else np.zeros(v[b].sum()), util[b][v[b]], rtol=1e-10, atol=1e-12)
        if valid is not None and not valid.any():
            assert (best == 0).all()


def test_consensus_first_maximum_and_select_with_groups():
    vids, caps, _, _ = ch.corpus()
    m = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    T = 6
    a, b2 = [5, 6, 7, 8, EOS, 0], [9, 10, 11, EOS, 0, 0]
    best, util = m.consensus([[b2, a, a, b2]])                   # two pairs of duplicates: equal utilities, the first index wins
    assert util[0, 0] == util[0, 3] and util[0, 1] == util[0, 2] and best[0] == int(np.argmax(util[0])) and best[0] in (0, 1)
    best, util = m.consensus([[a, a, a]])
    assert best[0] == 0 and util[0, 0] == util[0, 1] == util[0, 2] > 0
    B, G, n = 3, 2, 3
    rows = torch.tensor(ch.candidates(5, B, G * n, T, caps))
    scores = torch.zeros(B, G, n)
    scores[0, 1, 2], scores[1, 0, 0], scores[2] = float("-inf"), float("nan"), float("inf")
    chosen, bs, us = consensus.select(m, rows.view(B, G, n, T), scores)
    wb, wu = m.consensus(rows.tolist(), torch.isfinite(scores).view(B, -1).numpy())
    assert bs.tolist() == wb.tolist() and np.array_equal(us.numpy(), wu) and tuple(chosen.shape) == (B, T)
    assert all(torch.equal(chosen[b], rows[b, bs[b]]) for b in range(B))
    assert np.isneginf(wu[0, 5]) and np.isneginf(wu[1, 0]) and np.isneginf(wu[2]).all() and bs[2] == 0


# ------------------------------------------------------------------ the flags
def test_train_parses_the_reward_weights():
    import train
    opt = train.parse(["--self-critical", "--sc-reward", "device", "--sc-bleu-weight", "0.5"])
    assert opt.sc_bleu_weight == 0.5 and opt.sc_cider_weight == 1.0
    assert train.parse(["--self-critical", "--sc-cider-weight", "0.25", "--sc-bleu-weight", "2", "--sc-samples", "5", "--sc-baseline", "mean",
                        "--sc-distinct", "--sc-shared-encode"]).sc_cider_weight == 0.25
    assert train.parse([]).sc_bleu_weight == 0.0 and train.parse(["--self-critical"]).sc_cider_weight == 1.0
    for bad in (["--sc-bleu-weight", "0.5"], ["--sc-cider-weight", "0.5"], ["--self-critical", "--sc-bleu-weight", "nan"],
                ["--self-critical", "--sc-cider-weight", "inf"], ["--self-critical", "--sc-bleu-weight", "much"]):
        with pytest.raises(SystemExit):
            train.parse(bad)


def test_eval_parses_the_consensus_weights(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval as ev
    a = ev.build_parser().parse_args(["--model-path", "m", "--consensus", "--sample", "3", "--consensus-bleu-weight", "0.5"])
    assert a.consensus_bleu_weight == 0.5 and a.consensus_cider_weight == 1.0
    for bad in (["--consensus-bleu-weight", "0.5"], ["--sample", "3", "--consensus-cider-weight", "2"],
                ["--consensus", "--sample", "3", "--consensus-bleu-weight", "nan"],
                ["--consensus", "--sample", "3", "--consensus-cider-weight", "-inf"]):
        with pytest.raises(SystemExit):
            ev.main(["--model-path", "m"] + bad)
    # the weights reach consensus_captions and the file; without them the call and the file are what they were
    seen = []

    def fake_consensus(*args, **kw):
        seen.append(kw.get("weights"))
        return {"v": "a"}, {"v": {"chosen": 0, "utility": [0.0, 0.0], "captions": ["a", "b"]}}, {"v": [0.0, 0.0]}

    monkeypatch.setattr(ev, "consensus_captions", fake_consensus)
    import json
    for extra, want in (([], None), (["--consensus-bleu-weight", "0.5"], (1.0, 0.5))):
        out = str(tmp_path / ("p%d.json" % len(seen)))
        ev.main(["--model-path", "m", "--beam", "3", "--beam-mode", "cumulative", "--n-best", "2", "--consensus", "--out", out] + extra)
        assert seen[-1] == want
        cons = json.load(open(out + ".consensus.json"))
        assert sorted(cons) == (["v"] if want is None else ["_weights", "v"])
        if want is not None:
            assert cons["_weights"] == {"cider": 1.0, "bleu": 0.5}
