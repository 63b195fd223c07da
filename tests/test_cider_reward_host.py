"""Host-side checks of the device-resident self-critical reward (train.py --sc-reward device): the C surface, the flat reference
table self_critical.DeviceCiderRewarder builds (keys, CSR offsets, error cases) and its numpy walk against CiderRewarder.score -
the same arrays and the same walk s2vt_cider_rewards runs on the card (tests/test_gpu_cider_reward.py).  No device needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import s2vt_video_caption_amd  # noqa: F401
from caption_metrics import cider_vector
from s2vt_video_caption_amd import capi
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder, pack_key, unpack_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOS, EOS = 3, 4
NEW_SYMBOLS = ("s2vt_cider_rewards", "s2vt_sc_weights")


# ---- shared with test_gpu_cider_reward.py
def random_corpus(seed, n_clips=9, lo=5, hi=14, max_refs=3, ref_words=(2, 7)):
    """the recipe of test_rewarder_equals_caption_metrics_cider_on_the_training_split: {clip: [<sos> words <eos>, ...]}, ids in
    [lo, hi), 1..max_refs references of ref_words[0]..ref_words[1]-1 words per clip"""
    rng = np.random.RandomState(seed)
    vids = ["v%02d" % i for i in range(n_clips)]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(lo, hi, size=rng.randint(*ref_words))] + [EOS]
                for _ in range(rng.randint(1, max_refs + 1))] for v in vids}
    return vids, caps, rng


def edge_corpus(seed, lo=5, hi=14, max_refs=3, **kw):
    """random_corpus plus what the edge cases need: token `hi` opens one reference of EVERY clip (its unigram has idf 0), the last
    reference of clip 0 is shorter than 4 words, and ids hi+1 .. hi+3 occur nowhere"""
    vids, caps, rng = random_corpus(seed, lo=lo, hi=hi, max_refs=max_refs, **kw)
    for v in vids:
        caps[v][0] = [SOS, hi] + caps[v][0][1:]
    if len(caps[vids[0]]) == max_refs:
        caps[vids[0]].pop()
    caps[vids[0]].append([SOS, lo, lo + 1, EOS])
    return vids, caps, rng


def edge_candidates(vids, caps, lo, hi, T):
    """(clip, id row of T tokens) for the cases the issue lists"""
    ref = caps[vids[1]][0][1:-1]
    pad = lambda row: (row + [0] * T)[:T]                        # noqa: E731
    return [
        (vids[0], pad([EOS, lo, lo + 1])),                           # empty candidate: the first token is <eos>
        (vids[1], pad(ref * T)),                                     # no <eos>: the whole row counts
        (vids[1], pad([SOS] + ref + [EOS])),                         # a leading <sos> is dropped
        (vids[2], pad([lo, SOS, lo + 1, EOS])),                      # ... but only at position 0
        (vids[1], pad([0, ref[0], 0, 0] + ref[1:] + [0, EOS, lo])),  # interior pads are dropped
        (vids[3], pad([hi, EOS])),                                   # an n-gram present in every clip: idf 0
        (vids[3], pad([hi] + caps[vids[3]][0][2:-1] + [EOS])),       # the same inside an exact match
        (vids[4], pad([hi + 1, hi + 2, hi + 3, hi + 1, EOS])),       # no n-gram of the corpus
        (vids[0], pad([lo, lo + 1, EOS])),                           # the reference shorter than 4 words, matched exactly
        (vids[0], pad([lo] * 9 + [EOS])),                            # tf > 1 on the candidate side: the clipping is active
    ]


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.s2vt_abi_version() == 9 == capi.ABI_VERSION
    assert re.search(r"#define S2VT_CIDER_MAX_T %d\b" % capi.CIDER_MAX_T, header) and capi.CIDER_MAX_T >= 256
    # the struct binding follows the header field by field
    body = re.search(r"typedef struct s2vt_cider_table \{(.*?)\} s2vt_cider_table;", header, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.replace("*", " "))]
    assert fields == [f[0] for f in capi.CiderTable._fields_]
    assert ctypes.sizeof(capi.CiderTable) == 9 * 8 + 8 + 8 + 3 * 4 + 4


def test_bad_arguments_are_rejected_on_the_host(lib):
    """non-null (never dereferenced) pointers: every rejection comes before the first device call"""
    fake = ctypes.c_void_p(4096)
    tb = capi.CiderTable()
    for f, _ in capi.CiderTable._fields_[:9]:
        setattr(tb, f, 4096)
    tb.n_idf, tb.n_clips, tb.n_refs, tb.n_pen = 1, 1, 1, 1
    err = lambda: lib.s2vt_last_error().decode()                 # noqa: E731
    assert lib.s2vt_cider_rewards(None, fake, fake, 2, 8, 8, SOS, EOS, fake, None) == -1
    assert err().startswith("s2vt_cider_rewards:")
    assert lib.s2vt_cider_rewards(ctypes.byref(tb), fake, None, 2, 8, 8, SOS, EOS, fake, None) == -1
    assert lib.s2vt_cider_rewards(ctypes.byref(tb), fake, fake, 2, 8, 7, SOS, EOS, fake, None) == -1              # ld < T
    assert lib.s2vt_cider_rewards(ctypes.byref(tb), fake, fake, 2, capi.CIDER_MAX_T + 1, 1024, SOS, EOS, fake, None) == -1
    assert str(capi.CIDER_MAX_T) in err() and "LDS" in err()
    tb.pen = None
    assert lib.s2vt_cider_rewards(ctypes.byref(tb), fake, fake, 2, 8, 8, SOS, EOS, fake, None) == -1
    assert "table" in err()
    assert lib.s2vt_sc_weights(fake, fake, None, 2, 8, SOS, EOS, fake, fake, None) == -1
    assert err().startswith("s2vt_sc_weights:")
    assert lib.s2vt_sc_weights(fake, fake, fake, 2, 0, SOS, EOS, fake, fake, None) == -1


def test_train_parses_sc_reward():
    import train
    assert train.parse(["--self-critical", "--sc-reward", "device"]).sc_reward == "device"
    assert train.parse(["--self-critical"]).sc_reward == "host" and train.parse([]).sc_reward == "host"
    with pytest.raises(SystemExit):
        train.parse(["--sc-reward", "elsewhere"])


def test_keys_round_trip_and_order():
    rng = np.random.RandomState(0)
    for _ in range(200):
        g = tuple(int(x) for x in rng.randint(1, 65536, size=rng.randint(1, 5)))
        k = pack_key(g)
        assert 0 < k < 2 ** 64 and unpack_key(k) == g
    assert pack_key((65535,) * 4) == 2 ** 64 - 1 and pack_key((1,)) == 1 << 48
    assert pack_key((5, 6)) < pack_key((5, 6, 1)) < pack_key((5, 7))     # a prefix sorts before its extensions
    for bad in ((), (1, 2, 3, 4, 5), (0,), (5, 65536), (-1,)):
        with pytest.raises(ValueError):
            pack_key(bad)


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_table_invariants(seed):
    vids, caps, _ = edge_corpus(seed)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS)
    h = d.host
    base = CiderRewarder(caps, vids, SOS, EOS)
    n_refs = sum(len(caps[v]) for v in vids)
    assert h["clip_ref_off"].tolist() == np.cumsum([0] + [len(caps[v]) for v in vids]).tolist()
    assert len(h["ref_len"]) == n_refs and len(h["ref_norm"]) == 4 * n_refs and len(h["ent_off"]) == 4 * n_refs + 1
    assert h["ent_off"][0] == 0 and h["ent_off"][-1] == len(h["ent_keys"]) == len(h["ent_w"]) and np.all(np.diff(h["ent_off"]) >= 0)
    assert np.all(np.diff(h["idf_keys"].astype(object)) > 0) and len(h["idf_keys"]) == len(base.df) == len(h["idf_vals"])
    assert {unpack_key(k) for k in h["idf_keys"]} == set(base.df)
    r = 0
    for v in vids:
        for ci, c in enumerate(caps[v]):
            words = c[1:-1]
            vec, norm, length = cider_vector(base.refs[v][ci], base.df, base.log_n, base.n)
            assert h["ref_len"][r] == length
            assert h["ref_len"][r] == max(len(words) - 1, 0)
            for k in range(4):
                lo, hi = h["ent_off"][4 * r + k], h["ent_off"][4 * r + k + 1]
                keys = h["ent_keys"][lo:hi].astype(object)
                assert np.all(np.diff(keys) > 0)                                      # strictly increasing: unique and sorted
                assert {unpack_key(x) for x in keys} == {tuple(words[i:i + k + 1]) for i in range(len(words) - k)}
                assert h["ref_norm"][4 * r + k] == norm[k]
                assert [vec[k][unpack_key(x)] for x in keys] == h["ent_w"][lo:hi].tolist()
            r += 1
    sigma = 6.0
    assert len(h["pen"]) > max(int(h["ref_len"].max()), capi.CIDER_MAX_T)
    assert h["pen"][0] == 1.0 and h["pen"][7] == np.e ** (-(float(7) ** 2) / (2 * sigma ** 2))
    assert h["idf_vals"].min() == 0.0 and h["idf_vals"].max() == base.log_n - np.log(1.0)  # idf 0 present; df 1 present


def test_constructor_and_lookup_errors():
    vids, caps, _ = random_corpus(3)
    big = dict(caps)
    big[vids[0]] = caps[vids[0]] + [[SOS, 5, 65536, EOS]]
    with pytest.raises(ValueError):
        DeviceCiderRewarder(big, vids, SOS, EOS)
    with pytest.raises(ValueError):
        DeviceCiderRewarder(caps, vids, SOS, EOS, vocab_size=65537)
    with pytest.raises(ValueError):
        DeviceCiderRewarder(caps, vids, SOS, EOS, n=3)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS, vocab_size=65536)
    with pytest.raises(KeyError):
        d.table_walk("no such clip", [5, 6, EOS])
    import torch
    with pytest.raises(capi.S2VTHipError):                       # a host tensor: there is no CPU fallback
        d.rewards([vids[0]], torch.tensor([[5, 6, EOS]]))


@pytest.mark.parametrize("seed,lo,hi", [(3, 5, 14), (11, 5, 14), (12, 5, 12000)])
def test_table_walk_equals_the_host_scorer(seed, lo, hi):
    """the flat table and the kernel's walk over it give CiderRewarder.score: rtol 1e-12 (sums of at most a few hundred non-negative
    float64 terms in another order)"""
    vids, caps, rng = edge_corpus(seed, lo=lo, hi=hi)
    host = CiderRewarder(caps, vids, SOS, EOS)
    d = DeviceCiderRewarder(caps, vids, SOS, EOS)
    T = 24
    cases = edge_candidates(vids, caps, lo, hi, T)
    for v in vids:                                                                     # the recipe's random candidates
        cases.append((v, [int(x) for x in rng.randint(lo, hi, size=rng.randint(1, 7))] + [EOS, 0, 0]))
    cases.append((vids[0], caps[vids[0]][0][1:]))                                      # one exact match
    want = np.array([host.score(v, row) for v, row in cases])
    got = np.array([d.table_walk(v, row) for v, row in cases])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert want[0] == 0.0 == got[0] and want[5] == 0.0 == got[5] and want[7] == 0.0 == got[7]
    assert want.max() > 1.0 and (want > 0).sum() >= 6
