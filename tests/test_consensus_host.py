"""Host-side checks of consensus (MBR) caption selection: the C surface of s2vt_cider_consensus, the host oracle
self_critical.CiderRewarder.consensus against a direct loop over caption_metrics.cider_of_vectors, DeviceCiderRewarder.consensus_walk
(the kernels' walk in numpy) against the oracle, consensus.select's shapes and eval.py's flag.  No device needed; the device side is
tests/test_gpu_consensus.py, which shares the candidate recipe below."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from caption_metrics import cider_of_vectors, cider_vector, ngrams
from s2vt_video_caption_amd import capi, consensus
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder, strip_caption

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cider_reward_host as hc  # noqa: E402

SOS, EOS = hc.SOS, hc.EOS
LO, HI = 5, 14
NEW_SYMBOLS = ("s2vt_cider_consensus_workspace_bytes", "s2vt_cider_consensus")
RTOL, ATOL = 1e-10, 1e-12


# ---- shared with test_gpu_consensus.py
def corpus(seed=3):
    """the corpus of tests/test_cider_reward_host.py (ids LO .. HI, HI in every clip: idf 0) and its two rewarders"""
    vids, caps, rng = hc.edge_corpus(seed, lo=LO, hi=HI)
    return vids, caps, CiderRewarder(caps, vids, SOS, EOS), DeviceCiderRewarder(caps, vids, SOS, EOS)


def candidates(seed, B, K, T, caps):
    """ids [B][K][T] built as test_cider_reward_host builds rows, from the corpus vocabulary so that n-grams overlap: per clip a base
    caption (a reference of the corpus or random words) and K variants of it - the base itself (duplicates), one word replaced, a
    pad inserted, a leading <sos>, a prefix of 0..3 words (0: <eos> first), no <eos> at all, random words, a word outside the corpus"""
    rng = np.random.RandomState(seed)
    refs = [c[1:-1] for v in sorted(caps) for c in caps[v]]
    out = []
    for b in range(B):
        base = list(refs[rng.randint(len(refs))]) if rng.randint(3) else [int(x) for x in rng.randint(LO, HI, size=rng.randint(2, 9))]
        clip = []
        for k in range(K):
            kind = (seed + b + k) % 9 if K > 2 else rng.randint(9)
            w = list(base)
            if kind == 1 and w:
                w[rng.randint(len(w))] = int(rng.randint(LO, HI))
            elif kind == 2:
                w.insert(rng.randint(len(w) + 1), 0)
            elif kind == 3:
                w = [SOS] + w
            elif kind == 4:
                w = w[:rng.randint(4)]                                  # 0, 1, 2 or 3 words
            elif kind == 5:
                w = (w * T)[:T] if w else [LO] * T                      # no <eos>: the whole row counts
            elif kind == 6:
                w = [int(x) for x in rng.randint(LO, HI + 1, size=rng.randint(1, 8))]
            elif kind == 7:
                w = w + [HI + 1 + int(rng.randint(3))]                  # a word the corpus does not hold: idf log_n
            elif kind == 8 and len(w) > 1:
                w = w[1:] + w[:1]
            row = w if kind == 5 else w + [EOS] + [int(x) for x in rng.randint(LO, HI, size=T)]   # behind <eos>: never read
            clip.append((row + [0] * T)[:T])
        out.append(clip)
    return out


def words_of(row):
    return tuple(strip_caption(row, SOS, EOS))


def direct(host, rows, valid=None):
    """the definition, literally: cider_of_vectors of every valid candidate against the other valid ones in ascending order"""
    B, K = len(rows), len(rows[0])
    valid = np.ones((B, K), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    util, best = np.full((B, K), -np.inf), np.zeros(B, dtype=np.int64)
    for b in range(B):
        vec = [cider_vector(ngrams(strip_caption(r, SOS, EOS), 4), host.df, host.log_n, 4) for r in rows[b]]
        top = None
        for i in range(K):
            if not valid[b, i]:
                continue
            others = [vec[j] for j in range(K) if j != i and valid[b, j]]
            util[b, i] = cider_of_vectors(vec[i], others, 4, 6.0) if others else 0.0
            if top is None or util[b, i] > util[b, top]:
                top = i
        best[b] = 0 if top is None else top
    return best, util


def clear_clips(rows, best, util, valid=None, margin=1e-6):
    """bool [B]: clips whose best candidate beats every valid candidate with DIFFERENT words by more than `margin` (and has a valid
    candidate at all): there a utility within the tolerance of the oracle's must choose a caption of the same words"""
    out = np.zeros(len(rows), dtype=bool)
    for b, clip in enumerate(rows):
        ok = [k for k in range(len(clip)) if valid is None or valid[b][k]]
        top = words_of(clip[best[b]])
        out[b] = bool(ok) and all(util[b][best[b]] - util[b][k] > margin for k in ok if words_of(clip[k]) != top)
    return out


# (B, K, T) of the device sweep -> the seed of its candidates, chosen so that at least half of the clips are clear_clips
# (test_sweep_seeds_leave_half_of_every_batch_clear checks that here, with the oracle alone)
SWEEP = {(1, 2, 1): 11, (3, 2, 4): 5, (5, 5, 3): 1, (70, 7, 79): 1, (2, 64, 12): 1, (2, 3, 512): 2}
_CASES = {}


def sweep_case(shape):
    """(rows, oracle best, oracle utility) of one shape of the sweep, computed once per process"""
    if shape not in _CASES:
        vids, caps, host, _ = corpus()
        rows = candidates(SWEEP[shape], shape[0], shape[1], shape[2], caps)
        _CASES[shape] = (rows,) + host.consensus(rows)
    return _CASES[shape]


@pytest.mark.parametrize("shape", sorted(SWEEP))
def test_sweep_seeds_leave_half_of_every_batch_clear(shape):
    rows, best, util = sweep_case(shape)
    B, K, T = shape
    assert len(rows) == B and all(len(c) == K and all(len(r) == T for r in c) for c in rows)
    clear = clear_clips(rows, best, util)
    print(shape, "clear clips %d of %d, max utility %.4f" % (clear.sum(), B, util.max()))
    assert 2 * clear.sum() >= B and util.max() > 1.0
    lens = {len(words_of(r)) for c in rows for r in c}
    assert T < 3 or T in lens                                    # a row without <eos>: all T ids are words
    if B * K >= 25:
        assert {0, 1, 2, 3} <= lens                              # empty orders, zero norms


# ------------------------------------------------------------------ the C surface
def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define S2VT_CONSENSUS_MAX_K %d\b" % capi.CONSENSUS_MAX_K, header) and capi.CONSENSUS_MAX_K == 64
    assert len(capi.SIGNATURES["s2vt_cider_consensus"][1]) == 14


def _table():
    tb = capi.CiderTable()
    for f, _ in capi.CiderTable._fields_[:9]:
        setattr(tb, f, 4096)
    tb.n_idf, tb.n_clips, tb.n_refs, tb.n_pen = 1, 1, 1, 1
    return tb


def test_workspace_query(lib):
    q = lib.s2vt_cider_consensus_workspace_bytes
    assert q(2, 3, 8) > 0 and q(128, 20, 79) >= 128 * 20 * 4 * 79 * 16 and q(1, 64, 512) > q(1, 63, 512) > 0
    for bad in ((0, 3, 8), (-1, 3, 8), (2, 0, 8), (2, 65, 8), (2, 3, 0), (2, 3, 513), (2, -1, 8)):
        assert q(*bad) == 0, bad


def test_bad_arguments_are_rejected_on_the_host(lib):
    """non-null (never dereferenced) pointers: every rejection comes before the first device call"""
    fake = ctypes.c_void_p(4096)
    tb = _table()
    need = lib.s2vt_cider_consensus_workspace_bytes(2, 3, 8)

    def call(table=ctypes.byref(tb), ids=fake, B=2, K=3, T=8, ld=8, valid=None, util=fake, best=fake, ws=fake, nbytes=None):
        nb = lib.s2vt_cider_consensus_workspace_bytes(B, K, T) if nbytes is None else nbytes
        return lib.s2vt_cider_consensus(table, ids, B, K, T, ld, SOS, EOS, valid, util, best, ws, nb or need, None)
    for kw in (dict(table=None), dict(ids=None), dict(util=None), dict(best=None), dict(ws=None),        # null pointers
               dict(K=0), dict(K=65), dict(T=513, ld=1024), dict(T=0), dict(B=0), dict(ld=7),           # dims
               dict(nbytes=need - 1)):                                                                  # one byte short
        assert call(**kw) == -1, kw
        assert lib.s2vt_last_error().decode().startswith("s2vt_cider_consensus:"), (kw, lib.s2vt_last_error())
    tb.pen = None                                                                                        # an incomplete table
    assert call() == -1 and "s2vt_cider_consensus" in lib.s2vt_last_error().decode() and "table" in lib.s2vt_last_error().decode()
    tb = _table()
    tb.idf_vals = None
    assert call(table=ctypes.byref(tb)) == -1 and "table" in lib.s2vt_last_error().decode()


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("seed,B,K,T", [(1, 4, 2, 6), (2, 6, 5, 12), (3, 3, 9, 24)])
def test_oracle_equals_a_direct_loop_over_cider_of_vectors(seed, B, K, T):
    vids, caps, host, _ = corpus()
    rows = candidates(seed, B, K, T, caps)
    rng = np.random.RandomState(seed)
    for valid in (None, rng.rand(B, K) < 0.7):
        want_best, want = direct(host, rows, valid)
        for ids in (rows, np.array(rows), torch.tensor(rows)):
            best, util = host.consensus(ids, valid)
            assert best.dtype == np.int64 and util.dtype == np.float64 and util.shape == (B, K)
            assert np.array_equal(util, want) and np.array_equal(best, want_best)
    assert np.isfinite(want_best).all() and direct(host, rows)[1].max() > 1.0


def test_oracle_edge_cases():
    vids, caps, host, _ = corpus()
    ref = caps[vids[1]][0][1:-1]
    T = 12
    pad = lambda row: (row + [0] * T)[:T]                        # noqa: E731
    best, util = host.consensus([[pad(ref + [EOS])]])                                   # K = 1
    assert best.tolist() == [0] and util.tolist() == [[0.0]]
    best, util = host.consensus([[pad(ref + [EOS])] * 4])                               # all identical
    assert best.tolist() == [0] and util[0].min() > 1.0 and np.ptp(util[0]) <= 1e-12 * util[0].max()
    rows = [[pad(ref + [EOS]), pad([LO, LO + 1, EOS]), pad(ref + [EOS]), pad(ref[:-1] + [EOS])]]
    best, util = host.consensus(rows, [[True, False, True, True]])                      # an invalid candidate: -inf, nobody's reference
    b3, u3 = host.consensus([[rows[0][0], rows[0][2], rows[0][3]]])
    assert util[0, 1] == -np.inf and util[0, [0, 2, 3]].tolist() == u3[0].tolist() and best[0] == [0, 2, 3][b3[0]]
    best, util = host.consensus(rows, [[False, False, False, True]])                    # one valid candidate: no others
    assert best.tolist() == [3] and util[0].tolist() == [-np.inf, -np.inf, -np.inf, 0.0]
    best, util = host.consensus(rows, [[False] * 4])                                    # none valid
    assert best.tolist() == [0] and np.isneginf(util).all()
    best, util = host.consensus([[pad([EOS] + ref), pad(ref + [EOS]), pad(ref + [EOS])]])    # an empty caption: utility 0
    assert util[0, 0] == 0.0 and best.tolist() == [1] and util[0, 1] == util[0, 2] > 0
    with pytest.raises(ValueError):
        host.consensus(rows, [[True] * 3])
    with pytest.raises(ValueError):
        host.consensus([])


# ------------------------------------------------------------------ the kernels' walk in numpy
@pytest.mark.parametrize("seed,B,K,T", [(1, 4, 2, 6), (2, 6, 5, 12), (3, 3, 9, 24), (4, 2, 7, 79)])
def test_consensus_walk_equals_the_oracle(seed, B, K, T):
    vids, caps, host, dev = corpus()
    rows = candidates(seed, B, K, T, caps)
    rng = np.random.RandomState(seed + 100)
    for valid in (None, rng.rand(B, K) < 0.7):
        want_best, want = host.consensus(rows, valid)
        for b in range(B):
            best, util = dev.consensus_walk(rows[b], None if valid is None else valid[b])
            fin = np.isfinite(want[b])
            assert np.array_equal(np.isneginf(util), ~fin)
            np.testing.assert_allclose(util[fin], want[b][fin], rtol=RTOL, atol=ATOL)
            assert best == (np.nonzero(fin)[0][np.argmax(util[fin])] if fin.any() else 0)
            if fin.any():
                assert want[b][best] >= want[b][fin].max() - 2 * (ATOL + RTOL * abs(want[b][fin].max()))
    assert (want[np.isfinite(want)] > 0).sum() >= 2


# ------------------------------------------------------------------ consensus.select
def test_select_flattens_groups_and_refuses_bad_shapes():
    vids, caps, host, _ = corpus()
    B, G, n, T = 3, 2, 3, 10
    rows = torch.tensor(candidates(7, B, G * n, T, caps))
    scores = torch.zeros(B, G, n)
    scores[0, 1, 2], scores[1, 0, 0], scores[2] = float("-inf"), float("nan"), float("inf")
    flat, valid = consensus.flatten_candidates(rows.view(B, G, n, T), scores)
    assert torch.equal(flat, rows) and valid.shape == (B, G * n)
    assert valid[0].tolist() == [True] * 5 + [False] and valid[1].tolist() == [False] + [True] * 5 and not valid[2].any()
    chosen, best, util = consensus.select(host, rows.view(B, G, n, T), scores)
    wb, wu = host.consensus(rows, valid)
    assert best.dtype == torch.int64 and util.dtype == torch.float64 and tuple(chosen.shape) == (B, T) and tuple(util.shape) == (B, G * n)
    assert np.array_equal(best.numpy(), wb) and np.array_equal(util.numpy(), wu) and best[2] == 0
    assert all(torch.equal(chosen[b], rows[b, wb[b]]) for b in range(B))
    c3, b3, u3 = consensus.select(host, rows)                                         # [B, K, T], no scores: all valid
    assert np.array_equal(u3.numpy(), host.consensus(rows)[1]) and torch.equal(c3, rows[torch.arange(B), b3])
    for bad_ids, bad_scores in ((rows[0], None), (rows.view(B, 1, G, n, T), None), (rows.tolist(), None), (rows, torch.zeros(B, G, n)),
                                (rows.view(B, G, n, T), torch.zeros(B, G * n)), (rows[:, :0], None)):
        with pytest.raises(ValueError, match="consensus.select"):
            consensus.select(host, bad_ids, bad_scores)


def test_device_paths_refuse_host_tensors():
    vids, caps, _, dev = corpus()
    ids = torch.tensor(candidates(1, 2, 3, 6, caps))
    with pytest.raises(capi.S2VTHipError):                       # there is no CPU fallback behind the device rewarder
        dev.consensus(ids)
    with pytest.raises(capi.S2VTHipError):
        consensus.select(dev, ids)


# ------------------------------------------------------------------ eval.py --consensus
def test_eval_refuses_the_flag_without_candidates():
    sys.path.insert(0, ROOT)
    import eval as ev
    assert ev.build_parser().parse_args(["--model-path", "m.pth"]).consensus is False
    base = ["--model-path", "m.pth", "--consensus"]
    for bad in (base,                                                                        # alone
                base + ["--sample", "1"], base + ["--beam", "3"],                            # one candidate; the reference's search
                base + ["--beam", "3", "--beam-mode", "cumulative"],                         # n-best 1
                base + ["--beam", "3", "--beam-mode", "cumulative", "--beam-groups", "1"],
                base + ["--beam", "4", "--beam-mode", "cumulative", "--n-best", "2", "--sample", "3"],    # two sources
                base + ["--sample", "3", "--perplexity"]):
        with pytest.raises(SystemExit):
            ev.main(bad)


def test_eval_routes_the_flag(monkeypatch, tmp_path):
    """main() with the flag: the beam sources take their prediction from consensus_captions, --sample keeps generate's; without the
    flag neither consensus_captions nor a consensus file appears"""
    import json
    sys.path.insert(0, ROOT)
    import eval as ev
    calls = []

    def fake_consensus(model_path, caption_file, feats_path, source, batch_size=10, **kw):
        calls.append((source, kw))
        det = {"v": {"chosen": 1, "utility": [0.5, 1.5], "captions": ["a", "b"]}}
        return {"v": "b"}, det, (None if source == "sample" else {"v": [-1.0, float("-inf")]})
    monkeypatch.setattr(ev, "consensus_captions", fake_consensus)
    monkeypatch.setattr(ev, "generate", lambda *a, **kw: {"v": "greedy"})
    monkeypatch.setattr(ev, "sample_captions", lambda *a, **kw: {"v": ["a", "b"]})
    load = lambda p: json.load(open(p))                          # noqa: E731
    out = str(tmp_path / "s.json")
    ev.main(["--model-path", "m.pth", "--sample", "2", "--consensus", "--sample-seed", "5", "--out", out])
    assert calls[-1][0] == "sample" and calls[-1][1]["n_samples"] == 2 and calls[-1][1]["seed"] == 5
    assert load(out) == {"v": "greedy"} and load(out + ".samples.json") == {"v": ["a", "b"]}
    assert load(out + ".consensus.json") == {"v": {"chosen": 1, "utility": [0.5, 1.5], "captions": ["a", "b"]}}
    out = str(tmp_path / "n.json")
    ev.main(["--model-path", "m.pth", "--beam", "4", "--beam-mode", "cumulative", "--n-best", "2", "--consensus", "--out", out])
    assert calls[-1][0] == "nbest" and calls[-1][1]["n_best"] == 2 and calls[-1][1]["beam_width"] == 4
    assert load(out) == {"v": "b"} and load(out + ".nbest.json") == {"v": ["a", "b"]} and os.path.exists(out + ".consensus.json")
    out = str(tmp_path / "g.json")
    ev.main(["--model-path", "m.pth", "--beam", "4", "--beam-mode", "cumulative", "--beam-groups", "2", "--consensus", "--out", out])
    assert calls[-1][0] == "groups" and calls[-1][1]["beam_groups"] == 2 and calls[-1][1]["diversity_lambda"] == 0.5
    assert load(out) == {"v": "b"}
    assert load(out + ".groups.json") == {"v": [{"caption": "a", "score": -1.0}, {"caption": "b", "score": None}]}
    n = len(calls)
    out = str(tmp_path / "p.json")
    ev.main(["--model-path", "m.pth", "--sample", "2", "--out", out])
    assert len(calls) == n and load(out) == {"v": "greedy"} and not os.path.exists(out + ".consensus.json")
