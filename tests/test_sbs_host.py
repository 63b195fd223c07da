"""Host-side checks of stochastic beam search (S2VT.sample_distinct): the numpy restatement (tests/sbs_ref.py) against itself and
against the distribution it must sample, the surface (argument errors, refusals, symbols, eval.py's parser), and the CPU
preconditions of tests/test_gpu_sbs.py (the policy cases' reference gaps, the whole-path cases' share of decided clips)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi, sampling

import beam_cum_ref
import sbs_ref
from test_sampling_host import CHI2_BOUND, DIST_LOGITS, DIST_V, SEEDS, chi_square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- shared with test_gpu_sbs.py
PATH_CASES = (("tiny5", 4, 2.5), ("tiny5", 8, 2.5), ("mid64", 5, 4.0))     # (case of beam_cum_ref, W, what out_linear.bias[eos] is raised by)
PATH_D, PATH_SEED = 12, 2024
MAX_UNDECIDED = 0.25
POLICY_B, POLICY_D, POLICY_WS = 7, 6, (1, 3, 8)
POLICY_SEED = 5
POLICY_MIN_GAP = 1e-9
DIST_W, DIST_ROWS = 3, 64


def path_inputs(name, bump):
    sd, feats, _, _ = beam_cum_ref.case_inputs(name)
    sd["out_linear.bias"][beam_cum_ref.EOS] += bump
    return sd, feats


_PATHS = {}


def path_search(name, W, bump):
    """search_fp64 of a whole-path case - computed once per process, shared by the tests, never modified"""
    key = (name, W)
    if key not in _PATHS:
        sd, feats = path_inputs(name, bump)
        _PATHS[key] = sbs_ref.search_fp64(sd, feats, W, PATH_D, 1.0, PATH_SEED)
    return _PATHS[key]


def policy_case(W, seed=POLICY_SEED, B=POLICY_B, D=POLICY_D):
    """Synthetic per-depth head outputs for the policy alone: per depth (top_ix int32 [B*W, 20], top_lp fp32, top_g fp32), every row
    a head's output (20 distinct words, g descending).  <eos> is planted at random so that slots finish at mixed depths (none at depth
    D: some samples stay unfinished).  Clip 1 finishes everything at depth 2: at depth 1 its second-best child is <eos> and no other,
    at depth 2 the best child of every row is <eos> and the others lie 40 below it, so that no second child of one parent overtakes
    the best child of another.  In clip 2 nothing ends at depth 1 and the rows of slots 0 and 1 carry the SAME g at depth 2: two
    parents whose best children have the same g - their G~ are the parents' own scores."""
    rng = np.random.RandomState(seed * 100 + W)
    R = B * W
    eos = sbs_ref.EOS
    depths = []
    for t in range(1, D + 1):
        ix = np.stack([rng.permutation(50)[:20] + 5 for _ in range(R)]).astype(np.int32)          # words 5..54: never <eos>
        lp = -(rng.exponential(2.0, size=(R, 20)) + 0.05).astype(np.float32)
        g = -np.sort(-(rng.gumbel(size=(R, 20)) * 1.5).astype(np.float32), axis=1)
        plant = rng.rand(R, 20) < (0.08 if t < D else 0.0)
        if t <= 2:
            plant[1 * W:2 * W] = False
        if t == 1:
            plant[2 * W:3 * W] = False
        for r in np.nonzero(plant.any(axis=1))[0]:                      # (a row holds a word once: one <eos> at most)
            ix[r, np.argmax(plant[r])] = eos
        if t == 1:
            ix[1 * W, 1] = eos
        if t == 2:
            ix[1 * W:2 * W, 0] = eos
            g[1 * W:2 * W, 1:] -= np.float32(40)
            if W >= 2:
                g[2 * W + 1] = g[2 * W]
        depths.append((np.ascontiguousarray(ix), np.ascontiguousarray(lp), np.ascontiguousarray(g)))
    return depths


def run_policy_ref(W, depths, B=POLICY_B, D=POLICY_D):
    """PolicyF64 over a policy case: (policy, rows after every call [D + 1][2][B*W], frozen counts after every call)"""
    pol = sbs_ref.PolicyF64(B, W, D)
    rows, frozen = [pol.rows()], [0]
    for ix, lp, g in depths:
        pol.step(ix, lp, g)
        rows.append(pol.rows())
        frozen.append(int(pol.frozen().sum()))
    return pol, rows, frozen


def dist_head(seed):
    """the float64 head of the distribution check for one call seed: rows b * W (slot 0 of DIST_ROWS clips), step 0"""
    logits = np.tile(DIST_LOGITS[None, :], (DIST_ROWS, 1))
    return sbs_ref.head_ref(logits, 1.0, seed, 0, np.arange(DIST_ROWS) * DIST_W)[:3]


def spread(top, R, rows):
    """a head's output for `rows` (slot 0 of every clip) spread into the [R, 20] array of the policy (other rows: zeros)"""
    out = np.zeros((R, 20), dtype=top.dtype)
    out[rows] = top
    return out


# ------------------------------------------------------------------ the reference against itself
def test_cond_gumbel_identities():
    G = -1.25
    g = np.array([0.7, 0.7 - 1e-12, 0.2, -3.0, -40.0, -800.0])
    gt = sbs_ref.cond_gumbel(G, 0.7, g)
    assert gt[0] == G                                                   # the best child inherits the parent's score exactly
    assert np.all(np.diff(gt) < 0) and np.all(gt <= G)                  # increasing in g, never above the parent
    naive = -np.log(np.exp(-G) - np.exp(-0.7) + np.exp(-g[2:4]))
    assert np.allclose(gt[2:4], naive, rtol=1e-12)
    assert np.isfinite(gt).all()                                        # far below the maximum: no overflow, no -inf
    assert sbs_ref.cond_gumbel(0.0, 3.0, 3.0) == 0.0 and sbs_ref.cond_gumbel(-5.5, -2.0, -2.0) == -5.5


@pytest.mark.parametrize("name,W,bump", PATH_CASES[:2])
def test_reference_properties(name, W, bump):
    res = path_search(name, W, bump)
    for r in res:
        assert len(r["ids"]) == W
        assert len(set(tuple(x) for x in r["ids"])) == W                # pairwise distinct
        G = np.array(r["G"])
        assert np.all(np.diff(G) <= 0) and np.all(G <= 0)
        assert r["kappa"] <= G[W - 1]
        for toks, lp in zip(r["ids"], r["logprob"]):
            assert 1 <= len(toks) <= PATH_D and lp <= 0
            assert beam_cum_ref.EOS not in toks[:-1]
            assert len(toks) == PATH_D or toks[-1] == beam_cum_ref.EOS


def test_one_sample_is_the_ancestral_gumbel_max_draw():
    sd, feats = path_inputs("tiny5", 2.5)
    res = sbs_ref.search_fp64(sd, feats, 1, PATH_D, 0.8, 77)
    want = sbs_ref.ancestral_fp64(sd, feats, PATH_D, 0.8, 77)
    assert [r["ids"][0] for r in res] == want
    assert any(len(w) < PATH_D for w in want) and any(len(w) > 1 for w in want)


def test_policy_on_the_heads_top20_is_the_search_over_all_children():
    """PolicyF64 over head_ref's 20 best per row gives what search_fp64 gives over all V children: the fan-out of 20 is exact"""
    sd, feats = path_inputs("tiny5", 2.5)
    W = 8
    res = path_search("tiny5", W, 2.5)
    # replay: the logits along the policy's own rows, from the float64 model
    from oracle import s2vt_oracle as oracle
    p = {k: v.double() for k, v in sd.items()}
    f = feats.double()
    B, L, _ = f.shape
    x1 = f @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    R = B * W
    tab_h, tab_c = x1.new_zeros(R, x1.shape[2]), x1.new_zeros(R, x1.shape[2])
    tab_h[:B], tab_c[:B] = h2, c2
    pol = sbs_ref.PolicyF64(B, W, PATH_D)
    for t in range(1, PATH_D + 1):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        rows = pol.rows()
        st, tok = torch.from_numpy(rows[0].astype(np.int64)), torch.from_numpy(rows[1].astype(np.int64))
        nh, nc = oracle._word_step(p, p["embedding.weight"][tok], h1.repeat_interleave(W, 0), tab_h[st], tab_c[st])
        tab_h, tab_c = nh, nc
        logits = (nh @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy()
        ix, lp, g, _, _ = sbs_ref.head_ref(logits, 1.0, PATH_SEED, t - 1, np.arange(R))
        pol.step(ix, lp.astype(np.float32), g.astype(np.float32))
    ids, lens, lp, G, kappa = pol.result()
    for b, r in enumerate(res):
        if r["gap"] < beam_cum_ref.ROBUST_GAP:
            continue
        assert [ids[b, k, :lens[b, k]].tolist() for k in range(W)] == r["ids"], b
        assert np.allclose(G[b], r["G"], atol=1e-4) and np.isclose(kappa[b], r["kappa"], atol=1e-4)


# ------------------------------------------------------------------ the distribution
def test_first_sample_follows_the_softmax_chi_square():
    """W = 3, D = 1 on the fixed logits: slot 0's word is distributed as softmax(logits) (the first draw of sampling without
    replacement is a draw with replacement), and the three words of a row are distinct"""
    p = np.exp(DIST_LOGITS - DIST_LOGITS.max())
    p /= p.sum()
    counts = np.zeros(DIST_V)
    R = DIST_ROWS * DIST_W
    rows0 = np.arange(DIST_ROWS) * DIST_W
    for s in SEEDS:
        ix, lp, g = dist_head(s)
        pol = sbs_ref.PolicyF64(DIST_ROWS, DIST_W, 1)
        pol.step(spread(ix.astype(np.int32), R, rows0), spread(lp.astype(np.float32), R, rows0), spread(g.astype(np.float32), R, rows0))
        ids, lens, _, G, kappa = pol.result()
        assert np.all(lens == 1)
        w = ids[:, :, 0]
        assert np.all(w[:, 0] != w[:, 1]) and np.all(w[:, 0] != w[:, 2]) and np.all(w[:, 1] != w[:, 2])
        assert np.all(kappa <= G[:, -1])
        counts += np.bincount(w[:, 0], minlength=DIST_V)
    assert counts.sum() == DIST_ROWS * len(SEEDS)
    stat = chi_square(counts, p)
    print("chi2 = %.2f (bound %.2f), N = %d" % (stat, CHI2_BOUND, counts.sum()))
    assert stat < CHI2_BOUND


# ------------------------------------------------------------------ CPU preconditions of the GPU tests
@pytest.mark.parametrize("W", POLICY_WS)
def test_policy_cases_have_no_close_decision(W):
    """the policy test excuses a clip whose reference gap is below 1e-9: with these seeds there is none, so nothing is excused; and
    the cases do what they claim (mixed finishing depths, one clip frozen at depth 2, the tie of two parents' best children)"""
    depths = policy_case(W)
    pol, rows, frozen = run_policy_ref(W, depths)
    assert pol.gap.min() >= POLICY_MIN_GAP, pol.gap
    ids, lens, lp, G, kappa = pol.result()
    assert frozen[2] >= 1 and pol.frozen()[1] and np.all(lens[1] <= 2)  # clip 1 finished everything at depth 2
    assert len(np.unique(lens)) >= (3 if W > 1 else 2)                  # mixed lengths
    assert np.all(np.diff(G, axis=1) <= 0) and np.all(kappa <= G[:, -1])
    if W >= 2:
        assert np.array_equal(depths[1][2][2 * W], depths[1][2][2 * W + 1])


@pytest.mark.parametrize("name,W,bump", PATH_CASES)
def test_whole_path_cases_are_mostly_decided(name, W, bump):
    """at most 25 % of a case's clips may be undecided (smallest gap below beam_cum_ref.ROBUST_GAP) - met by the reference alone;
    and some clips stop before depth 12, so the device's early stop is exercised against a reference without one"""
    res = path_search(name, W, bump)
    undecided = sum(r["gap"] < beam_cum_ref.ROBUST_GAP for r in res)
    stopped = sum(r["stopped"] is not None for r in res)
    print("%s W=%d: %d/%d undecided, %d stopped early" % (name, W, undecided, len(res), stopped))
    assert undecided <= MAX_UNDECIDED * len(res)
    assert stopped >= 1


# ------------------------------------------------------------------ surface
NEW_SYMBOLS = ("s2vt_top20_gumbel", "s2vt_beam_step_gumbel", "s2vt_sbs_bytes", "s2vt_sbs_step", "s2vt_sbs_result")


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header) and name in capi.SIGNATURES and hasattr(lib, name), name
    assert lib.s2vt_abi_version() == 9 == capi.ABI_VERSION
    assert "stochastic beam" in header
    from s2vt_video_caption_amd import build, ops
    assert "gumbel_top.hip" in build.SOURCES and "sbs_policy.hip" in build.SOURCES
    assert callable(ops.top20_gumbel) and callable(ops.sbs_step) and callable(ops.sbs_result)
    assert lib.s2vt_sbs_bytes(4, 5, 30) > 0
    for bad in ((0, 5, 30), (4, 0, 30), (4, 9, 30), (4, 5, 0)):
        assert lib.s2vt_sbs_bytes(*bad) == 0, bad


def test_library_refuses_bad_arguments_on_the_host(lib):
    import ctypes
    fake = ctypes.c_void_p(4096)
    for args in ((None, 64, 2, 50, 1.0, 1, 0, 0, fake, fake, fake), (fake, 64, 2, 19, 1.0, 1, 0, 0, fake, fake, fake),
                 (fake, 40, 2, 50, 1.0, 1, 0, 0, fake, fake, fake), (fake, 64, 2, 50, 0.0, 1, 0, 0, fake, fake, fake),
                 (fake, 64, 2, 50, float("nan"), 1, 0, 0, fake, fake, fake), (fake, 64, 2, 50, float("inf"), 1, 0, 0, fake, fake, fake),
                 (fake, 64, 2, 50, 1.0, 1, -1, 0, fake, fake, fake), (fake, 64, 2, 50, 1.0, 1, 0, 0, fake, fake, None),
                 (fake, 40000, 2, 38401, 1.0, 1, 0, 0, fake, fake, fake)):
        assert lib.s2vt_top20_gumbel(*args, None) == -1, args
        assert lib.s2vt_last_error().decode().startswith("s2vt_top20_gumbel:")
    n = lib.s2vt_sbs_bytes(2, 3, 4)
    assert lib.s2vt_sbs_step(2, 3, 4, 3, 4, 1, None, n, None, None, None, fake, fake, fake, None) == -1
    assert lib.s2vt_last_error().decode().startswith("s2vt_sbs_step:")
    assert lib.s2vt_sbs_step(2, 3, 4, 3, 4, 1, fake, n - 1, None, None, None, fake, fake, fake, None) == -1
    assert lib.s2vt_sbs_step(2, 3, 4, 3, 4, 2, fake, n, fake, fake, None, fake, fake, fake, None) == -1       # no top_g
    assert lib.s2vt_sbs_step(2, 3, 4, 3, 4, 5, fake, n, fake, fake, fake, fake, fake, fake, None) == -1       # depth > max_depth
    assert lib.s2vt_sbs_step(2, 9, 4, 3, 4, 1, fake, n, None, None, None, fake, fake, fake, None) == -1
    assert lib.s2vt_sbs_result(2, 3, 4, 4, fake, n, fake, fake, fake, fake, None, None) == -1
    assert lib.s2vt_last_error().decode().startswith("s2vt_sbs_result:")


def _model(**kw):
    import S2VTModel
    return S2VTModel.S2VT(vocab_size=kw.pop("V", 30), feat_dim=16, length=6, dim_hid=8, dim_embed=8, **kw)


def test_sample_distinct_checks_its_arguments_before_the_library():
    import S2VTModel
    sig = inspect.signature(S2VTModel.S2VT.sample_distinct)
    assert list(sig.parameters) == ["self", "feats", "n_samples", "temperature", "seed", "max_depth"]
    assert [sig.parameters[k].default for k in ("n_samples", "temperature", "seed", "max_depth")] == [5, 1.0, None, 30]
    assert list(inspect.signature(S2VTModel.S2VT.sample).parameters) == ["self", "feats", "n_samples", "temperature", "seed"]      # pinned
    m = _model()
    feats = torch.zeros(2, 6, 16)                                       # a CPU tensor: every refusal below comes before it is looked at
    for kw in (dict(n_samples=0), dict(n_samples=9), dict(n_samples=2.0), dict(n_samples="3"), dict(n_samples=True),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(temperature="1"), dict(max_depth=0), dict(max_depth=-3), dict(max_depth=2.5), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            m.sample_distinct(feats, **dict(dict(seed=1), **kw))
    with pytest.raises(ValueError, match="vocab_size"):
        _model(V=19).sample_distinct(feats, seed=1)
    with pytest.raises(ValueError, match="sample"):
        _model(rnn_type="gru").sample_distinct(feats, seed=1)
    with pytest.raises(ValueError, match="sample"):
        _model(num_layers=2).sample_distinct(feats, seed=1)
    with pytest.raises(capi.S2VTHipError):                              # valid arguments: the first thing refused is the CPU tensor
        m.sample_distinct(feats, seed=1)
    torch.manual_seed(5)
    a = beam.check_stochastic_args(5, 1.0, None, 30, 30)[2]
    torch.manual_seed(5)
    assert beam.check_stochastic_args(5, 1.0, None, 30, 30)[2] == a == (torch.manual_seed(5), sampling.draw_seed())[1]
    assert beam.check_stochastic_args(np.int64(3), 0.5, 9, np.int32(4), 30) == (3, 0.5, 9, 4)
    assert beam.inv_temperature(0.7) == float(np.float32(1.0) / np.float32(0.7)) == sbs_ref.inv_temperature(0.7)


def test_eval_parser():
    sys.path.insert(0, ROOT)
    import eval as ev
    assert ev.build_parser().parse_args(["--model-path", "m.pth"]).sample_distinct is False
    a = ev.build_parser().parse_args(["--model-path", "m.pth", "--sample", "4", "--sample-distinct", "--temperature", "0.7"])
    assert a.sample_distinct is True and a.sample == 4
    base = ["--model-path", "m.pth", "--sample-distinct"]
    for bad in (base,                                                   # no --sample
                base + ["--sample", "9"],                               # K > 8
                base + ["--sample", "4", "--top-k", "5"], base + ["--sample", "4", "--top-p", "0.9"],
                base + ["--sample", "4", "--no-repeat-ngram", "2"], base + ["--sample", "4", "--repetition-penalty", "1.2"],
                base + ["--sample", "4", "--min-length", "3"], base + ["--sample", "4", "--ban-words", "<unk>"]):
        with pytest.raises(SystemExit):                                 # refused before a model is loaded
            ev.main(bad)
    assert inspect.signature(ev.sample_captions).parameters["distinct"].default is False
    assert inspect.signature(ev.consensus_captions).parameters["distinct"].default is False
