"""GPU: stochastic beam search, S2VT.sample_distinct (csrc/gumbel_top.hip + csrc/sbs_policy.hip + beam.stochastic).

The fan-out head is compared by value with the float64 restatement (tests/sbs_ref.head_ref); the policy kernel alone, over synthetic
head outputs, with the numpy restatement of the definition (sbs_ref.PolicyF64: bitwise in ids, lengths and log-probs); the whole path
with the float64 search without early stop on every clip whose decisions are clear (tests/test_sbs_host.py caps how many may be left
out); then the properties a caller relies on, the distribution of the first sample, and eval.py --sample-distinct."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref  # noqa: E402
import sbs_ref as ref  # noqa: E402
import test_sbs_host as host  # noqa: E402
from test_sampling_host import CHI2_BOUND, DIST_LOGITS, DIST_V, NOISE_TOL, SEEDS, chi_square, eps_for, replay_sample_fp64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LP_TOL = 5e-6          # what tests/test_gpu_kernels.py grants top20_logprob's log-probs against float64
SCORE_TOL = 1e-4       # what tests/test_gpu_beam_cum.py grants mode='beam''s scores against float64
SCORE_VS_SEARCH = 2e-4  # what tests/test_gpu_score.py grants mode='score' against a search's scores (each side within 1e-4 of float64)


def _model(dims, sd, **kw):
    import S2VTModel
    B, L, F, H, E, V = dims
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ 1. the head by value
HEAD_SHAPES = [(5, 20), (3, 50), (4, 4096), (4, 4097), (2, 12289), (2, 16385)]      # V = 20: every word is returned; both sides of a
HEAD_STEP, HEAD_ROW0, HEAD_SEED = 3, 11, (7 << 32) + 12345                           # RegRow boundary; the LDS form


@pytest.mark.parametrize("rows,V", HEAD_SHAPES)
def test_head_by_value(lib, rows, V):
    inv_t = ref.inv_temperature(0.7)
    x = (np.random.RandomState(1000 + V).randn(rows, V + 7)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)[:, :V]                              # ld = V + 7 > V
    assert xd.stride(0) == V + 7
    ix, lp, g = ops.top20_gumbel(xd, inv_t, HEAD_SEED, HEAD_STEP, HEAD_ROW0)
    again = ops.top20_gumbel(xd, inv_t, HEAD_SEED, HEAD_STEP, HEAD_ROW0)
    assert all(torch.equal(a, b) for a, b in zip((ix, lp, g), again))    # the same inputs give the same bits
    assert ix.dtype == torch.int32 and lp.dtype == g.dtype == torch.float32 and tuple(ix.shape) == tuple(lp.shape) == tuple(g.shape) == (rows, 20)
    ix, lp, g = ix.cpu().numpy().astype(np.int64), lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    rix, rlp, rg, lp64, g64 = ref.head_ref(x[:, :V], inv_t, HEAD_SEED, HEAD_STEP, HEAD_ROW0 + np.arange(rows))
    # values at the device's own ids, on every row
    assert (ix >= 0).all() and (ix < V).all() and all(len(set(r)) == 20 for r in ix.tolist())
    e_lp = float(np.abs(lp - np.take_along_axis(lp64, ix, 1)).max())
    e_g = float(np.abs(g - np.take_along_axis(g64, ix, 1)).max())
    print("%d x %d: max |top_lp - fp64| = %.3g, max |top_g - fp64| = %.3g" % (rows, V, e_lp, e_g))
    assert e_lp <= LP_TOL and e_g <= LP_TOL + NOISE_TOL
    assert (lp <= 0).all()
    # output order: strictly (g descending, v ascending)
    dg = np.diff(g, axis=1)
    assert (dg <= 0).all() and (np.diff(ix, axis=1)[dg == 0] > 0).all()
    # the ranked ids wherever the reference's adjacent gaps, the 20th / 21st included, exceed twice the tolerance of g
    srt = -np.sort(-g64, axis=1)[:, :21]
    decided = (-np.diff(srt, axis=1) > 2 * (LP_TOL + NOISE_TOL))
    if V == 20:
        assert sorted(ix[0].tolist()) == list(range(20))
    n_ok = 0
    for r in range(rows):
        upto = 20 if decided[r].all() else int(np.argmin(decided[r]))    # the prefix in front of the first close pair
        assert ix[r, :upto].tolist() == rix[r, :upto].tolist(), r
        n_ok += upto == 20
    assert n_ok == rows                                                  # (seeded inputs: no close pair, nothing is excused)


def test_head_noise_is_keyed_by_row_step_and_seed(lib):
    x = torch.from_numpy((np.random.RandomState(5).randn(6, 300)).astype(np.float32)).to(DEV)
    base = ops.top20_gumbel(x, 1.0, 9, 2, 4)
    assert all(torch.equal(a[2:], b[:4]) for a, b in zip(base, ops.top20_gumbel(x[2:], 1.0, 9, 2, 6)))   # a row's draw, wherever it is launched
    for other in (ops.top20_gumbel(x, 1.0, 10, 2, 4), ops.top20_gumbel(x, 1.0, 9, 3, 4), ops.top20_gumbel(x, 1.0, 9 + (1 << 32), 2, 4)):
        assert not torch.equal(base[0], other[0])


# ------------------------------------------------------------------ 2. the policy kernel alone
def _drive_policy(W, depths, B, D):
    """the device policy over a case: (rows after every call, frozen counter after every call, result on the host)"""
    state, rows = ops.sbs_state(B, W, D, torch.device(DEV))
    counter = state[:4].view(torch.int32)
    got_rows, got_frozen = [], []
    ops.sbs_step(state, rows, B, W, D, ref.SOS, ref.EOS, 1)
    got_rows.append(rows.cpu().numpy().copy())
    got_frozen.append(int(counter.item()))
    for t, (ix, lp, g) in enumerate(depths, start=1):
        ops.sbs_step(state, rows, B, W, D, ref.SOS, ref.EOS, 0 if t == D else t + 1, torch.from_numpy(ix).to(DEV),
                     torch.from_numpy(lp).to(DEV), torch.from_numpy(g).to(DEV))
        got_rows.append(rows.cpu().numpy().copy())
        got_frozen.append(int(counter.item()))
    return got_rows, got_frozen, [t.cpu().numpy() for t in ops.sbs_result(state, B, W, D, ref.EOS)]


@pytest.mark.parametrize("W", host.POLICY_WS)
def test_policy_exact(lib, W):
    B, D = host.POLICY_B, host.POLICY_D
    depths = host.policy_case(W)
    pol, want_rows, want_frozen = host.run_policy_ref(W, depths)
    assert pol.gap.min() >= host.POLICY_MIN_GAP                          # nothing is excused (tests/test_sbs_host.py holds the seeds to it)
    rows, frozen, (ids, lens, lp, G, kappa) = _drive_policy(W, depths, B, D)
    for t in range(D + 1):
        assert (rows[t][0] == np.repeat(np.arange(B), W)).all()
        assert np.array_equal(rows[t][1:], want_rows[t]), t              # state rows and tokens, 0 where a slot is not live
        assert frozen[t] == want_frozen[t], (t, frozen, want_frozen)
    wids, wlens, wlp, wG, wkappa = pol.result()
    assert np.array_equal(ids, wids) and np.array_equal(lens, wlens)
    assert np.array_equal(lp.view(np.uint32), wlp.view(np.uint32))       # the fp32 sums, bit for bit
    assert np.allclose(G, wG, rtol=1e-6, atol=0) and np.allclose(kappa, wkappa, rtol=1e-6, atol=0)
    assert frozen[-1] >= 1 and frozen[2] >= 1 and frozen[-1] < B         # a clip stopped at depth 2; some never stop


# ------------------------------------------------------------------ 3. the whole path against the float64 search
@pytest.mark.parametrize("name,W,bump", host.PATH_CASES)
def test_whole_path_against_the_restatement(lib, name, W, bump):
    want = host.path_search(name, W, bump)
    decided = np.array([r["gap"] >= beam_cum_ref.ROBUST_GAP for r in want])
    assert (~decided).sum() <= host.MAX_UNDECIDED * len(want)
    sd, feats = host.path_inputs(name, bump)
    m = _model(beam_cum_ref.CASES[name][0], sd)
    D = host.PATH_D
    out = m.sample_distinct(feats.to(DEV), n_samples=W, temperature=1.0, seed=host.PATH_SEED, max_depth=D)
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.float32, torch.float32, torch.float32]
    assert all(t.device.type == "cuda" for t in out)
    B = feats.shape[0]
    assert [tuple(t.shape) for t in out] == [(B, W, D), (B, W), (B, W), (B, W), (B,)]
    ids, lens, lp, G, kappa = [t.cpu().numpy() for t in out]
    e_lp = e_G = e_k = 0.0
    for b in np.nonzero(decided)[0]:
        assert [ids[b, k, :lens[b, k]].tolist() for k in range(W)] == want[b]["ids"], b
        assert (ids[b][np.arange(D)[None, :] >= lens[b][:, None]] == ref.EOS).all()       # padded with <eos>
        e_lp = max(e_lp, float(np.abs(lp[b] - np.array(want[b]["logprob"])).max()))
        e_G = max(e_G, float(np.abs(G[b] - np.array(want[b]["G"])).max()))
        e_k = max(e_k, abs(float(kappa[b]) - want[b]["kappa"]))
    stopped = sum(r["stopped"] is not None for r in want)
    print("%s W=%d: %d/%d clips decided and identical (%d stop early), max |logprob - fp64| %.3g, |perturbed - fp64| %.3g, |kappa - fp64| %.3g"
          % (name, W, int(decided.sum()), B, stopped, e_lp, e_G, e_k))
    assert e_lp <= SCORE_TOL and e_G <= SCORE_TOL and e_k <= SCORE_TOL
    capi.check_async_error(True)


# ------------------------------------------------------------------ 4. properties on the device
def _tiny():
    sd, feats = host.path_inputs("tiny5", 2.5)
    return sd, feats, _model(beam_cum_ref.CASES["tiny5"][0], sd)


def test_properties(lib):
    sd, feats, m = _tiny()
    f = feats.to(DEV)
    B, L, W = f.shape[0], f.shape[1], 5
    D = L - 1                                                            # (mode='score' takes captions of at most L tokens)
    out = m.sample_distinct(f, n_samples=W, temperature=1.0, seed=31, max_depth=D)
    ids, lens, lp, G, kappa = out
    rows = ids.cpu().numpy()
    for b in range(B):
        assert len(set(tuple(r) + (int(n),) for r, n in zip(rows[b].tolist(), lens[b].tolist()))) == W      # pairwise distinct
    Gh = G.cpu().numpy()
    assert (np.diff(Gh, axis=1) <= 0).all() and (Gh <= 0).all() and (kappa.cpu().numpy() <= Gh[:, -1]).all()
    assert (lp.cpu().numpy() <= 0).all() and int(lens.min()) >= 1 and int(lens.max()) <= D
    assert len(set(lens.flatten().tolist())) >= 2                        # finished at mixed depths
    # logprobs = mode='score' of the returned captions (temperature 1, plain sums)
    caps = torch.cat([torch.full((B, W, 1), ref.SOS, dtype=torch.long, device=DEV), ids], dim=2)
    scores, slen, _ = m(f, targets=caps, mode="score", length_alpha=0.0)
    assert torch.equal(slen, lens)
    e = float((scores - lp).abs().max())
    print("max |logprob - mode='score'| = %.3g" % e)
    assert e <= SCORE_VS_SEARCH
    # the same seed gives the same bits, another seed other captions
    again = m.sample_distinct(f, n_samples=W, temperature=1.0, seed=31, max_depth=D)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    other = m.sample_distinct(f, n_samples=W, temperature=1.0, seed=32, max_depth=D)
    assert not torch.equal(other[0], ids)
    torch.manual_seed(3)
    a = m.sample_distinct(f, n_samples=2, max_depth=D)
    torch.manual_seed(3)
    assert all(torch.equal(x, y) for x, y in zip(a, m.sample_distinct(f, n_samples=2, max_depth=D)))      # seed=None draws one, as sample does
    capi.check_async_error(True)


@pytest.mark.parametrize("temperature", [1.0, 0.6])
def test_one_sample_is_the_sampled_decode_up_to_the_first_eos(lib, temperature):
    sd, feats = host.path_inputs("tiny5", 1.0)                           # (<eos> raised less: draws of 2 to 7 words)
    m = _model(beam_cum_ref.CASES["tiny5"][0], sd)
    f = feats.to(DEV)
    B, L = f.shape[0], f.shape[1]
    D, seed = L - 1, 909
    ids, lens, lp, G, kappa = [t.cpu().numpy() for t in m.sample_distinct(f, n_samples=1, temperature=temperature, seed=seed, max_depth=D)]
    drawn = m.sample(f, 1, temperature, seed).cpu().numpy()[:, 0]
    want, marg = replay_sample_fp64(sd, feats, seed, temperature)
    want = want.numpy()
    checked = 0
    for b in range(B):
        w = want[b].tolist()
        n = w.index(ref.EOS) + 1 if ref.EOS in w else D
        if marg[b, :n].min() < eps_for(temperature):
            continue
        checked += 1
        assert lens[b, 0] == n and ids[b, 0, :n].tolist() == w[:n] == drawn[b, :n].tolist(), b
        assert (ids[b, 0, n:] == ref.EOS).all()
    assert checked == B                                                  # (this seed: every row's float64 margins are clear)
    assert (G[:, 0] == 0).all()                                          # the best child inherits the root's score exactly, at every depth


# ------------------------------------------------------------------ 5. the distribution on the device
def test_first_sample_follows_the_softmax_on_the_device(lib):
    """the chi-square of tests/test_sbs_host.py through ops.top20_gumbel + ops.sbs_step: W = 3, D = 1, 64 clips x the call seeds"""
    Bd, W = host.DIST_ROWS, host.DIST_W
    R = Bd * W
    p = np.exp(DIST_LOGITS - DIST_LOGITS.max())
    p /= p.sum()
    logits = torch.from_numpy(np.tile(DIST_LOGITS.astype(np.float32)[None, :], (R, 1))).to(DEV)
    state, rows = ops.sbs_state(Bd, W, 1, torch.device(DEV))
    counts = torch.zeros(DIST_V, dtype=torch.int64, device=DEV)
    first_seed = None
    for s in SEEDS:
        ops.sbs_step(state, rows, Bd, W, 1, ref.SOS, ref.EOS, 1)
        ix, lp, g = ops.top20_gumbel(logits, 1.0, s, 0, 0)                # row r draws with batch row r; the policy reads rows b * W
        ops.sbs_step(state, rows, Bd, W, 1, ref.SOS, ref.EOS, 0, ix, lp, g)
        ids, lens, _, G, kappa = ops.sbs_result(state, Bd, W, 1, ref.EOS)
        w = ids[:, :, 0]
        assert bool((lens == 1).all())
        assert bool(((w[:, 0] != w[:, 1]) & (w[:, 0] != w[:, 2]) & (w[:, 1] != w[:, 2])).all())
        assert bool((kappa <= G[:, -1]).all())
        counts += torch.bincount(w[:, 0].long(), minlength=DIST_V)
        if first_seed is None:
            first_seed = w.cpu().numpy()
    hix, hlp, hg = host.dist_head(SEEDS[0])                              # the draws of the float64 restatement, where its top-2 gap is clear
    clear = hg[:, 0] - hg[:, 1] > 2 * (LP_TOL + NOISE_TOL)
    assert clear.sum() >= 60 and (first_seed[clear, 0] == hix[clear, 0]).all()
    counts = counts.cpu().numpy().astype(np.float64)
    assert counts.sum() == Bd * len(SEEDS)
    stat = chi_square(counts, p)
    print("chi2 = %.2f (bound %.2f), N = %d" % (stat, CHI2_BOUND, counts.sum()))
    assert stat < CHI2_BOUND


# ------------------------------------------------------------------ 6. eval.py
_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""


def test_eval_writes_distinct_samples_and_their_consensus(lib, tmp_path):
    import subprocess
    import S2VTModel
    from s2vt_video_caption_amd import synth
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path), V=64)
    V = len(data["word2ix"])
    m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
    m.load_state_dict(synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=38, out_scale=16.0))
    torch.save(m, tmp_path / "model.pth")
    common = ["--model-path", str(tmp_path / "model.pth"), "--caption-file", str(tmp_path / "captions.json"), "--feats-path",
              str(tmp_path / "feats"), "--batch-size", "3"]
    runs = [common + ["--sample", "4", "--sample-distinct", "--sample-seed", "3", "--consensus", "--out", str(tmp_path / "sbs.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    load = lambda n: json.loads(open(str(tmp_path / n), "rb").read())    # noqa: E731
    samples, cons = load("sbs.json.samples.json"), load("sbs.json.consensus.json")
    assert set(samples) == set(cons) == set(data["splits"]["test"]) == set(load("sbs.json"))
    for vid, caps in samples.items():
        assert len(caps) == 4 and len(set(caps)) == 4, (vid, caps)       # four different captions per clip
        e = cons[vid]
        assert set(e) == {"chosen", "utility", "captions"} and e["captions"] == caps and len(e["utility"]) == 4
        assert e["chosen"] == e["utility"].index(max(e["utility"])) and min(e["utility"]) >= 0
