"""GPU: the cumulative-score beam search, S2VT.forward(mode='beam') (csrc/beam_policy.hip + beam.beam_cumulative).

The policy kernel alone is compared bit for bit with the float32 restatement of the definition (tests/beam_cum_ref.PolicyF32: same
adds, same power table, same division); the whole path with the fp64 restatement on every sample whose decisions are clear
(both gaps >= 2e-4; tests/test_beam_cum_host.py caps how many may be left out), with mode='test' and with mode='train' logits."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import test_beam_cum_host as host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V_SYN = 50


def _model(dims, sd, **kw):
    import S2VTModel
    B, L, F, H, E, V = dims
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ 1. the policy kernel alone, through the C ABI
def _ptr(t):
    return t.data_ptr()


def _random_tops(B, W, D, seed, eos=True, quantum=None):
    """per depth (ids [B*W][20] ascending, never 0; lp [B*W][20] <= 0).  quantum: log-probs on a grid, so sums tie bit for bit"""
    rng = np.random.RandomState(seed)
    tops = []
    for _ in range(D):
        lo = 1 if eos else ref.EOS + 1
        ix = np.stack([np.sort(rng.choice(np.arange(lo, V_SYN), 20, replace=False)) for _ in range(B * W)]).astype(np.int32)
        lp = -3.0 * rng.rand(B * W, 20)
        if quantum:
            lp = np.round(lp / quantum) * quantum
        tops.append((ix, lp.astype(np.float32)))
    return tops


def _with_eos(ix, lp, rows, eos_lp):
    """put <eos> into the given rows' top-20 at log-prob eos_lp (replacing the entry at its sorted place), ids stay ascending"""
    for r in rows:
        if ref.EOS in ix[r]:
            lp[r, list(ix[r]).index(ref.EOS)] = eos_lp
            continue
        ids = ix[r].tolist()
        ids[0] = ref.EOS                                # (ids are >= 1: slot 0 holds the smallest)
        order = np.argsort(ids, kind="stable")
        l = lp[r].copy()
        l[0] = eos_lp
        ix[r], lp[r] = np.asarray(ids, dtype=np.int32)[order], l[order]


def _drive(lib, B, W, D, alpha, tops):
    """the kernel and the restatement side by side, one policy call per depth; -> (frozen counter after every call, bool: some
    sample was frozen by the early stop)"""
    R = B * W
    nbytes = lib.s2vt_beam_cum_bytes(B, W, D)
    assert nbytes > 0
    qs = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rows = torch.full((3, R), -7, dtype=torch.int32, device=DEV)
    ix_d = torch.zeros(R, 20, dtype=torch.int32, device=DEV)
    lp_d = torch.zeros(R, 20, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    pol = ref.PolicyF32(B, W, D, alpha)

    def call(depth):
        capi.check(lib.s2vt_beam_cum_step(B, W, D, ref.SOS, ref.EOS, alpha, depth, _ptr(qs), nbytes, _ptr(ix_d), _ptr(lp_d), _ptr(rows[0]),
                                          _ptr(rows[1]), _ptr(rows[2]), st), "s2vt_beam_cum_step")
        return rows.cpu().numpy(), int(qs[:4].view(torch.int32).item())
    got, count = call(1)
    assert count == 0
    assert np.array_equal(got[0], np.repeat(np.arange(B), W))
    assert np.array_equal(got[1:], pol.rows())
    frozen = np.zeros(B, dtype=bool)
    counts, early = [], False
    for t in range(1, D + 1):
        ix_d.copy_(torch.from_numpy(tops[t - 1][0]))
        lp_d.copy_(torch.from_numpy(tops[t - 1][1]))
        got, count = call(t + 1 if t < D else 0)
        pol.step(*tops[t - 1])
        frozen |= pol.done | pol.may_stop()             # (sticky: a frozen sample ignores every later call)
        early |= bool((frozen & ~pol.done).any())
        want = pol.rows()
        want[:, np.repeat(frozen, W)] = 0
        assert np.array_equal(got[0], np.repeat(np.arange(B), W))
        assert np.array_equal(got[1:], want), (t, got[1:], want)
        assert count == int(frozen.sum()), (t, count, frozen)
        counts.append(count)
    assert counts[-1] == B
    ids = torch.empty(B, W, D, dtype=torch.int32, device=DEV)
    lens = torch.empty(B, W, dtype=torch.int32, device=DEV)
    scores = torch.empty(B, W, dtype=torch.float32, device=DEV)
    capi.check(lib.s2vt_beam_cum_result(B, W, D, ref.EOS, W, _ptr(qs), nbytes, _ptr(ids), _ptr(lens), _ptr(scores), st), "s2vt_beam_cum_result")
    wi, wl, ws = pol.result()
    assert np.array_equal(ids.cpu().numpy(), wi)
    assert np.array_equal(lens.cpu().numpy(), wl)
    sc = scores.cpu().numpy()
    assert (np.abs(sc - ws) <= np.spacing(np.abs(ws))).all(), (sc, ws)
    # fewer than W: the first n_best rows of the same answer
    if W > 1:
        capi.check(lib.s2vt_beam_cum_result(B, W, D, ref.EOS, 1, _ptr(qs), nbytes, _ptr(ids), _ptr(lens), _ptr(scores), st),
                   "s2vt_beam_cum_result")
        assert np.array_equal(ids.cpu().numpy().reshape(-1)[:B * D].reshape(B, D), wi[:, 0])
        assert np.array_equal(lens.cpu().numpy().reshape(-1)[:B], wl[:, 0])
    return counts, early


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 6])
def test_policy_kernel_is_the_float32_restatement(lib, W, D):
    """random top-20 arrays: continuous log-probs, and log-probs on a grid of 1/4 (candidate sums of different parents tie bit for
    bit at every depth: the (slot, token) rule decides); alpha = 0.7 and alpha = 0"""
    B = 3
    for seed, quantum, alpha in ((1, None, 0.7), (2, 0.25, 0.7), (3, 0.25, 0.0), (4, None, 0.0)):
        _drive(lib, B, W, D, alpha, _random_tops(B, W, D, 100 * W + 10 * D + seed, quantum=quantum))


def test_policy_kernel_on_crafted_inputs(lib):
    B, W, D = 3, 3, 6
    R = B * W
    # two parents with bit-equal candidate sums everywhere: every log-prob is -1 (no <eos>), the order is (slot, token) alone
    tops = _random_tops(B, W, D, 11, eos=False)
    for ix, lp in tops:
        lp[:] = -1.0
    _drive(lib, B, W, D, 0.7, tops)
    # <eos> the best token at depth 1
    tops = _random_tops(B, W, D, 12)
    _with_eos(tops[0][0], tops[0][1], range(R), -0.001)
    _drive(lib, B, W, D, 0.7, tops)
    # every selected candidate <eos> at depth 2: live empties
    tops = _random_tops(B, W, D, 13, eos=False)
    tops[1][1][:] -= 5.0
    _with_eos(tops[1][0], tops[1][1], range(R), -0.001)
    counts, _ = _drive(lib, B, W, D, 0.7, tops)
    assert counts[1] == B
    # <eos> never in any top 20: all unfinished at D
    counts, early = _drive(lib, B, W, D, 0.7, _random_tops(B, W, D, 14, eos=False))
    assert counts[:-1] == [0] * (D - 1) and not early
    # <eos> at log-prob 0 from depth 2 on, every other word a little below: the pool fills with sums no live hypothesis can reach
    # any more while some are still live, and the early stop must fire (alpha = 0: the score is the sum itself)
    tops = _random_tops(B, W, D, 15, eos=False)
    tops[0][1][:] = tops[0][1] / 3.0 * 0.04 - 0.01                # depth 1 in [-0.05, -0.01]
    for t in range(1, D):
        tops[t][1][:] = tops[t][1] / 3.0 * 0.004 - 0.001          # then in [-0.005, -0.001]
        _with_eos(tops[t][0], tops[t][1], range(R), 0.0)
    counts, early = _drive(lib, B, W, D, 0.0, tops)
    assert early and counts[D - 2] == B, counts


# ------------------------------------------------------------------ 2. the whole path against the fp64 restatement
_RUNS = {}


def _case_model(name):
    sd, feats, _, _ = ref.case_inputs(name)
    return _model(ref.CASES[name][0], sd), feats.to(DEV)


def _run_case(name):
    """(ids, lens, scores) on the host of a case with n_best = W, run once (nothing stays on the device between tests)"""
    if name not in _RUNS:
        _, _, W, D = ref.case_inputs(name)
        m, f = _case_model(name)
        with torch.no_grad():
            ids, lens, scores = m(f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=W)
        assert ids.dtype == torch.int64 and lens.dtype == torch.int64 and scores.dtype == torch.float32
        assert ids.device.type == "cuda" and tuple(ids.shape) == (f.shape[0], W, D) and tuple(lens.shape) == tuple(scores.shape) == (f.shape[0], W)
        _RUNS[name] = (ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy())
    return _RUNS[name]


@pytest.mark.parametrize("name", ["tiny", "tiny5", "mid64"])
def test_whole_path_against_the_restatement(lib, name):
    want = ref.case_search(name)
    rb = ref.robust(want)
    assert int(rb.sum()) == host.ROBUST[name]
    ids, lens, scores = _run_case(name)
    W, D = ref.CASES[name][3], ref.CASES[name][4]
    worst = 0.0
    for b in np.nonzero(rb)[0]:
        assert [ids[b, k, :lens[b, k]].tolist() for k in range(W)] == want[b]["ids"], b
        assert (ids[b][np.arange(D)[None, :] >= lens[b][:, None]] == ref.EOS).all()       # padded with <eos>
        worst = max(worst, float(np.abs(scores[b] - np.array(want[b]["scores"])).max()))
    print("%s: %d robust samples identical, max |score - fp64| = %.3g" % (name, int(rb.sum()), worst))
    assert worst <= 1e-4
    assert (np.diff(scores, axis=1) <= 0).all()                                        # best first, on every sample


# ------------------------------------------------------------------ 3. against the pinned paths
def test_width_one_is_mode_test_up_to_the_first_eos(lib):
    name = "mid64"
    sd, feats, _, D = ref.case_inputs(name)
    m, f = _case_model(name)
    with torch.no_grad():
        greedy = m(f, mode="test").cpu().numpy()
        ids, lens, scores = [t.cpu().numpy() for t in m(f, mode="beam", beam_width=1, max_beam_depth=D, length_alpha=0.0, n_best=1)]
    _, margins = ref.greedy_fp64(sd, feats, D)
    rows = np.nonzero(margins[:, :D].min(axis=1) >= 1e-5)[0]
    assert len(rows) >= 48
    for b in rows:
        g = greedy[b, :D].tolist()
        n = g.index(ref.EOS) + 1 if ref.EOS in g else D
        assert lens[b, 0] == n and ids[b, 0, :n].tolist() == g[:n], b


def test_scores_are_the_sums_of_the_train_logits_log_softmax(lib):
    """score * length**alpha of every returned hypothesis = the sum of log_softmax(mode='train' logits) at its own tokens"""
    name = "mid64"
    m, f = _case_model(name)
    ids, lens, scores = _run_case(name)
    (B, L, _, _, _, _), W, D = ref.CASES[name][0], ref.CASES[name][3], ref.CASES[name][4]
    assert D <= L - 1
    worst = 0.0
    for k in range(W):
        targets = torch.full((B, L - 1), ref.EOS, dtype=torch.int64)
        targets[:, 0] = ref.SOS
        targets[:, 1:D + 1] = torch.from_numpy(ids[:, k, :min(D, L - 2)])
        with torch.no_grad():
            logp = torch.log_softmax(m(f, targets=targets.to(DEV), mode="train").double(), dim=2).cpu()
        tok = torch.from_numpy(ids[:, k])
        lp = logp[:, :D].gather(2, tok[:, :, None])[:, :, 0].numpy()
        total = (lp * (np.arange(D)[None, :] < lens[:, k][:, None])).sum(axis=1)
        got = scores[:, k].astype(np.float64) * lens[:, k].astype(np.float64) ** ref.ALPHA
        worst = max(worst, float(np.abs(got - total).max()))
    print("max |score * len**alpha - sum of train log-probs| = %.3g" % worst)
    assert worst <= 1e-4


# ------------------------------------------------------------------ 4. the plane-path depth step
def test_plane_path_depth_step_and_determinism(lib):
    d = dict(synth.CONFIGS["c5"])
    B, W, D = 64, 5, 12
    feats = synth.make_batch(B, d["L"], d["F"], d["V"], seed=77)[0].to(DEV)
    m = _model((B, d["L"], d["F"], d["H"], d["E"], d["V"]), synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21))

    def run(plane):
        keep = beam.PLANE_STEP
        beam.PLANE_STEP = plane
        try:
            with torch.no_grad():
                out = m(feats, mode="beam", beam_width=W, max_beam_depth=D)
        finally:
            beam.PLANE_STEP = keep
        assert beam.LAST_PATH.startswith("cumulative beam") and ("plane-path" in beam.LAST_PATH) == plane, beam.LAST_PATH
        return out
    a = run(True)                                           # first call of a fresh model: fills the weight-image cache itself
    b = run(False)
    same = sum(x[0, :n[0]].tolist() == y[0, :k[0]].tolist() for x, n, y, k in zip(a[0].cpu(), a[1].cpu(), b[0].cpu(), b[1].cpu()))
    print("plane path vs fp32 path: %d/%d best captions identical" % (same, B))
    assert same >= 0.95 * B
    c = run(True)
    assert all(torch.equal(x, y) for x, y in zip(a, c))     # the search is deterministic


# ------------------------------------------------------------------ 5. error paths
def test_error_paths_and_beam_search_is_untouched(lib):
    sd, feats, W, D = ref.case_inputs("tiny")
    dims = ref.CASES["tiny"][0]
    m = _model(dims, sd)
    f = feats.to(DEV)
    for kw in (dict(beam_width=0), dict(beam_width=9), dict(n_best=0), dict(beam_width=3, n_best=4), dict(max_beam_depth=0),
               dict(length_alpha=-0.5), dict(length_alpha=float("nan")), dict(length_alpha=float("inf"))):
        with pytest.raises(ValueError, match="mode='beam'"):
            m(f, mode="beam", **kw)
    import S2VTModel
    small = S2VTModel.S2VT(19, dims[2], dims[1], dim_hid=dims[3], dim_embed=dims[4]).to(DEV)
    with pytest.raises(ValueError, match="vocab_size"):
        small(f, mode="beam")
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        other = S2VTModel.S2VT(dims[5], dims[2], dims[1], dim_hid=dims[3], dim_embed=dims[4], **kw).to(DEV).eval()
        with pytest.raises(NotImplementedError, match="mode='test'"):
            other(f, mode="beam")
    with pytest.raises(capi.S2VTHipError):
        m(feats, mode="beam")                               # a CPU tensor
    with torch.no_grad():
        before = [[int(t.item()) for t in s] for s in m(f, mode="beam_search", beam_width=3, max_beam_depth=30)]
        m(f, mode="beam", beam_width=W, max_beam_depth=D)
        after = [[int(t.item()) for t in s] for s in m(f, mode="beam_search", beam_width=3, max_beam_depth=30)]
    assert before == after and all(s[0] == ref.SOS for s in before)


def test_beam_search_on_the_tiny_fixture_after_a_cumulative_search(lib, golden):
    """mode='beam_search' still gives the reference's ids of the tiny fixture, on a model that has just run mode='beam'"""
    g = golden("tiny")
    d = synth.CONFIGS["tiny"]
    seed = int(g["seed"])
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=float(g["out_scale"]))
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)[0].to(DEV)
    m = _model((d["B"], d["L"], d["F"], d["H"], d["E"], d["V"]), sd)
    with torch.no_grad():
        m(feats, mode="beam", beam_width=3, max_beam_depth=10, n_best=2)
        out = m(feats, mode="beam_search", beam_width=int(g["beam_width"]), max_beam_depth=30)
    for b, s in enumerate(out):
        assert [int(t.item()) for t in s] == [int(x) for x in g["beam_ids"][b] if x >= 0]


# ------------------------------------------------------------------ 6. eval.py --beam-mode cumulative
_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""


def test_eval_cumulative_mode_writes_predictions_and_width_one_is_greedy(lib, tmp_path):
    """eval.py's command line, three runs in ONE child process (the tool brings its own feed thread and copy stream: they stay out
    of the test process): greedy, --beam 1 --beam-mode cumulative --length-alpha 0, and --beam 3 with --n-best 3"""
    import subprocess
    import S2VTModel
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path))
    V = len(data["word2ix"])
    # untrained weights under which the greedy caption of every test clip ends in <eos> inside its L-1 words, after 1 to 3 words
    # (so a width-1 search, which goes on to <eos>, says the same), with a top-2 margin of 2.7e-3 at every step
    sd = synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=38, out_scale=16.0)
    sd["out_linear.bias"][ref.EOS] += 3.0
    m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
    m.load_state_dict(sd)
    torch.save(m, tmp_path / "model.pth")
    common = ["--model-path", str(tmp_path / "model.pth"), "--caption-file", str(tmp_path / "captions.json"), "--feats-path",
              str(tmp_path / "feats"), "--batch-size", "3"]
    runs = [common + ["--out", str(tmp_path / "greedy.json")],
            common + ["--beam", "1", "--beam-mode", "cumulative", "--length-alpha", "0", "--out", str(tmp_path / "beam1.json")],
            common + ["--beam", "3", "--beam-mode", "cumulative", "--n-best", "3", "--out", str(tmp_path / "beam3.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    greedy = json.load(open(tmp_path / "greedy.json"))
    beam1 = json.load(open(tmp_path / "beam1.json"))
    beam3 = json.load(open(tmp_path / "beam3.json"))
    nbest = json.load(open(str(tmp_path / "beam3.json") + ".nbest.json"))
    assert len(greedy) == len(data["splits"]["test"]) and set(beam1) == set(beam3) == set(nbest) == set(greedy)
    import dataloader
    ds = dataloader.VideoDataset(str(tmp_path / "captions.json"), str(tmp_path / "feats"), max_len=toy.L, mode="test")
    rows, margins = ref.greedy_fp64(sd, torch.stack([ds[i][0] for i in range(len(ds))]), toy.L - 1)
    assert all(r[-1] == ref.EOS for r in rows) and len({len(r) for r in rows}) > 1 and margins.min() >= 1e-3       # (the fixture)
    assert beam1 == greedy
    assert len({len(c.split()) for c in greedy.values()}) > 1
    assert all(len(v) == 3 and v[0] == beam3[k] for k, v in nbest.items())
