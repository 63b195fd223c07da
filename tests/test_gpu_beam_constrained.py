"""GPU: the constrained cumulative-score beam search, S2VT.beam_constrained (include/s2vt_hip.h "constrained beam").

The fan-out head (csrc/ce.hip: the constraint phase in front of the top 20) by value against sampling.constrain_logits; the policy
kernel with per-slot histories (csrc/beam_policy.hip) bit for bit against the float32 restatement and against the plain policy
entry; the whole path against the fp64 restatement (tests/beam_constrained_ref.py) on every sample whose decisions are clear;
width 1 against greedy decode_constrained; default constraints against mode='beam'; both depth-step paths; eval.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi, ops, sampling, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import beam_constrained_ref as cref  # noqa: E402
import test_beam_constrained_host as host  # noqa: E402
from test_gpu_beam_cum import _random_tops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptr(t):
    return t.data_ptr()


def _model(dims, sd, **kw):
    import S2VTModel
    B, L, F, H, E, V = dims
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _kwargs(spec_args):
    n, theta, m, banned = spec_args
    return dict(no_repeat_ngram_size=n, repetition_penalty=theta, min_length=m, banned_ids=list(banned))


# ------------------------------------------------------------------ 1. the fan-out head by value
HEAD_T = 12              # words of history the fixture holds
HEAD_SPEC = (3, 1.2, 2, (5, 7))          # n = 3; <eos> banned at t = 0, 1 and free at t = 2, 12


def _head_case(V, rows):
    """(logits fp32 [rows, V], hist int32 [rows, 16]).  Even rows are crafted, a b c w w w a b d <eos> a b with c = 5: a word three
    times (w), a banned id in the history (5), <eos> in the history, and at t = 12 the suffix (a, b) matches at two starts - c and d
    are blocked.  Odd rows draw from 12 ids: many repeats, the banned ids and <eos> among them."""
    rng = np.random.RandomState(1000 + V + rows)
    x = (3.0 * rng.randn(rows, V)).astype(np.float32)
    h = rng.randint(0, 12, size=(rows, 16)).astype(np.int32)
    for r in range(0, rows, 2):
        a, b, d, w = rng.choice(np.arange(8, V), 4, replace=False)
        h[r, :HEAD_T] = [a, b, 5, w, w, w, a, b, d, ref.EOS, a, b]
    return x, h


@pytest.mark.parametrize("V", [50, 4097, 16385])          # RegRow<16>'s smallest, the first above a bracket edge, the first LdsRow size
@pytest.mark.parametrize("rows", [3, 65])
def test_head_edits_the_rows_and_fans_out_the_edited_rows(lib, V, rows):
    x, h = _head_case(V, rows)
    spec = cref.spec_of(HEAD_SPEC, V)
    hd = torch.from_numpy(h).to(DEV)
    for t in (0, 1, 2, HEAD_T):
        xd = torch.from_numpy(x).to(DEV)
        ix, lp = ops.top20_logprob_constrained(xd, hd if t else None, t, spec)
        ix, lp, got = ix.cpu().numpy(), lp.cpu().numpy(), xd.cpu().numpy()
        want = sampling.constrain_logits(x, h, t, spec)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, rows, t)          # the buffer: bit for bit
        if t == HEAD_T:                                      # (the fixture: both continuations of the suffix are blocked)
            assert np.isneginf(want[0, h[0, 2]]) and np.isneginf(want[0, h[0, 8]]) and want[0, h[0, 3]] == x[0, h[0, 3]] * (
                np.float32(1 / np.float32(1.2)) if x[0, h[0, 3]] > 0 else np.float32(1.2))
        assert np.isneginf(want[:, ref.EOS]).all() == (t < 2)
        w64 = want.astype(np.float64)
        top = np.sort(np.argsort(-w64, axis=1, kind="stable")[:, :20], axis=1)       # (value descending, id ascending), then by id
        assert np.array_equal(ix, top), (V, rows, t)
        m = w64.max(axis=1, keepdims=True)
        lsm = w64 - m - np.log(np.exp(w64 - m).sum(axis=1, keepdims=True))
        picked = np.take_along_axis(lsm, top, axis=1)
        assert np.isfinite(picked).all() and np.isfinite(lp).all()                 # no -inf among the 20
        err = float(np.abs(lp - picked).max())
        print("V=%d rows=%d t=%d: max |top_lp - fp64| = %.3g" % (V, rows, t, err))
        assert err <= 2e-6 * 8
    # neutral constraints: the unconstrained head, bit for bit, and the buffer untouched
    off = cref.spec_of((0, 1.0, 0, ()), V)
    xd = torch.from_numpy(x).to(DEV)
    a = ops.top20_logprob_constrained(xd, hd, HEAD_T, off)
    b = ops.top20_logprob(torch.from_numpy(x).to(DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------ 2. the policy kernel with histories
def _drive_hist(lib, B, W, D, alpha, tops):
    """the policy with histories, the plain policy and the restatement side by side, one call per depth"""
    R = B * W
    nb_h, nb_p = lib.s2vt_beam_cum_hist_bytes(B, W, D), lib.s2vt_beam_cum_bytes(B, W, D)
    assert nb_h >= nb_p + 2 * R * D * 4
    qh = torch.empty(nb_h, dtype=torch.uint8, device=DEV)
    qp = torch.empty(nb_p, dtype=torch.uint8, device=DEV)
    rows_h = torch.full((3, R), -7, dtype=torch.int32, device=DEV)
    rows_p = torch.full((3, R), -7, dtype=torch.int32, device=DEV)
    ix_d = torch.zeros(R, 20, dtype=torch.int32, device=DEV)
    lp_d = torch.zeros(R, 20, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    pol = cref.PolicyHist(B, W, D, alpha)
    words, words_ld = ctypes.c_void_p(), ctypes.c_int64()

    def call(depth):
        capi.check(lib.s2vt_beam_cum_hist_step(B, W, D, ref.SOS, ref.EOS, alpha, depth, _ptr(qh), nb_h, _ptr(ix_d), _ptr(lp_d), _ptr(rows_h[0]),
                                               _ptr(rows_h[1]), _ptr(rows_h[2]), ctypes.byref(words), ctypes.byref(words_ld), st),
                   "s2vt_beam_cum_hist_step")
        capi.check(lib.s2vt_beam_cum_step(B, W, D, ref.SOS, ref.EOS, alpha, depth, _ptr(qp), nb_p, _ptr(ix_d), _ptr(lp_d), _ptr(rows_p[0]),
                                          _ptr(rows_p[1]), _ptr(rows_p[2]), st), "s2vt_beam_cum_step")
        assert torch.equal(rows_h, rows_p)                                       # the plain entry on the same inputs
        assert int(qh[:4].view(torch.int32).item()) == int(qp[:4].view(torch.int32).item())
        off = words.value - qh.data_ptr()                                        # the buffer the next depth step must read
        assert words_ld.value == D and nb_p <= off and off + R * D * 4 <= nb_h and off % 4 == 0
        return rows_h.cpu().numpy(), qh[off:off + R * D * 4].view(torch.int32).view(R, D).cpu().numpy()
    got, hist = call(1)
    assert np.array_equal(got[1:], pol.rows()) and not hist.any()                # no words yet; every row defined
    frozen = np.zeros(B, dtype=bool)
    for t in range(1, D + 1):
        ix_d.copy_(torch.from_numpy(tops[t - 1][0]))
        lp_d.copy_(torch.from_numpy(tops[t - 1][1]))
        got, hist = call(t + 1 if t < D else 0)
        pol.step(*tops[t - 1])
        frozen |= pol.done | pol.may_stop()
        want = pol.rows()
        want[:, np.repeat(frozen, W)] = 0
        assert np.array_equal(got[1:], want), (t, got[1:], want)
        h, live = pol.histories()
        live &= ~np.repeat(frozen, W)
        assert np.array_equal(hist[live, :t], h[live, :t]), (t, hist, h)         # each live slot's words
        assert hist.min() >= 0 and hist.max() < 50                               # every row readable: defined words, in bounds
    wi, wl, ws = pol.result()
    outs = []
    for qs, nbytes in ((qh, nb_h), (qp, nb_p)):
        ids = torch.empty(B, W, D, dtype=torch.int32, device=DEV)
        lens = torch.empty(B, W, dtype=torch.int32, device=DEV)
        scores = torch.empty(B, W, dtype=torch.float32, device=DEV)
        capi.check(lib.s2vt_beam_cum_result(B, W, D, ref.EOS, W, _ptr(qs), nbytes, _ptr(ids), _ptr(lens), _ptr(scores), st),
                   "s2vt_beam_cum_result")
        outs.append((ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()))
    for ids, lens, scores in outs:
        assert np.array_equal(ids, wi) and np.array_equal(lens, wl)
        assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32)), (scores, ws)


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 6])
def test_policy_with_histories_is_the_restatement_and_the_plain_policy(lib, W, D):
    B = 3
    for seed, quantum, alpha in ((1, None, 0.7), (2, 0.25, 0.0)):
        _drive_hist(lib, B, W, D, alpha, _random_tops(B, W, D, 100 * W + 10 * D + seed, quantum=quantum))


# ------------------------------------------------------------------ 3. the whole path against the fp64 restatement
_MODELS = {}


def _case_model(name):
    if name not in _MODELS:
        sd, feats, _, _ = ref.case_inputs(name)
        _MODELS[name] = (_model(ref.CASES[name][0], sd), feats.to(DEV))
    return _MODELS[name]


def _run(name, spec_args, **kw):
    _, _, W, D = ref.case_inputs(name)
    m, f = _case_model(name)
    args = dict(beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=W)
    args.update(kw)
    ids, lens, scores = m.beam_constrained(f, **args, **_kwargs(spec_args))
    assert ids.dtype == torch.int64 and lens.dtype == torch.int64 and scores.dtype == torch.float32 and ids.device.type == "cuda"
    return ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def _check_against(name, spec_args, out):
    """ids identical and scores within 1e-4 on the robust samples; padding, order and the constraints on every sample"""
    want = cref.case_search(name, spec_args)
    rb = ref.robust(want)
    assert int(rb.sum()) == host.ROBUST[(name, spec_args)]
    ids, lens, scores = out
    (B, _, _, _, _, V), W, D = ref.CASES[name][0], ref.CASES[name][3], ref.CASES[name][4]
    assert ids.shape == (B, W, D) and lens.shape == scores.shape == (B, W)
    spec = cref.spec_of(spec_args, V)
    worst = 0.0
    for b in range(B):
        got = [ids[b, k, :lens[b, k]].tolist() for k in range(W)]
        assert all(cref.satisfies(g, spec) for g in got), (b, got)                        # on every returned hypothesis
        assert (ids[b][np.arange(D)[None, :] >= lens[b][:, None]] == ref.EOS).all()       # padded with <eos>
        if rb[b]:
            assert got == want[b]["ids"], b
            worst = max(worst, float(np.abs(scores[b] - np.array(want[b]["scores"])).max()))
    print("%s %r: %d robust samples identical, max |score - fp64| = %.3g" % (name, spec_args, int(rb.sum()), worst))
    assert worst <= 1e-4
    assert (np.diff(scores, axis=1) <= 0).all()                                        # best first, on every sample


@pytest.mark.parametrize("name,spec_args", sorted(host.ROBUST))
def test_whole_path_against_the_restatement(lib, name, spec_args):
    _check_against(name, spec_args, _run(name, spec_args))


# ------------------------------------------------------------------ 4. width 1 is greedy decode_constrained
def test_width_one_is_greedy_decode_constrained_up_to_the_first_eos(lib):
    name, sp = "mid64", cref.SPEC_A
    D = ref.CASES[name][4]
    m, f = _case_model(name)
    greedy = m.decode_constrained(f, **_kwargs(sp))[:, 0].cpu().numpy()
    ids, lens, _ = _run(name, sp, beam_width=1, length_alpha=0.0, n_best=1)
    g64 = cref.greedy_search(name, sp)
    rows = [b for b, r in enumerate(g64) if r["cand_gap"] >= 1e-5]
    assert len(rows) == host.WIDTH_ONE_ROWS >= 48
    for b in rows:
        g = greedy[b, :D].tolist()
        n = g.index(ref.EOS) + 1 if ref.EOS in g else D
        assert lens[b, 0] == n and ids[b, 0, :n].tolist() == g[:n] == g64[b]["ids"][0], b


# ------------------------------------------------------------------ 5. default constraints are mode='beam'
def test_default_constraints_are_mode_beam_bit_for_bit(lib):
    for name in ("tiny5", "mid64"):
        _, _, W, D = ref.case_inputs(name)
        m, f = _case_model(name)
        with torch.no_grad():
            a = m(f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=W)
        b = m.beam_constrained(f, beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=W)
        assert beam.LAST_PATH.startswith("cumulative beam")                       # today's launches, not a neutral form of the new ones
        c = m.beam_constrained(f, beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=W, repetition_penalty=1, banned_ids=[])
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ------------------------------------------------------------------ 6. both depth-step paths
def test_both_depth_step_paths_and_determinism(lib):
    name, sp = "mid64", cref.SPEC_A

    def run(plane):
        keep = beam.PLANE_STEP
        beam.PLANE_STEP = plane
        try:
            out = _run(name, sp)
        finally:
            beam.PLANE_STEP = keep
        assert beam.LAST_PATH.startswith("constrained cumulative beam") and ("plane-path" in beam.LAST_PATH) == plane, beam.LAST_PATH
        return out
    a = run(True)
    b = run(False)
    _check_against(name, sp, a)
    _check_against(name, sp, b)
    c, d = run(True), run(False)
    for x, y in zip(a + b, c + d):                         # two runs of one path: the same bits
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 7. eval.py --beam N --beam-mode cumulative with the flags
_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""
EVAL_V, EVAL_SEED, EVAL_SCALE = 64, 38, 16.0


def _repeats_a_bigram(caption):
    w = caption.split()
    grams = list(zip(w, w[1:]))
    return len(grams) != len(set(grams))


def test_eval_cumulative_beam_takes_the_constraint_flags(lib, tmp_path):
    """two runs in ONE child process (the tool brings its own feed thread and copy stream): --beam 3 --beam-mode cumulative without
    and with --no-repeat-ngram 2"""
    import subprocess
    import S2VTModel
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path), V=EVAL_V)          # (20 + the tool's depth of 30 + 1 words at least)
    V = len(data["word2ix"])
    sd = synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=EVAL_SEED, out_scale=EVAL_SCALE)
    m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
    m.load_state_dict(sd)
    torch.save(m, tmp_path / "model.pth")
    common = ["--model-path", str(tmp_path / "model.pth"), "--caption-file", str(tmp_path / "captions.json"), "--feats-path",
              str(tmp_path / "feats"), "--batch-size", "3", "--beam", "3", "--beam-mode", "cumulative"]
    runs = [common + ["--out", str(tmp_path / "plain.json")],
            common + ["--no-repeat-ngram", "2", "--out", str(tmp_path / "ngram.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    plain = json.load(open(tmp_path / "plain.json"))
    ngram = json.load(open(tmp_path / "ngram.json"))
    assert len(ngram) == len(data["splits"]["test"]) and set(ngram) == set(plain)
    assert all(c for c in ngram.values())
    assert not any(_repeats_a_bigram(c) for c in ngram.values())
    assert any(_repeats_a_bigram(c) for c in plain.values())          # (the fixture: without the flag some caption does repeat one)
