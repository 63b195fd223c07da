"""GPU: the ensemble beam search, S2VTModel.Ensemble (include/s2vt_hip.h "ensemble beam"; csrc/ensemble.hip, ensemble.py).

The fan-out head by value against the fp64 restatement (tests/ensemble_ref.py) on every Row policy, its edges, its constrained
form against sampling.constrain_logits; a member's depth step stopped at its logits against the existing depth steps bit for bit;
the whole path against the fp64 search on every sample whose decisions are clear (tests/test_ensemble_host.py pins how many are);
one member against mode='beam' / beam_constrained bit for bit; the scores against the members' mode='score'; both depth-step paths;
the members' own decoders before and after; eval.py --ensemble."""
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
import beam_cum_ref as cum  # noqa: E402
import beam_constrained_ref as cref  # noqa: E402
import ensemble_ref as ref  # noqa: E402
import test_ensemble_host as host  # noqa: E402
from test_gpu_beam_constrained import HEAD_SPEC, HEAD_T, _head_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(dims, sd, **kw):
    import S2VTModel
    B, L, F, H, E, V = dims
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the head by value
def _check_head(x, w, ix, lp, tag, cap):
    """ids on every row that fp64 decides (at most `cap` rows left out), values within HEAD_TOL of fp64 at the returned ids"""
    c64 = ref.combine64(x, w)
    ids, vals, ok = ref.top20_of(c64)
    ix, lp = ix.cpu().numpy(), lp.cpu().numpy()
    assert int((~ok).sum()) <= cap, (tag, int((~ok).sum()))
    assert np.array_equal(ix[ok], ids[ok]), tag
    assert (np.diff(ix, axis=1) > 0).all() and ix.min() >= 0 and ix.max() < x.shape[2], tag       # ascending ids, every row
    assert np.isfinite(lp).all(), tag
    err = float(np.abs(lp - np.take_along_axis(c64, ix.astype(np.int64), axis=1)).max())
    print("%s: %d of %d rows by id, max |top_lp - fp64| = %.3g" % (tag, int(ok.sum()), len(ok), err))
    assert err <= ref.HEAD_TOL, (tag, err)


@pytest.mark.parametrize("V", host.HEAD_V)
@pytest.mark.parametrize("rows", host.HEAD_ROWS)
def test_head_by_value(lib, V, rows):
    for M in host.HEAD_M:
        x, w = ref.head_case(V, rows, M)
        xd = torch.from_numpy(x).to(DEV)
        ix, lp = ops.ensemble_top20(xd, w)
        _check_head(x, w, ix, lp, "V=%d rows=%d M=%d" % (V, rows, M), host.MAX_LEFT_OUT[rows])
        assert _same_bits((ix, lp), ops.ensemble_top20(xd, w))                   # the same inputs give the same bits
        if M == 1:
            assert _same_bits((ix, lp), ops.top20_logprob(xd[0]))


def test_head_register_rows_of_48_and_64_and_eight_members(lib):
    for V in host.HEAD_EXTRA_V:
        x, w = ref.head_case(V, 3, 3)
        ix, lp = ops.ensemble_top20(torch.from_numpy(x).to(DEV), w)
        _check_head(x, w, ix, lp, "V=%d rows=3 M=3" % V, 0)
    x, w = ref.head_case(50, 3, 8)
    ix, lp = ops.ensemble_top20(torch.from_numpy(x).to(DEV), w)
    _check_head(x, w, ix, lp, "V=50 rows=3 M=8", host.MAX_LEFT_OUT[3])
    # one member whose weight is not 1 at the C ABI (log_w < 0): the general kernel, every value shifted by log_w
    x, _ = ref.head_case(4097, 3, 1)
    xd = torch.from_numpy(x).to(DEV)
    ix = torch.empty(3, 20, dtype=torch.int32, device=DEV)
    lp = torch.empty(3, 20, dtype=torch.float32, device=DEV)
    lw = (ctypes.c_float * 1)(-0.5)
    capi.check(lib.s2vt_ensemble_top20(xd.data_ptr(), xd.stride(0), xd.stride(1), 1, 3, 4097, lw, ix.data_ptr(), lp.data_ptr(),
                                       torch.cuda.current_stream(DEV).cuda_stream), "s2vt_ensemble_top20")
    bix, blp = ops.top20_logprob(xd[0])
    assert torch.equal(ix, bix) and float((lp - (blp - 0.5)).abs().max()) <= 1e-6


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("V", [50, 4097, 8193, 12289, 16385])
def test_head_strides_ties_and_minus_infinity(lib, V):
    rows, M = 3, 3
    x, w = ref.head_case(V, rows, M)
    packed = ops.ensemble_top20(torch.from_numpy(x).to(DEV), w)
    # row stride V + 3 and a member stride with slack, the padding NaN
    buf = torch.full((M, rows + 2, V + 3), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :rows, :V] = torch.from_numpy(x).to(DEV)
    view = buf[:, :rows, :V]
    assert view.stride(0) == (rows + 2) * (V + 3) and view.stride(1) == V + 3
    assert _same_bits(packed, ops.ensemble_top20(view, w))
    # integer-valued logits, equal in every member: many ties, the lower id wins
    t = np.random.RandomState(7 + V).randint(-3, 4, size=(1, rows, V)).astype(np.float32)
    t = np.repeat(t, M, axis=0)
    ix, lp = ops.ensemble_top20(torch.from_numpy(t).to(DEV), w)
    want = np.sort(np.argsort(-t[0].astype(np.float64), axis=1, kind="stable")[:, :20], axis=1)
    assert np.array_equal(ix.cpu().numpy(), want)
    assert _same_bits((ix,), (ops.top20_logprob(torch.from_numpy(t[0]).to(DEV))[0],))
    c64 = ref.combine64(t, w)
    assert float(np.abs(lp.cpu().numpy() - np.take_along_axis(c64, want, axis=1)).max()) <= ref.HEAD_TOL
    # a word at -inf in every member and a word at -inf in one member only: 20 finite results, no NaN
    y = x.copy()
    top = ref.top20_of(ref.combine64(x, w))[0]
    a, b = int(top[0, 0]), int(top[0, 1])                 # two of row 0's winners
    y[:, :, a] = -np.inf
    y[1, :, b] = -np.inf
    ix, lp = ops.ensemble_top20(torch.from_numpy(y).to(DEV), w)
    ix, lp = ix.cpu().numpy(), lp.cpu().numpy()
    assert np.isfinite(lp).all() and not (ix == a).any()
    c64 = ref.combine64(y, w)
    assert np.isneginf(c64[:, a]).all() and np.isfinite(c64[:, b]).all()
    assert float(np.abs(lp - np.take_along_axis(c64, ix.astype(np.int64), axis=1)).max()) <= ref.HEAD_TOL
    ids, _, ok = ref.top20_of(c64)
    assert np.array_equal(ix[ok], ids[ok])


# ------------------------------------------------------------------ 3. the constrained head
@pytest.mark.parametrize("V", [50, 4097])
def test_constrained_head_edits_every_member_and_fans_out_the_edited_rows(lib, V):
    rows, M = 65, 2
    x, w = ref.head_case(V, rows, M)
    _, h = _head_case(V, rows)
    spec = cref.spec_of(HEAD_SPEC, V)
    hd = torch.from_numpy(h).to(DEV)
    for t in (0, 2, HEAD_T):
        xd = torch.from_numpy(x).to(DEV)
        ix, lp = ops.ensemble_top20_constrained(xd, hd if t else None, t, spec, w)
        want = np.stack([sampling.constrain_logits(x[m], h, t, spec) for m in range(M)])
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), want.view(np.uint32)), (V, t)       # every member's buffer, bit for bit
        assert np.isneginf(want[:, :, 5]).all() and np.isneginf(want[:, :, cum.EOS]).all() == (t < 2)
        _check_head(want, w, ix, lp, "constrained V=%d t=%d" % (V, t), host.MAX_LEFT_OUT[rows])
        assert not np.isin(ix.cpu().numpy(), [5, 7]).any()
    # a spec that constrains nothing: the unconstrained head bit for bit, the buffers untouched
    off = cref.spec_of((0, 1.0, 0, ()), V)
    xd = torch.from_numpy(x).to(DEV)
    a = ops.ensemble_top20_constrained(xd, hd, HEAD_T, off, w)
    assert _same_bits(a, ops.ensemble_top20(torch.from_numpy(x).to(DEV), w))
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # one member: top20_logprob_constrained bit for bit
    one = torch.from_numpy(x[:1]).to(DEV)
    two = torch.from_numpy(x[0]).to(DEV)
    assert _same_bits(ops.ensemble_top20_constrained(one, hd, HEAD_T, spec), ops.top20_logprob_constrained(two, hd, HEAD_T, spec))
    assert torch.equal(_bits(one[0]), _bits(two))


# ------------------------------------------------------------------ 4. a member's depth step, stopped at its logits
def test_beam_step_logits_is_the_depth_step_without_its_fan_out(lib):
    from s2vt_video_caption_amd import functional
    from s2vt_video_caption_amd.functional import _params_struct, _ptr, _stream
    dims = cum.CASES["tiny"][0]
    B, L, F, H, E, V = dims
    W = 3
    R = B * W
    sd = cum.case_inputs("tiny")[0]
    m = _model(dims, sd)
    plist = tuple(m.state_dict()[key] for key in capi.PARAM_KEYS)
    d = capi.Dims(*dims)
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(5)
    ins = [(torch.arange(R) // W).int(), torch.randint(0, R, (R,), generator=g).int(), torch.randint(0, V, (R,), generator=g).int()]
    ins = [t.to(DEV) for t in ins]
    vid_h, vid_c = [(torch.tanh(torch.randn(B, H, generator=g)) * s).to(DEV) for s in (1.0, 2.0)]
    word_h, word_c = [(torch.tanh(torch.randn(R, H, generator=g)) * s).to(DEV) for s in (1.0, 2.0)]
    ps = _params_struct(capi.Params, plist)
    nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(d), R)
    st = _stream(dev)
    # the decode cache of these weights, filled as beam.py fills it: by one decode (a batch of 64: a small one fills nothing)
    functional.clear_decode_cache(m)
    functional.greedy_decode(synth.make_batch(64, L, F, V, seed=12)[0].to(DEV), plist, cum.SOS, owner=m)
    cache, valid = functional.decode_cache_entry(m, plist, d, dev, lib)
    assert cache is not None and valid

    def run(entry, cached):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = [torch.full((B, H), 7.0, device=DEV) for _ in range(2)] + [torch.full((R, H), 7.0, device=DEV) for _ in range(2)]
        head = [_ptr(t) for t in ins] + [_ptr(vid_h), _ptr(vid_c), _ptr(out[0]), _ptr(out[1])]
        word = [_ptr(word_h), _ptr(word_c), _ptr(out[2]), _ptr(out[3])]
        c = (_ptr(cache), cache.numel()) if cached else (None, 0)
        if entry == "logits":
            logits = torch.full((R, V + 5), float("nan"), device=DEV)            # (a row stride of its own)
            capi.check(lib.s2vt_beam_step_logits(ctypes.byref(d), ctypes.byref(ps), R, *head, None, *word, _ptr(logits), logits.stride(0),
                                                 _ptr(ws), nbytes, c[0], c[1], st), "s2vt_beam_step_logits")
            assert torch.isnan(logits[:, V:]).all()
            top = ops.top20_logprob(logits[:, :V])
        else:
            top = (torch.empty(R, 20, dtype=torch.int32, device=DEV), torch.empty(R, 20, device=DEV))
            if cached:
                capi.check(lib.s2vt_beam_step_cached(ctypes.byref(d), ctypes.byref(ps), R, *head, *word, _ptr(top[0]), _ptr(top[1]), _ptr(ws),
                                                     nbytes, c[0], c[1], st), "s2vt_beam_step_cached")
            else:
                capi.check(lib.s2vt_beam_step(ctypes.byref(d), ctypes.byref(ps), R, *head, *word, _ptr(top[0]), _ptr(top[1]), _ptr(ws),
                                              nbytes, st), "s2vt_beam_step")
        torch.cuda.synchronize()
        capi.check_async_error()
        return out + list(top)
    for cached in (False, True):
        a, b = run("step", cached), run("logits", cached)
        assert not any(bool((t == 7.0).all()) for t in a[:4])
        assert _same_bits(a, b), cached


# ------------------------------------------------------------------ 5. the whole path against the fp64 search
_RUNS = {}


def _members(name):
    sds, feats, w, W, D = ref.member_dicts(name)
    return [_model(dims, sd) for dims, sd in zip(ref.member_dims(name), sds)], feats.to(DEV), w, W, D


def _run_case(name):
    """(ids, lens, scores) on the host of a case with n_best = W, run once"""
    if name not in _RUNS:
        import S2VTModel
        models, f, w, W, D = _members(name)
        ids, lens, scores = S2VTModel.Ensemble(models, w).beam(f, beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W)
        assert beam.LAST_PATH.startswith("ensemble cumulative beam"), beam.LAST_PATH
        assert ids.dtype == torch.int64 and lens.dtype == torch.int64 and scores.dtype == torch.float32
        assert ids.device.type == "cuda" and tuple(ids.shape) == (f.shape[0], W, D) and tuple(lens.shape) == tuple(scores.shape) == (f.shape[0], W)
        _RUNS[name] = (ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy())
    return _RUNS[name]


@pytest.mark.parametrize("name", ["tiny", "tiny5", "mid64", "mixed"])
def test_whole_path_against_the_restatement(lib, name):
    want = ref.case_search(name)
    rb = cum.robust(want)
    assert int(rb.sum()) == host.ROBUST[name]
    ids, lens, scores = _run_case(name)
    W, D = ids.shape[1], ids.shape[2]
    worst = 0.0
    for b in np.nonzero(rb)[0]:
        assert [ids[b, k, :lens[b, k]].tolist() for k in range(W)] == want[b]["ids"], b
        assert (ids[b][np.arange(D)[None, :] >= lens[b][:, None]] == cum.EOS).all()       # padded with <eos>
        worst = max(worst, float(np.abs(scores[b] - np.array(want[b]["scores"])).max()))
    print("%s: %d robust samples identical, max |score - fp64| = %.3g" % (name, int(rb.sum()), worst))
    assert worst <= 1e-4
    assert (np.diff(scores, axis=1) <= 0).all()                                        # best first, on every sample


# ------------------------------------------------------------------ 6. against the pinned paths
def test_one_member_is_mode_beam_and_beam_constrained(lib):
    import S2VTModel
    sd, feats, W, D = cum.case_inputs("tiny5")
    m = _model(cum.CASES["tiny5"][0], sd)
    f = feats.to(DEV)
    ens = S2VTModel.Ensemble([m])
    with torch.no_grad():
        a = m(f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W)
        path = beam.LAST_PATH
        b = ens.beam(f, beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W)
        assert beam.LAST_PATH == path and _same_bits(a, b)
        kw = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=3, banned_ids=[5, 7])
        a = m.beam_constrained(f, beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W, **kw)
        path = beam.LAST_PATH
        b = ens.beam(f, beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W, **kw)
        assert beam.LAST_PATH == path and path.startswith("constrained cumulative beam") and _same_bits(a, b)


def test_copies_of_one_model_give_its_captions(lib):
    import S2VTModel
    sd, feats, W, D = cum.case_inputs("tiny")
    dims = cum.CASES["tiny"][0]
    models = [_model(dims, sd) for _ in range(3)]
    f = feats.to(DEV)
    rb = cum.robust(cum.case_search("tiny"))
    assert int(rb.sum()) == 8
    with torch.no_grad():
        a = models[0](f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W)
        b = S2VTModel.Ensemble(models).beam(f, beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA, n_best=W)
    assert torch.equal(a[0][rb], b[0][rb]) and torch.equal(a[1][rb], b[1][rb])
    assert float((a[2] - b[2]).abs().max()) <= 1e-4


def test_the_ensemble_differs_from_its_members_and_scores_are_the_members_mixed_log_probs(lib):
    name = "mid64"
    models, f, w, W, D = _members(name)
    ids, lens, scores = _run_case(name)
    B = ids.shape[0]
    wn = ref.norm_weights(w, len(models))
    targets = torch.full((B, W, D + 1), cum.EOS, dtype=torch.int64)
    targets[:, :, 0] = cum.SOS
    targets[:, :, 1:] = torch.from_numpy(ids)
    mix = np.zeros((B, W, D))
    with torch.no_grad():
        for m, wm in zip(models, wn):
            own = m(f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=cum.ALPHA)
            oi, ol = own[0][:, 0].cpu().numpy(), own[1][:, 0].cpu().numpy()
            differ = sum(ids[b, 0, :lens[b, 0]].tolist() != oi[b, :ol[b]].tolist() for b in range(B))
            print("best caption differs from a member's own on %d of %d samples" % (differ, B))
            assert differ >= 16
            _, ln, tlp = m(f, targets=targets.to(DEV), mode="score", length_alpha=0.0)
            assert np.array_equal(ln.cpu().numpy(), lens)
            mix += wm * np.exp(tlp.double().cpu().numpy())
    live = np.arange(D)[None, None, :] < lens[:, :, None]
    total = (np.log(np.where(live, mix, 1.0))).sum(axis=2)
    got = scores.astype(np.float64) * lens.astype(np.float64) ** cum.ALPHA
    worst = float(np.abs(got - total).max())
    print("max |score * len**alpha - sum_t log sum_m w_m p_m(token_t)| = %.3g" % worst)
    assert worst <= 1e-4


# ------------------------------------------------------------------ 7. the plane-path and the fp32 depth steps
def test_plane_and_fp32_depth_steps_determinism_and_constraints(lib):
    import S2VTModel
    d = dict(synth.CONFIGS["c5"])
    B, W, D, M = 64, 5, 12, 2
    feats = synth.make_batch(B, d["L"], d["F"], d["V"], seed=77)[0].to(DEV)
    models = [_model((B, d["L"], d["F"], d["H"], d["E"], d["V"]), synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21 + 100 * i))
              for i in range(M)]
    ens = S2VTModel.Ensemble(models)

    def run(plane, **kw):
        keep = beam.PLANE_STEP
        beam.PLANE_STEP = plane
        try:
            out = ens.beam(feats, beam_width=W, max_beam_depth=D, **kw)
        finally:
            beam.PLANE_STEP = keep
        assert beam.LAST_PATH.startswith("ensemble cumulative beam") and ("plane-path" in beam.LAST_PATH) == plane, beam.LAST_PATH
        assert ("fp32-MFMA" in beam.LAST_PATH) != plane
        return out
    a = run(True)                                           # first call of fresh models: each fills its weight-image cache itself
    b = run(False)
    same = sum(x[0, :n[0]].tolist() == y[0, :k[0]].tolist() for x, n, y, k in zip(a[0].cpu(), a[1].cpu(), b[0].cpu(), b[1].cpu()))
    print("plane path vs fp32 path: %d/%d best captions identical" % (same, B))
    assert same >= 0.95 * B
    assert _same_bits(a, run(True))                         # the search is deterministic
    ids, lens, scores = run(True, no_repeat_ngram_size=2, min_length=4, banned_ids=[5, 7])
    assert "constrained" in beam.LAST_PATH
    for row, n in zip(ids[:, 0].cpu().tolist(), lens[:, 0].cpu().tolist()):
        cap = row[:n]
        grams = list(zip(cap, cap[1:]))
        assert len(set(grams)) == len(grams) and not {5, 7} & set(cap) and n >= 5, cap


# ------------------------------------------------------------------ 8. the members stay untouched; eval.py
def test_members_decode_the_same_before_and_after(lib):
    import S2VTModel
    models, f, w, W, D = _members("tiny")

    def own():
        out = []
        with torch.no_grad():
            for m in models:
                out.append(tuple(t.clone() for t in m(f, mode="beam", beam_width=W, max_beam_depth=D, n_best=W)))
                out.append(tuple(torch.stack([torch.as_tensor(int(t.item())) for t in s]) for s in
                                 m(f, mode="beam_search", beam_width=3, max_beam_depth=30)))
        return out
    before = own()
    S2VTModel.Ensemble(models, w).beam(f, beam_width=W, max_beam_depth=D)
    S2VTModel.Ensemble(models, w).beam(f, beam_width=W, max_beam_depth=D, no_repeat_ngram_size=2)
    after = own()
    assert len(before) == len(after) and all(len(x) == len(y) and _same_bits(x, y) for x, y in zip(before, after))


_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""


def test_eval_ensemble_round_trip(lib, tmp_path):
    """eval.py --ensemble on the toy split, three runs in ONE child process: uniform weights by default and spelled out must write
    the same files, and they are the captions of a direct Ensemble call on the split's batches; --n-best and a constraint flag
    compose"""
    import subprocess
    import S2VTModel
    import dataloader
    import eval as ev
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path), V=64)              # (20 + the tool's depth of 30 + 1 words at least, for the constrained run)
    V = len(data["word2ix"])
    paths = []
    for i, seed in enumerate((38, 39)):
        sd = synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=seed, out_scale=16.0)
        sd["out_linear.bias"][cum.EOS] += 3.0
        m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
        m.load_state_dict(sd)
        paths.append(str(tmp_path / ("model%d.pth" % i)))
        torch.save(m, paths[-1])
    common = ["--model-path", paths[0], "--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
              "--batch-size", "3", "--beam", "3", "--beam-mode", "cumulative", "--ensemble", paths[1]]
    runs = [common + ["--n-best", "3", "--out", str(tmp_path / "a.json")],
            common + ["--n-best", "3", "--ensemble-weights", "2,2", "--out", str(tmp_path / "b.json")],
            common + ["--ensemble-weights", "0.7,0.3", "--no-repeat-ngram", "1", "--out", str(tmp_path / "c.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    a, b, c = [json.load(open(tmp_path / n)) for n in ("a.json", "b.json", "c.json")]
    nbest = json.load(open(str(tmp_path / "a.json") + ".nbest.json"))
    assert a == b and nbest == json.load(open(str(tmp_path / "b.json") + ".nbest.json"))
    assert len(a) == len(data["splits"]["test"]) and set(a) == set(c) == set(nbest)
    assert all(len(v) == 3 and v[0] == a[k] for k, v in nbest.items())
    assert all(len(set(cap.split())) == len(cap.split()) for cap in c.values())        # --no-repeat-ngram 1: no word twice
    ds = dataloader.VideoDataset(str(tmp_path / "captions.json"), str(tmp_path / "feats"), max_len=toy.L, mode="test")
    feats = torch.stack([ds[i][0] for i in range(len(ds))]).to(DEV)
    members = [torch.load(p, weights_only=False).to(DEV).eval() for p in paths]
    for m in members:
        m.rnn_type, m.sos_ix, m.eos_ix = 'lstm', ds.word2ix.get('<sos>', 3), ds.word2ix.get('<eos>', 4)
    direct = {}
    for i in range(0, len(ds), 3):
        ids, lens, _ = S2VTModel.Ensemble(members).beam(feats[i:i + 3], beam_width=3, max_beam_depth=30, n_best=1)
        for j, (row, n) in enumerate(zip(ids[:, 0].cpu().tolist(), lens[:, 0].cpu().tolist())):
            direct[ds[i + j][2]] = ev.ids_to_caption(row[:n], ds.ix2word)
    assert direct == a
