"""GPU: caption scoring, S2VT.forward(mode='score') (csrc/api_score.hip, the head kernel in csrc/ce.hip, score.score_captions).

The head kernel alone against fp64 log_softmax; the whole path against the fp64 restatement of the definition (tests/score_ref.py)
on the fp32 launch-per-timestep path (`tiny`) and on the plane path with the decode cache (`mid64`); against mode='beam' scores and
mode='train' logits of the same captions; views, determinism, cache fill and refresh; the asynchronous index error."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, functional, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import score_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_OF = {"tiny": 8, "mid64": 13}       # tiny: L = 8 caps a caption at 7 scored tokens; mid64: up to 12, the depth of the beam cases
SEED_OF = {"tiny": 5, "mid64": 6}
TOKEN_BOUND = 1e-4                    # the project's logits bound
SUM_BOUND = 1e-4                      # what test_scores_are_the_sums_of_the_train_logits_log_softmax holds at the same 12-term depth


def _model(dims, sd, **kw):
    import S2VTModel
    B, L, F, H, E, V = dims
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _case(name, K):
    """(model on the device, feats on the device, captions [B, K, T] on the host, fp64 reference at alpha = 0)"""
    sd, feats, _, _ = ref.case_inputs(name)
    caps, want = score_ref.case_reference(name, K, T_OF[name], SEED_OF[name])
    return _model(ref.CASES[name][0], sd), feats.to(DEV), caps, want


def _check_against_fp64(got, want, alpha, what):
    scores, lengths, tlp = (t.cpu() for t in got)
    n = want["lengths"]
    assert lengths.dtype == torch.int64 and torch.equal(lengths, n), what
    assert scores.dtype == torch.float32 and tlp.dtype == torch.float32
    behind = torch.arange(tlp.shape[-1])[None, None, :] >= n[..., None]
    assert float(tlp[behind].abs().max()) == 0.0 if bool(behind.any()) else True, what
    e_tok = float((tlp.double() - want["token_lp"]).abs().max())
    e_sum = float((scores.double() * n.double() ** alpha - want["sums"]).abs().max())
    print("%s alpha %.1f: token log-prob error %.3g, sum error %.3g" % (what, alpha, e_tok, e_sum))
    assert float(tlp.max()) <= 0.0
    assert e_tok <= TOKEN_BOUND, (what, e_tok)
    assert e_sum <= SUM_BOUND, (what, e_sum)


# ------------------------------------------------------------------ 1. the head kernel alone
# Largest |lp - fp64 log_softmax| over these inputs, measured on an MI355X: 1.46e-06 at V = 12001 (profiles/score.txt) - the
# rounding of a result of magnitude 8..16 (ulp 9.5e-7) plus the fp32 logsumexp.  The bound is 4 x that, and no looser than 1e-5.
HEAD_MEASURED = 1.46e-06
HEAD_BOUND = min(4 * HEAD_MEASURED, 1e-5)


def _head_inputs(V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    rows = 5
    x = torch.randn(rows, ld, generator=g) * 5 + torch.tensor([-1e4, 0.0, 1e4, 0.0, 1e4])[:, None]
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[0], tgt[1] = 0, V - 1
    return x, tgt.int()


@pytest.mark.parametrize("V,ld", [(1, 1), (50, 50), (257, 259), (1000, 1004), (12001, 12001)])
def test_head_kernel_against_fp64_log_softmax(lib, V, ld):
    x, tgt = _head_inputs(V, ld, seed=100 + V)
    xd = x.to(DEV)
    lp, flag = ops.pick_logprob(xd[:, :V], tgt.to(DEV))
    want = torch.log_softmax(x[:, :V].double(), dim=1).gather(1, tgt.long()[:, None])[:, 0]
    err = float((lp.cpu().double() - want).abs().max())
    print("pick_logprob V=%d ld=%d: largest error %.3g (bound %.3g)" % (V, ld, err, HEAD_BOUND))
    assert int(flag.item()) == 0
    assert float(lp.max()) <= 0.0
    assert err <= HEAD_BOUND, err
    # a target outside [0, V): the flag is raised and the clamped column is read
    bad = tgt.clone()
    bad[2], bad[3] = -1, V
    lp2, flag2 = ops.pick_logprob(xd[:, :V], bad.to(DEV))
    fixed = tgt.clone()
    fixed[2], fixed[3] = 0, V - 1
    lp3, flag3 = ops.pick_logprob(xd[:, :V], fixed.to(DEV))
    assert int(flag2.item()) != 0 and int(flag3.item()) == 0
    assert torch.equal(lp2, lp3)


# ------------------------------------------------------------------ 2. the whole path against the fp64 restatement
@pytest.mark.parametrize("name,K", [("tiny", 1), ("tiny", 2), ("mid64", 1), ("mid64", 3), ("mid64", 5)])
def test_scores_against_the_fp64_definition(lib, name, K):
    m, feats, caps, want = _case(name, K)
    assert int(want["lengths"][0, 0]) == T_OF[name] - 1 and not bool((caps[0, 0, 1:] == ref.EOS).any())     # the row without <eos>
    assert len(set(want["lengths"].flatten().tolist())) >= 2                                            # <eos> at mixed positions
    on_cache = bool(capi.decode_plan(functional._dims(feats, tuple(p.detach() for p in m._hip_params())), encode_only=False)[1])
    assert on_cache == (name == "mid64")                 # tiny: fp32 launches per timestep; mid64: plane path with the decode cache
    for alpha in (0.0, 0.7):
        got = m(feats, targets=caps.to(DEV), mode="score", length_alpha=alpha)
        assert tuple(got[0].shape) == tuple(caps.shape[:2]) and tuple(got[2].shape) == tuple(caps.shape[:2]) + (caps.shape[2] - 1,)
        _check_against_fp64(got, want, alpha, "%s K=%d" % (name, K))
    capi.check_async_error(True)
    entry = functional._DECODE_CACHES.get(m)
    assert (entry is not None and entry[2]) == on_cache


# ------------------------------------------------------------------ 3. against the pinned paths
def test_scores_of_beam_hypotheses_are_the_beams_and_the_train_logits(lib):
    name = "mid64"
    dims = ref.CASES[name][0]
    sd, feats, _, _ = ref.case_inputs(name)
    m, f = _model(dims, sd), feats.to(DEV)
    B, L = dims[0], dims[1]
    ids, lens, bscores = m(f, mode="beam", beam_width=5, max_beam_depth=12, n_best=5, length_alpha=0.7)
    caps = torch.cat([torch.full((B, 5, 1), ref.SOS, dtype=torch.long, device=DEV), ids], dim=2)        # [B, 5, 13], <eos>-padded
    scores, lengths, tlp = m(f, targets=caps, mode="score", length_alpha=0.7)
    assert torch.equal(lengths, lens)
    e_beam = float((scores - bscores).abs().max())
    # the same captions through mode='train' logits + torch log_softmax
    e_train = 0.0
    for k in range(5):
        inp = torch.full((B, L - 1), ref.EOS, dtype=torch.long, device=DEV)
        inp[:, :12] = caps[:, k, :-1]
        with torch.no_grad():
            logits = m(f, targets=inp, mode="train")[:, :12]
        lp = torch.log_softmax(logits, dim=-1).gather(2, caps[:, k, 1:, None])[..., 0].clamp(max=0.0)
        keep = torch.arange(12, device=DEV)[None, :] < lengths[:, k, None]
        e_train = max(e_train, float(((tlp[:, k] - lp) * keep).abs().max()))
    print("mid64 beam hypotheses: |score - beam score| %.3g, |token log-prob - train log_softmax| %.3g" % (e_beam, e_train))
    assert e_beam <= 2e-4, e_beam              # each side within 1e-4 of fp64
    assert e_train <= 1e-4, e_train
    capi.check_async_error(True)


# ------------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("name", ["tiny", "mid64"])
def test_views_shapes_and_determinism(lib, name):
    m, feats, caps, want = _case(name, 3 if name == "mid64" else 2)
    B, K, T = caps.shape
    cd = caps.to(DEV)
    a = m(feats, targets=cd, mode="score")
    b = m(feats, targets=cd, mode="score")
    assert all(torch.equal(x, y) for x, y in zip(a, b))                      # deterministic
    # the same K sentences against every clip: an expanded stride-0 view and its contiguous copy
    shared = cd[0][None].expand(B, -1, -1)
    assert shared.stride(0) == 0 and not shared.is_contiguous()
    v = m(feats, targets=shared, mode="score", length_alpha=0.0)
    c = m(feats, targets=shared.contiguous(), mode="score", length_alpha=0.0)
    assert all(torch.equal(x, y) for x, y in zip(v, c))
    assert torch.equal(v[0][0], m(feats, targets=cd, mode="score", length_alpha=0.0)[0][0])      # clip 0 scores its own captions
    # a column slice of a wider tensor (row stride > T), and [B, T] = the K = 1 result of [B, 1, T] squeezed
    wide = torch.full((B, K, T + 3), ref.EOS, dtype=torch.long, device=DEV)
    wide[..., :T] = cd
    w = m(feats, targets=wide[..., :T], mode="score")
    assert all(torch.equal(x, y) for x, y in zip(a, w))
    one = m(feats, targets=cd[:, 1], mode="score")
    k1 = m(feats, targets=cd[:, 1:2], mode="score")
    assert tuple(one[0].shape) == (B,) and tuple(one[1].shape) == (B,) and tuple(one[2].shape) == (B, T - 1)
    assert all(torch.equal(x, y.squeeze(1)) for x, y in zip(one, k1))
    # a caption's score does not depend on its neighbours (another row count may take another step kernel: each side is within
    # 1e-4 of fp64, so within 2e-4 of the other)
    assert torch.equal(one[1], a[1][:, 1]) and float((one[0] - a[0][:, 1]).abs().max()) <= 2e-4
    capi.check_async_error(True)


def test_first_call_fills_the_cache_and_a_weight_change_refreshes_it(lib):
    name = "mid64"
    m, feats, caps, want = _case(name, 1)
    cd = caps.to(DEV)
    assert functional._DECODE_CACHES.get(m) is None                          # a freshly built model: no images yet
    first = m(feats, targets=cd, mode="score", length_alpha=0.0)
    _check_against_fp64(first, want, 0.0, "mid64 first call")
    entry = functional._DECODE_CACHES.get(m)
    assert entry is not None and entry[2]
    assert torch.equal(m(feats, targets=cd, mode="score", length_alpha=0.0)[0], first[0])      # the cached images give the same
    # an optimiser-style in-place step: the version counters move, the next call must see the new weights
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.02)
    after = m(feats, targets=cd, mode="score", length_alpha=0.0)
    assert float((after[0] - first[0]).abs().max()) > 1e-2
    was = functional.DECODE_CACHE
    functional.DECODE_CACHE = False                                           # the fp32-MFMA path reads the weights themselves
    try:
        plain = m(feats, targets=cd, mode="score", length_alpha=0.0)
    finally:
        functional.DECODE_CACHE = was
    e = float((after[0] - plain[0]).abs().max())
    print("mid64 after a weight change: plane path vs fp32-MFMA path %.3g" % e)
    assert e <= 2e-4 and torch.equal(after[1], plain[1])                      # each within 1e-4 of fp64
    capi.check_async_error(True)


def test_other_modes_are_unchanged_after_a_score_call(lib, golden):
    g = golden("tiny")
    d = synth.CONFIGS["tiny"]
    seed = int(g["seed"])
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=float(g["out_scale"]))
    feats, caps, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    m = _model((d["B"], d["L"], d["F"], d["H"], d["E"], d["V"]), sd)
    f = feats.to(DEV)

    def others():
        beam = m(f, mode="beam_search", beam_width=int(g["beam_width"]), max_beam_depth=30)
        return m(f, mode="test").cpu(), [[int(t.item()) for t in s] for s in beam]
    ids0, beam0 = others()
    scores, lengths, _ = m(f, targets=caps.to(DEV), mode="score")
    assert bool(torch.isfinite(scores).all()) and int(lengths.min()) >= 1
    ids1, beam1 = others()
    assert torch.equal(ids0, ids1) and beam0 == beam1
    for b, s in enumerate(beam1):
        assert s == [int(x) for x in g["beam_ids"][b] if x >= 0]
    capi.check_async_error(True)


# ------------------------------------------------------------------ 5. errors
@pytest.mark.parametrize("name", ["tiny", "mid64"])
def test_an_id_outside_the_vocabulary_is_reported_and_clamped(lib, name):
    m, feats, caps, want = _case(name, 2)
    V = ref.CASES[name][0][5]
    capi.check_async_error(True)
    bad = caps.clone()
    bad[1, 1, T_OF[name] - 1] = V                   # behind the caption's <eos> or not: every id of the tensor is checked
    m(feats, targets=bad.to(DEV), mode="score")
    torch.cuda.synchronize()
    with pytest.raises((capi.S2VTHipError, IndexError)):
        capi.check_async_error(True)
    capi.check_async_error(True)                    # reported once
    got = m(feats, targets=caps.to(DEV), mode="score", length_alpha=0.0)
    _check_against_fp64(got, want, 0.0, "%s after a bad id" % name)
    capi.check_async_error(True)


def test_unsupported_models_and_cpu_tensors(lib):
    import S2VTModel
    caps = torch.full((2, 4), ref.EOS, dtype=torch.long, device=DEV)
    x = torch.zeros(2, 8, 64, device=DEV)                            # (the tiny case's dims)
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        other = S2VTModel.S2VT(50, 64, 8, dim_hid=32, dim_embed=24, **kw).to(DEV).eval()
        with pytest.raises(NotImplementedError, match="mode='train'"):
            other(x, targets=caps, mode="score")
    m = S2VTModel.S2VT(50, 64, 8, dim_hid=32, dim_embed=24).to(DEV).eval()
    with pytest.raises(capi.S2VTHipError):
        m(x.cpu(), targets=caps, mode="score")
    with pytest.raises(capi.S2VTHipError):
        m(x, targets=caps.cpu(), mode="score")
    scores, lengths, tlp = m(x, targets=caps, mode="score")          # (and the smallest legal call works)
    assert tuple(scores.shape) == (2,) and lengths.tolist() == [1, 1] and tuple(tlp.shape) == (2, 3)
