"""CPU: the ensemble beam search (S2VTModel.Ensemble, csrc/ensemble.hip, include/s2vt_hip.h "ensemble beam") - the C ABI's
surface, the argument checks that come before any device call, the refusals of Ensemble and eval.py, the float32 restatement of
the head against the fp64 one, and the CPU preconditions of test_gpu_ensemble.py (how many rows / samples the fp64 reference alone
leaves undecided)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as cum  # noqa: E402
import ensemble_ref as ref  # noqa: E402

NEW = ("s2vt_ensemble_top20", "s2vt_ensemble_top20_constrained", "s2vt_beam_step_logits")

# ---- shared with test_gpu_ensemble.py
HEAD_V = (50, 4097, 16385)          # RegRow<16>'s smallest size, the first past a bracket edge, the first LdsRow size
HEAD_ROWS = (3, 65)
HEAD_M = (1, 2, 3, 4)
HEAD_EXTRA_V = (8193, 12289)        # RegRow<48>, RegRow<64>: rows = 3, M = 3 (the recipe's own seed passes the gap condition)
MAX_LEFT_OUT = {3: 1, 65: 5}        # rows of a case that the gap condition may leave out
# samples of the whole-path cases whose decisions are clear in fp64 (both gaps >= beam_cum_ref.ROBUST_GAP); "mixed": members of
# dim_hid 32 and 48 on the tiny dims
ROBUST = {"tiny": 8, "tiny5": 5, "mid64": 55, "mixed": 7}


# ---- the C ABI
def test_new_symbols_declared_exported_bound_and_abi_9(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in capi.SIGNATURES, name
    assert "ensemble beam" in header
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9


def _lw(*vals):
    return (ctypes.c_float * len(vals))(*vals)


def test_library_refusals_come_before_the_device(lib):
    """made-up addresses stand for device memory: every rejection happens before anything is enqueued"""
    one = ctypes.c_void_p(256)
    half = float(np.log(0.5))

    def head(logits=one, stride=4 * 30, ld=30, M=2, rows=4, V=30, lw=_lw(half, half), ix=one, lp=one):
        return lib.s2vt_ensemble_top20(logits, stride, ld, M, rows, V, lw, ix, lp, None)
    bad = (dict(logits=None), dict(lw=None), dict(ix=None), dict(lp=None), dict(M=0), dict(M=9, lw=_lw(*([-3.0] * 9))), dict(V=19, ld=19),
           dict(V=38401, ld=38401, stride=4 * 38401), dict(ld=29), dict(stride=4 * 30 - 1), dict(rows=0), dict(lw=_lw(half, 0.25)),
           dict(lw=_lw(half, float("nan"))), dict(lw=_lw(float("-inf"), half)))
    for kw in bad:
        assert head(**kw) == -1, kw
        assert b"s2vt_ensemble_top20" in lib.s2vt_last_error() and b"constrained" not in lib.s2vt_last_error(), kw

    banned = (ctypes.c_int32 * 2)(5, 7)
    con = capi.Constraints()
    con.no_repeat_ngram, con.repetition_penalty, con.min_length, con.n_banned, con.eos_ix = 2, 1.2, 0, 2, 4
    con.banned = ctypes.cast(banned, type(con.banned))

    def chead(logits=one, stride=4 * 60, ld=60, M=2, rows=4, V=60, lw=_lw(half, half), hist=one, hist_ld=16, t=3, c=con, ix=one, lp=one):
        return lib.s2vt_ensemble_top20_constrained(logits, stride, ld, M, rows, V, lw, hist, hist_ld, t, ctypes.byref(c) if c else None,
                                                   ix, lp, None)
    for kw in bad + (dict(c=None), dict(t=-1), dict(t=1024), dict(hist=None), dict(hist_ld=2), dict(V=25, ld=25, stride=100)):
        kw = dict(kw)
        if kw.get("stride") == 4 * 30 - 1:
            kw["stride"] = 4 * 60 - 1
        if kw.get("ld") == 29:
            kw["ld"] = 59
        assert chead(**kw) == -1, kw
        assert b"s2vt_ensemble_top20_constrained" in lib.s2vt_last_error(), kw

    d = capi.Dims(4, 6, 16, 8, 8, 30)
    prm = capi.Params()
    big = 1 << 40

    def step(logits=one, ld=30, ws=one, nbytes=big, gx=None, cache=None, rows=one):
        return lib.s2vt_beam_step_logits(ctypes.byref(d), ctypes.byref(prm), 8, rows, one, one, one, one, one, one, gx, one, one, one, one,
                                         logits, ld, ws, nbytes, cache, 0, None)
    for kw in (dict(logits=None), dict(ld=29), dict(gx=one)):
        assert step(**kw) == -1, kw
        assert b"s2vt_beam_step_logits" in lib.s2vt_last_error(), kw
    for kw in (dict(ws=None), dict(nbytes=16), dict(rows=None)):
        assert step(**kw) == -1, kw


def test_log_weights():
    lw = ops.ensemble_log_weights(None, 4)
    assert list(lw) == [float(np.float32(np.log(0.25)))] * 4
    lw = ops.ensemble_log_weights([5, 3, 2], 3)
    assert list(lw) == [float(np.float32(np.log(w))) for w in (0.5, 0.3, 0.2)]
    assert list(ops.ensemble_log_weights([7.0], 1)) == [0.0]
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, 0.0], [1.0, -1.0], [1.0, float("nan")], [1.0, float("inf")], [1.0, "x"], 3.0):
        with pytest.raises(ValueError, match="Ensemble:"):
            ops.ensemble_log_weights(bad, 2)


# ---- Ensemble's refusals
def _s2vt(V=60, F=16, L=5, H=8, E=8, **kw):
    import S2VTModel
    return S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, **kw)


def test_ensemble_refusals_come_before_the_device():
    import S2VTModel
    assert S2VTModel.Ensemble.__module__ == "s2vt_video_caption_amd.ensemble"
    a, b = _s2vt(), _s2vt(H=12, E=4)                     # dim_hid and dim_embed may differ
    S2VTModel.Ensemble([a, b])
    S2VTModel.Ensemble([a, b], weights=[2, 1])
    for models, w in (([], None), ([a] * 9, None), ([a, b], [1.0]), ([a, b], [1.0, 0.0]), ([a, b], [1.0, float("nan")]),
                      ([a, b], [1.0, float("inf")]), ([a, b], [-1.0, 2.0])):
        with pytest.raises(ValueError, match="Ensemble:"):
            S2VTModel.Ensemble(models, w)
    for attr, kw in (("vocab_size", dict(V=61)), ("length", dict(L=6)), ("feat_dim", dict(F=17)), ("sos_ix", dict(sos_ix=2)),
                     ("eos_ix", dict(eos_ix=5))):
        with pytest.raises(ValueError, match=attr):
            S2VTModel.Ensemble([a, _s2vt(**kw)])
    x = torch.zeros(2, 5, 16)                            # a CPU tensor: a bad argument is refused before the tensor is looked at
    ens = S2VTModel.Ensemble([a, b])
    for kw in (dict(beam_width=0), dict(beam_width=9), dict(n_best=6), dict(max_beam_depth=0), dict(length_alpha=-1.0)):
        with pytest.raises(ValueError, match="mode='beam'"):
            ens.beam(x, **kw)
    with pytest.raises(ValueError, match="repetition_penalty"):
        ens.beam(x, repetition_penalty=0.5)
    with pytest.raises(ValueError, match="beam_constrained: vocab_size"):
        ens.beam(x, max_beam_depth=40, no_repeat_ngram_size=2)          # 60 < 20 + 40 + 0 + 1
    with pytest.raises(ValueError, match=re.escape(S2VTModel._BEAM_GRU)):
        S2VTModel.Ensemble([a, _s2vt(rnn_type="gru")]).beam(x)
    with pytest.raises(ValueError, match=re.escape(S2VTModel._BEAM_STACKED)):
        S2VTModel.Ensemble([_s2vt(num_layers=2), a]).beam(x)
    with pytest.raises(capi.S2VTHipError):               # good arguments: the CPU tensor fails loudly
        ens.beam(x)
    sig = inspect.signature(S2VTModel.Ensemble.beam)
    assert list(sig.parameters)[1:] == ["feats", "beam_width", "max_beam_depth", "length_alpha", "n_best", "no_repeat_ngram_size",
                                        "repetition_penalty", "min_length", "banned_ids"]
    assert (sig.parameters["beam_width"].default, sig.parameters["max_beam_depth"].default, sig.parameters["length_alpha"].default) == (5, 30, 0.7)


def test_eval_flags_and_refusals():
    sys.path.insert(0, ROOT)
    import eval as ev
    a = ev.build_parser().parse_args(["--model-path", "m.pth"])
    assert (a.ensemble, a.ensemble_weights) == ("", "")
    a = ev.build_parser().parse_args(["--model-path", "m.pth", "--ensemble", "a.pth,b.pth", "--ensemble-weights", "0.5,0.3,0.2"])
    assert (a.ensemble, a.ensemble_weights) == ("a.pth,b.pth", "0.5,0.3,0.2")
    base = ["--model-path", "m.pth", "--ensemble", "a.pth"]
    for bad in (base,                                                                  # no --beam
                base + ["--beam", "3"],                                                # --beam-mode reference (the default)
                base + ["--beam", "3", "--beam-mode", "reference"],
                base + ["--beam", "4", "--beam-mode", "cumulative", "--beam-groups", "2"],
                base + ["--beam", "3", "--beam-mode", "cumulative", "--sample", "2"],
                base + ["--beam", "3", "--beam-mode", "cumulative", "--perplexity"],
                base + ["--beam", "3", "--beam-mode", "cumulative", "--ensemble-weights", "1,2,3"],
                base + ["--beam", "3", "--beam-mode", "cumulative", "--ensemble-weights", "1,x"],
                ["--model-path", "m.pth", "--beam", "3", "--beam-mode", "cumulative", "--ensemble-weights", "1,2"]):
        with pytest.raises(SystemExit):
            ev.main(bad)
    sig = inspect.signature(ev.generate)
    assert list(sig.parameters)[-2:] == ["ensemble_paths", "ensemble_weights"]
    assert sig.parameters["ensemble_paths"].default is None and sig.parameters["ensemble_weights"].default is None


# ---- the restatements and the CPU preconditions of the GPU tests
def test_combine_known_answers():
    x = np.log(np.array([[[0.5, 0.25, 0.25]], [[0.1, 0.6, 0.3]]]))
    for w, mean in ((None, [0.3, 0.425, 0.275]), ([3, 1], [0.4, 0.3375, 0.2625])):
        assert np.allclose(np.exp(ref.combine64(x + 7.0, w)), mean, rtol=1e-12)       # (a shift of the logits changes nothing)
        assert np.allclose(np.exp(ref.combine_f32(x, w)), mean, rtol=1e-6)
    one = (3.0 * np.random.RandomState(1).randn(1, 4, 300)).astype(np.float32)
    a = (one[0] - ref.lse_f32(one[0])[:, None]).astype(np.float32)
    assert np.array_equal(ref.combine_f32(one, [1.0]).view(np.uint32), a.view(np.uint32))     # M = 1: c = a_0 exactly
    x = (3.0 * np.random.RandomState(2).randn(2, 3, 40)).astype(np.float32)
    x[:, :, 5] = -np.inf                                                 # a word at -inf in every member, one in one member only
    x[0, :, 9] = -np.inf
    for c in (ref.combine64(x), ref.combine_f32(x)):
        assert np.isneginf(c[:, 5]).all() and np.isfinite(np.delete(c, 5, axis=1)).all() and not np.isnan(c).any()


@pytest.mark.parametrize("V", HEAD_V)
def test_head_fixtures_in_float32_and_the_rows_fp64_decides(V):
    for rows in HEAD_ROWS:
        for M in HEAD_M:
            x, w = ref.head_case(V, rows, M)
            c64 = ref.combine64(x, w)
            err = float(np.abs(ref.combine_f32(x, w) - c64).max())
            ids, vals, ok = ref.top20_of(c64)
            print("V=%d rows=%d M=%d: max |combine_f32 - combine64| = %.3g, %d rows left out" % (V, rows, M, err, int((~ok).sum())))
            assert err <= ref.HEAD_TOL
            assert int((~ok).sum()) <= MAX_LEFT_OUT[rows]
            assert (np.diff(ids, axis=1) > 0).all() and np.isfinite(vals).all()


def test_head_extra_fixtures():
    for V in HEAD_EXTRA_V:
        x, w = ref.head_case(V, 3, 3)
        c64 = ref.combine64(x, w)
        assert ref.top20_of(c64)[2].all()                                 # (no seed shift needed)
        assert float(np.abs(ref.combine_f32(x, w) - c64).max()) <= ref.HEAD_TOL
    x, w = ref.head_case(50, 3, 8)
    assert int((~ref.top20_of(ref.combine64(x, w))[2]).sum()) <= MAX_LEFT_OUT[3]


@pytest.mark.parametrize("name", ["tiny", "tiny5", "mid64", "mixed"])
def test_whole_path_cases_robust_counts(name):
    res = ref.case_search(name)
    rb = cum.robust(res)
    assert int(rb.sum()) == ROBUST[name], (name, int(rb.sum()))
    assert 2 * int(rb.sum()) >= len(res)
    assert all(len(r["ids"]) == len(r["scores"]) for r in res)
    assert all(np.all(np.diff(r["scores"]) <= 0) for r in res)


def test_search_with_one_member_is_the_single_model_search():
    sd, feats, W, D = cum.case_inputs("tiny")
    a = cum.case_search("tiny")
    b = ref.search_fp64([sd], None, feats, W, D)
    for x, y in zip(a, b):
        assert x["ids"] == y["ids"] and np.allclose(x["scores"], y["scores"], rtol=0, atol=1e-12)
    c = ref.search_fp64([sd, sd, sd], None, feats, W, D)                  # copies of one model: the same distribution
    for x, y in zip(a, c):
        assert x["ids"] == y["ids"] and np.allclose(x["scores"], y["scores"], rtol=0, atol=1e-9)
