"""CPU: the constrained cumulative-score beam search (S2VT.beam_constrained; include/s2vt_hip.h "constrained beam") - the fp64
restatement the GPU tests compare against (tests/beam_constrained_ref.py: how many samples of each case decide clearly, that every
hypothesis keeps the constraints, that default constraints give the unconstrained search), the argument checks that come before
the library, the signatures, the C ABI's surface and eval.py's flags."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import beam_constrained_ref as cref  # noqa: E402

# (case, spec) -> robust samples (both gaps >= beam_cum_ref.ROBUST_GAP), measured with the fp64 restatement; the GPU tests assert the
# same counts.  tiny5 under spec B has 4 of 8 and is not used: it breaks the cap of three quarters.
ROBUST = {("tiny", cref.SPEC_A): 8, ("tiny5", cref.SPEC_A): 6, ("mid64", cref.SPEC_A): 59,
          ("tiny", cref.SPEC_B): 8, ("mid64", cref.SPEC_B): 54}
# rows of mid64 whose constrained greedy caption (spec A) has a top-2 margin >= 1e-5 at every step up to its first <eos>
WIDTH_ONE_ROWS = 64
NEW = ("s2vt_beam_cum_hist_bytes", "s2vt_beam_cum_hist_step", "s2vt_top20_logprob_constrained", "s2vt_beam_step_constrained")


@pytest.mark.parametrize("name,spec_args", sorted(ROBUST))
def test_robust_counts_and_constraints_hold(name, spec_args):
    """at least three quarters of a batch decide every selection and the n-best order by >= 2e-4, the counts are pinned, and EVERY
    returned fp64 hypothesis - robust or not - keeps the constraints"""
    res = cref.case_search(name, spec_args)
    rb = ref.robust(res)
    B, W = len(res), ref.CASES[name][3]
    print("%s %r: robust %d/%d" % (name, spec_args, int(rb.sum()), B))
    assert 4 * int(rb.sum()) >= 3 * B
    assert int(rb.sum()) == ROBUST[(name, spec_args)]
    spec = cref.spec_of(spec_args, ref.CASES[name][0][5])
    for r in res:
        assert len(r["ids"]) == W
        for ids in r["ids"]:
            assert cref.satisfies(ids, spec), ids
            if spec_args == cref.SPEC_A:                     # spelled out once, beside the helper
                assert not set(ids) & {5, 7} and ref.EOS not in ids[:4]
                grams = list(zip(ids, ids[1:]))
                assert len(grams) == len(set(grams))


def test_the_constraints_change_the_answer():
    """the unconstrained best hypothesis repeats a bigram on some samples of mid64, and spec A changes most best captions"""
    plain = ref.case_search("mid64")
    spec = cref.spec_of(cref.SPEC_B, 1000)
    assert any(not cref.satisfies(r["ids"][0], spec) for r in plain)
    con = cref.case_search("mid64", cref.SPEC_A)
    assert sum(a["ids"][0] != b["ids"][0] for a, b in zip(plain, con)) >= 32


def test_default_constraints_are_the_unconstrained_search():
    for name in ("tiny", "tiny5"):
        sd, feats, W, D = ref.case_inputs(name)
        off = cref.spec_of((0, 1.0, 0, ()), ref.CASES[name][0][5])
        assert not sampling.constrains(off)
        assert cref.search_fp64(sd, feats, W, D, off) == ref.case_search(name)


def test_width_one_rows_are_pinned():
    """the rows the GPU's width-1 test compares: clear constrained greedy margins, at least 48 of 64"""
    g = cref.greedy_search("mid64", cref.SPEC_A)
    rows = sum(r["cand_gap"] >= 1e-5 for r in g)
    assert rows == WIDTH_ONE_ROWS and rows >= 48
    spec = cref.spec_of(cref.SPEC_A, 1000)
    assert all(cref.satisfies(r["ids"][0], spec) for r in g)
    assert sum(r["ids"][0][-1] == ref.EOS for r in g) >= 8       # (the cut at <eos> is exercised)


def test_policy_with_histories_is_the_policy():
    """PolicyHist shows the token lists PolicyF32 keeps, per live row"""
    rng = np.random.RandomState(5)
    B, W, D = 2, 3, 4
    pol = cref.PolicyHist(B, W, D, 0.7)
    h, live = pol.histories()
    assert not h.any() and live.tolist() == [True, False, False] * B
    for t in range(1, D + 1):
        ix = np.stack([np.sort(rng.choice(np.arange(5, 50), 20, replace=False)) for _ in range(B * W)]).astype(np.int32)
        pol.step(ix, (-3.0 * rng.rand(B * W, 20)).astype(np.float32))
        h, live = pol.histories()
        for b in range(B):
            for j, (_, tk, _, _) in enumerate(pol.live[b]):
                assert len(tk) == t and h[b * W + j, :t].tolist() == tk and live[b * W + j]
        assert int(live.sum()) == sum(len(l) for l in pol.live)


def test_signatures():
    import S2VTModel
    S = S2VTModel.S2VT
    sig = inspect.signature(S.beam_constrained)
    assert list(sig.parameters) == ["self", "feats", "beam_width", "max_beam_depth", "length_alpha", "n_best", "no_repeat_ngram_size",
                                    "repetition_penalty", "min_length", "banned_ids"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [3, 30, 0.7, 1, 0, 1.0, 0, None]
    assert list(inspect.signature(S.forward).parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob",
                                                             "ss_temperature", "length_alpha", "n_best", "temperature", "seed"]
    sig = inspect.signature(beam.beam_cumulative)
    assert list(sig.parameters)[-1] == "constraints" and sig.parameters["constraints"].default is None


def test_argument_errors_before_the_library():
    import S2VTModel
    x = torch.zeros(2, 5, 16)                       # a CPU tensor: a bad argument is refused before the tensor is looked at
    m = S2VTModel.S2VT(60, 16, 5, dim_hid=8, dim_embed=8)
    ok = dict(no_repeat_ngram_size=2)
    for kw, match in ((dict(max_beam_depth=38, banned_ids=[5, 7]), "vocab_size"),            # 20 + 38 + 2 + 1 = 61 > 60 (59 without the ids)
                      (dict(max_beam_depth=40), "vocab_size"),
                      (dict(beam_width=9), "mode='beam'"), (dict(n_best=4), "mode='beam'"), (dict(length_alpha=-1.0), "mode='beam'"),
                      (dict(repetition_penalty=0.5), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                      (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(min_length=-1), "min_length"),
                      (dict(banned_ids=[60]), "banned_ids")):
        with pytest.raises(ValueError, match=match):
            m.beam_constrained(x, **dict(ok, **kw))
    big = S2VTModel.S2VT(2000, 16, 5, dim_hid=8, dim_embed=8)
    with pytest.raises(ValueError, match="max_beam_depth 1024"):
        big.beam_constrained(x, max_beam_depth=1024, **ok)
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        other = S2VTModel.S2VT(60, 16, 5, dim_hid=8, dim_embed=8, **kw)
        with pytest.raises(ValueError, match="mode='beam' of a"):
            other.beam_constrained(x, **ok)
    # good arguments: the CPU tensor fails loudly, constrained or not
    with pytest.raises(capi.S2VTHipError):
        m.beam_constrained(x, max_beam_depth=38, **ok)
    with pytest.raises(capi.S2VTHipError):
        m.beam_constrained(x)
    spec = sampling.check_constraints(2, 1.0, 0, [5, 7], 60, 4)
    beam.check_beam_constraints(spec, 37, 60)
    with pytest.raises(ValueError):
        beam.check_beam_constraints(spec, 38, 60)


def test_header_declares_and_capi_binds_the_new_symbols(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and name in capi.SIGNATURES and hasattr(lib, name), name
    assert lib.s2vt_abi_version() == 9              # the API is additive
    nb, nh = lib.s2vt_beam_cum_bytes(64, 5, 12), lib.s2vt_beam_cum_hist_bytes(64, 5, 12)
    assert nh >= nb + 2 * 64 * 5 * 12 * 4
    for bad in ((0, 5, 12), (64, 9, 12), (64, 5, 0)):
        assert lib.s2vt_beam_cum_hist_bytes(*bad) == 0, bad


def test_c_abi_refuses_bad_arguments_before_a_launch(lib):
    import ctypes
    p = ctypes.c_void_p(256)                        # never dereferenced: every call below is refused before a launch
    out, ld = ctypes.c_void_p(), ctypes.c_int64()
    rc = lib.s2vt_beam_cum_hist_step(4, 3, 6, 3, 4, 0.7, 1, p, 1 << 20, p, p, p, p, p, None, ctypes.byref(ld), None)
    assert rc == -1 and b"s2vt_beam_cum_hist_step" in lib.s2vt_last_error()
    rc = lib.s2vt_beam_cum_hist_step(4, 9, 6, 3, 4, 0.7, 1, p, 1 << 20, p, p, p, p, p, ctypes.byref(out), ctypes.byref(ld), None)
    assert rc == -1 and b"s2vt_beam_cum_hist_step" in lib.s2vt_last_error()
    rc = lib.s2vt_beam_cum_hist_step(4, 3, 6, 3, 4, 0.7, 1, p, lib.s2vt_beam_cum_bytes(4, 3, 6), p, p, p, p, p, ctypes.byref(out),
                                     ctypes.byref(ld), None)
    assert rc == -1 and b"state" in lib.s2vt_last_error()          # the plain state is too small for the form with histories

    def head(V=50, rows=3, t=2, hist=p, hist_ld=8, n=2, theta=1.0, m=0, banned=(), ix=p):
        arr = (ctypes.c_int32 * max(1, len(banned)))(*banned)
        c = capi.Constraints(n, theta, m, 4, len(banned), ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)))
        return lib.s2vt_top20_logprob_constrained(p, V, rows, V, hist, hist_ld, t, ctypes.byref(c), ix, p, None)
    for kw in (dict(V=19), dict(V=38401), dict(rows=0), dict(t=-1), dict(t=1024, V=2000, hist_ld=2000), dict(hist=None), dict(hist_ld=1),
               dict(theta=0.5), dict(n=-1), dict(m=-1), dict(banned=(50,)), dict(ix=None),
               dict(V=24, t=2, banned=(5, 7)),          # 20 + 2 + 2 + 1 = 25 > 24: a row could keep fewer than 20 words
               dict(V=30, t=10, hist_ld=10)):
        rc = head(**kw)
        assert rc == -1 and b"s2vt_top20_logprob_constrained" in lib.s2vt_last_error(), kw


def test_eval_accepts_the_flags_with_the_cumulative_beam_only(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval as ev
    with pytest.raises(SystemExit):                      # the reference's search: refused before a model is loaded
        ev.main(["--model-path", "m.pth", "--beam", "3", "--beam-mode", "reference", "--no-repeat-ngram", "2"])
    with pytest.raises(SystemExit):
        ev.main(["--model-path", "m.pth", "--beam", "3", "--min-length", "2"])
    seen = {}

    def generate(*args, **kw):
        seen["mode"], seen["kw"] = args[4], kw
        return {}
    monkeypatch.setattr(ev, "generate", generate)
    ev.main(["--model-path", "m.pth", "--beam", "3", "--beam-mode", "cumulative", "--no-repeat-ngram", "2", "--ban-words", "<unk>",
             "--out", str(tmp_path / "out.json")])
    assert seen["mode"] == "beam" and seen["kw"]["beam_width"] == 3
    assert seen["kw"]["constraints"] == dict(no_repeat_ngram_size=2, repetition_penalty=1.0, min_length=0, ban_words=["<unk>"])

