"""CPU: diverse (group) beam search (S2VT.beam_diverse; include/s2vt_hip.h "diverse beam") - the restatements the GPU tests compare
against (tests/beam_div_ref.py: their identities with the cumulative-score search, how many samples of each case decide clearly, what
the penalty does), the fp32 policy against the fp64 search, the argument checks that come before the library, the signatures, the
C ABI's surface and eval.py's flags."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import beam_constrained_ref as cref  # noqa: E402
import beam_div_ref as dref  # noqa: E402

# (inputs of a beam_cum_ref case, D, G, Wg, lambda, constraint spec) -> robust samples (both gaps >= beam_cum_ref.ROBUST_GAP), measured
# with the fp64 restatement; the GPU tests assert the same counts.  Every case keeps the cap: at least three quarters of its batch.
ROBUST = {("tiny", 10, 2, 2, 0.5, None): 8, ("tiny", 10, 3, 1, 0.5, None): 7, ("tiny5", 12, 4, 2, 0.5, None): 7,
          ("tiny5", 12, 3, 2, 1.0, None): 8, ("mid64", 12, 3, 2, 0.5, None): 57, ("mid64", 12, 4, 2, 0.5, None): 56,
          ("mid64", 12, 8, 1, 0.5, None): 58, ("mid64", 12, 2, 3, 1.0, None): 62,
          ("tiny", 10, 2, 2, 0.5, cref.SPEC_A): 8, ("tiny5", 12, 4, 2, 0.5, cref.SPEC_A): 8, ("mid64", 12, 3, 2, 0.5, cref.SPEC_A): 61,
          ("mid64", 12, 4, 2, 0.5, cref.SPEC_A): 58, ("mid64", 12, 3, 2, 0.5, cref.SPEC_B): 54}
CASE_IDS = ["%s-D%d-G%d-Wg%d-lam%g-%s" % (c[0], c[1], c[2], c[3], c[4], {None: "plain", cref.SPEC_A: "specA", cref.SPEC_B: "specB"}[c[5]])
            for c in ROBUST]
NEW = ("s2vt_beam_div_bytes", "s2vt_beam_div_step", "s2vt_beam_div_result")


def _close(a, b):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0.0, atol=1e-9)


# ------------------------------------------------------------------ identities of the restatement
def test_one_group_is_the_cumulative_search():
    for name in ("tiny", "tiny5"):
        sd, feats, W, D = ref.case_inputs(name)
        want = ref.case_search(name)
        got = dref.search_fp64(sd, feats, W, 1, 0.5, D)
        for g, w in zip(got, want):
            assert g["ids"] == [w["ids"]] and _close(g["scores"][0], w["scores"])
            assert g["cand_gap"] == w["cand_gap"] and g["pool_gap"] == w["pool_gap"] and not g["changed"]


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_groups_against_the_cumulative_search_at_the_group_width(lam):
    """lambda = 0: EVERY group is mode='beam' at width Wg; any lambda: group 0 is"""
    name, G, Wg = "tiny5", 3, 2
    sd, feats, _, D = ref.case_inputs(name)
    want = ref.search_fp64(sd, feats, Wg, D)
    got = dref.search_fp64(sd, feats, G * Wg, G, lam, D)
    for g, w in zip(got, want):
        for k in range(G if lam == 0.0 else 1):
            assert g["ids"][k] == w["ids"] and _close(g["scores"][k], w["scores"]), k
        assert g["changed"] == (lam > 0)                     # (on this case the penalty changes a selection on every sample)


def test_a_spec_that_constrains_nothing_is_the_unconstrained_search():
    from s2vt_video_caption_amd import sampling
    name, D, G, Wg, lam = "tiny", 10, 2, 2, 0.5
    sd, feats, _, _ = ref.case_inputs(name)
    off = cref.spec_of((0, 1.0, 0, ()), ref.CASES[name][0][5])
    assert not sampling.constrains(off)
    assert dref.search_fp64(sd, feats, G * Wg, G, lam, D, off) == dref.case_search(name, D, G, Wg, lam)


# ------------------------------------------------------------------ the cases of the GPU tests
@pytest.mark.parametrize("case", sorted(ROBUST, key=str), ids=sorted(CASE_IDS))
def test_robust_counts_and_what_the_penalty_does(case):
    """at least three quarters of a batch decide every selection and every pool order by >= 2e-4 and the counts are pinned; on every
    sample the penalty changed at least one selection and the groups' best captions are pairwise distinct; under a spec EVERY
    returned hypothesis keeps the constraints"""
    name, D, G, Wg, lam, spec_args = case
    res = dref.case_search(*case)
    rb = dref.robust(res)
    B = len(res)
    print("%r: robust %d/%d" % (case, int(rb.sum()), B))
    assert 4 * int(rb.sum()) >= 3 * B
    assert int(rb.sum()) == ROBUST[case]
    spec = cref.spec_of(spec_args, ref.CASES[name][0][5]) if spec_args is not None else None
    for r in res:
        assert r["changed"]
        assert len(r["ids"]) == G and all(len(g) == Wg for g in r["ids"])
        best = [tuple(g[0]) for g in r["ids"]]
        assert len(set(best)) == G, best
        for g, sc in zip(r["ids"], r["scores"]):
            assert all(len(ids) <= D for ids in g) and all(a >= b for a, b in zip(sc, sc[1:]))
            if spec is not None:
                assert all(cref.satisfies(ids, spec) for ids in g), g


# ------------------------------------------------------------------ the fp32 policy against the fp64 search
def _tops_fp64(params, feats, pol, D, spec=None, sos=ref.SOS):
    """drive PolicyDivF32 with the model's own top 20 (fp64 log-probs rounded to fp32), slot states followed through pol.rows(); with
    a spec every row is first edited with the words pol.histories() shows for its slot (rows of unused slots: zeros, never consumed)"""
    from oracle import s2vt_oracle as oracle
    from s2vt_video_caption_amd import sampling
    p = {k: v.double() for k, v in params.items()}
    feats = feats.double()
    B, L, _ = feats.shape
    W = pol.W
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    H = h2.shape[1]
    tab_h, tab_c = torch.zeros(B * W, H, dtype=torch.float64), torch.zeros(B * W, H, dtype=torch.float64)
    tab_h[:B], tab_c[:B] = h2, c2
    for t in range(D):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        rows = pol.rows()
        state, tok = torch.from_numpy(rows[0]).long(), torch.from_numpy(rows[1]).long()
        vid = h1.repeat_interleave(W, 0)
        tab_h, tab_c = oracle._word_step(p, p["embedding.weight"][tok], vid, tab_h[state], tab_c[state])
        x = tab_h @ p["out_linear.weight"].t() + p["out_linear.bias"]
        if spec is not None:
            x = torch.from_numpy(sampling.constrain_logits(x.numpy(), pol.histories()[0][:, :t].astype(np.int64), t, spec))
        lp = torch.log_softmax(x, dim=1)
        top = torch.sort(torch.sort(lp, dim=1, descending=True, stable=True).indices[:, :20], dim=1).values
        pol.step(top.numpy().astype(np.int32), lp.gather(1, top).numpy().astype(np.float32))


@pytest.mark.parametrize("case", [("tiny", 10, 2, 2, 0.5, None), ("tiny", 10, 3, 1, 0.5, None), ("tiny5", 12, 4, 2, 0.5, None),
                                  ("tiny", 10, 2, 2, 0.5, cref.SPEC_A), ("tiny5", 12, 4, 2, 0.5, cref.SPEC_A)], ids=str)
def test_the_fp32_policy_agrees_with_the_fp64_search_on_robust_samples(case):
    name, D, G, Wg, lam, spec_args = case
    spec = cref.spec_of(spec_args, ref.CASES[name][0][5]) if spec_args is not None else None
    sd, feats, _, _ = ref.case_inputs(name)
    want = dref.case_search(*case)
    rb = dref.robust(want)
    pol = dref.PolicyDivF32(feats.shape[0], G * Wg, G, D, ref.ALPHA, lam)
    rows = pol.rows().reshape(2, feats.shape[0], G, Wg)
    assert (rows[0, :, :, 0] == np.arange(feats.shape[0])[:, None]).all() and (rows[1, :, :, 0] == ref.SOS).all()
    assert not rows[:, :, :, 1:].any()
    _tops_fp64(sd, feats, pol, D, spec)
    assert pol.settled().all()
    ids, lens, scores = pol.result()
    for b in np.nonzero(rb)[0]:
        got = [[ids[b, g, k, :lens[b, g, k]].tolist() for k in range(Wg)] for g in range(G)]
        assert got == want[b]["ids"], b
        assert np.abs(scores[b] - np.array(want[b]["scores"])).max() <= 1e-4


# The input that tells the two roundings of the penalty from one (an FMA): four groups of one slot, lambda = 0.7, word 10 at s = -0.1
# far on top of every row, so group 3 sees cnt[10] == 3.  fl(0.7f * 3) is inexact: its key of word 10 is x = fl(s - fl(fl(lambda) * 3))
# = -2.1999998, where one rounding of s - lambda * 3 gives -2.2.  Word 11 of group 3's row at log-prob x loses the tie to word 10
# (token ascending) - under an FMA it would win; at the next float above x it wins either way.
TWO_S, TWO_LAM = np.float32(-0.1), 0.7
TWO_X = np.float32(TWO_S - np.float32(np.float32(TWO_LAM) * np.float32(3)))


def two_roundings_tops(B, lp11):
    """(ids, lp) [B*4][20] of that input's first depth, for B samples alike"""
    ix = np.tile(np.arange(10, 30, dtype=np.int32), (4 * B, 1))
    lp = np.full((4 * B, 20), -9.0, dtype=np.float32)
    lp[:, 0] = TWO_S
    lp[3::4, 1] = lp11
    return ix, lp


def test_the_fp32_policy_rounds_the_product_and_the_difference_separately():
    s, x = TWO_S, TWO_X
    fused = np.float32(np.float64(s) - np.float64(np.float32(TWO_LAM)) * 3.0)
    assert fused != x and fused < x                          # (an FMA's key of word 10 lies BELOW x: word 11 at x would beat it)
    for lp11, last in ((x, 10), (np.nextafter(x, np.float32(0)), 11), (fused, 10)):
        pol = dref.PolicyDivF32(2, 4, 4, 2, 0.0, TWO_LAM)
        pol.step(*two_roundings_tops(2, lp11))
        for live in pol.live:
            assert [l[0][3] for l in live] == [10, 10, 10, last], lp11
            assert [l[0][0] for l in live] == [s, s, s, s if last == 10 else lp11]       # the sums carry no penalty


# ------------------------------------------------------------------ signatures and argument checks
def test_signatures():
    import S2VTModel
    S = S2VTModel.S2VT
    sig = inspect.signature(S.beam_diverse)
    assert list(sig.parameters) == ["self", "feats", "beam_width", "num_groups", "diversity_lambda", "max_beam_depth", "length_alpha",
                                    "n_best", "no_repeat_ngram_size", "repetition_penalty", "min_length", "banned_ids"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [6, 3, 0.5, 30, 0.7, 1, 0, 1.0, 0, None]
    sig = inspect.signature(beam.beam_diverse)
    assert list(sig.parameters) == ["model", "feats", "params", "beam_width", "num_groups", "diversity_lambda", "max_depth", "length_alpha",
                                    "n_best", "constraints"]
    assert sig.parameters["constraints"].default is None
    # the pinned ones are unchanged
    assert list(inspect.signature(S.forward).parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob",
                                                             "ss_temperature", "length_alpha", "n_best", "temperature", "seed"]
    assert list(inspect.signature(S.beam_constrained).parameters) == ["self", "feats", "beam_width", "max_beam_depth", "length_alpha", "n_best",
                                                                      "no_repeat_ngram_size", "repetition_penalty", "min_length", "banned_ids"]
    assert list(inspect.signature(beam.beam_cumulative).parameters) == ["model", "feats", "params", "beam_width", "max_depth", "length_alpha",
                                                                        "n_best", "constraints"]


def test_argument_errors_before_the_library():
    import S2VTModel
    x = torch.zeros(2, 5, 16)                       # a CPU tensor: a bad argument is refused before the tensor is looked at
    m = S2VTModel.S2VT(60, 16, 5, dim_hid=8, dim_embed=8)
    for kw, match in ((dict(beam_width=6, num_groups=4), "num_groups"),                      # W % G
                      (dict(beam_width=4, num_groups=8), "num_groups"),                      # G > W
                      (dict(num_groups=0), "num_groups"), (dict(num_groups=1.5), "num_groups"),
                      (dict(beam_width=6, num_groups=3, n_best=3), "n_best"),                # n_best > Wg
                      (dict(n_best=0), "n_best"),
                      (dict(diversity_lambda=-0.1), "diversity_lambda"), (dict(diversity_lambda=float("nan")), "diversity_lambda"),
                      (dict(diversity_lambda=float("inf")), "diversity_lambda"), (dict(diversity_lambda=1e39), "diversity_lambda"),
                      (dict(beam_width=9, num_groups=3), "mode='beam'"), (dict(max_beam_depth=0), "mode='beam'"),
                      (dict(length_alpha=-1.0), "mode='beam'"),
                      (dict(max_beam_depth=38, no_repeat_ngram_size=2, banned_ids=[5, 7]), "vocab_size"),      # 20 + 38 + 2 + 1 = 61 > 60
                      (dict(max_beam_depth=40, no_repeat_ngram_size=2), "vocab_size"),
                      (dict(repetition_penalty=0.5), "repetition_penalty"), (dict(banned_ids=[60]), "banned_ids")):
        with pytest.raises(ValueError, match=match):
            m.beam_diverse(x, **kw)
    big = S2VTModel.S2VT(2000, 16, 5, dim_hid=8, dim_embed=8)
    with pytest.raises(ValueError, match="max_beam_depth 1024"):
        big.beam_diverse(x, max_beam_depth=1024, no_repeat_ngram_size=2)
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        other = S2VTModel.S2VT(60, 16, 5, dim_hid=8, dim_embed=8, **kw)
        with pytest.raises(ValueError, match="mode='beam' of a"):
            other.beam_diverse(x)
    # good arguments: the CPU tensor fails loudly, constrained or not, one group or several
    for kw in (dict(), dict(num_groups=1), dict(max_beam_depth=38, no_repeat_ngram_size=2), dict(max_beam_depth=40)):
        with pytest.raises(capi.S2VTHipError):
            m.beam_diverse(x, **kw)
    assert beam.check_diverse_args(6, 3, 0.5, 2) == (3, 0.5, 2)


# ------------------------------------------------------------------ the C ABI's surface
def test_header_declares_and_capi_binds_the_new_symbols(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header) and name in capi.SIGNATURES and hasattr(lib, name), name
    assert "diverse beam" in header
    assert lib.s2vt_abi_version() == 9              # the API is additive
    nb, nh = lib.s2vt_beam_div_bytes(64, 6, 3, 12, 0), lib.s2vt_beam_div_bytes(64, 6, 3, 12, 1)
    assert nb > 0 and nh >= nb + 2 * 64 * 6 * 12 * 4
    for bad in ((0, 6, 3, 12), (64, 9, 3, 12), (64, 6, 4, 12), (64, 4, 8, 12), (64, 6, 0, 12), (64, 6, 3, 0)):
        assert lib.s2vt_beam_div_bytes(*bad, 0) == 0 and lib.s2vt_beam_div_bytes(*bad, 1) == 0, bad


def test_the_cumulative_entries_size_the_one_group_state(lib):
    """one policy, one state: s2vt_beam_cum_bytes IS s2vt_beam_div_bytes at one group, plain and with histories, and both refuse the
    same dims"""
    for B, W, D in ((1, 1, 1), (3, 5, 6), (64, 5, 12), (128, 8, 30), (7, 3, 1023)):
        nb, nh = lib.s2vt_beam_cum_bytes(B, W, D), lib.s2vt_beam_cum_hist_bytes(B, W, D)
        assert nb > 0 and nb == lib.s2vt_beam_div_bytes(B, W, 1, D, 0), (B, W, D)
        assert nh >= nb + 2 * B * W * D * 4 and nh == lib.s2vt_beam_div_bytes(B, W, 1, D, 1), (B, W, D)
    for bad in ((0, 5, 12), (64, 0, 12), (64, 9, 12), (64, 5, 0), (-1, 5, 12), (1 << 20, 8, 1 << 10)):
        assert lib.s2vt_beam_cum_bytes(*bad) == 0 and lib.s2vt_beam_cum_hist_bytes(*bad) == 0, bad
        assert lib.s2vt_beam_div_bytes(bad[0], bad[1], 1, bad[2], 0) == 0 and lib.s2vt_beam_div_bytes(bad[0], bad[1], 1, bad[2], 1) == 0, bad


def test_c_abi_refuses_bad_arguments_before_a_launch(lib):
    import ctypes
    p = ctypes.c_void_p(256)                        # never dereferenced: every call below is refused before a launch
    out, ld = ctypes.c_void_p(), ctypes.c_int64()
    big = 1 << 22

    def step(B=4, W=6, G=3, D=6, alpha=0.7, lam=0.5, depth=1, state=p, nbytes=big, top=p, rows=p, ho=None, hl=None):
        return lib.s2vt_beam_div_step(B, W, G, D, 3, 4, alpha, lam, depth, state, nbytes, top, top, rows, rows, rows, ho, hl, None)
    for kw in (dict(G=4), dict(W=4, G=8), dict(G=0), dict(W=9, G=3), dict(B=0), dict(D=0), dict(depth=7), dict(depth=-1),
               dict(alpha=-1.0), dict(alpha=float("nan")), dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")),
               dict(lam=1e39), dict(state=None), dict(rows=None), dict(depth=2, top=None),
               dict(ho=ctypes.byref(out)), dict(hl=ctypes.byref(ld)),
               dict(nbytes=lib.s2vt_beam_div_bytes(4, 6, 3, 6, 0) - 1),
               dict(nbytes=lib.s2vt_beam_div_bytes(4, 6, 3, 6, 0), ho=ctypes.byref(out), hl=ctypes.byref(ld))):     # too small for the words
        rc = step(**kw)
        assert rc == -1 and b"s2vt_beam_div_step" in lib.s2vt_last_error(), kw

    def result(B=4, W=6, G=3, D=6, n_best=1, state=p, nbytes=big, o=p):
        return lib.s2vt_beam_div_result(B, W, G, D, 4, n_best, state, nbytes, o, o, o, None)
    for kw in (dict(G=4), dict(W=4, G=8), dict(G=0), dict(W=9, G=3), dict(n_best=0), dict(n_best=3), dict(B=0), dict(D=0),
               dict(state=None), dict(o=None), dict(nbytes=lib.s2vt_beam_div_bytes(4, 6, 3, 6, 0) - 1)):
        rc = result(**kw)
        assert rc == -1 and b"s2vt_beam_div_result" in lib.s2vt_last_error(), kw


# ------------------------------------------------------------------ eval.py's flags
def test_eval_accepts_the_flags_with_the_cumulative_beam_only(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval as ev
    for argv in (["--beam", "6", "--beam-mode", "reference", "--beam-groups", "3"], ["--beam-groups", "3"],
                 ["--beam", "6", "--beam-groups", "3"], ["--beam", "6", "--beam-mode", "cumulative", "--diversity-lambda", "0.5"],
                 ["--beam", "6", "--beam-mode", "cumulative", "--beam-groups", "3", "--n-best", "2"],
                 ["--beam", "6", "--beam-mode", "cumulative", "--beam-groups", "-1"]):
        with pytest.raises(SystemExit):                  # refused before a model is loaded
            ev.main(["--model-path", "m.pth"] + argv)
    seen = {}

    def generate(*args, **kw):
        seen["mode"], seen["kw"] = args[4], kw
        if kw.get("groups") is not None:
            kw["groups"]["v"] = [{"caption": "a", "score": -1.0}]
        return {}
    monkeypatch.setattr(ev, "generate", generate)
    out = str(tmp_path / "out.json")
    ev.main(["--model-path", "m.pth", "--beam", "6", "--beam-mode", "cumulative", "--beam-groups", "3", "--no-repeat-ngram", "2", "--out", out])
    assert seen["mode"] == "beam" and seen["kw"]["beam_width"] == 6 and seen["kw"]["beam_groups"] == 3
    assert seen["kw"]["diversity_lambda"] == 0.5 and seen["kw"]["constraints"]["no_repeat_ngram_size"] == 2
    import json
    assert json.load(open(out + ".groups.json")) == {"v": [{"caption": "a", "score": -1.0}]}
    ev.main(["--model-path", "m.pth", "--beam", "6", "--beam-mode", "cumulative", "--beam-groups", "2", "--diversity-lambda", "1.5", "--out", out])
    assert seen["kw"]["beam_groups"] == 2 and seen["kw"]["diversity_lambda"] == 1.5 and seen["kw"]["constraints"] is None
    # without the flags nothing changes: no new keyword reaches generate, no groups file is written
    plain = str(tmp_path / "plain.json")
    ev.main(["--model-path", "m.pth", "--beam", "3", "--beam-mode", "cumulative", "--out", plain])
    assert not {"beam_groups", "diversity_lambda", "groups"} & set(seen["kw"]) and not os.path.exists(plain + ".groups.json")
