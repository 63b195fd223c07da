"""CPU: caption scoring (S2VT.forward(mode='score'), csrc/api_score.hip) - the fp64 restatement the GPU tests compare against
(tests/score_ref.py) checked against a second formulation and for its invariances, the argument checks of the Python surface
(score.check_score_args) before anything is launched, the pure workspace-size query, and eval.py --perplexity's host side."""
import ctypes
import inspect
import math
import os
import re
import sys

import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402
import score_ref  # noqa: E402

T_TINY = 8            # the tiny case has L = 8: the longest caption it takes


@pytest.fixture(scope="module")
def tiny():
    sd, feats, _, _ = ref.case_inputs("tiny")
    caps = score_ref.make_captions(feats.shape[0], 2, T_TINY, ref.CASES["tiny"][0][5], seed=5, min_scored=3, max_scored=7)
    return sd, feats, caps


def test_the_two_formulations_agree(tiny):
    sd, feats, caps = tiny
    for alpha in (0.0, 0.7):
        a = score_ref.scores_fp64(sd, feats, caps, ref.EOS, alpha)
        b = score_ref.scores_stepwise(sd, feats, caps, ref.EOS, alpha)
        assert torch.equal(a["lengths"], b["lengths"])
        assert float((a["token_lp"] - b["token_lp"]).abs().max()) <= 1e-12
        assert float((a["scores"] - b["scores"]).abs().max()) <= 1e-12
    n = a["lengths"]
    assert int(n[0, 0]) == T_TINY - 1 and EOS_absent(caps[0, 0])         # the row without <eos>: n = T-1
    assert int(n.min()) >= 3 and len(set(n.flatten().tolist())) > 2      # <eos> at mixed positions
    assert float(a["token_lp"].max()) <= 0.0


def EOS_absent(row):
    return not bool((row[1:] == ref.EOS).any())


def test_invariances_of_the_definition(tiny):
    sd, feats, caps = tiny
    base = score_ref.scores_fp64(sd, feats, caps, ref.EOS, 0.7)
    # ids behind the first <eos> do not matter
    other = caps.clone()
    n = base["lengths"]
    g = torch.Generator().manual_seed(9)
    for b in range(caps.shape[0]):
        for k in range(caps.shape[1]):
            m = int(n[b, k])
            if m < T_TINY - 1:
                other[b, k, m + 1:] = torch.randint(0, 50, (T_TINY - 1 - m,), generator=g)
    assert not torch.equal(other, caps)
    got = score_ref.scores_fp64(sd, feats, other, ref.EOS, 0.7)
    assert torch.equal(got["lengths"], n) and torch.equal(got["scores"], base["scores"]) and torch.equal(got["token_lp"], base["token_lp"])
    behind = torch.arange(T_TINY - 1)[None, None, :] >= n[..., None]
    assert bool(behind.any()) and float(base["token_lp"][behind].abs().max()) == 0.0 and float(base["token_lp"][~behind].max()) < 0.0
    # alpha = 0 is the plain sum; any alpha divides that sum by n ** alpha
    plain = score_ref.scores_fp64(sd, feats, caps, ref.EOS, 0.0)
    assert torch.equal(plain["scores"], plain["sums"]) and torch.equal(plain["sums"], base["sums"])
    assert float((base["scores"] - base["sums"] / n.double() ** 0.7).abs().max()) == 0.0
    # K copies of a caption give K equal scores; [B, T] is K = 1
    rep = caps[:, :1].expand(-1, 3, -1)
    r = score_ref.scores_fp64(sd, feats, rep, ref.EOS, 0.7)
    assert torch.equal(r["scores"][:, 0], r["scores"][:, 1]) and torch.equal(r["scores"][:, 0], r["scores"][:, 2])
    assert torch.equal(score_ref.scores_fp64(sd, feats, caps[:, 0], ref.EOS, 0.7)["scores"][:, 0], r["scores"][:, 0])


def test_forward_signature_is_unchanged_and_mode_score_checks_first():
    import S2VTModel
    sig = inspect.signature(S2VTModel.S2VT.forward)
    assert list(sig.parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob", "ss_temperature",
                                    "length_alpha", "n_best", "temperature", "seed"]
    assert sig.parameters["length_alpha"].default == 0.7 and sig.parameters["mode"].default == "train"
    m = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8)
    x = torch.zeros(2, 5, 16)                        # a CPU tensor: a bad argument is refused before the tensor is looked at
    good = torch.full((2, 4), 4, dtype=torch.long)
    for targets, kw in ((None, {}), (good.int(), {}), (good[0], {}), (good[:1], {}), (torch.zeros(2, 6, dtype=torch.long), {}),
                        (torch.zeros(2, 1, dtype=torch.long), {}), (good, dict(length_alpha=-1)),
                        (good, dict(length_alpha=float("nan"))), (good, dict(length_alpha=float("inf")))):
        with pytest.raises(ValueError, match="mode='score'"):
            m(x, targets=targets, mode="score", **kw)
    with pytest.raises(capi.S2VTHipError):           # good arguments: the CPU tensor fails loudly
        m(x, targets=good, mode="score", length_alpha=0)
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        other = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8, **kw)
        with pytest.raises(capi.S2VTHipError):      # (the CPU tensor is refused first, as in every mode)
            other(x, targets=good, mode="score")


def test_check_score_args(lib):
    d = capi.Dims(4, 10, 16, 8, 8, 30)
    ok = torch.zeros(4, 3, 7, dtype=torch.long)
    assert score.check_score_args(ok, 4, 10, d, 0.7) == (3, 7, False, 0.7)
    assert score.check_score_args(ok[:, 0], 4, 10, d, 0) == (1, 7, True, 0.0)
    assert score.check_score_args(torch.zeros(4, 2, dtype=torch.long), 4, 10, d, 0.0)[:2] == (1, 2)
    assert score.check_score_args(torch.zeros(4, 10, dtype=torch.long), 4, 10, d, 0.0)[:2] == (1, 10)
    # views: a stride-0 batch (the same K sentences for every clip), a column slice of a wider tensor
    shared = ok[0][None].expand(4, -1, -1)
    assert shared.stride(0) == 0 and score.check_score_args(shared, 4, 10, d, 0.7)[:2] == (3, 7)
    assert score.check_score_args(torch.zeros(4, 3, 9, dtype=torch.long)[..., :7], 4, 10, d, 0.7)[:2] == (3, 7)
    bad = [(ok.int(), 0.7), (ok.float(), 0.7), (ok[0, 0], 0.7), (ok[None], 0.7), (ok[:3], 0.7), (ok[:, :0], 0.7),
           (torch.zeros(4, 3, 1, dtype=torch.long), 0.7), (torch.zeros(4, 3, 11, dtype=torch.long), 0.7),
           (torch.zeros(4, 3, 14, dtype=torch.long)[..., ::2], 0.7), (ok, -0.5), (ok, float("nan")), (ok, float("inf")), (ok, "x"),
           ([[1, 2]], 0.7), (None, 0.7)]
    for caps, alpha in bad:
        with pytest.raises(ValueError, match="mode='score'"):
            score.check_score_args(caps, 4, 10, d, alpha)
    # a shape the library does not serve: 2^31 or more token rows
    wide = torch.zeros(1, dtype=torch.long).expand(4, 1 << 28, 10)
    assert lib.s2vt_score_workspace_bytes(ctypes.byref(d), 1 << 28, 10) == 0
    with pytest.raises(ValueError, match="mode='score'"):
        score.check_score_args(wide, 4, 10, d, 0.7)


def test_c_abi_is_declared_bound_and_the_workspace_stays_below_the_logits(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in ("s2vt_score_workspace_bytes", "s2vt_score_captions", "s2vt_pick_logprob"):
        assert re.search(r"\b%s\(" % name, header) and name in capi.SIGNATURES, name
    assert lib.s2vt_abi_version() == 9               # the API is additive
    rows = int(re.search(r"#define S2VT_SCORE_HEAD_ROWS (\d+)", header).group(1))
    B, L, F, H, E, V = 128, 80, 4096, 1000, 1000, 12000          # the c5 dims
    d = capi.Dims(B, L, F, H, E, V)
    K, T = 5, 31
    full_logits = B * K * (T - 1) * V * 4
    assert full_logits == 921600000
    nb = lib.s2vt_score_workspace_bytes(ctypes.byref(d), K, T)
    print("score workspace at c5, K=5, T=31: %.1f MB (all logits: %.1f MB)" % (nb / 1e6, full_logits / 1e6))
    assert 0 < nb < full_logits // 2
    assert nb > rows * V * 4                         # one chunk of logits is in there ...
    # ... and its row count is a constant: more candidates or longer captions add h_t rows and tokens, never logits
    big = lib.s2vt_score_workspace_bytes(ctypes.byref(d), 2 * K, T)
    assert 0 < big - nb < 2 * (B * K * (T - 1)) * (3 * 1024 * 2 + 4 * H * 4)
    for k, t in ((0, 31), (-1, 31), (5, 1), (5, 81), (5, 0)):
        assert lib.s2vt_score_workspace_bytes(ctypes.byref(d), k, t) == 0
    assert lib.s2vt_score_workspace_bytes(None, 5, 31) == 0
    assert lib.s2vt_score_workspace_bytes(ctypes.byref(capi.Dims(0, L, F, H, E, V)), 5, 31) == 0
    # null pointers are refused with a message before any GPU call
    rc = lib.s2vt_score_captions(ctypes.byref(d), None, None, None, 0, 0, 5, 31, 4, 0.7, None, None, None, None, 0, None, 0, 0, None)
    assert rc == -1 and b"s2vt_score_captions" in lib.s2vt_last_error()
    rc = lib.s2vt_pick_logprob(None, 0, 1, 10, None, None, None, None)
    assert rc == -1 and b"s2vt_pick_logprob" in lib.s2vt_last_error()


def test_eval_perplexity_arguments_and_arithmetic():
    sys.path.insert(0, ROOT)
    import eval as s2vt_eval
    a = s2vt_eval.build_parser().parse_args(["--model-path", "m.pth"])
    assert a.perplexity is False and a.out == "predictions.json" and a.beam == 0          # nothing changes without the flag
    a = s2vt_eval.build_parser().parse_args(["--model-path", "m.pth", "--perplexity", "--out", "x.json", "--batch-size", "4"])
    assert a.perplexity is True and a.out == "x.json" and a.batch_size == 4
    # canned per-caption numbers: three captions, 2 + 3 + 5 scored tokens
    s = s2vt_eval.perplexity_summary([-2.0, -4.5, -3.5], [2, 3, 5])
    assert s["tokens"] == 10 and s["total_loglik"] == -10.0
    assert s["perplexity"] == pytest.approx(math.e, rel=1e-15) and s["mean_caption_loglik"] == pytest.approx(-10.0 / 3, rel=1e-15)
    with pytest.raises(ValueError):
        s2vt_eval.perplexity_summary([], [])
    # the references of a batch as one [B, K, T] input: right-padded with <eos>, T the batch's longest, cut at max_len
    caps, counts = s2vt_eval.pack_references([[[3, 7, 8, 4], [3, 9, 4]], [[3, 5, 6, 7, 8, 9, 4]]], eos_ix=4, max_len=6)
    assert counts == [2, 1] and tuple(caps.shape) == (2, 2, 6) and caps.dtype == torch.int64
    assert caps[0].tolist() == [[3, 7, 8, 4, 4, 4], [3, 9, 4, 4, 4, 4]]
    assert caps[1].tolist() == [[3, 5, 6, 7, 8, 9]] * 2                   # (cut at max_len; the missing reference repeats the first)
    with pytest.raises(ValueError):
        s2vt_eval.pack_references([[]], 4, 6)
