"""CPU: top-k / nucleus truncation of the sampled draw (csrc/truncate.hip, S2VT.sample_truncated, Att_Baseline.forward) -
known answers of the numpy restatement (sampling.truncation_mask), the C ABI's surface, the argument checks that come before any
device call, and the fixtures and brackets that the GPU tests of test_gpu_truncated.py share (with their CPU preconditions)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sampling_host as hs  # noqa: E402

NEW = ("s2vt_truncated_draw", "s2vt_sample_rows_trunc_workspace_bytes", "s2vt_sample_decode_rows_trunc", "s2vt_top20_logprob")

# ---- shared with test_gpu_truncated.py
# The nucleus bracket.  The device decides "A(s_v) < p * Z" on fp32 sums; the float64 reference cannot say which way an element
# falls whose A / Z is within the sums' rounding of p, so it brackets the cut-off with p (1 -+ DELTA) and the device must land
# between the two kept sets.  DELTA is derived, not measured: a thread adds at most 65 terms serially (64 elements + the start),
# the block adds 6 butterfly levels + 2 for the four waves = 8 tree additions, every term is positive, so the relative error of A
# and of Z is at most (65 + 8) * 2^-24 for the additions plus 2 ulp = 2 * 2^-24 for expf: 75 * 2^-24 = 4.5e-6 each.  A / Z is off
# by at most twice that (9e-6); doubled once more for margin (and the rounding of p * Z, 2^-24): 2e-5.
DELTA = 2e-5
assert 2 * 2 * 75 * 2.0 ** -24 <= DELTA
NUCLEUS_T = 0.0625                               # 1 / t = 16: s = x * 16 is exact in fp32, both sides see the same scores
NUCLEUS_V = (301, 1027, 4099, 12001, 16388)
NUCLEUS_P = (0.1, 0.5, 0.9)
# chi2.ppf(1 - 1e-6, 4): both truncations of the distribution checks keep 5 of the 23 elements (scipy.stats.chi2.ppf(1 - 1e-6, 4)
# = 33.37684158165888).  4 degrees of freedom have the closed-form survival function exp(-x/2) (1 + x/2), which is 1e-6 there.
DIST_KEPT = 5
CHI2_BOUND_KEPT = 33.37684158165888
DIST_TRUNC = ((5, 1.0), (0, 0.6))


def step_logits(B, H, V, seed):
    """fp32 logits [B, V] of test_gpu_sampling._step_inputs, computed ONCE on the CPU: both the device and the reference get them"""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(H)
    h = torch.tanh(torch.randn(B, H, generator=g))
    w = (torch.rand(V, H, generator=g) * 2 - 1) * k
    b = (torch.rand(V, generator=g) * 2 - 1) * k
    return h @ w.t() + b


def nucleus_logits(V):
    return step_logits(64, 32, V, 4242 + 64 + 32 + V)


def bracket(scores, top_k, top_p, delta, value_margin=0.0):
    """(S_lo, S_hi) bool [rows, V]: the smallest and the largest kept set the definition allows when the nucleus cut-off may sit
    anywhere in p (1 -+ delta) and a score may be off by value_margin against the k-th largest.  Built from the restatement only:
    the nucleus over a given survivor set is truncation_mask on the scores with the others at -inf (mass 0, never kept)."""
    s = np.asarray(scores, dtype=np.float64)
    V = s.shape[1]
    if 0 < top_k < V:
        tau = np.sort(s, axis=1)[:, V - top_k][:, None]
        lo_k, hi_k = s >= tau + value_margin, s >= tau - value_margin
        if value_margin == 0.0:
            assert np.array_equal(lo_k, sampling.truncation_mask(s, top_k, 1.0))
    else:
        lo_k = hi_k = np.ones(s.shape, dtype=bool)
    if top_p >= 1.0:
        return lo_k, hi_k

    def nucleus(keep, p):
        return keep if p >= 1.0 else keep & sampling.truncation_mask(np.where(keep, s, -np.inf), 0, p)
    return nucleus(lo_k, top_p * (1.0 - delta)), nucleus(hi_k, top_p * (1.0 + delta))


def check_draws(score, ids, lo, hi, tol):
    """every row: the id is in S_hi and its float64 score is within tol of the largest score over S_lo"""
    rows = np.arange(score.shape[0])
    assert hi[rows, ids].all(), "a draw outside the kept set: rows %s" % (np.nonzero(~hi[rows, ids])[0][:8],)
    best = np.where(lo, score, -np.inf).max(1)
    gap = best - score[rows, ids]
    assert (gap <= tol).all(), "largest float64 gap %.3g > %.3g" % (gap.max(), tol)
    return float(gap.max())


# ---- the restatement: known answers
def test_top_k_ties_at_the_kth_place_all_stay():
    s = np.array([[3.0, 1.0, 2.0, 2.0, 0.5, 2.0, -1.0]])
    assert sampling.truncation_mask(s, 1, 1.0)[0].tolist() == [True, False, False, False, False, False, False]
    for k in (2, 3, 4):                                  # the k-th largest is one of the three 2.0: all of them stay
        assert sampling.truncation_mask(s, k, 1.0)[0].tolist() == [True, False, True, True, False, True, False], k
    assert sampling.truncation_mask(s, 5, 1.0)[0].sum() == 5
    assert sampling.truncation_mask(s, 7, 1.0).all() and sampling.truncation_mask(s, 0, 1.0).all()      # k = V and k = 0: off
    two = np.array([[1.0, 5.0, 5.0, 0.0]])              # k = 1 with two maxima: both stay (the draw then takes the lower index)
    assert sampling.truncation_mask(two, 1, 1.0)[0].tolist() == [False, True, True, False]


def test_nucleus_known_answers_and_the_maximum_always_stays():
    p6 = np.array([0.4, 0.25, 0.15, 0.1, 0.06, 0.04])
    s = np.log(p6)[None, [3, 0, 5, 1, 4, 2]]            # (not sorted: the rule is about values, not positions)
    inv = np.argsort([3, 0, 5, 1, 4, 2])

    def kept(k, p):
        return sampling.truncation_mask(s, k, p)[0][inv].astype(int).tolist()
    assert kept(0, 0.85) == [1, 1, 1, 1, 0, 0]           # masses in front: 0, .4, .65, .8 < .85 <= .9
    assert kept(0, 0.55) == [1, 1, 0, 0, 0, 0]           # 0, .4 < .55 <= .65
    assert kept(0, 1e-9) == [1, 0, 0, 0, 0, 0]           # the maximum always stays: nothing is in front of it
    assert kept(0, 1.0) == [1] * 6
    # top-k, then top-p over the RENORMALISED top-k set: k = 2 leaves Z = .65, p * Z = .3575, and .4 in front of the second
    assert kept(2, 1.0) == [1, 1, 0, 0, 0, 0]
    assert kept(2, 0.55) == [1, 0, 0, 0, 0, 0]
    assert kept(2, 0.55) != kept(0, 0.55) and kept(2, 0.55) != kept(2, 1.0)
    # equal values stay or go together
    t = np.log(np.array([[0.3, 0.2, 0.2, 0.2, 0.1]]))
    assert sampling.truncation_mask(t, 0, 0.4)[0].tolist() == [True, True, True, True, False]     # .3 < .4: the run of .2 stays
    assert sampling.truncation_mask(t, 0, 0.25)[0].tolist() == [True, False, False, False, False]  # .3 >= .25: the run goes
    # rows are independent
    both = sampling.truncation_mask(np.concatenate([s, s[:, ::-1]]), 2, 0.55)
    assert np.array_equal(both[0], both[1][::-1])


def test_check_truncation():
    assert sampling.check_truncation(0, 1.0, 30) == (0, 1.0)
    assert sampling.check_truncation(np.int64(30), np.float32(0.5), 30) == (30, 0.5)
    assert sampling.check_truncation(5, 1, 30) == (5, 1.0)
    for bad in (True, 2.5, "3", -1, 31, None):
        with pytest.raises(ValueError, match="top_k"):
            sampling.check_truncation(bad, 1.0, 30)
    for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match="top_p"):
            sampling.check_truncation(0, bad, 30)
    assert not sampling.truncates(0, 1.0, 30) and not sampling.truncates(30, 1.0, 30)
    assert sampling.truncates(29, 1.0, 30) and sampling.truncates(0, 0.999, 30)


# ---- the C ABI
def test_new_symbols_declared_exported_bound_and_abi_9(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in capi.SIGNATURES, name
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9


def test_workspace_query(lib):
    d = capi.Dims(16, 80, 4096, 512, 512, 3000)
    for K in (1, 2, 5):
        plain = lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(d), K)
        trunc = lib.s2vt_sample_rows_trunc_workspace_bytes(ctypes.byref(d), K)
        rows = (16 * K + 63) // 64 * 64
        assert plain + rows * 3000 * 4 <= trunc <= plain + rows * 3000 * 4 + 512           # + the [rows64, V] logits
    assert lib.s2vt_sample_rows_trunc_workspace_bytes(ctypes.byref(d), 0) == 0
    assert lib.s2vt_sample_rows_trunc_workspace_bytes(ctypes.byref(capi.Dims(16, 80, 4096, 512, 512, 38401)), 1) == 0
    assert lib.s2vt_sample_rows_trunc_workspace_bytes(ctypes.byref(capi.Dims(16, 80, 4096, 512, 512, 38400)), 1) > 0


def test_library_refusals_come_before_the_device(lib):
    """made-up addresses stand for device memory: every rejection happens before anything is enqueued"""
    one = ctypes.c_void_p(256)

    def draw(logits=one, ld=30, rows=4, V=30, t=1.0, k=0, p=1.0, step=0, row0=0, packed=one):
        return lib.s2vt_truncated_draw(logits, ld, rows, V, t, k, p, 5, step, row0, packed, None, None)
    for kw in (dict(k=-1), dict(k=31), dict(p=0.0), dict(p=-0.5), dict(p=1.5), dict(p=float("nan")), dict(t=0.0), dict(t=float("nan")),
               dict(t=float("inf")), dict(t=1e-45), dict(logits=None), dict(packed=None), dict(ld=29), dict(rows=0), dict(V=0),
               dict(V=38401, ld=38401, k=0), dict(step=-1), dict(row0=-1)):
        assert draw(**kw) == -1, kw
        assert b"s2vt_truncated_draw" in lib.s2vt_last_error(), kw
    assert lib.s2vt_top20_logprob(None, 30, 4, 30, one, one, None) == -1 and b"s2vt_top20_logprob" in lib.s2vt_last_error()
    assert lib.s2vt_top20_logprob(one, 30, 4, 19, one, one, None) == -1            # fewer than 20 tokens
    d = capi.Dims(4, 6, 16, 8, 8, 30)
    prm = capi.Params()
    big = 1 << 40

    def rows(K=2, sos=3, t=1.0, k=5, p=0.9, ws=big, feats=one):
        return lib.s2vt_sample_decode_rows_trunc(ctypes.byref(d), ctypes.byref(prm), feats, K, sos, t, 5, k, p, one, one, ws, None, 0, 0,
                                                 None)
    for kw in (dict(k=-1), dict(k=31), dict(p=0.0), dict(p=1.0001), dict(p=float("nan")), dict(K=0), dict(sos=30), dict(t=0.0),
               dict(t=float("nan")), dict(ws=16), dict(feats=None)):
        assert rows(**kw) == -1, kw
        assert b"s2vt_sample_decode_rows_trunc" in lib.s2vt_last_error(), kw
    # the workspace bound is the truncated one: the plain size is too small
    plain = lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(d), 2)
    assert rows(ws=plain) == -1 and b"workspace" in lib.s2vt_last_error()


def test_model_refusals_come_before_the_device():
    import S2VTModel
    import attention_baseline
    x = torch.zeros(2, 5, 16)                            # a CPU tensor: a bad argument is refused before the tensor is looked at
    bad_k = (True, 2.5, "3", -1, 31)
    bad_p = (0.0, -1.0, 1.5, float("nan"), "0.5")
    for kw in ({}, dict(rnn_type="gru"), dict(num_layers=2)):
        m = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8, **kw)
        for k in bad_k:
            with pytest.raises(ValueError, match="top_k"):
                m.sample_truncated(x, 2, top_k=k)
        for p in bad_p:
            with pytest.raises(ValueError, match="top_p"):
                m.sample_truncated(x, 2, top_p=p)
        for bad in (dict(n_samples=0), dict(n_samples=2.5), dict(n_samples=True), dict(temperature=0.0), dict(seed=-1)):
            with pytest.raises(ValueError):
                m.sample_truncated(x, **dict(dict(n_samples=2, top_k=5), **bad))
        with pytest.raises(capi.S2VTHipError):           # good arguments: the CPU tensor fails loudly
            m.sample_truncated(x, 2, top_k=5, top_p=0.9, seed=1)
        with pytest.raises(capi.S2VTHipError):
            m.sample_truncated(x, 1, seed=1)
    att = attention_baseline.Att_Baseline(30, 16, 5, dim_hid=8, dim_embed=8)
    with pytest.raises(ValueError, match="top_k"):
        att(torch.zeros(2, 5, 16), mode="sample", top_k=31)
    for fn in (S2VTModel.S2VT.sample_truncated, attention_baseline.Att_Baseline.forward):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[-2:] == ["top_k", "top_p"]
        assert sig.parameters["top_k"].default == 0 and sig.parameters["top_p"].default == 1.0
    # sample_truncated is sample's parameter list with the two behind it; forward and sample keep theirs
    assert list(inspect.signature(S2VTModel.S2VT.sample_truncated).parameters)[:-2] == list(inspect.signature(S2VTModel.S2VT.sample).parameters)
    assert "top_k" not in inspect.signature(S2VTModel.S2VT.forward).parameters


def test_train_and_eval_flags():
    sys.path.insert(0, ROOT)
    import eval as ev
    import train
    opt = train.parse(["--self-critical"])
    assert opt.sc_top_k == 0 and opt.sc_top_p == 1.0
    opt = train.parse(["--self-critical", "--sc-top-k", "5", "--sc-top-p", "0.9"])
    assert opt.sc_top_k == 5 and opt.sc_top_p == 0.9
    for bad in (["--sc-top-k", "5"], ["--sc-top-p", "0.5"], ["--self-critical", "--sc-top-k", "-1"], ["--self-critical", "--sc-top-p", "0"],
                ["--self-critical", "--sc-top-p", "1.5"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
    sig = inspect.signature(train.make_self_critical_step)
    assert sig.parameters["top_k"].default == 0 and sig.parameters["top_p"].default == 1.0
    a = ev.build_parser().parse_args(["--model-path", "m.pth"])
    assert (a.sample, a.temperature, a.top_k, a.top_p, a.sample_seed) == (0, 1.0, 0, 1.0, 0)
    a = ev.build_parser().parse_args(["--model-path", "m.pth", "--sample", "3", "--top-k", "5", "--top-p", "0.8", "--sample-seed", "9"])
    assert (a.sample, a.top_k, a.top_p, a.sample_seed) == (3, 5, 0.8, 9)


# ---- CPU preconditions of the GPU tests
@pytest.mark.parametrize("V", NUCLEUS_V)
def test_nucleus_fixture_is_decided_in_float64(V):
    """at most 2 of the 64 rows of a case may have a cut-off inside the bracket (for these inputs the reference has none)"""
    s = nucleus_logits(V).double().numpy() / NUCLEUS_T
    for p in NUCLEUS_P:
        lo, hi = bracket(s, 0, p, DELTA)
        open_rows = int((lo.sum(1) != hi.sum(1)).sum())
        print("V=%d p=%.1f: kept %d..%d, rows with an undecided cut-off: %d" % (V, p, lo.sum(1).min(), hi.sum(1).max(), open_rows))
        assert (lo <= hi).all() and open_rows <= 2
        assert lo.sum(1).min() >= 1 and hi.sum(1).max() < V             # a real cut: something goes, the maximum stays


def test_distribution_fixture():
    s = hs.DIST_LOGITS.astype(np.float32).astype(np.float64)[None, :]
    for k, p in DIST_TRUNC:
        lo, hi = bracket(s, k, p, DELTA)
        assert np.array_equal(lo, hi) and int(lo.sum()) == DIST_KEPT
    try:
        from scipy.stats import chi2
        assert abs(float(chi2.ppf(1 - 1e-6, DIST_KEPT - 1)) - CHI2_BOUND_KEPT) < 1e-9
    except ImportError:                                  # pragma: no cover
        pass
    x = CHI2_BOUND_KEPT / 2
    assert abs(np.exp(-x) * (1 + x) - 1e-6) < 1e-12      # the closed form for 4 degrees of freedom
