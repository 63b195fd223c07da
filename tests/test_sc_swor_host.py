"""CPU: self-critical training on stochastic-beam samples (train.py --sc-distinct) - the C ABI's surface of s2vt_sc_weights_swor, the
inclusion probability by Monte Carlo, the numpy restatement self_critical.swor_advantages case by case and against a literal scalar
transcription of include/s2vt_hip.h "without-replacement weights", and train.py's flags."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi
from s2vt_video_caption_amd.self_critical import inclusion_log_q, swor_advantages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "s2vt_sc_weights_swor"


# ------------------------------------------------------------------ 1. the surface
def test_symbol_declared_exported_bound_and_abi_9(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    assert "without-replacement weights" in header
    assert re.search(r"\b%s\(" % NAME, header)
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME][1]) == 15
    assert re.search(r"#define S2VT_ABI_VERSION 9\b", header)
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9
    assert re.search(r"#define S2VT_SWOR_MAX_K 8\b", header) and capi.SWOR_MAX_K == 8


def test_argument_errors_come_before_the_device(lib):
    """null pointers stand for device memory: every rejection happens before anything is enqueued"""
    one = ctypes.c_void_p(256)

    def call(sampled=one, logprob=one, kappa=one, r_sample=one, B=3, K=3, T=5, caps=one, weight=one):
        return lib.s2vt_sc_weights_swor(sampled, logprob, kappa, r_sample, None, B, K, T, 3, 4, caps, weight, None, None, None)
    for kw in (dict(sampled=None), dict(logprob=None), dict(kappa=None), dict(r_sample=None), dict(caps=None), dict(weight=None),
               dict(K=1), dict(K=9), dict(K=0), dict(T=0), dict(B=0)):
        assert call(**kw) == -1, kw
        assert NAME.encode() in lib.s2vt_last_error(), kw


# ------------------------------------------------------------------ 2. the inclusion probability, by Monte Carlo
def test_inclusion_log_q_makes_the_importance_weighted_sum_unbiased():
    """7 outcomes, K = 3 kept of a Gumbel-top-k draw, the fourth perturbed score as kappa: sum over the kept of p_i / q_i * r_i is
    an unbiased estimate of sum p_i r_i (Kool et al. 2019) - with q = 1 - exp(-exp(phi - kappa)); the formula with the argument's
    sign turned overflows.  400 000 draws with a fixed seed; the bound is 5 standard errors of the sample itself."""
    rng = np.random.RandomState(0)
    logits = rng.randn(7) * 1.5
    r = rng.rand(7) * 3
    phi = logits - np.log(np.exp(logits).sum())
    n, K = 400000, 3
    G = phi[None, :] + rng.gumbel(size=(n, 7))
    order = np.argsort(-G, axis=1)
    kept = order[:, :K]
    kappa = np.take_along_axis(G, order[:, K:K + 1], 1)[:, 0]
    lq = inclusion_log_q(phi[kept], kappa)
    assert lq.shape == (n, K) and (lq <= 0).all() and np.isfinite(lq).all()
    est = (np.exp(phi[kept] - lq) * r[kept]).sum(1)
    true = float((np.exp(phi) * r).sum())
    se = float(est.std(ddof=1) / math.sqrt(n))
    print("importance-weighted mean %.4f, true %.4f, standard error %.4f: %.2f standard errors" % (est.mean(), true, se,
                                                                                                     abs(est.mean() - true) / se))
    assert abs(float(est.mean()) - true) <= 5 * se
    with np.errstate(all="ignore"):
        wrong = np.exp(-np.exp(kappa[:, None] - phi[kept]))              # the formula the documentation used to state
        assert not np.isfinite((np.exp(phi[kept]) / wrong * r[kept]).sum(1).mean())
    # kappa = -inf: everything is kept, log q = 0
    assert np.array_equal(inclusion_log_q(phi[None, :3], np.array([-np.inf])), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        inclusion_log_q(phi, kappa[:2])


# ------------------------------------------------------------------ 3. swor_advantages
def _case(seed, B, K):
    """random log-probs in [-40, 0], rewards in [0, 3) and a threshold a little below each clip's smallest perturbed score"""
    rng = np.random.RandomState(seed)
    phi = -40.0 * rng.rand(B, K)
    G = phi + rng.gumbel(size=(B, K))
    kappa = G.min(1) - 0.5 * rng.rand(B)
    return phi, kappa, rng.rand(B, K) * 3


def transcription(logprob, kappa, rewards, greedy=None):
    """include/s2vt_hip.h "without-replacement weights", steps 1-6 and the rules, literally: scalar float64 loops"""
    B, K = len(rewards), len(rewards[0])
    f = np.float64
    adv, coef, base = np.zeros((B, K)), np.zeros((B, K)), np.zeros(B)
    with np.errstate(all="ignore"):
        for b in range(B):
            phi, kap, r = [f(x) for x in logprob[b]], f(kappa[b]), [f(x) for x in rewards[b]]
            bad = np.isnan(kap) or kap == np.inf or any(not np.isfinite(x) or x > 0 for x in phi) or any(not np.isfinite(x) for x in r)
            bad = bad or (greedy is not None and not np.isfinite(greedy[b]))
            lw = []
            for i in range(K):
                a = phi[i] - kap
                e = np.exp(a)
                lq = a - f(0.5) * e if a < -30.0 else np.log(-np.expm1(-e))
                lw.append(phi[i] - lq)
            m = max(lw) if not bad else f(0.0)
            om = [np.exp(lw[i] - m) for i in range(K)]
            pi = [np.exp(phi[i] - m) for i in range(K)]
            W, N = f(0.0), f(0.0)
            for j in range(K):
                W = W + om[j]
                N = N + om[j] * r[j]
            same = greedy is None and all(x == r[0] for x in r)
            bs = f(greedy[b]) if greedy is not None else r[0] if same else N / W
            c = [om[i] / ((W - om[i]) + pi[i]) for i in range(K)]
            ad = [f(0.0) if same else c[i] * (r[i] - bs) for i in range(K)]
            bad = bad or any(not np.isfinite(np.float32(x)) for x in ad)
            if bad:
                base[b] = np.nan
            else:
                adv[b], coef[b], base[b] = ad, c, bs
    return adv, coef, base


def test_kappa_minus_inf_is_the_renormalised_distribution():
    phi, _, r = _case(1, 4, 5)
    phi = phi / 10.0
    adv, coef, base = swor_advantages(phi, np.full(4, -np.inf), r)
    p = np.exp(phi)
    assert np.allclose(coef, p / p.sum(1, keepdims=True), rtol=1e-12, atol=0)
    assert np.allclose(base, (coef * r).sum(1), rtol=1e-12, atol=0)
    assert np.allclose(adv, coef * (r - base[:, None]), rtol=1e-12, atol=0)


def test_shifting_phi_and_kappa_together_changes_nothing():
    """step 3: 79-word captions with phi ~ -700 do not underflow"""
    phi, kappa, r = _case(2, 6, 5)
    a0, c0, b0 = swor_advantages(phi, kappa, r)
    a1, c1, b1 = swor_advantages(phi - 700.0, kappa - 700.0, r)
    assert (c0 > 0).all() and np.isfinite(c1).all()
    print("shift by -700: max relative change of coef %.3g" % np.abs(c1 / c0 - 1).max())
    assert np.allclose(c1, c0, rtol=1e-10, atol=0) and np.allclose(b1, b0, rtol=1e-10, atol=0)
    assert np.allclose(a1, a0, rtol=1e-9, atol=1e-12)


def test_the_two_forms_of_log_q_meet_at_minus_30():
    a = np.array([np.nextafter(-30.0, -np.inf), -30.0, -30.5, -29.5, -100.0, -750.0])
    lq = inclusion_log_q(a[None, :], np.array([0.0]))[0]
    assert np.isfinite(lq).all()
    assert abs(lq[0] - lq[1]) <= 1e-12                            # the series form just below, log(-expm1(-e)) at -30
    e = np.exp(a)
    series = a - 0.5 * e
    with np.errstate(divide="ignore"):
        closed = np.log(-np.expm1(-e))
    assert np.abs(series[:4] - closed[:4]).max() <= 1e-12         # both forms on both sides
    assert np.array_equal(lq[4:], series[4:]) and not np.isfinite(closed[5])
    # and in the estimator: a clip with a_i on both sides
    phi = np.array([[-1.0, -2.0, -35.0 + 4.0]])
    kap = np.array([4.0])                                         # a = -5, -6, -35
    _, c, _ = swor_advantages(phi, kap, np.array([[1.0, 2.0, 3.0]]))
    assert np.isfinite(c).all() and (c > 0).all()


def test_equal_rewards_greedy_and_bad_clips():
    phi, kappa, r = _case(3, 6, 3)
    r[2] = 0.1 + 0.2
    adv, coef, base = swor_advantages(phi, kappa, r)
    assert adv[2].tolist() == [0.0] * 3 and base[2] == 0.1 + 0.2 and (coef[2] > 0).all()
    assert (adv[[0, 1, 3, 4, 5]] != 0).all()
    g = np.arange(6) * 0.5
    adv_g, coef_g, base_g = swor_advantages(phi, kappa, r, g)
    assert np.array_equal(base_g, g) and np.array_equal(coef_g, coef) and np.array_equal(adv_g, coef * (r - g[:, None]))
    assert (adv_g[2] != 0).all()                                  # (equal rewards are no special case against a greedy reward)
    for what in ("phi nan", "phi -inf", "phi positive", "kappa nan", "kappa +inf", "reward inf", "reward nan", "greedy nan"):
        p2, k2, r2, g2 = phi.copy(), kappa.copy(), r.copy(), None
        if what == "phi nan":
            p2[1, 0] = np.nan
        elif what == "phi -inf":
            p2[1, 2] = -np.inf
        elif what == "phi positive":
            p2[1, 1] = 1e-3
        elif what == "kappa nan":
            k2[1] = np.nan
        elif what == "kappa +inf":
            k2[1] = np.inf
        elif what == "reward inf":
            r2[1, 1] = np.inf
        elif what == "reward nan":
            r2[1, 0] = np.nan
        else:
            g2 = g.copy()
            g2[1] = np.nan
        a2, c2, b2 = swor_advantages(p2, k2, r2, g2)
        keep = np.arange(6) != 1
        assert a2[1].tolist() == [0.0] * 3 and c2[1].tolist() == [0.0] * 3 and np.isnan(b2[1]), what
        ref = (adv_g, coef_g, base_g) if g2 is not None else (adv, coef, base)
        assert np.array_equal(a2[keep], ref[0][keep]) and np.array_equal(c2[keep], ref[1][keep]), what
        assert np.array_equal(b2[keep], ref[2][keep]) and np.isfinite(a2).all() and np.isfinite(c2).all(), what
    # a threshold so far above the log-probs that q itself underflows: log q does not, and the coefficients stay finite
    a3, c3, b3 = swor_advantages(np.array([[-800.0, -801.0]]), np.array([0.0]), np.array([[1.0, 2.0]]))
    assert np.isfinite(a3).all() and (c3 > 0).all() and np.isfinite(c3).all() and 1.0 < b3[0] < 2.0
    # finite rewards whose advantage does not fit fp32: a weight of inf would reach the gradient - a bad clip
    a3, c3, b3 = swor_advantages(phi[:1], kappa[:1], np.array([[1e300, 0.0, 0.0]]))
    assert not a3.any() and not c3.any() and np.isnan(b3[0])
    for bad in (dict(rewards=r[:, :1], logprob=phi[:, :1]), dict(kappa=kappa[:3]), dict(greedy=g[:2]),
                dict(rewards=np.zeros((6, 9)), logprob=np.zeros((6, 9)))):
        kw = dict(dict(logprob=phi, kappa=kappa, rewards=r), **bad)
        with pytest.raises(ValueError):
            swor_advantages(**kw)


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_bit_for_bit_the_literal_transcription(K):
    phi, kappa, r = _case(10 + K, 40, K)
    kappa[0] = -np.inf
    phi[1], kappa[1] = phi[1] - 700.0, kappa[1] - 700.0
    kappa[2] = phi[2].max() + 33.0                                # a_i < -30 on every row
    r[3] = r[3, 0]
    phi[4, 0] = np.nan
    r[5, K - 1] = np.inf
    phi, kappa = phi.astype(np.float32), kappa.astype(np.float32)        # as the search returns them
    g = np.random.RandomState(K).rand(40) * 3
    for greedy in (None, g):
        got = swor_advantages(phi, kappa, r, greedy)
        want = transcription(phi, kappa, r, greedy)
        for x, y in zip(got, want):
            assert x.dtype == np.float64 and np.array_equal(x, y, equal_nan=True)
        assert np.isnan(got[2][[4, 5]]).all() and np.isfinite(np.delete(got[2], [4, 5])).all()
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert not swor_advantages(phi, kappa, r)[0][3].any()


# ------------------------------------------------------------------ 4. train.py's flags
def test_train_flags():
    sys.path.insert(0, ROOT)
    import train
    assert train.parse([]).sc_distinct is False and train.parse(["--self-critical", "--sc-samples", "3"]).sc_distinct is False
    opt = train.parse(["--self-critical", "--sc-samples", "3", "--sc-distinct", "--sc-baseline", "mean", "--sc-shared-encode",
                       "--sc-reward", "device"])
    assert opt.sc_distinct is True and opt.sc_samples == 3
    assert train.parse(["--self-critical", "--sc-samples", "8", "--sc-distinct"]).sc_baseline == "greedy"
    ok = ["--self-critical", "--sc-samples", "3", "--sc-distinct"]
    for bad in (["--sc-distinct"], ["--sc-samples", "3", "--sc-distinct"], ["--self-critical", "--sc-distinct"],
                ["--self-critical", "--sc-samples", "1", "--sc-distinct"], ["--self-critical", "--sc-samples", "9", "--sc-distinct"],
                ok + ["--sc-top-k", "5"], ok + ["--sc-top-p", "0.9"], ok + ["--sc-temperature", "0.8"], ok + ["--rnn-type", "gru"],
                ok + ["--num-layers", "2"], ok + ["--model", "att_baseline"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
    sig = inspect.signature(train.make_self_critical_step)
    assert list(sig.parameters)[-2:] == ["samples", "baseline"]
    assert list(sig.parameters)[-3] == "distinct" and sig.parameters["distinct"].default is False
    for kw in (dict(samples=1), dict(samples=9), dict(samples=3, top_k=5), dict(samples=3, temperature=0.5)):
        with pytest.raises(ValueError):
            train.make_self_critical_step(None, None, None, None, {}, 3, 4, "cpu", distinct=True, **kw)


def test_the_documented_formula_is_the_right_one():
    import S2VTModel
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for text in (readme, S2VTModel.S2VT.sample_distinct.__doc__):
        assert "exp(-exp(kappa - logprob))" not in text
        assert "1 - exp(-exp(logprob - kappa))" in text
