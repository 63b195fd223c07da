"""GPU: diverse (group) beam search, S2VT.beam_diverse (csrc/beam_policy.hip + beam.beam_diverse; include/s2vt_hip.h "diverse beam").

The policy kernel alone, plain and with per-slot histories, is compared bit for bit with the float32 restatement of the definition
(tests/beam_div_ref.PolicyDivF32: the same adds, the product and the difference of the penalty rounded separately, the same power
table and division); the whole path with the fp64 restatement on every sample whose decisions are clear (both gaps >= 2e-4;
tests/test_beam_div_host.py pins how many); the identities with mode='beam' / beam_constrained bit for bit; eval.py's flags."""
import ctypes
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
import beam_constrained_ref as cref  # noqa: E402
import beam_div_ref as dref  # noqa: E402
import test_beam_div_host as host  # noqa: E402
from test_gpu_beam_cum import _random_tops, _with_eos  # noqa: E402

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
    if spec_args is None:
        return {}
    n, theta, m, banned = spec_args
    return dict(no_repeat_ngram_size=n, repetition_penalty=theta, min_length=m, banned_ids=list(banned))


# ------------------------------------------------------------------ 1. the policy kernel alone, through the C ABI
def _trace(B, W, G, D, alpha, lam, tops):
    """what the device must show after every policy call, from the restatement (host only): a list over the calls (the initialising
    one first) of (rows [2][B*W], words [B*W][D], which rows' words are compared, frozen-sample count), the final (ids, lens, scores),
    and two flags - some sample had a settled group beside an unsettled one; some sample was frozen while a group was still live"""
    pol = dref.PolicyDivF32(B, W, G, D, alpha, lam)
    h, live = pol.histories()
    calls = [(pol.rows(), h, live, 0)]
    frozen = np.zeros(B, dtype=bool)
    partial = early = False
    for t in range(1, D + 1):
        pol.step(*tops[t - 1])
        st = pol.settled()
        open_ = np.array([[bool(pol.live[b][g]) for g in range(G)] for b in range(B)])
        partial |= bool((st.any(axis=1) & ~st.all(axis=1) & ~frozen).any())
        early |= bool((st.all(axis=1) & open_.any(axis=1) & ~frozen).any())
        frozen |= st.all(axis=1)                        # (sticky: a frozen sample ignores every later call)
        want = pol.rows()
        want[:, np.repeat(frozen, W)] = 0
        h, live = pol.histories()
        calls.append((want, h, live & ~np.repeat(frozen, W), int(frozen.sum())))
    assert frozen.all()
    return calls, pol.result(), partial, early


def _drive(lib, B, W, G, D, alpha, lam, tops, hist):
    """the kernel against _trace, one policy call per depth; hist: the form that keeps the live slots' words"""
    R, Wg = B * W, W // G
    nbytes = lib.s2vt_beam_div_bytes(B, W, G, D, int(hist))
    assert nbytes > 0
    qs = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rows = torch.full((3, R), -7, dtype=torch.int32, device=DEV)
    ix_d = torch.zeros(R, 20, dtype=torch.int32, device=DEV)
    lp_d = torch.zeros(R, 20, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    words, words_ld = ctypes.c_void_p(), ctypes.c_int64()
    calls, (wi, wl, ws), partial, early = _trace(B, W, G, D, alpha, lam, tops)

    def call(depth):
        capi.check(lib.s2vt_beam_div_step(B, W, G, D, ref.SOS, ref.EOS, alpha, lam, depth, _ptr(qs), nbytes, _ptr(ix_d), _ptr(lp_d),
                                          _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), ctypes.byref(words) if hist else None,
                                          ctypes.byref(words_ld) if hist else None, st), "s2vt_beam_div_step")
        h = None
        if hist:
            off = words.value - qs.data_ptr()                                    # the buffer the next depth step must read
            assert words_ld.value == D and lib.s2vt_beam_div_bytes(B, W, G, D, 0) <= off and off + R * D * 4 <= nbytes and off % 4 == 0
            h = qs[off:off + R * D * 4].view(torch.int32).view(R, D).cpu().numpy()
        return rows.cpu().numpy(), h, int(qs[:4].view(torch.int32).item())
    for t in range(D + 1):
        if t:
            ix_d.copy_(torch.from_numpy(tops[t - 1][0]))
            lp_d.copy_(torch.from_numpy(tops[t - 1][1]))
        got, h, count = call(1 if t == 0 else (t + 1 if t < D else 0))
        want, wh, cmp_rows, wcount = calls[t]
        assert np.array_equal(got[0], np.repeat(np.arange(B), W))
        assert np.array_equal(got[1:], want), (t, got[1:], want)
        assert count == wcount, (t, count, wcount)
        if hist:
            assert np.array_equal(h[cmp_rows, :t], wh[cmp_rows, :t]), (t, h, wh)  # each live slot's words
            assert h.min() >= 0 and h.max() < 50                                 # every row readable: defined words, in bounds
    for n_best in sorted({Wg, 1}):
        ids = torch.empty(B, G, n_best, D, dtype=torch.int32, device=DEV)
        lens = torch.empty(B, G, n_best, dtype=torch.int32, device=DEV)
        scores = torch.empty(B, G, n_best, dtype=torch.float32, device=DEV)
        capi.check(lib.s2vt_beam_div_result(B, W, G, D, ref.EOS, n_best, _ptr(qs), nbytes, _ptr(ids), _ptr(lens), _ptr(scores), st),
                   "s2vt_beam_div_result")
        assert np.array_equal(ids.cpu().numpy(), wi[:, :, :n_best])
        assert np.array_equal(lens.cpu().numpy(), wl[:, :, :n_best])
        sc = scores.cpu().numpy()
        assert np.array_equal(sc.view(np.uint32), np.ascontiguousarray(ws[:, :, :n_best]).view(np.uint32)), (sc, ws)
    return [c[3] for c in calls[1:]], partial, early


@pytest.mark.parametrize("W,G", [(2, 2), (4, 2), (6, 3), (8, 8), (8, 2), (8, 1)])
@pytest.mark.parametrize("D", [1, 6])
def test_policy_kernel_is_the_float32_restatement(lib, W, G, D):
    """random top-20 arrays, continuous and on a grid of 1/4 (keys of different parents and penalised keys tie bit for bit: the
    (slot, token) rule decides); lambda = 0, 0.5 (on the grid) and 0.3 (not representable: the two roundings matter); plain and with
    histories"""
    B = 5
    for seed, quantum, alpha, lam, hist in ((1, 0.25, 0.7, 0.0, False), (2, 0.25, 0.7, 0.5, False), (3, 0.25, 0.0, 0.5, True),
                                            (4, 0.25, 0.7, 0.3, True), (5, None, 0.7, 0.3, False), (6, None, 0.0, 0.5, True)):
        _drive(lib, B, W, G, D, alpha, lam, _random_tops(B, W, D, 1000 * G + 100 * W + 10 * D + seed, quantum=quantum), hist)


def crafted_same_word(B, W, D):
    """word 10 far on top of every row at every depth: with a small lambda every group takes it, cnt[10] reaches G - 1"""
    tops = _random_tops(B, W, D, 21, eos=False)
    for ix, lp in tops:
        ix[:] = np.arange(10, 30, dtype=np.int32)[None, :]
        lp[:] -= 1.0
        lp[:, 0] = -0.01
    return tops


def crafted_eos_first(B, W, D):
    """depth 1: every row holds <eos> at -0.01, word 11 at -0.2, word 12 at -0.3 and 17 words below -1; <eos> is in no top 20
    afterwards.  At one slot per group and lambda = 0.5 group 0 takes <eos> and closes, group 1 sees it at -0.51 and takes word 11,
    group 2 sees word 11 at -0.7 and takes word 12"""
    tops = _random_tops(B, W, D, 22, eos=False)
    ix, lp = tops[0]
    ix[:] = np.arange(10, 30, dtype=np.int32)[None, :]
    lp[:] -= 1.0
    _with_eos(ix, lp, range(B * W), -0.01)              # (<eos> replaces word 10, in front)
    lp[:, 1], lp[:, 2] = -0.2, -0.3
    return tops


def crafted_early(B, W, D, rows=None):
    """<eos> at log-prob 0 from depth 2 on (in the given rows; None: all), every other word a little below (alpha = 0: the score is
    the sum): pools fill with sums no live hypothesis can reach any more"""
    tops = _random_tops(B, W, D, 15, eos=False)
    tops[0][1][:] = tops[0][1] / 3.0 * 0.04 - 0.01                # depth 1 in [-0.05, -0.01]
    for t in range(1, D):
        tops[t][1][:] = tops[t][1] / 3.0 * 0.004 - 0.001          # then in [-0.005, -0.001]
        _with_eos(tops[t][0], tops[t][1], range(B * W) if rows is None else rows, 0.0)
    return tops


def crafted_inf(B, W, D):
    """-inf entries: 15 of every row's 20 at every depth; at depth 2, 19 of 20 in the even rows and all 20 in the odd ones (a group
    of two slots then has one finite candidate, so a -inf candidate IS selected)"""
    tops = _random_tops(B, W, D, 23)
    rng = np.random.RandomState(24)
    for t, (ix, lp) in enumerate(tops):
        for r in range(B * W):
            lp[r, rng.choice(20, (19 + r % 2) if t == 1 else 15, replace=False)] = -np.inf
    return tops


def test_policy_kernel_on_crafted_inputs(lib):
    B, D = 3, 6
    # one word on top in every group
    tops = crafted_same_word(B, 4, D)
    pol = dref.PolicyDivF32(B, 4, 4, D, 0.7, 0.05)
    pol.step(*tops[0])
    assert all(l[0][3] == 10 for per in pol.live for l in per)       # (the fixture: all four groups chose word 10)
    for hist in (False, True):
        _drive(lib, B, 4, 4, D, 0.7, 0.05, tops, hist)
    # <eos> chosen by group 0 and thereby penalised in group 1; group 0 closes at depth 1, the others run to D; the sample freezes only
    # with its last group
    tops = crafted_eos_first(B, 3, D)
    pol = dref.PolicyDivF32(B, 3, 3, D, 0.7, 0.5)
    pol.step(*tops[0])
    assert all(not per[0] and per[1][0][3] == 11 and per[2][0][3] == 12 for per in pol.live)       # (the fixture)
    assert all(len(per[0]) == 1 and not per[1] and not per[2] for per in pol.pool)
    for hist in (False, True):
        counts, partial, early = _drive(lib, B, 3, 3, D, 0.7, 0.5, tops, hist)
        assert counts[:-1] == [0] * (D - 1) and counts[-1] == B and partial and not early
    # lambda = 0 on the same inputs: every group takes <eos>, every sample is done after depth 1
    counts, _, _ = _drive(lib, B, 3, 3, D, 0.7, 0.0, tops, False)
    assert counts[0] == B
    # -inf entries
    tops = crafted_inf(B, 4, D)
    pol = dref.PolicyDivF32(B, 4, 2, D, 0.7, 0.5)
    pol.step(*tops[0])
    pol.step(*tops[1])
    assert any(np.isneginf(l[0]) for per in pol.live for grp in per for l in grp)      # (the fixture: a -inf candidate was selected)
    for hist in (False, True):
        _drive(lib, B, 4, 2, D, 0.7, 0.5, tops, hist)
    # the two roundings of the penalty (tests/test_beam_div_host.py: two_roundings_tops): cnt == 3 with an inexact fl(lambda * 3) and a
    # competitor exactly at fl(s - fl(lambda * 3)) - a kernel that fused the product and the difference into one FMA selects word 11 in
    # group 3 and fails here; one float higher word 11 wins under either arithmetic
    for lp11, last in ((host.TWO_X, 10), (np.nextafter(host.TWO_X, np.float32(0)), 11)):
        tops = [host.two_roundings_tops(B, lp11)] + _random_tops(B, 4, D - 1, 25, eos=False)
        pol = dref.PolicyDivF32(B, 4, 4, D, 0.0, host.TWO_LAM)
        pol.step(*tops[0])
        assert all([l[0][3] for l in per] == [10, 10, 10, last] for per in pol.live)        # (the fixture)
        for hist in (False, True):
            _drive(lib, B, 4, 4, D, 0.0, host.TWO_LAM, tops, hist)
    # the early stop: samples frozen while a group is still live, and only once their LAST group has settled - at (4, 2, 0.0012) one
    # sample's group 0 settles a depth before its group 1, which keeps the sample stepping
    for W, G, lam, late in ((4, 2, 0.0012, True), (6, 3, 1e-4, False)):
        for hist in (False, True):
            counts, partial, early = _drive(lib, B, W, G, D, 0.0, lam, crafted_early(B, W, D), hist)
            assert early and counts[D - 2] == B and (partial or not late), (W, G, counts)


def _drive_one_group(lib, B, W, D, alpha, tops, hist):
    """s2vt_beam_cum_step / s2vt_beam_cum_hist_step beside s2vt_beam_div_step at one group with lambda = 0.5, each on its own zeroed
    state and rows, fed the same top-20 arrays: after every call the rows and the WHOLE states (the counter at byte 0 and both word
    buffers included) are equal, and the returned word buffers are the same place; at the end both result entries give the same
    bits on either state.  -> the depth after which the restatement has each sample frozen"""
    R = B * W
    plain = lib.s2vt_beam_cum_bytes(B, W, D)
    nbytes = lib.s2vt_beam_cum_hist_bytes(B, W, D) if hist else plain
    assert 0 < plain <= nbytes == lib.s2vt_beam_div_bytes(B, W, 1, D, int(hist))
    q_cum, q_div = (torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(2))
    r_cum, r_div = (torch.full((3, R), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    ix_d = torch.zeros(R, 20, dtype=torch.int32, device=DEV)
    lp_d = torch.zeros(R, 20, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    w_cum, w_div, ld_cum, ld_div = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()

    def call(depth):
        a = (alpha, depth, _ptr(q_cum), nbytes, _ptr(ix_d), _ptr(lp_d), _ptr(r_cum[0]), _ptr(r_cum[1]), _ptr(r_cum[2]))
        if hist:
            capi.check(lib.s2vt_beam_cum_hist_step(B, W, D, ref.SOS, ref.EOS, *a, ctypes.byref(w_cum), ctypes.byref(ld_cum), st),
                       "s2vt_beam_cum_hist_step")
        else:
            capi.check(lib.s2vt_beam_cum_step(B, W, D, ref.SOS, ref.EOS, *a, st), "s2vt_beam_cum_step")
        capi.check(lib.s2vt_beam_div_step(B, W, 1, D, ref.SOS, ref.EOS, alpha, 0.5, depth, _ptr(q_div), nbytes, _ptr(ix_d), _ptr(lp_d),
                                          _ptr(r_div[0]), _ptr(r_div[1]), _ptr(r_div[2]), ctypes.byref(w_div) if hist else None,
                                          ctypes.byref(ld_div) if hist else None, st), "s2vt_beam_div_step")
        assert torch.equal(r_cum, r_div), (depth, r_cum, r_div)
        assert torch.equal(q_cum, q_div), depth
        count = int(q_cum[:4].view(torch.int32).item())
        assert count == int(q_div[:4].view(torch.int32).item())
        if hist:
            off = w_cum.value - q_cum.data_ptr()
            assert off == w_div.value - q_div.data_ptr() and ld_cum.value == ld_div.value == D
            assert plain <= off and off % 4 == 0 and off + R * D * 4 <= nbytes
            assert torch.equal(q_cum[off:off + R * D * 4], q_div[off:off + R * D * 4])
        return r_cum.cpu().numpy(), count
    pol = ref.PolicyF32(B, W, D, alpha)
    got, count = call(1)
    assert count == 0 and np.array_equal(got[0], np.repeat(np.arange(B), W)) and np.array_equal(got[1:], pol.rows())
    frozen = np.zeros(B, dtype=bool)
    when = np.zeros(B, dtype=np.int64)
    for t in range(1, D + 1):
        ix_d.copy_(torch.from_numpy(tops[t - 1][0]))
        lp_d.copy_(torch.from_numpy(tops[t - 1][1]))
        got, count = call(t + 1 if t < D else 0)
        pol.step(*tops[t - 1])
        now = (pol.done | pol.may_stop()) & ~frozen
        when[now] = t
        frozen |= now
        want = pol.rows()
        want[:, np.repeat(frozen, W)] = 0
        assert np.array_equal(got[1:], want) and count == int(frozen.sum()), (t, got[1:], want, count)
    assert frozen.all()
    wi, wl, _ = pol.result()
    outs = []
    for q in (q_cum, q_div):
        for entry in ("s2vt_beam_cum_result", "s2vt_beam_div_result"):
            ids = torch.empty(B, W, D, dtype=torch.int32, device=DEV)
            lens = torch.empty(B, W, dtype=torch.int32, device=DEV)
            scores = torch.empty(B, W, dtype=torch.float32, device=DEV)
            groups = (1,) if entry == "s2vt_beam_div_result" else ()
            capi.check(getattr(lib, entry)(B, W, *groups, D, ref.EOS, W, _ptr(q), nbytes, _ptr(ids), _ptr(lens), _ptr(scores), st), entry)
            outs.append((ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()))
    assert np.array_equal(outs[0][0], wi) and np.array_equal(outs[0][1], wl)
    assert all(_same_bits(o, outs[0]) for o in outs[1:])
    return when


@pytest.mark.parametrize("W", [1, 5, 8])
@pytest.mark.parametrize("hist", [False, True], ids=["plain", "hist"])
def test_one_group_is_the_cumulative_entries_launch_for_launch(lib, W, hist):
    """one policy kernel: the cumulative entries are the group entries at one group, where lambda is inert.  Two inputs, on each of
    which the restatement freezes some sample early and runs some to D: sample 0 selects nothing but <eos> at depth 2 (its live list
    empties; alpha = 0.7) - the others never see <eos>; and crafted_early without <eos> for the last sample (alpha = 0: at W > 1 the
    early stop fires while hypotheses are live)"""
    B, D = 3, 6
    tops = _random_tops(B, W, D, 40 + W, eos=False)
    tops[1][1][:W] -= 5.0
    _with_eos(tops[1][0], tops[1][1], range(W), -0.001)
    when = _drive_one_group(lib, B, W, D, 0.7, tops, hist)
    assert when.tolist() == [2, D, D]
    when = _drive_one_group(lib, B, W, D, 0.0, crafted_early(B, W, D, rows=range((B - 1) * W)), hist)
    assert (when[:B - 1] < D).all() and when[B - 1] == D, when


# ------------------------------------------------------------------ 2. the whole path against the fp64 restatement
_MODELS = {}


def _case_model(name):
    if name not in _MODELS:
        sd, feats, _, _ = ref.case_inputs(name)
        _MODELS[name] = (_model(ref.CASES[name][0], sd), feats.to(DEV))
    return _MODELS[name]


def _run(name, D, G, Wg, lam, spec_args, n_best=None, alpha=ref.ALPHA):
    m, f = _case_model(name)
    n_best = Wg if n_best is None else n_best
    ids, lens, scores = m.beam_diverse(f, beam_width=G * Wg, num_groups=G, diversity_lambda=lam, max_beam_depth=D, length_alpha=alpha,
                                       n_best=n_best, **_kwargs(spec_args))
    assert ids.dtype == torch.int64 and lens.dtype == torch.int64 and scores.dtype == torch.float32 and ids.device.type == "cuda"
    assert not ids.requires_grad and not scores.requires_grad
    assert tuple(ids.shape) == (f.shape[0], G, n_best, D) and tuple(lens.shape) == tuple(scores.shape) == (f.shape[0], G, n_best)
    return ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


@pytest.mark.parametrize("case", sorted(host.ROBUST, key=str), ids=sorted(host.CASE_IDS))
def test_whole_path_against_the_restatement(lib, case):
    name, D, G, Wg, lam, spec_args = case
    want = dref.case_search(*case)
    rb = dref.robust(want)
    assert int(rb.sum()) == host.ROBUST[case]
    ids, lens, scores = _run(*case)
    assert beam.LAST_PATH.startswith("constrained diverse beam" if spec_args is not None else "diverse beam"), beam.LAST_PATH
    spec = cref.spec_of(spec_args, ref.CASES[name][0][5]) if spec_args is not None else None
    worst = 0.0
    for b in range(len(want)):
        got = [[ids[b, g, k, :lens[b, g, k]].tolist() for k in range(Wg)] for g in range(G)]
        assert (ids[b][np.arange(D)[None, None, :] >= lens[b][:, :, None]] == ref.EOS).all()       # padded with <eos>
        if spec is not None:
            assert all(cref.satisfies(h, spec) for g in got for h in g), (b, got)                  # on every returned hypothesis
        if rb[b]:
            assert got == want[b]["ids"], b
            worst = max(worst, float(np.abs(scores[b] - np.array(want[b]["scores"])).max()))
    print("%r: %d robust samples identical, max |score - fp64| = %.3g" % (case, int(rb.sum()), worst))
    assert worst <= 1e-4                                    # (tests/test_gpu_beam_cum.py's whole-path bound: the same sums of <= D log-probs)
    assert (np.diff(scores, axis=2) <= 0).all()             # every group best first, on every sample


# ------------------------------------------------------------------ 3. identities on the device, bit for bit
def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def _beam(name, W, D, n_best, spec_args=None):
    m, f = _case_model(name)
    with torch.no_grad():
        if spec_args is None:
            out = m(f, mode="beam", beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=n_best)
        else:
            out = m.beam_constrained(f, beam_width=W, max_beam_depth=D, length_alpha=ref.ALPHA, n_best=n_best, **_kwargs(spec_args))
    return tuple(t.cpu().numpy() for t in out)


def test_one_group_is_mode_beam_and_beam_constrained(lib):
    for name in ("tiny5", "mid64"):
        _, _, W, D = ref.case_inputs(name)
        for spec_args in (None, cref.SPEC_A):
            want = _beam(name, W, D, W, spec_args)
            got = _run(name, D, 1, W, 0.5, spec_args)
            assert beam.LAST_PATH.startswith("constrained cumulative beam" if spec_args else "cumulative beam")     # today's launches
            assert all(x.shape[1] == 1 for x in got) and _same_bits(tuple(x[:, 0] for x in got), want), (name, spec_args)


def test_groups_are_mode_beam_at_the_group_width(lib):
    """lambda = 0: every group is mode='beam' at width Wg; lambda = 0.5: group 0 is"""
    for name, G, Wg in (("tiny5", 3, 2), ("mid64", 3, 2), ("mid64", 2, 3)):
        D = ref.CASES[name][4]
        want = _beam(name, Wg, D, Wg)
        zero = _run(name, D, G, Wg, 0.0, None)
        for g in range(G):
            assert _same_bits(tuple(x[:, g] for x in zero), want), (name, G, g)
        half = _run(name, D, G, Wg, 0.5, None)
        assert _same_bits(tuple(x[:, 0] for x in half), want), (name, G)
        if (name, G, Wg) == ("mid64", 3, 2):                                # (a pinned case: every sample's group-best captions differ)
            assert not np.array_equal(half[0][:, 1], want[0])


def test_two_calls_give_the_same_bits(lib):
    for spec_args in (None, cref.SPEC_A):
        a = _run("mid64", 12, 3, 2, 0.5, spec_args)
        b = _run("mid64", 12, 3, 2, 0.5, spec_args)
        assert _same_bits(a, b) and np.array_equal(a[0], b[0])
    # fewer than Wg per group: the first n_best of the same answer
    c = _run("mid64", 12, 3, 2, 0.5, None, n_best=1)
    a = _run("mid64", 12, 3, 2, 0.5, None)
    assert _same_bits(c, tuple(x[:, :, :1] for x in a))


# ------------------------------------------------------------------ 4. the other searches are untouched
def test_beam_and_beam_search_on_the_tiny_fixture_after_a_diverse_search(lib, golden):
    g = golden("tiny")
    d = synth.CONFIGS["tiny"]
    seed = int(g["seed"])
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=float(g["out_scale"]))
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)[0].to(DEV)
    m = _model((d["B"], d["L"], d["F"], d["H"], d["E"], d["V"]), sd)

    def both():
        with torch.no_grad():
            cum = m(feats, mode="beam", beam_width=3, max_beam_depth=10, n_best=2)
            bs = m(feats, mode="beam_search", beam_width=int(g["beam_width"]), max_beam_depth=30)
        return [t.cpu().numpy() for t in cum], [[int(t.item()) for t in s] for s in bs]
    cum0, bs0 = both()
    out = m.beam_diverse(feats, beam_width=4, num_groups=2, diversity_lambda=0.5, max_beam_depth=10)
    assert tuple(out[0].shape) == (d["B"], 2, 1, 10)
    m.beam_diverse(feats, beam_width=4, num_groups=2, max_beam_depth=10, no_repeat_ngram_size=2)
    cum1, bs1 = both()
    assert _same_bits(cum0, cum1) and bs0 == bs1
    for b, s in enumerate(bs1):
        assert s == [int(x) for x in g["beam_ids"][b] if x >= 0]


# ------------------------------------------------------------------ 5. eval.py --beam-groups / --diversity-lambda
_EVAL_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import eval as s2vt_eval
for argv in json.loads(sys.argv[2]):
    s2vt_eval.main(argv)
"""
EVAL_V, EVAL_SEED, EVAL_SCALE = 64, 38, 16.0


def test_eval_writes_the_best_group_caption_and_all_groups(lib, tmp_path):
    """four runs in ONE child process (the tool brings its own feed thread and copy stream): --beam 6 --beam-groups 3, the same with
    --no-repeat-ngram 2, --beam 3 alone and --beam 3 --beam-groups 1"""
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
              str(tmp_path / "feats"), "--batch-size", "3", "--beam-mode", "cumulative"]
    runs = [common + ["--beam", "6", "--beam-groups", "3", "--diversity-lambda", "0.5", "--out", str(tmp_path / "div.json")],
            common + ["--beam", "6", "--beam-groups", "3", "--no-repeat-ngram", "2", "--out", str(tmp_path / "divcon.json")],
            common + ["--beam", "3", "--out", str(tmp_path / "plain.json")],
            common + ["--beam", "3", "--beam-groups", "1", "--out", str(tmp_path / "one.json")]]
    r = subprocess.run([sys.executable, "-c", _EVAL_CHILD, ROOT, json.dumps(runs)], capture_output=True, text=True, cwd=ROOT, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    load = lambda n: json.load(open(str(tmp_path / n)))
    div, divcon, plain, one = load("div.json"), load("divcon.json"), load("plain.json"), load("one.json")
    assert len(div) == len(data["splits"]["test"]) and set(div) == set(divcon) == set(plain) == set(one)
    assert one == plain and not os.path.exists(str(tmp_path / "plain.json") + ".groups.json")
    og = load("one.json.groups.json")
    assert all(len(v) == 1 and v[0]["caption"] == one[k] for k, v in og.items())
    for preds, groups in ((div, load("div.json.groups.json")), (divcon, load("divcon.json.groups.json"))):
        assert set(groups) == set(preds)
        for k, v in groups.items():
            assert len(v) == 3 and all(set(e) == {"caption", "score"} and e["score"] <= 0 for e in v)
            sc = [e["score"] for e in v]
            assert preds[k] == v[sc.index(max(sc))]["caption"]           # the best group-best caption; the lowest group wins a tie
            assert v[0]["caption"]
    words = lambda c: list(zip(c.split(), c.split()[1:]))
    assert not any(len(words(e["caption"])) != len(set(words(e["caption"]))) for v in load("divcon.json.groups.json").values() for e in v)
