"""CPU: K sampled captions per clip (S2VT.sample, csrc/api_sample_rows.hip) and the grouped self-critical weights
(s2vt_sc_weights_group) - the C ABI's surface, the numpy restatement of the grouped baseline, train.py's flags and the argument
checks that come before any device call."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi
from s2vt_video_caption_amd.self_critical import advantage_weights, group_advantages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("s2vt_sample_rows_workspace_bytes", "s2vt_sample_decode_rows", "s2vt_sc_weights_group")


def test_new_symbols_declared_exported_bound_and_abi_9(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in capi.SIGNATURES, name
    assert re.search(r"#define S2VT_ABI_VERSION 9\b", header)
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9


def test_workspace_query(lib):
    d = capi.Dims(16, 80, 4096, 512, 512, 3000)
    sizes = [lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(d), K) for K in (0, 1, 2, 5)]
    assert sizes[0] == 0 and 0 < sizes[1] < sizes[2] < sizes[3]
    assert lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(d), -1) == 0
    assert lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(capi.Dims(0, 80, 4096, 512, 512, 3000)), 2) == 0
    # (L - 1) * rows64(B * K) packed words must stay below 2^31
    assert lib.s2vt_sample_rows_workspace_bytes(ctypes.byref(d), (1 << 31) // 79 // 16 + 8) == 0


def test_group_advantages_by_hand():
    r = np.array([[1.0, 2.0, 6.0], [0.3, 0.3, 0.3]])
    adv, base = group_advantages(r)
    assert base.dtype == np.float64 and adv.dtype == np.float64
    # clip 0: sum 9; the others' means 4, 3.5, 1.5
    assert base[0].tolist() == [4.0, 3.5, 1.5] and adv[0].tolist() == [-3.0, -1.5, 4.5]
    # equal rewards: the baseline is the reward itself and the weight exactly zero - although the rounded sum alone,
    # ((0.3 + 0.3 + 0.3) - 0.3) / 2, is not 0.3
    assert ((0.0 + 0.3 + 0.3 + 0.3) - 0.3) / 2.0 != 0.3
    assert base[1].tolist() == [0.3] * 3 and adv[1].tolist() == [0.0] * 3
    w = advantage_weights(torch.full((6, 4), 7), adv.reshape(-1), 4)
    assert (w[3:] == 0).all() and (w[:3, 1:] != 0).all()
    for k in (2.0, 1.0 / 3.0, 1e-9, 0.0):
        e, _ = group_advantages(np.full((1, 5), k))
        assert (advantage_weights(torch.full((5, 4), 7), e.reshape(-1), 4) == 0).all()
    # one reward off by an ulp is no equal group: the stated formula
    r = np.array([[0.3, 0.3, np.nextafter(0.3, 1.0)]])
    s = ((0.0 + r[0, 0]) + r[0, 1]) + r[0, 2]
    assert group_advantages(r)[1][0].tolist() == [(s - x) / 2.0 for x in r[0]]


def test_group_advantages_k2_greedy_and_errors():
    rng = np.random.RandomState(3)
    r = rng.rand(7, 2) * 3
    adv, base = group_advantages(r)
    # each row's baseline is the other row: exactly where a + b is exact, else within the two roundings of (a + b) - a, each at
    # most 2^-53 relative to a number below a + b
    e_adv, e_base = group_advantages(np.array([[1.5, 0.25], [3.0, 3.0]]))
    assert e_base.tolist() == [[0.25, 1.5], [3.0, 3.0]] and e_adv.tolist() == [[1.25, -1.25], [0.0, 0.0]]
    assert np.array_equal(base[:, 0], (r[:, 0] + r[:, 1]) - r[:, 0]) and np.array_equal(base[:, 1], (r[:, 0] + r[:, 1]) - r[:, 1])
    assert (np.abs(base - r[:, ::-1]) <= 2.0 ** -52 * r.sum(1, keepdims=True)).all()
    assert np.array_equal(adv, r - base)
    g = rng.rand(7) * 3
    r5 = rng.rand(7, 5) * 3
    adv, base = group_advantages(r5, g)
    assert np.array_equal(adv, r5 - g[:, None]) and np.array_equal(base, np.repeat(g[:, None], 5, 1))
    # K = 1 with the greedy reward is advantage_weights' advantage r - r_g
    r1 = rng.rand(7, 1)
    assert np.array_equal(group_advantages(r1, g)[0][:, 0], r1[:, 0] - g)
    with pytest.raises(ValueError):
        group_advantages(r1)
    with pytest.raises(ValueError):
        group_advantages(r5, g[:3])


def test_group_sum_is_sequential():
    """the restatement adds in ascending k (np.sum adds pairwise from 8 elements on): rewards where the two orders differ"""
    r = np.array([[1e16, 1.0, -1e16, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    total = 0.0
    for x in r[0]:
        total = total + x
    _, base = group_advantages(r)
    assert base[0, 1] == (total - 1.0) / 8.0


def test_train_flags():
    sys.path.insert(0, ROOT)
    import train
    opt = train.parse([])
    assert opt.sc_samples == 1 and opt.sc_baseline == "greedy"
    opt = train.parse(["--self-critical"])
    assert opt.sc_samples == 1 and opt.sc_baseline == "greedy"
    opt = train.parse(["--self-critical", "--sc-samples", "5", "--sc-baseline", "mean"])
    assert opt.sc_samples == 5 and opt.sc_baseline == "mean"
    assert train.parse(["--self-critical", "--sc-samples", "3"]).sc_baseline == "greedy"
    for bad in (["--self-critical", "--sc-baseline", "mean"], ["--sc-samples", "5"], ["--sc-baseline", "mean"],
                ["--sc-samples", "5", "--sc-baseline", "mean"], ["--self-critical", "--sc-samples", "0"],
                ["--self-critical", "--sc-baseline", "median", "--sc-samples", "2"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
    sig = inspect.signature(train.make_self_critical_step)
    assert list(sig.parameters)[-2:] == ["samples", "baseline"]
    assert sig.parameters["samples"].default == 1 and sig.parameters["baseline"].default == "greedy"


def test_sample_argument_errors_come_before_the_device():
    import S2VTModel
    x = torch.zeros(2, 5, 16)                        # a CPU tensor: a bad argument is refused before the tensor is looked at
    for kw in ({}, dict(rnn_type="gru"), dict(num_layers=2)):
        m = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8, **kw)
        for bad in (dict(n_samples=0), dict(n_samples=2.5), dict(n_samples=-3), dict(n_samples="2"), dict(n_samples=True),
                    dict(n_samples=2, temperature=0.0), dict(n_samples=2, temperature=float("nan")),
                    dict(n_samples=2, temperature=float("inf")), dict(n_samples=2, seed=-1), dict(n_samples=2, seed=2 ** 64)):
            with pytest.raises(ValueError):
                m.sample(x, **bad)
        with pytest.raises(capi.S2VTHipError):       # good arguments: the CPU tensor fails loudly
            m.sample(x, n_samples=2, seed=1)
    sig = inspect.signature(S2VTModel.S2VT.sample)
    assert list(sig.parameters) == ["self", "feats", "n_samples", "temperature", "seed"]
    assert [sig.parameters[k].default for k in ("n_samples", "temperature", "seed")] == [1, 1.0, None]


def test_forward_signature_is_unchanged():
    import S2VTModel
    sig = inspect.signature(S2VTModel.S2VT.forward)
    assert list(sig.parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob", "ss_temperature",
                                    "length_alpha", "n_best", "temperature", "seed"]


def test_library_argument_errors_come_before_the_device(lib):
    """null pointers stand for device memory: every rejection happens before anything is enqueued"""
    d = capi.Dims(4, 6, 16, 8, 8, 30)
    p = capi.Params()
    one = ctypes.c_void_p(256)
    big = 1 << 40

    def call(K=2, sos=3, t=1.0, ws=big, feats=one):
        return lib.s2vt_sample_decode_rows(ctypes.byref(d), ctypes.byref(p), feats, K, sos, t, 5, one, one, ws, None, 0, 0, None)
    for kw in (dict(K=0), dict(K=-2), dict(sos=-1), dict(sos=30), dict(t=0.0), dict(t=float("nan")), dict(t=float("inf")),
               dict(ws=16), dict(feats=None)):
        assert call(**kw) == -1, kw
        assert b"s2vt_sample_decode_rows" in lib.s2vt_last_error()
    # the grouped weights: K >= 2 without a greedy reward, K >= 1 with one
    assert lib.s2vt_sc_weights_group(one, one, None, 3, 1, 5, 3, 4, one, one, None, None) == -1
    assert b"K >= 2" in lib.s2vt_last_error()
    assert lib.s2vt_sc_weights_group(one, one, one, 3, 0, 5, 3, 4, one, one, None, None) == -1
    assert lib.s2vt_sc_weights_group(None, one, one, 3, 2, 5, 3, 4, one, one, None, None) == -1
