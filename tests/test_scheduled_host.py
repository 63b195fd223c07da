"""CPU: the scheduled-sampling coin restated in numpy (sampling.ss_coin), the epoch ramp of train.py, the refused option
combinations and the argument checks of the Python surface that fire before the library is reached."""
import os
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("s2vt_scheduled_decode", "s2vt_scheduled_decode_cached", "s2vt_ss_mix", "s2vt_ss_unpack", "s2vt_gru_step_fwd_token_ss")


def test_coin_shape_and_range():
    c = sampling.ss_coin(12345, 3, 17)
    assert c.shape == (17,) and c.dtype == np.float32
    assert (c > 0).all() and (c < 1).all()
    rows = np.array([0, 5, 64, 129], dtype=np.uint32)
    assert np.array_equal(sampling.ss_coin(12345, 3, rows), sampling.ss_coin(12345, 3, 130)[rows])
    # the ends of the 23-bit grid are inside (0, 1) in fp32
    lo, hi = sampling.uniform_from_bits(np.uint32(0)), sampling.uniform_from_bits(np.uint32(0xFFFFFFFF))
    assert np.float32(lo) == lo > 0 and np.float32(hi) == hi < 1


def test_coin_stream_differs_from_the_gumbel_stream():
    """same key, same (0, row, step) counter words: the tags differ, so the words do"""
    assert sampling.SS_STREAM_TAG != sampling.STREAM_TAG == 0x47554D42
    seed, step, rows = 99, 4, np.arange(64, dtype=np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    counter = np.zeros((64, 4), dtype=np.uint32)
    counter[:, 1], counter[:, 2], counter[:, 3] = rows, step, sampling.STREAM_TAG
    u_gumbel = sampling.uniform_from_bits(sampling.philox4x32_10(counter, key)[:, 0])
    coin = sampling.ss_coin(seed, step, rows).astype(np.float64)
    assert (coin != u_gumbel).all()
    counter[:, 3] = sampling.SS_STREAM_TAG
    assert np.array_equal(coin, sampling.uniform_from_bits(sampling.philox4x32_10(counter, key)[:, 0]))


def test_coin_statistics():
    n = 100000
    u = sampling.ss_coin(5, 2, n).astype(np.float64)
    se = np.sqrt(1.0 / 12.0 / n)
    assert abs(u.mean() - 0.5) <= 4 * se
    share = (sampling.ss_coin(5, 2, n) < np.float32(0.25)).mean()
    assert abs(share - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / n)


def test_coin_known_answers():
    """frozen from the numpy restatement: seed 0x1234567890ABCDEF, step 3, rows 7..10 (the fp32 bit patterns)"""
    c = sampling.ss_coin(0x1234567890ABCDEF, 3, np.arange(7, 11))
    assert [int(x) for x in c.view(np.uint32)] == [1050882530, 1026262640, 1051781010, 1062124683]


def test_ss_used_rule():
    targets = np.arange(40).reshape(4, 10)
    draws = 100 + targets
    assert np.array_equal(sampling.ss_used(targets, draws, 0.0, 1), targets)
    one = sampling.ss_used(targets, draws, 1.0, 1)
    assert np.array_equal(one[:, 0], targets[:, 0]) and np.array_equal(one[:, 1:], draws[:, :-1])
    half = sampling.ss_used(targets, draws, 0.5, 1, row0=64)
    for j in range(1, 10):
        own = sampling.ss_coin(1, j, np.arange(64, 68)) < np.float32(0.5)
        assert np.array_equal(half[:, j], np.where(own, draws[:, j - 1], targets[:, j]))


def test_ramp():
    from train import ss_prob_for_epoch as f
    assert f(0, 2, 3, 0.1, 0.25) == 0 and f(1, 2, 3, 0.1, 0.25) == 0          # before the start epoch
    assert f(2, 2, 3, 0.1, 0.25) == 0                                        # at the start: 0 increases so far
    assert f(4, 2, 3, 0.1, 0.25) == 0 and f(5, 2, 3, 0.1, 0.25) == pytest.approx(0.1)      # across an increase
    assert f(8, 2, 3, 0.1, 0.25) == pytest.approx(0.2)
    assert f(11, 2, 3, 0.1, 0.25) == 0.25 and f(500, 2, 3, 0.1, 0.25) == 0.25           # at the cap
    assert f(7, -1, 3, 0.1, 0.25) == 0                                        # off
    assert f(0, 0, 1, 0.25, 1.0) == 0 and f(1, 0, 1, 0.25, 1.0) == 0.25 and f(9, 0, 1, 0.25, 1.0) == 1.0


def test_train_options():
    import train
    opt = train.parse([])
    assert opt.scheduled_sampling_start == -1 and opt.ss_temperature is None
    opt = train.parse(["--scheduled-sampling-start", "3", "--scheduled-sampling-increase-every", "2",
                       "--scheduled-sampling-increase-prob", "0.1", "--scheduled-sampling-max-prob", "0.5", "--ss-temperature", "0.7"])
    assert (opt.scheduled_sampling_start, opt.scheduled_sampling_increase_every, opt.scheduled_sampling_increase_prob,
            opt.scheduled_sampling_max_prob, opt.ss_temperature) == (3, 2, 0.1, 0.5, 0.7)
    for bad in (["--self-critical"], ["--model", "att_baseline"], ["--scheduled-sampling-max-prob", "1.5"], ["--ss-temperature", "0"]):
        with pytest.raises(SystemExit):
            train.parse(["--scheduled-sampling-start", "0"] + bad)
    assert train.parse(["--self-critical"]).scheduled_sampling_start == -1      # (each alone is fine)


def _cpu_model():
    import S2VTModel
    return S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")])
def test_forward_refuses_ss_prob_outside_the_unit_interval(bad):
    m = _cpu_model()
    with pytest.raises(ValueError, match="ss_prob"):
        m(torch.zeros(2, 5, 16), targets=torch.zeros(2, 4, dtype=torch.long), mode="train", ss_prob=bad)
    from s2vt_video_caption_amd import functional
    with pytest.raises(ValueError):
        functional.check_ss_prob(bad)


def test_forward_needs_gpu_tensors_for_scheduled_sampling():
    import inspect
    import S2VTModel
    sig = inspect.signature(S2VTModel.S2VT.forward)
    assert sig.parameters["ss_prob"].default == 0.0 and sig.parameters["ss_temperature"].default is None
    m = _cpu_model()
    with pytest.raises(capi.S2VTHipError):
        m(torch.zeros(2, 5, 16), targets=torch.zeros(2, 4, dtype=torch.long), mode="train", ss_prob=0.5, seed=1)
    for kw in (dict(rnn_type="gru"), dict(num_layers=2)):
        g = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8, **kw)
        with pytest.raises(capi.S2VTHipError):
            g(torch.zeros(2, 5, 16), targets=torch.zeros(2, 4, dtype=torch.long), mode="train", ss_prob=0.5, seed=1)


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert "0x53534D58" in header and sampling.SS_STREAM_TAG == 0x53534D58
    philox = open(os.path.join(ROOT, "s2vt-video-caption_amd", "csrc", "philox.h")).read()
    assert "SS_STREAM_TAG = 0x53534D58u" in philox


def _last_error(lib):
    msg = lib.s2vt_last_error()
    return msg.decode() if msg else ""


@pytest.mark.parametrize("p,mode,temperature,match", [
    (-0.01, 0, 1.0, "ss_prob"), (1.01, 0, 1.0, "ss_prob"), (float("nan"), 0, 1.0, "ss_prob"), (float("inf"), 0, 1.0, "ss_prob"),
    (0.5, 2, 1.0, "draw_mode"), (0.5, 1, 0.0, "temperature"), (0.5, 1, float("nan"), "temperature"),
])
def test_scheduled_decode_arguments_rejected_on_the_host(lib, p, mode, temperature, match):
    """every argument is checked before anything is enqueued: fake (never dereferenced) pointers, no GPU needed"""
    d = capi.Dims(4, 6, 64, 32, 40, 301)
    ps = capi.Params()
    rc = lib.s2vt_scheduled_decode(d, ps, 16, 16, 5, p, mode, temperature, 7, 16, None, 16, 1 << 30, None)
    assert rc == -1 and match in _last_error(lib)
    rc = lib.s2vt_scheduled_decode_cached(d, ps, 16, 16, 5, p, mode, temperature, 7, 16, None, 16, 1 << 30, 16, 1 << 30, 0, None)
    assert rc == -1 and match in _last_error(lib)


def test_scheduled_decode_null_pointers_rejected_on_the_host(lib):
    d = capi.Dims(4, 6, 64, 32, 40, 301)
    ps = capi.Params()
    for args in ((None, 16, 5, 0.5, 0, 1.0, 7, 16), (16, None, 5, 0.5, 0, 1.0, 7, 16), (16, 16, 5, 0.5, 0, 1.0, 7, None),
                 (16, 16, 4, 0.5, 0, 1.0, 7, 16)):          # (the last: a row stride below L - 1)
        assert lib.s2vt_scheduled_decode(d, ps, *args, None, 16, 1 << 30, None) == -1
    assert lib.s2vt_scheduled_decode_cached(d, ps, 16, 16, 5, 0.5, 0, 1.0, 7, 16, None, 16, 1 << 30, None, 0, 0, None) == -1
    assert "null cache" in _last_error(lib)
    assert lib.s2vt_ss_mix(None, 16, 5, 4, 0.5, 7, 1, 0, 16, None) == -1
    assert lib.s2vt_ss_mix(16, 16, 5, 4, 1.5, 7, 1, 0, 16, None) == -1 and "ss_prob" in _last_error(lib)
    assert lib.s2vt_ss_mix(16, 16, 5, 4, 0.5, 7, 5, 0, 16, None) == -1           # step outside the row
    assert lib.s2vt_ss_unpack(16, 5, 4, 16, 4, 0.5, 7, 16, None, None) == -1      # row stride below the steps
