"""CPU: the clipped step's C-ABI entry points (include/s2vt_hip.h, "clipped step") are exported, bound and refuse bad arguments before
any device call; tests/optim_ref.step_ref - the numpy restatement the GPU tests compare the kernels with - agrees with torch's own
clip_grad_norm_ + Adam(weight_decay) / AdamW; optim.decay_segments builds the segments; train.py refuses the flag combinations."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref  # noqa: E402

ENTRIES = ("s2vt_grad_norm_workspace_bytes", "s2vt_grad_norm", "s2vt_adam_step_clipped")
EPS32 = float(np.finfo(np.float32).eps)


def test_clip_entry_points_exported_and_bound(lib):
    from s2vt_video_caption_amd import capi
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(raw, name), "libs2vt_hip.so does not export %s" % name
        assert name in capi.SIGNATURES, "capi.py does not bind %s" % name
        assert (name + "(") in header
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9
    assert "#define S2VT_GRAD_NORM_CHUNK %d\n" % capi.GRAD_NORM_CHUNK in header
    assert "#define S2VT_ADAM_MAX_SEGMENTS %d\n" % capi.ADAM_MAX_SEGMENTS in header
    assert ctypes.sizeof(capi.ClipRecord) == 24 and capi.ClipRecord.skipped_total.offset == 16


def test_grad_norm_workspace_depends_on_n_only(lib):
    from s2vt_video_caption_amd import capi
    C = capi.GRAD_NORM_CHUNK
    assert C % 1024 == 0
    ws = lib.s2vt_grad_norm_workspace_bytes
    assert ws(0) == 0 and ws(-5) == 0
    for n, parts in ((1, 1), (C - 1, 1), (C, 1), (C + 1, 2), (2 * C + 5, 3), (1000003, -(-1000003 // C))):
        assert ws(n) == 8 * parts, n
        assert ws(n) == ws(n)                      # the same on every call: no device property enters
    assert ws(48_000_000) // 8 <= 4096             # the largest model here: at most a few thousand partials


def _rejects(lib, name, rc, word):
    assert rc == -1, (name, rc)
    msg = lib.s2vt_last_error()
    assert name.encode() in msg and word.encode() in msg, (name, word, msg)


def test_grad_norm_rejects_bad_arguments(lib):
    """every refusal of s2vt_grad_norm returns S2VT_ERR_ARG with a message naming the rule; no device call is made (pointers are never
    dereferenced: the argument checks run first)"""
    p, n = ctypes.c_void_p(4096), 100
    ws = lib.s2vt_grad_norm_workspace_bytes(n)
    nan, inf = float("nan"), float("inf")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(None, n, 1.0, 0, p, ws, p, None), "gradient")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(ctypes.c_void_p(4098), n, 1.0, 0, p, ws, p, None), "gradient")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, 0, 1.0, 0, p, ws, p, None), "positive")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, 1.0, 0, p, ws, None, None), "record")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, 1.0, 0, p, ws, ctypes.c_void_p(4104), None), "record")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, nan, 0, p, ws, p, None), "max_norm")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, -inf, 0, p, ws, p, None), "max_norm")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, 1.0, 0, None, ws, p, None), "workspace")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, n, 1.0, 0, p, ws - 1, p, None), "workspace")
    _rejects(lib, "grad_norm", lib.s2vt_grad_norm(p, 40000, 1.0, 0, p, ws, p, None), "workspace")       # three partials, room for one


def test_adam_step_clipped_rejects_bad_arguments(lib):
    p, n = ctypes.c_void_p(4096), 100
    nan, inf = float("nan"), float("inf")
    i64 = lambda *a: (ctypes.c_int64 * len(a))(*a)
    i32 = lambda *a: (ctypes.c_int32 * len(a))(*a)

    def call(params=p, grads=p, m=p, v=p, n=n, step=1, wd=0.01, seg_end=None, seg_decay=None, n_seg=0, skip=0, record=p):
        return lib.s2vt_adam_step_clipped(params, grads, m, v, n, 1e-3, 0.9, 0.999, 1e-8, step, wd, 0, seg_end, seg_decay, n_seg, skip,
                                          record, None)
    name = "adam_flat_clipped"
    for kw in ({"params": None}, {"grads": None}, {"m": None}, {"v": None}, {"params": ctypes.c_void_p(4104)}, {"grads": ctypes.c_void_p(4100)}):
        _rejects(lib, name, call(**kw), "buffers")
    _rejects(lib, name, call(n=0), "positive")
    _rejects(lib, name, call(step=0), "step")
    for wd in (-1e-3, nan, inf):
        _rejects(lib, name, call(wd=wd), "weight_decay")
    _rejects(lib, name, call(seg_end=i64(*range(1, 18)), seg_decay=i32(*[1] * 17), n_seg=17), "n_seg")
    _rejects(lib, name, call(n_seg=-1), "n_seg")
    _rejects(lib, name, call(seg_end=None, seg_decay=i32(1, 0), n_seg=2), "segment")
    _rejects(lib, name, call(seg_end=i64(50, 50, 100), seg_decay=i32(1, 0, 1), n_seg=3), "ascend")
    _rejects(lib, name, call(seg_end=i64(60, 50, 100), seg_decay=i32(1, 0, 1), n_seg=3), "ascend")
    _rejects(lib, name, call(seg_end=i64(0, 100), seg_decay=i32(1, 0), n_seg=2), "ascend")
    _rejects(lib, name, call(seg_end=i64(50, 99), seg_decay=i32(1, 0), n_seg=2), "end at n")
    _rejects(lib, name, call(seg_end=i64(50, 101), seg_decay=i32(1, 0), n_seg=2), "end at n")
    _rejects(lib, name, call(record=ctypes.c_void_p(4104)), "record")
    _rejects(lib, name, call(record=None, skip=1), "record")


def _torch_leg(n, decoupled, feed_scale):
    """five steps (lr 1e-3, wd 0.01, max_norm 0.5, the gradient recipe of test_flat_adam_step_is_torch_adam) of step_ref beside torch on
    the CPU.  feed_scale False: torch.nn.utils.clip_grad_norm_ itself; True: torch steps on grad * step_ref's scale (torch's norm
    sums in fp32 and is ~200 fp32 eps off at a million elements - through no fault of either side that moves m, v, p by far more
    than the roundings this comparison is about).  Yields what the assertions need per step."""
    lr, wd, c = 1e-3, 0.01, 0.5
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_()
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], lr=lr, weight_decay=wd)
    p, m, v = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-4, 2, (1,), generator=g)))
        norm, scale, skipped = optim_ref.step_ref(p, grad.numpy(), m, v, step, lr, 0.9, 0.999, 1e-8, max_norm=c, wd=wd, decoupled=decoupled)
        assert not skipped
        if feed_scale:
            ref.grad = grad * float(scale)
            tnorm = None
        else:
            ref.grad = grad.clone()
            tnorm = float(torch.nn.utils.clip_grad_norm_([ref], c))
        opt.step()
        st = opt.state[ref]
        yield step, float(norm), tnorm, (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy()), (p, ref.detach().numpy())


def _assert_close(step, mm, vv, pp):
    for got, want in (mm, vv):
        assert np.abs(got - want).max() <= 4e-7 * np.abs(want).max()
    got, want = pp
    assert np.abs(got - want).max() <= 2 * step * float(np.spacing(np.float32(np.abs(want).max())))


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("n", [1, 5, 4096])
def test_step_ref_is_torch_clip_and_adam(n, decoupled):
    """step_ref against clip_grad_norm_ + torch.optim.Adam(weight_decay) / AdamW.  The norms agree within 8 fp32 eps: step_ref's is
    exact to its final rounding, torch's fp32 sum of n <= 4096 squares rounds about log2(n) = 12 times on its way (each 1/2 eps of the
    sum, halved by the square root) and once more at the root.  m, v within 4e-7 of their largest element (the bound of
    test_flat_adam_step_is_torch_adam); p within 2 * step spacings of its largest element: one final rounding of p per step on
    either side, doubled."""
    for step, norm, tnorm, mm, vv, pp in _torch_leg(n, decoupled, feed_scale=False):
        assert abs(norm - tnorm) <= 8 * EPS32 * tnorm
        _assert_close(step, mm, vv, pp)


@pytest.mark.parametrize("decoupled", [False, True])
def test_step_ref_is_torch_adam_at_a_million_elements(decoupled):
    """n = 1 000 003: torch steps on the gradient times step_ref's own scale (see _torch_leg); same bounds"""
    for step, _, _, mm, vv, pp in _torch_leg(1000003, decoupled, feed_scale=True):
        _assert_close(step, mm, vv, pp)


def test_step_ref_skip_scale_and_mask():
    f32 = np.float32
    rng = np.random.default_rng(3)
    p0, g = rng.standard_normal(64).astype(f32), rng.standard_normal(64).astype(f32)
    # a non-finite gradient: skipped, nothing moves
    for bad in (np.inf, np.nan):
        gb = g.copy(); gb[17] = bad
        p, m, v = p0.copy(), np.full(64, 0.5, f32), np.full(64, 0.25, f32)
        norm, _, skipped = optim_ref.step_ref(p, gb, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, max_norm=1.0, skip_nonfinite=True)
        assert skipped and not np.isfinite(norm) and np.array_equal(p, p0) and (m == 0.5).all() and (v == 0.25).all()
    # max_norm above the norm: scale exactly 1; below: the fp32 formula
    norm = optim_ref.grad_norm_ref(g)
    assert optim_ref.scale_ref(norm, 1e30) == f32(1.0) and optim_ref.scale_ref(norm, None) == f32(1.0) and optim_ref.scale_ref(norm, 0.0) == f32(1.0)
    assert optim_ref.scale_ref(norm, 0.5) == f32(0.5) / (norm + f32(1e-6)) < 1
    # the mask: undecayed elements take the step without decay, decayed ones the step with it
    mask = np.arange(64) % 3 == 0
    outs = []
    for wd, dm in ((0.01, mask), (0.0, None), (0.01, None)):
        p, m, v = p0.copy(), np.zeros(64, f32), np.zeros(64, f32)
        optim_ref.step_ref(p, g, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, wd=wd, decay_mask=dm)
        outs.append((p, m, v))
    for a, plain, full in zip(*outs):
        assert np.array_equal(a[~mask], plain[~mask]) and np.array_equal(a[mask], full[mask])


def test_decay_segments_merge_limit_and_order():
    from s2vt_video_caption_amd import capi, optim
    names = list(capi.PARAM_KEYS)
    sizes = [40, 40, 8, 8, 72, 40, 8, 8, 30, 5, 60, 12, 96]

    def tile(order):
        out, at = [], 0
        for i in order:
            out.append((at, at + sizes[i]))
            at += sizes[i]
        return out
    order = list(range(13))
    assert optim.decay_segments(names, tile(order), ()) == ([sum(sizes)], [1])
    ends, flags = optim.decay_segments(names, tile(order), ("bias",))
    # vid w w | b b | word w w | b b | feat w | b | out w | b | emb: neighbours with one flag are one segment
    assert flags == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert ends == [80, 96, 208, 224, 254, 259, 319, 331, 427]
    ends, flags = optim.decay_segments(names, tile(order), ("bias", "embedding.weight"))
    assert flags == [1, 0, 1, 0, 1, 0, 1, 0] and ends[-1] == 427 and ends[-2] == 319
    assert optim.matches_no_decay("vid_rnn.bias_ih_l0", ("bias",)) and optim.matches_no_decay("feat_linear.bias", ("bias",))
    assert not optim.matches_no_decay("embedding.weight", ("bias",)) and optim.matches_no_decay("embedding.weight", ("embedding.weight",))
    # another parameter order (a reducer's): the segments follow the slices handed over, not the model's order
    rorder = [12, 10, 11, 4, 5, 6, 7, 0, 1, 2, 3, 8, 9]
    ends, flags = optim.decay_segments([names[i] for i in rorder], tile(rorder), ("bias",))
    assert flags == [1, 0, 1, 0, 1, 0, 1, 0] and ends[:3] == [96 + 60, 96 + 60 + 12, 96 + 60 + 12 + 112] and ends[-1] == 427
    # more than 16 segments after merging: ValueError; exactly 16: accepted
    many = ["w%d.weight" % (i // 2) if i % 2 == 0 else "w%d.bias" % (i // 2) for i in range(17)]
    sl = [(4 * i, 4 * i + 4) for i in range(17)]
    with pytest.raises(ValueError, match="segments"):
        optim.decay_segments(many, sl, ("bias",))
    assert len(optim.decay_segments(many[:16], sl[:16], ("bias",))[0]) == 16
    assert optim.decay_segments(many, sl, ())[0] == [68]
    with pytest.raises(ValueError, match="tile"):
        optim.decay_segments(["a", "b"], [(0, 4), (8, 12)], ())


def test_flat_adam_checks_its_arguments_before_the_library():
    from s2vt_video_caption_amd import optim
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FlatAdam(None, max_grad_norm=bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            optim.FlatAdam(None, weight_decay=bad)
    with pytest.raises(TypeError):
        optim.FlatAdam(None, 1e-3, (0.9, 0.999), 1e-8, None, 1.0)          # the new arguments are keyword-only


def test_train_cli_clip_flags():
    sys.path.insert(0, ROOT)
    import train
    o = train.parse([])
    assert (o.grad_clip, o.weight_decay, o.adamw, o.no_decay_bias, o.skip_nonfinite) == (0.0, 0.0, False, False, False)
    o = train.parse(["--grad-clip", "1", "--weight-decay", "5e-5", "--adamw", "--no-decay-bias", "--skip-nonfinite"])
    assert (o.grad_clip, o.weight_decay, o.adamw, o.no_decay_bias, o.skip_nonfinite) == (1.0, 5e-5, True, True, True)
    assert train.parse(["--rnn-type", "gru", "--grad-clip", "2", "--weight-decay", "1e-4", "--adamw"]).grad_clip == 2.0
    for argv in (["--skip-nonfinite", "--rnn-type", "gru"], ["--skip-nonfinite", "--num-layers", "2"],
                 ["--skip-nonfinite", "--model", "att_baseline"], ["--grad-clip", "-1"], ["--grad-clip", "nan"],
                 ["--weight-decay", "-1e-5"], ["--weight-decay", "inf"], ["--adamw"], ["--no-decay-bias"]):
        with pytest.raises(SystemExit):
            train.parse(argv)
