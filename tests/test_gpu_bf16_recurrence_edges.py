"""GPU: the bf16-operand (config 3) LSTM recurrence kernels - csrc/lstm_bf16.hip (one launch per timestep) and the bf16 half of
csrc/lstm_persist.hip (persistent forward and BPTT) - against the fp64 restatements of tests/bf16_recur_ref.py, every step
teacher-forced from what the device itself wrote for the step before, at the places where such kernels break and the rest of the suite
does not go.  The case lists are bf16_recur_ref's; tests/test_bf16_recur_ref_host.py shows on the host that fp32 arithmetic stays
under half of each bound and that a structural mistake moves an output by thousands of bounds.

  a  per-timestep forward: B on both sides of the 32 / 64 row tiles and of the <1,2> / <2,2> switch at H = 37, B = 1; H on both sides of
     the 16-unit tile, H = 3 and 16 (Kp = 64: one k chunk, three of the four k-split waves load nothing), (5, 1000); n_gx = 0, between, T.
  b  per-timestep backward at the new bound: B in {1, 32, 33, 65}, H around the 32-unit tile, H = 3 and 16 (Kp = 64); dh_first = 0,
     between, == T, dh_out = None, T = 1.
  c  persistent forward: H = 8 and 5 (one ragged column slice, Kp = 64: the second k-half wave has no chunk), odd H = 37, 999 and 5 (the
     scalar path of CellLane; with block < T its carry()), H = 70, H = 1024 (the FULL template); the _pair entry bit-equal to solo runs.
  d  persistent BPTT at the new bound under bptt_units 0, 16 and 32: H = 8, H = 40 and 72 (the 32-unit slice ragged by 8), 1000, 1024
     (4H = 4096, the largest k), dh_first == T (nothing flows: dG = 0 exactly); one _pair case bit-equal to solo runs.
  e  refusals: persistent forward at B = 33 and H = 1032, BPTT at H = 36 and H = 1032 (and the _pair entries): an error that names the
     shape, no launch - the outputs still NaN, the workspace untouched, no asynchronous error.
  f  every case of a to d a second time on a workspace full of 0xFF bytes: bit-equal to the zero-workspace run.
  g  the bf16 row images (h rows / dG rows) read back from the poisoned workspace of ragged cases of all four kernels: rows [0, T*B)
     equal bf16(fp32 output) bit for bit in columns [0, H) / [0, 4H) - the last step's rows included, which no later step reads - and
     columns up to kpad are all zero bits.  The weight images of the same workspaces equal bf16(W_hh) / bf16(W_hh^T) likewise.

In every case of a to d: h / c outputs prefilled with NaN (the wrappers do it), the gx rows of the steps that take the bias alone NaN,
inputs compared bit for bit after the calls, a second call bit-equal, every output finite.  Bounds: forward 2e-5 absolute (the
project's); backward bf16_recur_ref.BWD_REL * max|ref| + 1e-9 = 5e-6 * max|ref| + 1e-9, where the free-running comparison of
test_gpu_kernels.py needs 2e-3 * max|ref|.  Every test prints its worst error / bound.
Seen on an MI355X (worst error / bound over the cases of a group; every case passed as the kernels stand, no product fix was needed):
  a  0.012 ((32, 37), n_gx = T: c 2.4e-7)              b  0.048 ((33, 37) at T = 1: dG 2.7e-8 of a bound of 5.6e-7)
  c  0.014 ((64, 1024): gates 2.8e-7), pair 0.009       d  0.039 ((64, 1024), 32 units: dG 4.5e-8 of 1.15e-6; 16 units 0.032), pair 0.033
     (the old 2e-3 * max|ref| + 1e-7 is 4.6e-4 there: 400 times the new bound)
  e  all eight refused with rc = -1, e.g. "s2vt_lstm_seq_bwd_bf16: shape B=32 H=36 (Kp=192) not supported by the persistent kernel"
  f  every poisoned run bit-equal                        g  0 elements differ, 0 pad elements are not zero bits in all seven images:
     the pad lanes of the persistent forward's ragged 16-unit tile are exact zeros (sigmoid(0) . tanh(0) of ActFast is 0.5 . 0)
Tried once on the device: with zero_pad_cols_u16 taken out of seq_bf16_prepare and seq_bwd_bf16_prepare, every case of a to d and g
whose k extent (H, 4H for the backward) is not a multiple of 64 and that has a contraction (T > 1) failed - 51 of the 60 tests, NaN
from the 0xFF padding in the poisoned run - and the others passed; a zeroed workspace hides it, the padding is then zero without the call."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_recur_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _fwd_device_inputs(T, B, H, n_gx, seed=11):
    """device (gx, bias, w_hh): the gx rows of the steps that run on the bias alone are NaN - the kernels must not read them, and write
    their gates there"""
    gx, bias, w = R.fwd_inputs(T, B, H, seed)
    gxd = gx.to(DEV)
    gxd[n_gx * B:] = NAN
    return gxd, bias.to(DEV), w.to(DEV)


def _check_fwd(lib, T, B, H, n_gx, persistent, block=0):
    """the forward of one case: zero workspace, again, poisoned workspace; teacher-forced.  Returns (results, poisoned workspace, error / bound)."""
    from s2vt_video_caption_amd import ops
    gx, bias, w = R.fwd_inputs(T, B, H)
    gxd, biasd, wd = _fwd_device_inputs(T, B, H, n_gx)
    keep = [t.clone() for t in (gxd, biasd, wd)]
    args = (gxd, n_gx, biasd, wd, T, B, H)
    first = ops.lstm_seq_fwd_bf16(*args, persistent=persistent, block=block)
    again = ops.lstm_seq_fwd_bf16(*args, persistent=persistent, block=block)
    *poisoned, ws = ops.lstm_seq_fwd_bf16(*args, persistent=persistent, block=block, poison=True, return_workspace=True)
    torch.cuda.synchronize()
    assert _finite(*first) and _finite(*again) and _finite(*poisoned)
    for name, a, b, c in zip(("h", "c", "gates"), first, again, poisoned):
        assert _same_bits(a, b), "%s: a second call differs" % name
        assert _same_bits(a, c), "%s: the run on a workspace of 0xFF bytes differs from the run on a zeroed one" % name
    for t, k in zip((gxd, biasd, wd), keep):
        assert _same_bits(t, k), "an input was written"
    e = R.fwd_teacher_forced(*first, gx, n_gx, bias, w, T, B, H)
    print("fwd T=%d B=%d H=%d n_gx=%d persistent=%s block=%d: h %.2e c %.2e gates %.2e / %.0e = %.3f"
          % (T, B, H, n_gx, persistent, block, e["h"], e["c"], e["gates"], R.TOL_FWD, e["worst"] / R.TOL_FWD))
    assert e["worst"] <= R.TOL_FWD, e
    return first, ws, e["worst"] / R.TOL_FWD


def _bwd_device_inputs(T, B, H, dh_first, seed=50):
    w, gates, c_all, dh = R.bwd_inputs(T, B, H, dh_first, seed)
    return w.to(DEV), (None if dh is None else dh.to(DEV)), c_all.to(DEV), gates.to(DEV)


def _check_bwd(lib, T, B, H, dh_first, persistent, block=0):
    """the BPTT of one case: zero workspace, again, poisoned workspace; teacher-forced at the new bound.  Returns (dG, poisoned workspace,
    error / bound)."""
    from s2vt_video_caption_amd import ops
    w, gates, c_all, dh = R.bwd_inputs(T, B, H, dh_first)
    wd, dhd, cd, gd = _bwd_device_inputs(T, B, H, dh_first)
    keep = [None if t is None else t.clone() for t in (wd, dhd, cd, gd)]
    args = (wd, dhd, dh_first or 0, cd, gd, T, B, H)
    first = ops.lstm_seq_bwd_bf16(*args, persistent=persistent, block=block)
    again = ops.lstm_seq_bwd_bf16(*args, persistent=persistent, block=block)
    poisoned, ws = ops.lstm_seq_bwd_bf16(*args, persistent=persistent, block=block, poison=True, return_workspace=True)
    torch.cuda.synchronize()
    assert _finite(first, again, poisoned)
    assert _same_bits(first, again), "a second call differs"
    assert _same_bits(first, poisoned), "the run on a workspace of 0xFF bytes differs from the run on a zeroed one"
    for t, k in zip((wd, dhd, cd, gd), keep):
        assert t is None or _same_bits(t, k), "an input was written"
    r = R.bwd_teacher_forced(first, w, dh, dh_first, c_all, gates, T, B, H)
    print("bwd T=%d B=%d H=%d dh_first=%s persistent=%s block=%d: dG %.2e / %.2e = %.3f (max|ref| %.3f; the old bound: %.2e)"
          % (T, B, H, dh_first, persistent, block, r["worst"], r["bound"], r["worst"] / r["bound"], r["ref_max"], 2e-3 * r["ref_max"] + 1e-7))
    assert r["worst"] <= r["bound"], r
    assert (r["ref_max"] > 0) == R.has_gradient(T, dh_first)
    if not R.has_gradient(T, dh_first):
        assert not bool(first.any()), "nothing flows: every dG is zero"
    return first, ws, r["worst"] / r["bound"]


class _bptt_units:
    def __init__(self, lib, units):
        self.lib, self.units = lib, units

    def __enter__(self):
        self.prev = self.lib.s2vt_set_option(b"bptt_units", self.units)

    def __exit__(self, *exc):
        self.lib.s2vt_set_option(b"bptt_units", self.prev)


# ------------------------------------------------------------------------------------------------------- a, b: one launch per step
@pytest.mark.parametrize("case", R.STEP_FWD_CASES, ids=_ids)
def test_a_step_forward_teacher_forced_zero_and_poisoned_workspace(lib, case):
    _check_fwd(lib, *case, persistent=False)


@pytest.mark.parametrize("case", R.STEP_BWD_CASES, ids=_ids)
def test_b_step_backward_teacher_forced_zero_and_poisoned_workspace(lib, case):
    _check_bwd(lib, *case, persistent=False)


# ------------------------------------------------------------------------------------------------------------- c, d: persistent
@pytest.mark.parametrize("case", R.PERSIST_FWD_CASES, ids=_ids)
def test_c_persistent_forward_teacher_forced_zero_and_poisoned_workspace(lib, case):
    T, B, H, n_gx, block = case
    assert lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H) > 0
    _check_fwd(lib, T, B, H, n_gx, persistent=True, block=block)


def test_c_persistent_forward_pair_is_bit_equal_to_solo_runs(lib):
    from s2vt_video_caption_amd import ops
    T, B, H, n_gx, block = R.PERSIST_FWD_PAIR
    ins = [_fwd_device_inputs(T, B, H, n_gx, seed=11 + 10 * k) for k in range(2)]
    host = [R.fwd_inputs(T, B, H, 11 + 10 * k) for k in range(2)]
    (g0, b0, w0), (g1, b1, w1) = ins
    worst = 0.0
    for poison in (False, True):
        pair = ops.lstm_seq_fwd_bf16_pair(g0, g1, n_gx, b0, b1, w0, w1, T, B, H, block=block, poison=poison)
        for (g, b, w), (gx, bias, wh), got in zip(ins, host, pair):
            solo = ops.lstm_seq_fwd_bf16(g, n_gx, b, w, T, B, H, persistent=True, block=block)
            assert _finite(*got)
            for x, y in zip(got, solo):
                assert _same_bits(x, y), "poison=%s" % poison
            worst = max(worst, R.fwd_teacher_forced(*got, gx, n_gx, bias, wh, T, B, H)["worst"])
    print("fwd pair T=%d B=%d H=%d: %.2e / %.0e = %.3f" % (T, B, H, worst, R.TOL_FWD, worst / R.TOL_FWD))
    assert worst <= R.TOL_FWD


@pytest.mark.parametrize("units", R.BPTT_UNITS)
@pytest.mark.parametrize("case", R.PERSIST_BWD_CASES, ids=_ids)
def test_d_persistent_bptt_teacher_forced_zero_and_poisoned_workspace(lib, case, units):
    T, B, H, dh_first, block = case
    with _bptt_units(lib, units):
        _check_bwd(lib, T, B, H, dh_first, persistent=True, block=block)


def test_d_persistent_bptt_pair_is_bit_equal_to_solo_runs(lib):
    from s2vt_video_caption_amd import ops
    T, B, H, dh_first, block = R.PERSIST_BWD_PAIR
    ins = [_bwd_device_inputs(T, B, H, dh_first, seed=50 + 20 * k) for k in range(2)]
    host = [R.bwd_inputs(T, B, H, dh_first, 50 + 20 * k) for k in range(2)]
    (w0, d0, c0, g0), (w1, d1, c1, g1) = ins
    frac = 0.0
    for poison in (False, True):
        pair = ops.lstm_seq_bwd_bf16_pair(w0, w1, d0, d1, dh_first, c0, c1, g0, g1, T, B, H, block=block, poison=poison)
        for (wd, dd, cd, gd), (w, gates, c_all, dh), got in zip(ins, host, pair):
            solo = ops.lstm_seq_bwd_bf16(wd, dd, dh_first, cd, gd, T, B, H, persistent=True, block=block)
            assert _finite(got) and _same_bits(got, solo), "poison=%s" % poison
            r = R.bwd_teacher_forced(got, w, dh, dh_first, c_all, gates, T, B, H)
            assert r["worst"] <= r["bound"], r
            frac = max(frac, r["worst"] / r["bound"])
    print("bwd pair T=%d B=%d H=%d: worst error / bound = %.3f" % (T, B, H, frac))


# ------------------------------------------------------------------------------------------------------------------ e: refusals
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _refused(lib, rc, what, B, H, outs, ws):
    from s2vt_video_caption_amd import capi
    msg = lib.s2vt_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    print("%s B=%d H=%d: rc=%d %s" % (what, B, H, rc, msg))
    assert rc != 0, "%s accepted B=%d H=%d" % (what, B, H)
    assert what in msg and "B=%d" % B in msg and "H=%d" % H in msg, msg
    capi.check_async_error()
    for o in outs:
        assert bool(torch.isnan(o).all()), "an output of a refused call was written"
    assert bool((ws == 0xFF).all()), "the workspace of a refused call was written: something was launched"


@pytest.mark.parametrize("B,H", R.REFUSE_FWD)
@pytest.mark.parametrize("pair", [False, True])
def test_e_persistent_forward_refuses_the_shape_before_any_launch(lib, B, H, pair):
    T = 2
    n = lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H)
    assert n > 0
    ws = torch.full((2 * n,), 0xFF, dtype=torch.uint8, device=DEV)
    st = [torch.full((T * B, 4 * H), NAN, device=DEV) for _ in range(2)]
    hc = [torch.full((T * B, H), NAN, device=DEV) for _ in range(4)]
    w = torch.zeros(4 * H, H, device=DEV)
    if pair:
        rc = lib.s2vt_lstm_seq_fwd_bf16_pair(T, B, H, _ptr(st[0]), _ptr(st[1]), T, None, None, _ptr(w), _ptr(w), _ptr(hc[0]), _ptr(hc[1]),
                                             _ptr(hc[2]), _ptr(hc[3]), _ptr(ws), 2 * n, 0, _stream())
    else:
        rc = lib.s2vt_lstm_seq_fwd_bf16(T, B, H, _ptr(st[0]), T, None, _ptr(w), _ptr(hc[0]), _ptr(hc[1]), _ptr(ws), n, 1, 0, _stream())
    _refused(lib, rc, "s2vt_lstm_seq_fwd_bf16_pair" if pair else "s2vt_lstm_seq_fwd_bf16", B, H, st + hc, ws)


@pytest.mark.parametrize("B,H", R.REFUSE_BWD)
@pytest.mark.parametrize("pair", [False, True])
def test_e_persistent_bptt_refuses_the_shape_before_any_launch(lib, B, H, pair):
    T = 2
    n = lib.s2vt_lstm_seq_bwd_bf16_workspace_bytes(T, B, H)
    assert n > 0
    ws = torch.full((2 * n,), 0xFF, dtype=torch.uint8, device=DEV)
    dg = [torch.full((T * B, 4 * H), NAN, device=DEV) for _ in range(2)]
    w, c, dh = torch.zeros(4 * H, H, device=DEV), torch.zeros(T * B, H, device=DEV), torch.zeros(T * B, H, device=DEV)
    if pair:
        rc = lib.s2vt_lstm_seq_bwd_bf16_pair(T, B, H, _ptr(w), _ptr(w), _ptr(dh), _ptr(dh), 0, _ptr(c), _ptr(c), _ptr(dg[0]), _ptr(dg[1]),
                                             _ptr(ws), 2 * n, 0, _stream())
    else:
        rc = lib.s2vt_lstm_seq_bwd_bf16(T, B, H, _ptr(w), _ptr(dh), 0, _ptr(c), _ptr(dg[0]), _ptr(ws), n, 1, 0, _stream())
    _refused(lib, rc, "s2vt_lstm_seq_bwd_bf16_pair" if pair else "s2vt_lstm_seq_bwd_bf16", B, H, dg, ws)


# ------------------------------------------------------------------------------------------------------------ g: the row images
def _check_image(ws, T, B, H, backward, fp32_rows, what):
    """the bf16 row image inside a (poisoned) workspace against the fp32 output the same run wrote"""
    from s2vt_video_caption_amd import ops
    lay = ops.seq_bf16_layout(T, B, H, backward=backward)
    img, kpad = R.image_view(ws, lay, T * B)
    k = fp32_rows.shape[1]
    assert k == (4 * H if backward else H) and kpad == R.pad64(k) and img.shape[1] >= kpad
    want = R.bf16_bits(fp32_rows)
    diff = img[:, :k] != want
    nz = img[:, k:kpad] != 0
    print("%s T=%d B=%d H=%d: image [%d, %d] of kpad %d: %d of %d elements differ from bf16(output), %d of %d pad elements are not zero bits"
          % (what, T, B, H, T * B, k, kpad, int(diff.sum()), diff.numel(), int(nz.sum()), nz.numel()))
    assert not bool(diff.any()), "%s: rows %s differ from bf16 of the fp32 output" % (what, sorted(set(diff.nonzero()[:, 0].tolist()))[:8])
    assert not bool(nz.any()), "%s: pad columns %s hold %s" % (what, sorted(set((nz.nonzero()[:, 1] + k).tolist()))[:16],
                                                              [hex(v & 0xFFFF) for v in img[:, k:kpad][nz][:4].tolist()])


def _check_weight_image(ws, T, B, H, backward, what):
    """the bf16 weight image of the same workspace: bf16(W_hh) rows (forward) or bf16(W_hh^T) rows (backward), k padding zero bits"""
    from s2vt_video_caption_amd import ops
    w = (R.bwd_inputs(T, B, H, 1)[0] if backward else R.fwd_inputs(T, B, H)[2]).to(DEV)
    w = w.t().contiguous() if backward else w
    img, kpad = R.image_view(ws, ops.seq_bf16_layout(T, B, H, backward=backward), w.shape[0], which="w")
    k = w.shape[1]
    assert kpad == R.pad64(k)
    assert torch.equal(img[:, :k], R.bf16_bits(w)), "%s: the weight image is not bf16 of the weights" % what
    assert not bool(img[:, k:kpad].any()), "%s: the k padding of the weight image is not zero" % what


def test_g_row_image_of_the_step_forward(lib):
    T, B, H, n_gx = R.IMAGE_STEP_FWD
    (h, c, s), ws, _ = _check_fwd(lib, T, B, H, n_gx, persistent=False)
    _check_image(ws, T, B, H, False, h, "step forward")
    _check_weight_image(ws, T, B, H, False, "step forward")


def test_g_row_image_of_the_step_backward(lib):
    T, B, H, dh_first = R.IMAGE_STEP_BWD
    dg, ws, _ = _check_bwd(lib, T, B, H, dh_first, persistent=False)
    _check_image(ws, T, B, H, True, dg, "step backward")
    _check_weight_image(ws, T, B, H, True, "step backward")


@pytest.mark.parametrize("case", R.IMAGE_PERSIST_FWD, ids=_ids)
def test_g_row_image_of_the_persistent_forward(lib, case):
    T, B, H, n_gx, block = case
    (h, c, s), ws, _ = _check_fwd(lib, T, B, H, n_gx, persistent=True, block=block)
    _check_image(ws, T, B, H, False, h, "persistent forward")
    _check_weight_image(ws, T, B, H, False, "persistent forward")


@pytest.mark.parametrize("units", [16, 32])
def test_g_row_image_of_the_persistent_bptt(lib, units):
    T, B, H, dh_first, block = R.IMAGE_PERSIST_BWD
    with _bptt_units(lib, units):
        dg, ws, _ = _check_bwd(lib, T, B, H, dh_first, persistent=True, block=block)
    _check_image(ws, T, B, H, True, dg, "persistent BPTT (%d units)" % units)
    _check_weight_image(ws, T, B, H, True, "persistent BPTT")
