"""GPU: the fp32 launch-per-timestep LSTM kernels (csrc/lstm.hip) and their loops (seq_fwd / seq_bwd of csrc/api_shared.hip, the fp32
train driver of csrc/api_train_f32.hip) against the fp64 references of tests/lstm_step_ref.py, where the rest of the suite does not
go:

  a  the backward step over a grid of batch x hidden sizes (H not a multiple of 4, of 16; B below, at and past a tile) and the
     32-row tile <2, 1, true> with a ragged last row block, a ragged last column block, both - and the 16-row side of the choice;
  b  the argument forms the BPTT loop issues: the last step (no dg_next, dc not read), step 0 (no c_prev), a step under dh_first
     (no dh_out), a step nothing flows into, and dG written in place over the activated gates;
  c  the scalar instantiation <1, 1, false>, reached through dg_next / W_hh^T views 4 bytes past a 16-byte boundary;
  d  the forward step the decode half of a layer runs (bias, no gx, a state), also on the scalar instantiation;
  e  whole layers through ops.lstm_seq_fwd / ops.lstm_seq_bwd: h, c, the gates, dG and dW_hh;
  f  the fp32 train driver with (L-1) * B * K = 72000 > 65535 rows, plain and grouped: the gather of the embedded rows in more
     than one launch, the column sums and the embedding gradient over that many rows.

Bounds (lstm_step_ref.TOL_*, driver_errors) are the project's: those of test_lstm_step_bwd_matches_autograd,
test_lstm_step_fwd_matches_cell, test_lstm_seq_fwd_bwd_vs_autograd and test_gpu_train_group._assert_close;
tests/test_lstm_step_ref_host.py shows on the host that they leave room and that these inputs can see an error.  Every test prints
its worst error.  Seen on an MI355X (worst over the cases of a group, beside the bound):
  a  dG 4.1e-7, dc 5.3e-7 (5e-6)                 b  dG 4.0e-7, dc 5.1e-7 (5e-6)
  c  dG 3.6e-7, dc 4.3e-7 (5e-6), to the aligned launch 3.0e-7 (1e-5)
  d  h 1.4e-7 (2e-6), c 2.2e-7 (4e-6), gates 3.2e-7 (2e-6)
  e  h 2.1e-7 (2e-6), c 2.4e-7 (4e-6), gates 2.0e-7 (2e-6), dG 4.7e-7 (5e-6), dW 3.1e-7 (2e-5)
  f  logits 1.2e-7 (2e-5); loss 3.0e-6 plain, 7.0e-6 grouped (1e-5: the criterion's one-workgroup fp32 sum over 72000 rows, the
     thinnest margin here); gradients at most 0.11 of their bounds against the oracle (vid_rnn.weight_hh 1.3e-4 of 1.2e-3), 0.13
     grouped against plain; dfeats 9.4e-10 (1.2e-6) where zeros would be 1.1e-3 off."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_step_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def _dev(t):
    return None if t is None else t.to(DEV)


def _off4(t):
    """a contiguous device copy of t whose first element lies 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _err(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item()


@functools.lru_cache(maxsize=None)
def _ref_bwd(B, H, form):
    a = R.form_args(B, H, form)
    return R.step_bwd(a["dg_next"], a["w_hh"], a["dh_out"], a["stash"], a["c"], a["c_prev"], a["dc_in"])


def _run_bwd(lib, B, H, form, off_dg=False, off_wt=False, in_place=False):
    """the device's (dg, dc_prev) of a form.  dc_in None: dc_is_zero with the dc buffer full of NaN (it must not be read)."""
    from s2vt_video_caption_amd import ops
    a = R.form_args(B, H, form)
    wt = a["w_hh"].t().contiguous()
    wt = _off4(wt) if off_wt else wt.to(DEV)
    dg_next = None if a["dg_next"] is None else (_off4(a["dg_next"]) if off_dg else a["dg_next"].to(DEV))
    dc = torch.full((B, H), float("nan"), device=DEV) if a["dc_in"] is None else a["dc_in"].to(DEV).clone()
    stash = a["stash"].to(DEV).clone()
    rest = (_dev(a["dh_out"]), stash, a["c"].to(DEV), _dev(a["c_prev"]), dc, a["dc_in"] is None)
    if not in_place:
        dg = ops.lstm_step_bwd(dg_next, wt, *rest)
        assert torch.equal(stash.cpu(), a["stash"])              # the inputs are left alone
    else:                                                        # as seq_bwd issues it: dG over the activated gates
        dh_out, _, c, c_prev, _, dc_is_zero = rest
        rc = lib.s2vt_lstm_step_bwd(B, H, _ptr(dg_next), _ptr(wt), _ptr(dh_out), _ptr(stash), _ptr(c), _ptr(c_prev), _ptr(dc),
                                    int(dc_is_zero), _ptr(stash), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0, lib.s2vt_last_error()
        dg = stash
    return dg.cpu(), dc.cpu()


def _check_bwd(got, B, H, form, what):
    dg_ref, dc_ref = _ref_bwd(B, H, form)
    e_dg, e_dc = _err(got[0], dg_ref), _err(got[1], dc_ref)
    print(what, (B, H), form, "dG %.3g dc %.3g (bound %.3g)" % (e_dg, e_dc, R.TOL_DG))
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all()), what
    assert e_dg < R.TOL_DG and e_dc < R.TOL_DG, (what, e_dg, e_dc)


# ------------------------------------------------------------------------------------------------------ a: backward step, shapes
@pytest.mark.parametrize("B,H", R.GRID_SHAPES + R.WIDE_SHAPES + R.NARROW_SHAPES)
def test_bwd_step_shapes(lib, B, H):
    """Every input present.  (250, 480): 30 x 8 = 240 tiles of 32 rows, the last row block 26 rows; (256, 472): the last column
    block 8 units; (250, 472): both; (224, 472): 30 x 7 = 210, the 16-row tile.  The count is asserted here so that a changed
    threshold in lstm_step_bwd2 fails this test instead of moving what it covers."""
    if (B, H) in R.WIDE_SHAPES:
        assert R.wide_tiles(B, H) >= 240
    if (B, H) in R.NARROW_SHAPES:
        assert R.wide_tiles(B, H) < 240
    _check_bwd(_run_bwd(lib, B, H, "all"), B, H, "all", "a")


# ---------------------------------------------------------------------------------------------- b: backward step, argument forms
@pytest.mark.parametrize("form", R.FORMS + ["in_place"])
@pytest.mark.parametrize("B,H", R.FORM_SHAPES)
def test_bwd_step_argument_forms(lib, B, H, form):
    if form == "in_place":
        got = _run_bwd(lib, B, H, "all", in_place=True)
        _check_bwd(got, B, H, "all", "b in place")
        out = _run_bwd(lib, B, H, "all")
        assert torch.equal(got[0], out[0]) and torch.equal(got[1], out[1])
        return
    got = _run_bwd(lib, B, H, form)
    _check_bwd(got, B, H, form, "b")               # (last_step: finite although dc came in as NaN - it was not read)
    dg, dc = got
    if form == "step0":
        assert float(dg[:, H:2 * H].abs().max()) == 0.0
        assert float(dg[:, :H].abs().max()) > 0.01
    if form == "nothing_flows":
        assert float(dg.abs().max()) == 0.0 and float(dc.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ c: backward step, scalar instantiation
@pytest.mark.parametrize("off_dg,off_wt", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("B,H", [(17, 36), (250, 480)])
def test_bwd_step_scalar_instantiation(lib, B, H, off_dg, off_wt):
    """lstm_step_bwd2 tests dg_next and w_hh_t for 16-byte alignment and launches <1, 1, false> when either fails ((250, 480)
    would take the 32-row tile otherwise); the outputs stay aligned"""
    got = _run_bwd(lib, B, H, "all", off_dg=off_dg, off_wt=off_wt)
    _check_bwd(got, B, H, "all", "c dg_next+4 %d w_hh_t+4 %d" % (off_dg, off_wt))
    aligned = _run_bwd(lib, B, H, "all")
    e = max(_err(got[0], aligned[0].double()), _err(got[1], aligned[1].double()))
    print("c", (B, H), "to the aligned launch %.3g (bound %.3g)" % (e, 2 * R.TOL_DG))
    assert e < 2 * R.TOL_DG


# ------------------------------------------------------------------------------------------------------------- d: forward step
@pytest.mark.parametrize("B,H,off", [(17, 36, False), (33, 30, False), (5, 1000, False), (17, 36, True)])
def test_fwd_step_without_gx_from_a_state(lib, B, H, off):
    """bias + h_prev + c_prev, what a layer's steps past n_gx run; off: h_prev and w_hh 4 bytes past a 16-byte boundary (VEC = false;
    H = 30 is on it too, H % 4 != 0)"""
    from s2vt_video_caption_amd import ops
    d = R.fwd_inputs(B, H)
    h_ref, c_ref, st_ref = R.cell_fwd(d["bias"], d["w_hh"], d["h_prev"], d["c_prev"])
    put = _off4 if off else _dev
    h, c, st = ops.lstm_step_fwd(None, d["bias"].to(DEV), put(d["w_hh"]), put(d["h_prev"]), d["c_prev"].to(DEV), want_stash=True)
    e = (_err(h, h_ref), _err(c, c_ref), _err(st, st_ref))
    print("d", (B, H), "offset" if off else "", "h %.3g (%.3g) c %.3g (%.3g) gates %.3g (%.3g)" % (e[0], R.TOL_H, e[1], R.TOL_C, e[2], R.TOL_H))
    assert e[0] < R.TOL_H and e[1] < R.TOL_C and e[2] < R.TOL_H


# --------------------------------------------------------------------------------------------------------------- e: layer loops
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=_ids)
def test_layer_loops(lib, case):
    """(T, B, H, n_gx, dh_first): one step with and without gx; gx for every step; none, with the gradient entering at the last step
    only; ragged 32-row blocks with H % 4 != 0; H = 512; and no gradient at all (dh_first None): dG exactly 0"""
    from s2vt_video_caption_amd import ops
    T, B, H, n_gx, dh_first = case
    d = R.layer_inputs(*case)
    ref = R.layer_ref(*case)
    w = d["w_hh"].to(DEV)
    h_all, c_all, stash = ops.lstm_seq_fwd(T, B, _dev(d["gx"]), n_gx, d["bias"].to(DEV), w, want_stash=True)
    e_f = (_err(h_all, ref["h_all"]), _err(c_all, ref["c_all"]), _err(stash, ref["stash"]))
    dg = ops.lstm_seq_bwd(T, B, w, _dev(d["dh_out"]), dh_first or 0, c_all, stash).cpu()
    e_dg = _err(dg, ref["dg"])
    e_dw = (R.dw_from_dg(T, B, dg, ref["h_all"]) - ref["dw"]).abs().max().item()
    print("e", case, "h %.3g (%.3g) c %.3g (%.3g) gates %.3g (%.3g) dG %.3g (%.3g) dW %.3g (%.3g)"
          % (e_f[0], R.TOL_H, e_f[1], R.TOL_C, e_f[2], R.TOL_H, e_dg, R.TOL_DG, e_dw, R.TOL_DW))
    assert e_f[0] < R.TOL_H and e_f[1] < R.TOL_C and e_f[2] < R.TOL_H
    assert bool(torch.isfinite(dg).all())
    assert e_dg < R.TOL_DG and e_dw < R.TOL_DW
    if dh_first is None:
        assert float(dg.abs().max()) == 0.0


# ----------------------------------------------------------------------------------- f: more than 65535 rows through the driver
@functools.lru_cache(maxsize=None)
def _device_step(shape, grouped):
    """forward + MaskCriterion + backward on loss * 4096 in gemm mode 0, on the host: (logits [B*K, L-1, V], loss, {name: grad},
    dfeats summed over each clip's K rows).  grouped False: mode='train' on the clips repeated K times."""
    import S2VTModel
    import utils
    from s2vt_video_caption_amd import capi
    B, K, L, Fd, H, E, V = shape
    sd, f0, caps, mask = R.driver_data(shape)
    lib = capi.load()
    prev = lib.s2vt_set_gemm_mode(0)
    try:
        m = S2VTModel.S2VT(V, Fd, L, dim_hid=H, dim_embed=E)
        m.load_state_dict(sd)
        m.to(DEV)
        c = caps.to(DEV)
        if grouped:
            f = f0.to(DEV).requires_grad_()
            logits = m(f, targets=c[:, :, :-1], mode="train")
            assert tuple(logits.shape) == (B, K, L - 1, V)
            logits = logits.flatten(0, 1)
        else:
            f = f0.repeat_interleave(K, 0).to(DEV).requires_grad_()
            logits = m(f, targets=c.view(B * K, L)[:, :-1], mode="train")
        loss = utils.MaskCriterion()(logits, c.view(B * K, L), mask.to(DEV).view(B * K, L))
        (loss * R.LOSS_SCALE).backward()
        torch.cuda.synchronize()
        capi.check_async_error()
    finally:
        lib.s2vt_set_gemm_mode(prev)
    dfeats = f.grad if grouped else f.grad.view(B, K, L, Fd).sum(1)
    return logits.detach().cpu(), float(loss.detach()), {n: p.grad.cpu() for n, p in m.named_parameters()}, dfeats.cpu()


def _assert_driver_close(got, ref, what):
    worst = 0.0
    for name, e, bound in R.driver_errors(got, ref):
        print("f", what, name, "%.3g (bound %.3g)" % (e, bound))
        worst = max(worst, e / bound)
        if name in ("logits", "loss"):
            assert e < bound, (what, name, e, bound)
        else:
            assert e <= bound, (what, name, e, bound)
    print("f", what, "worst error / bound %.3g" % worst)


def test_plain_train_step_over_65535_rows(lib):
    """B = 9000, L = 9: (L-1) * B = 72000 rows, 6465 of them in the second gather launch of the backward"""
    B, K, L = R.DRIVER_PLAIN[:3]
    assert (L - 1) * B * K == 72000 and 72000 - 65535 == 6465
    _assert_driver_close(_device_step(R.DRIVER_PLAIN, False), R.driver_ref(R.DRIVER_PLAIN), "plain against the fp64 oracle")


def test_grouped_train_step_over_65535_rows(lib):
    """B = 1800 clips x K = 5 captions: the same 9000 rows per decode step on one encode per clip"""
    B, K, L = R.DRIVER_GROUP[:3]
    assert (L - 1) * B * K == 72000
    _assert_driver_close(_device_step(R.DRIVER_GROUP, True), R.driver_ref(R.DRIVER_GROUP), "grouped against the fp64 oracle")


def test_grouped_equals_plain_on_repeated_clips_over_65535_rows(lib):
    _assert_driver_close(_device_step(R.DRIVER_GROUP, True), _device_step(R.DRIVER_GROUP, False), "grouped against plain on repeated clips")
