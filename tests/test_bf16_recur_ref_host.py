"""CPU: the restatements of tests/bf16_recur_ref.py, which tests/test_gpu_bf16_recurrence_edges.py holds the bf16 (config 3) recurrence
kernels to, are right, and their bounds have room and sight - for every case of the lists both files iterate.

  right   with the operand rounding switched off, the chains equal lstm_step_ref.layer_fwd / layer_bwd to 1e-12
  room    the same restatement evaluated in fp32 (products of bf16-rounded operands, fp32 sums: the device's arithmetic in another
          summation order) lands within HALF of each bound when it is teacher-forced like a device result
  sight   a structural mistake planted in that fp32 evaluation - the last row block of an output zeroed, the last column block zeroed,
          the last k chunk left out of the contraction, a stale cell state (forward: c_{t-2} for c_{t-1}; backward: c_t for c_{t-1}),
          dc dropped, dh_out shifted by one step - moves some output by at least 10 bounds

Measured here (fp32 emulation, worst over the case lists):
  forward   worst |error| of h, c, gates = 1.74e-7 against the bound 2e-5 absolute (T = 5, B = 64, H = 1024)
  backward  worst error = 1.69e-7 * max|ref dG| = 0.034 bounds (T = 3, B = 33, H = 130, dh_first = 0), against
            BWD_REL = lstm_step_ref.TOL_DG = 5e-6; at H = 1024: 1.35e-7 * max|ref|
  sight     the least visible mistake (the last k chunk left out, 2 of 130 columns) still moves an output by 4094 bounds
The backward emulation stays under half of TOL_DG * max|ref| + 1e-9 in every case, so that bound is kept as it is: 5e-6 * max|ref| + 1e-9,
under the ceiling of 2e-5 * max|ref| and 400 times under the 2e-3 * max|ref| the free-running comparison of test_gpu_kernels.py needs.
What the margin covers on the device: another fp32 summation order over the k-split waves and the ~2e-7 of the persistent kernels'
hardware exp / reciprocal activations.

A backward case without any gradient (dh_out None, or dh_first == T) has dG = 0 throughout: it has room (the emulation is exactly zero)
and no arithmetic to mutate; the cases with T == 1 have no contraction, no dc and no c_{t-1}, so only the mistakes that exist there
apply.  `applies` states this per mistake; every mistake applies to at least every case with T >= 2 and a gradient."""
import ctypes
import os
import re

import pytest
import torch

import bf16_recur_ref as R
import lstm_step_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32


def test_bounds_are_the_ones_the_issue_allows():
    assert R.TOL_FWD == 2e-5
    assert R.BWD_REL == sref.TOL_DG and R.BWD_REL <= R.BWD_REL_CEILING == 2e-5 and R.BWD_ABS == 1e-9
    assert R.bwd_bound(0.25) == R.BWD_REL * 0.25 + 1e-9


def test_case_lists_hold_what_the_gpu_test_must_cover():
    bs = {c[1] for c in R.STEP_FWD_CASES if c[2] == 37}
    hs = {c[2] for c in R.STEP_FWD_CASES if c[1] == 33}
    assert bs >= {1, 31, 32, 33, 64, 65} and hs >= {3, 15, 16, 17, 64, 130} and any(c[1:3] == (5, 1000) for c in R.STEP_FWD_CASES)
    assert {(c[3] == 0, 0 < c[3] < c[0], c[3] == c[0]) for c in R.STEP_FWD_CASES} == {(True, False, False), (False, True, False), (False, False, True)}
    assert {c[1] for c in R.STEP_BWD_CASES if c[2] == 37} >= {1, 32, 33, 65}
    assert {c[2] for c in R.STEP_BWD_CASES if c[1] == 33} >= {3, 16, 31, 32, 33, 130}
    forms = {(c[3] is None, c[3] == 0, c[3] is not None and 0 < c[3] < c[0], c[3] == c[0], c[0] == 1) for c in R.STEP_BWD_CASES}
    assert len(forms) >= 5 and all(any(f[i] for f in forms) for i in range(5))
    assert R.PERSIST_FWD_CASES[:6] == [(5, 32, 8, 5, 2), (4, 32, 37, 1, 2), (5, 64, 70, 3, 2), (3, 32, 999, 1, 0), (5, 64, 1024, 2, 0), (4, 32, 5, 4, 3)]
    assert R.PERSIST_BWD_CASES[:5] == [(5, 32, 8, 0, 2), (4, 32, 72, 1, 2), (4, 64, 40, 4, 0), (3, 32, 1000, 1, 0), (5, 64, 1024, 2, 0)]
    assert R.BPTT_UNITS == [0, 16, 32] and R.REFUSE_FWD == [(33, 37), (32, 1032)] and R.REFUSE_BWD == [(32, 36), (32, 1032)]
    assert all(c[0] <= 6 for c in R.FWD_CASES_ALL + R.BWD_CASES_ALL)
    assert {R.pad64(H) for H in (3, 16)} == {64} and {R.pad64(4 * H) for H in (3, 16)} == {64}       # Kp = 64: one k chunk


def test_bf16r_rounds_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0], dtype=F32)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 0.0, 0.0], dtype=F64)
    got = R.bf16r(x)
    assert got.dtype == F64 and torch.equal(got[:4], want[:4]) and got[5] == 0
    assert abs(got[4].item() + 0.3) <= 2.0 ** -10          # half an ulp of [0.25, 0.5): 8 significant bits
    assert torch.equal(R.bf16r(x, rounding=False), x.double())
    # the bit patterns the image checks compare with are the same rounding
    assert torch.equal(R.bf16_bits(x).view(torch.bfloat16).double(), got)


# ------------------------------------------------------------------------------------------------------------------------ right
@pytest.mark.parametrize("T,B,H,n_gx", R.FWD_CASES_ALL)
def test_forward_without_rounding_is_the_fp32_kernels_reference(T, B, H, n_gx):
    gx, bias, w = R.fwd_inputs(T, B, H)
    got = R.fwd_chain(gx, n_gx, bias, w, T, B, H, dtype=F64, rounding=False)
    ref = sref.layer_fwd(T, B, gx, n_gx, bias, w)
    for a, b in zip(got, ref):
        assert a.dtype == F64 and (a - b).abs().max().item() <= 1e-12


@pytest.mark.parametrize("T,B,H,dh_first", R.BWD_CASES_ALL)
def test_backward_without_rounding_is_the_fp32_kernels_reference(T, B, H, dh_first):
    w, gates, c_all, dh = R.bwd_inputs(T, B, H, dh_first)
    got = R.bwd_chain(w, dh, dh_first, c_all, gates, T, B, H, dtype=F64, rounding=False)
    ref = sref.layer_bwd(T, B, w, dh, dh_first or 0, c_all.double(), gates.double())
    assert got.dtype == F64 and (got - ref).abs().max().item() <= 1e-12
    assert (ref.abs().max().item() > 0) == R.has_gradient(T, dh_first)


def test_teacher_forcing_an_exact_chain_finds_nothing_and_a_nan_is_an_error():
    T, B, H, n_gx = 3, 5, 19, 1
    gx, bias, w = R.fwd_inputs(T, B, H)
    h, c, s = R.fwd_chain(gx, n_gx, bias, w, T, B, H, dtype=F64, rounding=True)
    assert R.fwd_teacher_forced(h, c, s, gx, n_gx, bias, w, T, B, H)["worst"] < 1e-7          # (only the fp32 storage of the outputs)
    h = h.clone()
    h[7, 3] = float("nan")
    assert R.fwd_teacher_forced(h, c, s, gx, n_gx, bias, w, T, B, H)["worst"] == float("inf")
    wb, gates, c_all, dh = R.bwd_inputs(T, B, H, 1)
    dg = R.bwd_chain(wb, dh, 1, c_all, gates, T, B, H, dtype=F64, rounding=True)
    r = R.bwd_teacher_forced(dg, wb, dh, 1, c_all, gates, T, B, H)
    assert r["worst"] < 1e-7 * r["ref_max"] and r["ref_max"] > 0.01
    dg = dg.clone()
    dg[2, 5] = float("nan")
    assert R.bwd_teacher_forced(dg, wb, dh, 1, c_all, gates, T, B, H)["worst"] == float("inf")


# ------------------------------------------------------------------------------------------------------------------ room, sight
def applies(mutation, T, dh_first=0):
    """does the mistake exist in a case: the contraction, dc and (forward) c_{t-1} start with the second step; a backward case
    without any gradient has nothing to get wrong"""
    if not R.has_gradient(T, dh_first):
        return False
    return T >= 2 or mutation in ("zero_last_rows", "zero_last_cols", "c_for_c_prev", "shift_dh_out")


@pytest.mark.parametrize("T,B,H,n_gx", R.FWD_CASES_ALL)
def test_forward_bound_has_room_and_sight(T, B, H, n_gx):
    gx, bias, w = R.fwd_inputs(T, B, H)
    emu = R.fwd_chain(gx, n_gx, bias, w, T, B, H, dtype=F32)
    e = R.fwd_teacher_forced(*emu, gx, n_gx, bias, w, T, B, H)
    print("fwd T=%d B=%d H=%d n_gx=%d: fp32 emulation %.2e / bound %.0e" % (T, B, H, n_gx, e["worst"], R.TOL_FWD))
    assert e["worst"] <= 0.5 * R.TOL_FWD
    for m in R.MUTATIONS_FWD:
        assert applies(m, T)
        bad = R.fwd_chain(gx, n_gx, bias, w, T, B, H, dtype=F32, mutate=m)
        moved = R.fwd_teacher_forced(*bad, gx, n_gx, bias, w, T, B, H)["worst"]
        print("    %-15s moves an output by %.2e = %.0f bounds" % (m, moved, moved / R.TOL_FWD))
        assert moved >= 10 * R.TOL_FWD, (m, moved)


@pytest.mark.parametrize("T,B,H,dh_first", R.BWD_CASES_ALL)
def test_backward_bound_has_room_and_sight(T, B, H, dh_first):
    w, gates, c_all, dh = R.bwd_inputs(T, B, H, dh_first)
    emu = R.bwd_chain(w, dh, dh_first, c_all, gates, T, B, H, dtype=F32)
    e = R.bwd_teacher_forced(emu, w, dh, dh_first, c_all, gates, T, B, H)
    print("bwd T=%d B=%d H=%d dh_first=%s: fp32 emulation %.2e / bound %.2e (%.2e of max|ref| = %.3f)"
          % (T, B, H, dh_first, e["worst"], e["bound"], e["worst"] / max(e["ref_max"], 1e-30), e["ref_max"]))
    assert e["worst"] <= 0.5 * e["bound"]
    assert e["bound"] <= R.BWD_REL_CEILING * e["ref_max"] + R.BWD_ABS
    if not R.has_gradient(T, dh_first):
        assert e["ref_max"] == 0 and e["worst"] == 0
    for m in R.MUTATIONS_BWD:
        if not applies(m, T, dh_first):
            continue
        bad = R.bwd_chain(w, dh, dh_first, c_all, gates, T, B, H, dtype=F32, mutate=m)
        r = R.bwd_teacher_forced(bad, w, dh, dh_first, c_all, gates, T, B, H)
        print("    %-15s moves an output by %.2e = %.0f bounds" % (m, r["worst"], r["worst"] / r["bound"]))
        assert r["worst"] >= 10 * r["bound"], (m, r)


def test_every_mistake_applies_wherever_there_are_two_steps_and_a_gradient():
    for T, B, H, f in R.BWD_CASES_ALL:
        for m in R.MUTATIONS_BWD:
            assert applies(m, T, f) or T < 2 or not R.has_gradient(T, f)
    assert sum(applies("drop_dc", c[0], c[3]) for c in R.BWD_CASES_ALL) >= len(R.BWD_CASES_ALL) - 6


# ------------------------------------------------------------------------------------------------- the layout entry point (host)
def test_layout_entry_point_declared_exported_bound_and_consistent(lib):
    """s2vt_lstm_seq_bf16_layout (test support: where the bf16 images lie inside the workspaces of the four bf16 recurrence entry
    points) is declared, exported and bound with the ABI version unchanged, refuses bad arguments with a message, and what it
    reports fits inside the workspace sizes the library itself reports."""
    from s2vt_video_caption_amd import capi, ops
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    assert re.search(r"\bs2vt_lstm_seq_bf16_layout\(", header) and "s2vt_lstm_seq_bf16_layout" in capi.SIGNATURES
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "s2vt_lstm_seq_bf16_layout") and lib.s2vt_abi_version() == capi.ABI_VERSION == 9
    out = (ctypes.c_int64 * 6)()
    for bad in ((0, 32, 8, 0, out), (3, 0, 8, 1, out), (3, 32, 0, 0, out), (3, 32, 8, 0, None)):
        assert lib.s2vt_lstm_seq_bf16_layout(*bad) == -1 and b"s2vt_lstm_seq_bf16_layout" in lib.s2vt_last_error()
    for T, B, H in [(3, 33, 37), (4, 32, 72), (5, 64, 1024), (3, 5, 1000), (3, 33, 3)]:
        for backward, k, wrows, total in ((False, H, 4 * H, lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H)),
                                          (True, 4 * H, H, lib.s2vt_lstm_seq_bwd_bf16_workspace_bytes(T, B, H))):
            lay = ops.seq_bf16_layout(T, B, H, backward=backward)
            (woff, wld, wk), (roff, rld, rk) = lay["w"], lay["rows"]
            assert wk == rk == R.pad64(k) and wld >= wk and rld >= rk and wld % 8 == 0 and rld % 8 == 0
            assert woff % 16 == 0 and roff % 16 == 0 and 0 < woff and woff + wrows * wld * 2 <= roff and roff + T * B * rld * 2 <= total


def test_persistent_entry_points_refuse_their_shapes_on_the_host(lib):
    """The refusals of tests/test_gpu_bf16_recurrence_edges.py (group e) without a GPU: the shape is refused with rc = -1 and a message
    that names it before the workspace is prepared, so no pointer is followed and no HIP call is made - on a machine without a
    device anything else would come back as a HIP error."""
    T = 2
    dummy = (ctypes.c_char * 256)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    for B, H in R.REFUSE_FWD:
        n = lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H)
        rc = lib.s2vt_lstm_seq_fwd_bf16(T, B, H, p, T, None, p, p, p, p, n, 1, 0, None)
        msg = lib.s2vt_last_error().decode()
        assert rc == -1 and "s2vt_lstm_seq_fwd_bf16:" in msg and "B=%d" % B in msg and "H=%d" % H in msg, (rc, msg)
        rc = lib.s2vt_lstm_seq_fwd_bf16_pair(T, B, H, p, p, T, None, None, p, p, p, p, p, p, p, 2 * n, 0, None)
        msg = lib.s2vt_last_error().decode()
        assert rc == -1 and "s2vt_lstm_seq_fwd_bf16_pair:" in msg and "B=%d" % B in msg and "H=%d" % H in msg, (rc, msg)
    for B, H in R.REFUSE_BWD:
        n = lib.s2vt_lstm_seq_bwd_bf16_workspace_bytes(T, B, H)
        rc = lib.s2vt_lstm_seq_bwd_bf16(T, B, H, p, p, 0, p, p, p, n, 1, 0, None)
        msg = lib.s2vt_last_error().decode()
        assert rc == -1 and "s2vt_lstm_seq_bwd_bf16:" in msg and "B=%d" % B in msg and "H=%d" % H in msg, (rc, msg)
        rc = lib.s2vt_lstm_seq_bwd_bf16_pair(T, B, H, p, p, p, p, 0, p, p, p, p, p, 2 * n, 0, None)
        msg = lib.s2vt_last_error().decode()
        assert rc == -1 and "s2vt_lstm_seq_bwd_bf16_pair:" in msg and "B=%d" % B in msg and "H=%d" % H in msg, (rc, msg)
    assert not any(dummy.raw.strip(b"\0"))
