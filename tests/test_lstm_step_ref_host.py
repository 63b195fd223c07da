"""Host: the fp64 references of tests/lstm_step_ref.py against torch's fp64 autograd, and the two things a bound needs besides a
right reference - room (plain fp32 arithmetic on the host lands within a quarter of it) and sight (the error a wrong kernel would
make is far above it: a k column of dg_next left out of the contraction moves dG by more than 20 bounds, a dropped optional input
by more than 1000).  Every step case of tests/test_gpu_lstm_step_edges.py is checked here, none needs a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_step_ref as R  # noqa: E402

F64 = torch.float64
STEP_CASES = [(B, H, "all") for B, H in R.GRID_SHAPES + R.WIDE_SHAPES + R.NARROW_SHAPES] + \
             [(B, H, f) for B, H in R.FORM_SHAPES for f in R.FORMS]
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def _d(t):
    return None if t is None else t.double()


def _autograd_step(a):
    """fp64 autograd of the cell from the gate pre-activations: (dL/d pre [B, 4H], dL/d c_prev [B, H]) for
    L = sum(h . dh) + sum(c . dc_in), dh = dh_out + dg_next . W_hh; the activated gates and c in fp64 too"""
    B, H4 = a["stash"].shape
    H = H4 // 4
    zero = torch.zeros(B, H, dtype=F64)
    pre = _d(a["gx"]).requires_grad_()
    cp = (zero.clone() if a["c_prev"] is None else _d(a["c_prev"])).requires_grad_()
    i, f, g, o = pre.chunk(4, 1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(g)
    h = torch.sigmoid(o) * torch.tanh(c)
    dh = zero.clone()
    if a["dg_next"] is not None:
        dh = dh + _d(a["dg_next"]) @ _d(a["w_hh"])
    if a["dh_out"] is not None:
        dh = dh + _d(a["dh_out"])
    loss = (h * dh).sum()
    if a["dc_in"] is not None:
        loss = loss + (c * _d(a["dc_in"])).sum()
    loss.backward()
    return pre.grad, cp.grad


def _args(B, H, form):
    a = dict(R.form_args(B, H, form))
    a["gx"] = R.step_inputs(B, H, zero_state=(form == "step0"))["gx"]
    return a


def _bwd(a, dtype=F64, **over):
    k = dict(a, **over)
    return R.step_bwd(k["dg_next"], k["w_hh"], k["dh_out"], k["stash"], k["c"], k["c_prev"], k["dc_in"], dtype)


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_step_reference_is_fp64_autograd(case):
    B, H, form = case
    a = _args(B, H, form)
    stash64, c64, _ = R.activate(_d(a["gx"]), _d(a["c_prev"]))
    dg, dcp = _bwd(a, stash=stash64, c=c64)
    dg_ref, dcp_ref = _autograd_step(a)
    assert (dg - dg_ref).abs().max().item() < 1e-12
    assert (dcp - dcp_ref).abs().max().item() < 1e-12         # (at step 0 too: dL/dc_prev at c_prev = 0 is still dc . f)
    if a["c_prev"] is None:
        assert float(dg[:, H:2 * H].abs().max()) == 0.0


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_fp32_arithmetic_is_within_a_quarter_of_the_step_bound(case):
    B, H, form = case
    a = _args(B, H, form)
    dg, dcp = _bwd(a)
    dg32, dcp32 = _bwd(a, torch.float32)
    e_dg, e_dc = (dg32.double() - dg).abs().max().item(), (dcp32.double() - dcp).abs().max().item()
    print(case, "fp32 dG", e_dg, "dc", e_dc)
    assert e_dg <= R.TOL_DG / 4 and e_dc <= R.TOL_DG / 4


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_step_inputs_can_see_an_error(case):
    """what a kernel that skips part of its work would be off by, in max-norm of the reference dG"""
    B, H, form = case
    a = _args(B, H, form)
    dg, _ = _bwd(a)
    if form == "nothing_flows":
        assert float(dg.abs().max()) == 0.0
        return
    moved = lambda **over: (_bwd(a, **over)[0] - dg).abs().max().item()  # noqa: E731
    if a["dg_next"] is not None:
        for cols in ([0], [4 * H - 1], [4 * H - 4, 4 * H - 3, 4 * H - 2, 4 * H - 1]):
            cut = a["dg_next"].clone()
            cut[:, cols] = 0
            m = moved(dg_next=cut)
            print(case, "k columns", cols, m)
            assert m > 20 * R.TOL_DG, (cols, m)
    for name in ("dh_out", "dc_in"):
        if a[name] is not None:
            m = moved(**{name: None})
            print(case, name, m)
            assert m > 1000 * R.TOL_DG, (name, m)
    if a["c_prev"] is not None:
        m = moved(c_prev=None)
        print(case, "c_prev", m)
        assert m > 1000 * R.TOL_DG, m


def test_the_tile_choice_of_the_edge_shapes():
    assert all(R.wide_tiles(B, H) >= 240 for B, H in R.WIDE_SHAPES)
    assert all(R.wide_tiles(B, H) < 240 for B, H in R.NARROW_SHAPES)
    assert R.wide_tiles(250, 480) == 240 and 250 % 32 == 26 and 472 % 16 == 8


@pytest.mark.parametrize("B,H", R.FWD_SHAPES)
def test_forward_cell_is_the_oracle_cell_and_fp32_has_room(B, H):
    """room here: half the bound.  The kernel sums the K = H products in another order than the host's fp32 matmul, so its error is
    another draw of the same size; a bound under twice one such draw could not hold both.  (The gate pre-activations of H = 1000 carry
    the rounding of a 1000-term fp32 sum: the host's lands at a quarter of the 2e-6 on the activated gates.)"""
    from oracle import s2vt_oracle as orc
    d = R.fwd_inputs(B, H)
    h, c, st = R.cell_fwd(d["bias"], d["w_hh"], d["h_prev"], d["c_prev"])
    h_ref, c_ref = orc.lstm_cell(None, _d(d["h_prev"]), _d(d["c_prev"]), None, _d(d["w_hh"]), _d(d["bias"]), torch.zeros(4 * H, dtype=F64))
    assert (h - h_ref).abs().max().item() < 1e-12 and (c - c_ref).abs().max().item() < 1e-12
    pre = _d(d["bias"]) + _d(d["h_prev"]) @ _d(d["w_hh"]).t()
    assert torch.equal(st[:, :H], torch.sigmoid(pre[:, :H])) and torch.equal(st[:, 2 * H:3 * H], torch.tanh(pre[:, 2 * H:3 * H]))
    h32, c32, st32 = R.cell_fwd(d["bias"], d["w_hh"], d["h_prev"], d["c_prev"], torch.float32)
    e = [(h32.double() - h).abs().max().item(), (c32.double() - c).abs().max().item(), (st32.double() - st).abs().max().item()]
    print((B, H), "fp32 h, c, stash", e)
    assert e[0] <= R.TOL_H / 2 and e[1] <= R.TOL_C / 2 and e[2] <= R.TOL_H / 2


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=_ids)
def test_layer_reference_is_fp64_autograd(case):
    """h_all, dG of every step (the steps past n_gx through a per-step copy of the bias) and dW_hh"""
    T, B, H, n_gx, dh_first = case
    d = R.layer_inputs(*case)
    ref = R.layer_ref(*case)
    w = _d(d["w_hh"]).requires_grad_()
    pres = [(_d(d["gx"][t * B:(t + 1) * B]) if t < n_gx else _d(d["bias"]).expand(B, -1).clone()).requires_grad_() for t in range(T)]
    h = c = torch.zeros(B, H, dtype=F64)
    hs = []
    for t in range(T):
        i, f, g, o = (pres[t] + h @ w.t()).chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    hs = torch.cat(hs)
    assert (ref["h_all"] - hs.detach()).abs().max().item() < 1e-12
    if dh_first is None:
        assert float(ref["dg"].abs().max()) == 0.0 and float(ref["dw"].abs().max()) == 0.0
        return
    (hs[dh_first * B:] * _d(d["dh_out"])).sum().backward()
    assert (ref["dg"] - torch.cat([p.grad for p in pres])).abs().max().item() < 1e-12
    assert (ref["dw"] - w.grad).abs().max().item() < 1e-11
    assert float(ref["dg"].abs().max()) > 0.01


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=_ids)
def test_fp32_layer_arithmetic_is_within_half_of_the_layer_bounds(case):
    """as for the forward cell: half the bound, for every compared quantity of the layer"""
    T, B, H, n_gx, dh_first = case
    d = R.layer_inputs(*case)
    ref = R.layer_ref(*case)
    h32, c32, st32 = R.layer_fwd(T, B, d["gx"], n_gx, d["bias"], d["w_hh"], torch.float32)
    dg32 = R.layer_bwd(T, B, d["w_hh"], d["dh_out"], dh_first or 0, c32, st32, torch.float32)
    dw = R.dw_from_dg(T, B, dg32, ref["h_all"])
    e = [(h32.double() - ref["h_all"]).abs().max().item(), (c32.double() - ref["c_all"]).abs().max().item(),
         (st32.double() - ref["stash"]).abs().max().item(), (dg32.double() - ref["dg"]).abs().max().item(),
         (dw - ref["dw"]).abs().max().item()]
    print(case, "fp32 h, c, stash, dG, dW", e)
    assert e[0] <= R.TOL_H / 2 and e[1] <= R.TOL_C / 2 and e[2] <= R.TOL_H / 2 and e[3] <= R.TOL_DG / 2 and e[4] <= R.TOL_DW / 2


def test_fp32_oracle_at_9000_clips_is_50x_inside_the_driver_bounds():
    """(L-1) * B = 72000 rows, backward on loss * 4096: the fp32 oracle against the fp64 one, every compared quantity"""
    assert (R.DRIVER_PLAIN[2] - 1) * R.DRIVER_PLAIN[0] == 72000 > 65535
    ref = R.driver_ref(R.DRIVER_PLAIN)
    # torch's fp32 sums on the host depend on the thread count (the mean over 72000 rows: 1.6e-7 off on 8 threads, 6.4e-7 on one) and
    # the embedding gradient's scatter-add on the arrival order of its threads (1e-4 .. 2e-4 from run to run): both are pinned here
    threads, det = torch.get_num_threads(), torch.are_deterministic_algorithms_enabled()
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    try:
        got = R.driver_oracle(R.DRIVER_PLAIN, torch.float32)
    finally:
        torch.use_deterministic_algorithms(det)
        torch.set_num_threads(threads)
    for name, e, bound in R.driver_errors(got, ref):
        print(name, e, bound)
        assert 50 * e <= bound, (name, e, bound)
    # without the factor zeros would pass for dfeats (all of it under the 1e-6 floor of its bound); with it they are far outside
    dmax = ref[3].abs().max().item()
    assert dmax / R.LOSS_SCALE < 1e-6 and dmax > 100 * (1e-6 + 1e-4 * dmax)
