"""GPU: the model variants that run on per-op autograd glue - S2VT(rnn_type='gru') (gru_functional.py), the stacked model's
projections and attention_baseline.Att_Baseline (att_functional.py) - against the fp64 restatements of tests/model_refs.py
(validated on the CPU by tests/test_model_refs_host.py against what the reference recorded).  From the ops upward:
att_functional.affine as an op in the plane mode and on s2vt_gemm_f32, s2vt_gru_seq_fwd / _bwd teacher-forced step by step, the
autograd layers gru_layer / lstm_layer against torch's fp64 nn.GRU / nn.LSTM, then the whole GRU model and the whole Att_Baseline
in GEMM modes 3 and 0.  Every tensor is compared whole, element by element; a repeated call must return the same bits."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@contextlib.contextmanager
def _gemm_mode(lib, mode):
    prev = lib.s2vt_set_gemm_mode(mode)
    try:
        yield
    finally:
        lib.s2vt_set_gemm_mode(prev)


def _err(got, ref):
    """(max |got - ref|, max |ref|, relative Frobenius error) of a whole tensor against its fp64 reference"""
    got, ref = R.d64(got), R.d64(ref)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    d = got - ref
    return d.abs().max().item(), ref.abs().max().item(), (d.norm() / ref.norm().clamp_min(1e-300)).item()


def _close(got, ref, what, rel, atol=0.0):
    err, top, _ = _err(got, ref)
    assert err <= rel * max(top, 1e-30) + atol, (what, err, top, err / max(top, 1e-30))
    return err / max(top, 1e-30)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _uni(g, *shape, k=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * k


# ------------------------------------------------------------------------------------------------- a. affine as an op
# (M, K, N); (17, 40, 40): a square W, where a dx product that read W in the wrong orientation would still have matching shapes
AFFINE_CASES = [(1, 1, 1), (5, 26, 97), (63, 64, 3), (64, 65, 130), (65, 100, 1000), (130, 1000, 37), (384, 48, 128), (17, 40, 40)]
# (x needs grad, w needs grad, with bias)
AFFINE_FLAGS = [(True, True, True), (False, True, True), (True, False, True), (True, True, False)]


def _affine_run(x, w, b, dy, gx=True, gw=True):
    """affine forward and backward on the device from CPU operands -> (y, dx, dw, db); a gradient not asked for is None"""
    from s2vt_video_caption_amd import att_functional as A
    xd = x.to(DEV).requires_grad_(gx)
    wd = w.to(DEV).requires_grad_(gw)
    bd = b.to(DEV).requires_grad_() if b is not None else None
    y = A.affine(xd, wd, bd)
    y.backward(dy.to(DEV))
    return y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad


def _affine_ref(x, w, b, dy):
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    y = R.affine64(xr, wr, br)
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad, None if br is None else br.grad


def _same_bits(a, b, what):
    for name, u, v in zip(("y", "dx", "dw", "db"), a, b):
        assert (u is None) == (v is None), (what, name)
        if u is not None:
            assert torch.equal(u, v), (what, name)


@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("M,K,N", AFFINE_CASES)
def test_affine_op_against_fp64(lib, mode, M, K, N):
    """y = x W^T + b, dx, dW, db of att_functional.affine against fp64 and its autograd under a random upstream gradient, N(0,1)
    operands: M off the 64-row plane blocks (the dW product relies on zero padding rows), K and N off 64 and off 4, with and
    without bias, with x or W needing no gradient.  Mode 3 (plane GEMMs): 4e-6 max|ref| + 1e-6, the bound of
    test_split_precision_gemm_blocked_planes; mode 0 (s2vt_gemm_f32): 8e-6 sqrt(k) + 1e-6 with k the contraction length of each
    product, the bound of test_gemm_all_layouts."""
    g = torch.Generator().manual_seed(M * 7919 + K * 31 + N)
    x, w, b, dy = _randn(g, M, K), _randn(g, N, K), _randn(g, N), _randn(g, M, N)
    klen = dict(y=K, dx=N, dw=M, db=M)
    with _gemm_mode(lib, mode):
        for gx, gw, bias in AFFINE_FLAGS:
            bb = b if bias else None
            got = _affine_run(x, w, bb, dy, gx, gw)
            ref = _affine_ref(x, w, bb, dy)
            assert (got[1] is None) == (not gx) and (got[2] is None) == (not gw) and (got[3] is None) == (not bias)
            for name, u, v in zip(("y", "dx", "dw", "db"), got, ref):
                if u is None:
                    continue
                err, top, _ = _err(u, v)
                tol = 4e-6 * top + 1e-6 if mode == 3 else 8e-6 * klen[name] ** 0.5 + 1e-6
                assert err <= tol, (name, (gx, gw, bias), err, tol, top)
            _same_bits(got, _affine_run(x, w, bb, dy, gx, gw), "repeat %s" % ((gx, gw, bias),))


@pytest.mark.parametrize("M,K,N", [(5, 26, 97), (65, 100, 1000), (384, 48, 128)])
def test_affine_backward_keeps_the_mode_of_its_forward(lib, M, K, N):
    """A forward in mode 3 whose backward runs after a switch to mode 0 gives the bits of an all-mode-3 run (ctx.planes pins the
    choice; the saved tensors are the plane images); and the other way round."""
    from s2vt_video_caption_amd import att_functional as A
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b, dy = _randn(g, M, K), _randn(g, N, K), _randn(g, N), _randn(g, M, N)
    for first, second in ((3, 0), (0, 3)):
        with _gemm_mode(lib, first):
            want = _affine_run(x, w, b, dy)
            xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
            y = A.affine(xd, wd, bd)
            with _gemm_mode(lib, second):
                y.backward(dy.to(DEV))
        _same_bits(want, (y.detach(), xd.grad, wd.grad, bd.grad), "forward in mode %d, backward in mode %d" % (first, second))


@pytest.mark.parametrize("M,K,N", [(5, 26, 97), (130, 1000, 37)])
def test_affine_mode_1_is_mode_0(lib, M, K, N):
    """att_functional keeps s2vt_gemm_f32 in modes 0 and 1 alike: the same bits."""
    g = torch.Generator().manual_seed(M + K + N + 1)
    x, w, b, dy = _randn(g, M, K), _randn(g, N, K), _randn(g, N), _randn(g, M, N)
    with _gemm_mode(lib, 0):
        want = _affine_run(x, w, b, dy)
    with _gemm_mode(lib, 1):
        got = _affine_run(x, w, b, dy)
    _same_bits(want, got, "mode 1 against mode 0")


@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("M,K,N,E", [(34, 37, 96, 26), (70, 128, 384, 100)])
def test_affine_of_a_column_slice_of_w(lib, mode, M, K, N, E):
    """W given as the column slice w_full[:, E:] (the vid half of word_rnn's input weight, not contiguous): the bits of its
    contiguous copy, and the gradient lands in the slice's columns of w_full alone."""
    from s2vt_video_caption_amd import att_functional as A
    g = torch.Generator().manual_seed(M + K + N + E)
    x, w_full, dy = _randn(g, M, K), _randn(g, N, E + K), _randn(g, M, N)
    with _gemm_mode(lib, mode):
        want = _affine_run(x, w_full[:, E:].contiguous(), None, dy)
        xd, wf = x.to(DEV).requires_grad_(), w_full.to(DEV).requires_grad_()
        sl = wf[:, E:]
        assert not sl.is_contiguous()
        y = A.affine(xd, sl, None)
        y.backward(dy.to(DEV))
    assert torch.equal(y.detach(), want[0]) and torch.equal(xd.grad, want[1])
    assert torch.equal(wf.grad[:, E:], want[2]) and float(wf.grad[:, :E].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------- b. GRU layer ops
# (T, B, H, n_gx): H = 30 the scalar-load kernels, H = 36 two K chunks, B = 65 / 130 five / nine 16-row tiles with a ragged last
# one, n_gx = 0 (b_ih alone from the first step), inside (0, T), and T
GRU_SEQ_CASES = [(1, 5, 30, 1), (1, 5, 32, 0), (4, 17, 36, 2), (6, 16, 30, 0), (5, 65, 64, 5), (3, 130, 1000, 1), (4, 33, 512, 4)]


def _gru_seq_inputs(T, B, H, n_gx):
    g = torch.Generator().manual_seed(T * 100000 + B * 1000 + H + n_gx)
    k = H ** -0.5
    return dict(w_hh=_uni(g, 3 * H, H, k=k), b_hh=_uni(g, 3 * H, k=k), b_ih=_uni(g, 3 * H, k=k),
                gx=_randn(g, max(n_gx, 1) * B, 3 * H)[:n_gx * B], g=g)


@pytest.mark.parametrize("T,B,H,n_gx", GRU_SEQ_CASES)
def test_gru_seq_fwd_teacher_forced_against_fp64(lib, T, B, H, n_gx):
    """s2vt_gru_seq_fwd: every step against the fp64 cell on the kernel's own h of the step before (one step of fp32 error per
    comparison, so the one-step bound of test_gpu_gru._close holds: 1e-5 max|ref|), h and each of the stash columns r, z, n,
    ghn, the b_ih-only steps >= n_gx included."""
    from s2vt_video_caption_amd import capi, ops
    from s2vt_video_caption_amd.functional import _ptr, _stream
    c = _gru_seq_inputs(T, B, H, n_gx)
    d = {k: c[k].to(DEV) for k in ("w_hh", "b_hh", "b_ih", "gx")}
    run = lambda: ops.gru_seq_fwd(T, B, d["gx"] if n_gx else None, n_gx, d["b_ih"], d["w_hh"], d["b_hh"], want_stash=True)
    h_all, stash = run()
    assert h_all.shape == (T * B, H) and stash.shape == (T * B, 4 * H)
    W, bh, bi, gx = c["w_hh"].double(), c["b_hh"].double(), c["b_ih"].double(), c["gx"].double()
    hk, sk = R.d64(h_all), R.d64(stash)
    worst = 0.0
    for t in range(T):
        gi = gx[t * B:(t + 1) * B] if t < n_gx else bi.expand(B, -1)
        hp = hk[(t - 1) * B:t * B] if t else torch.zeros(B, H, dtype=F64)
        ref = R.gru_cell64(gi, hp, W, bh)
        worst = max(worst, _close(hk[t * B:(t + 1) * B], ref[0], "h step %d" % t, 1e-5))
        for j, name in enumerate(("r", "z", "n", "ghn")):
            worst = max(worst, _close(sk[t * B:(t + 1) * B, j * H:(j + 1) * H], ref[1 + j], "%s step %d" % (name, t), 1e-5))
    print("gru_seq_fwd T=%d B=%d H=%d n_gx=%d: worst error / max|ref| %.3g" % (T, B, H, n_gx, worst))
    h2, s2 = run()
    assert torch.equal(h2, h_all) and torch.equal(s2, stash)
    h3, none = ops.gru_seq_fwd(T, B, d["gx"] if n_gx else None, n_gx, d["b_ih"], d["w_hh"], d["b_hh"])
    assert none is None and torch.equal(h3, h_all)                      # without a stash: the same states
    # the entry point itself on NaN-filled outputs: every element of h_all and of the stash is written
    hn, sn = torch.full_like(h_all, float("nan")), torch.full_like(stash, float("nan"))
    with torch.cuda.device(DEV):
        capi.check(lib.s2vt_gru_seq_fwd(T, B, H, _ptr(d["gx"] if n_gx else None), n_gx, _ptr(d["b_ih"]), _ptr(d["w_hh"]),
                                        _ptr(d["b_hh"]), _ptr(hn), _ptr(sn), _stream(torch.device(DEV))), "s2vt_gru_seq_fwd")
    assert torch.equal(hn, h_all) and torch.equal(sn, stash)


@pytest.mark.parametrize("T,B,H,n_gx", GRU_SEQ_CASES)
def test_gru_seq_bwd_against_fp64_bptt(lib, T, B, H, n_gx):
    """s2vt_gru_seq_bwd on the kernel's own h_all and stash against the hand-written fp64 BPTT on the same values, with the
    upstream gradient starting at step dh_first in {0, 2, T-1}: dgx and dgh over all T*B rows within 1e-5 max|ref| (the one-step
    bound; the T <= 6 steps of fp32 carry stay inside it: measured at most 1.5e-7 over the cases, at T=3 B=130 H=1000).
    Without an upstream gradient both are exactly zero.  ops.gru_seq_bwd allocates its outputs itself, so they cannot be
    pre-filled through it: every output must be finite, and one call goes to the entry point itself with NaN-filled outputs and
    scratch."""
    from s2vt_video_caption_amd import capi, ops
    from s2vt_video_caption_amd.functional import _ptr, _stream
    c = _gru_seq_inputs(T, B, H, n_gx)
    d = {k: c[k].to(DEV) for k in ("w_hh", "b_hh", "b_ih", "gx")}
    h_all, stash = ops.gru_seq_fwd(T, B, d["gx"] if n_gx else None, n_gx, d["b_ih"], d["w_hh"], d["b_hh"], want_stash=True)
    hk, sk, W = R.d64(h_all), R.d64(stash), c["w_hh"].double()
    h0, s0 = h_all.clone(), stash.clone()
    worst = 0.0
    for dh_first in sorted({min(f, T - 1) for f in (0, 2, T - 1)}):
        dh_out = _randn(c["g"], (T - dh_first) * B, H)
        dgx, dgh = ops.gru_seq_bwd(T, B, d["w_hh"], dh_out.to(DEV), dh_first, h_all, stash)
        rgx, rgh = R.gru_bptt64(W, dh_out.double(), dh_first, hk, sk, T, B)
        worst = max(worst, _close(dgx, rgx, "dgx, dh_first %d" % dh_first, 1e-5))
        worst = max(worst, _close(dgh, rgh, "dgh, dh_first %d" % dh_first, 1e-5))
        a, b = ops.gru_seq_bwd(T, B, d["w_hh"], dh_out.to(DEV), dh_first, h_all, stash)
        assert torch.equal(a, dgx) and torch.equal(b, dgh)
    print("gru_seq_bwd T=%d B=%d H=%d n_gx=%d: worst error / max|ref| %.3g" % (T, B, H, n_gx, worst))
    # the entry point itself on NaN-filled outputs and scratch (the last dh_first of the loop): every element of dgx and dgh is
    # written, and neither the dh scratch nor the W_hh^T scratch is read before it is written
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    xn, gn, dhs, wt, up = nan(T * B, 3 * H), nan(T * B, 3 * H), nan(B, H), nan(H, 3 * H), dh_out.to(DEV)
    with torch.cuda.device(DEV):
        capi.check(lib.s2vt_gru_seq_bwd(T, B, H, _ptr(d["w_hh"]), _ptr(up), dh_first, _ptr(h_all), _ptr(stash), _ptr(wt), _ptr(dhs),
                                        _ptr(xn), _ptr(gn), _stream(torch.device(DEV))), "s2vt_gru_seq_bwd")
    assert torch.equal(xn, dgx) and torch.equal(gn, dgh)
    dgx, dgh = ops.gru_seq_bwd(T, B, d["w_hh"], None, 0, h_all, stash)
    assert dgx.shape == dgh.shape == (T * B, 3 * H)
    assert float(dgx.abs().max()) == 0.0 and float(dgh.abs().max()) == 0.0
    assert torch.equal(h_all, h0) and torch.equal(stash, s0)            # the backward leaves h_all and the stash untouched


# ------------------------------------------------------------------------------------------------ c. autograd layers
def _rnn64_identity(cls, gi, w_hh, b_hh=None):
    """torch's fp64 nn.GRU / nn.LSTM over time-major gate inputs gi [T, B, G]: input weight = identity, input bias = 0"""
    G, H = gi.shape[2], w_hh.shape[1]
    cell = cls(G, H).double()
    zero = torch.zeros(G, dtype=F64)
    out, _ = torch.func.functional_call(cell, {"weight_ih_l0": torch.eye(G, dtype=F64), "weight_hh_l0": w_hh, "bias_ih_l0": zero,
                                               "bias_hh_l0": zero if b_hh is None else b_hh}, (gi,))
    return out.reshape(-1, H)


# (T, B, H, n_gx): T = 1 (dW_hh is a zero tensor), the b_ih-only steps (db_ih = the column sums of the steps >= n_gx)
@pytest.mark.parametrize("T,B,H,n_gx", [(1, 5, 32, 1), (1, 6, 30, 0), (5, 17, 36, 5), (5, 17, 36, 2), (4, 70, 64, 0),
                                        (3, 9, 30, 1)])
def test_gru_layer_autograd_against_fp64(lib, T, B, H, n_gx):
    """gru_functional.gru_layer under autograd against nn.GRU in fp64: h_all within 2e-5 max|ref|; d gx (n_gx*B rows), db_ih,
    dW_hh, db_hh within 1e-4 max|ref| - the bounds of the stacked composite (test_gpu_stack._check_train)."""
    from s2vt_video_caption_amd import gru_functional as G
    c = _gru_seq_inputs(T, B, H, n_gx)
    dh = _randn(c["g"], T * B, H)
    has_b_ih = n_gx < T
    dev = {k: c[k].to(DEV).requires_grad_() for k in ("w_hh", "b_hh", "b_ih", "gx")}

    def run():
        for p in dev.values():
            p.grad = None
        h = G.gru_layer(dev["gx"] if n_gx else None, dev["b_ih"] if has_b_ih else None, dev["w_hh"], dev["b_hh"], T, B, n_gx)
        h.backward(dh.to(DEV))
        return [h.detach()] + [None if p.grad is None else p.grad.clone() for p in dev.values()]

    got = run()
    ref = {k: c[k].double().requires_grad_() for k in ("w_hh", "b_hh", "b_ih", "gx")}
    gi = torch.cat([ref["gx"], ref["b_ih"].expand((T - n_gx) * B, -1)]).view(T, B, 3 * H)
    href = _rnn64_identity(torch.nn.GRU, gi, ref["w_hh"], ref["b_hh"])
    (href * dh.double()).sum().backward()
    _close(got[0], href, "h_all", 2e-5)
    if T == 1:
        assert float(dev["w_hh"].grad.abs().max()) == 0.0 and float(ref["w_hh"].grad.abs().max()) == 0.0
    else:
        _close(dev["w_hh"].grad, ref["w_hh"].grad, "dW_hh", 1e-4)
    _close(dev["b_hh"].grad, ref["b_hh"].grad, "db_hh", 1e-4)
    if n_gx:
        assert dev["gx"].grad.shape == (n_gx * B, 3 * H)
        _close(dev["gx"].grad, ref["gx"].grad, "d gx", 1e-4)
    else:
        assert dev["gx"].grad is None
    if has_b_ih:
        _close(dev["b_ih"].grad, ref["b_ih"].grad, "db_ih", 1e-4)
    else:
        assert dev["b_ih"].grad is None
    for a, b in zip(got, run()):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("T,B,H", [(1, 5, 32), (5, 17, 36), (3, 70, 30)])
def test_lstm_layer_autograd_against_fp64(lib, T, B, H):
    """att_functional.lstm_layer under autograd against nn.LSTM in fp64 (bounds of the stacked composite); T = 1 is the decoder
    of an Att_Baseline of length 2: dW_hh is a zero tensor.  A second backward through the layer raises RuntimeError (its
    stash is consumed in place)."""
    from s2vt_video_caption_amd import att_functional as A
    g = torch.Generator().manual_seed(T * 1000 + B + H)
    gx, w_hh, dh = _randn(g, T * B, 4 * H), _uni(g, 4 * H, H, k=H ** -0.5), _randn(g, T * B, H)
    gxd, wd = gx.to(DEV).requires_grad_(), w_hh.to(DEV).requires_grad_()
    h = A.lstm_layer(gxd, wd, T, B)
    h.backward(dh.to(DEV), retain_graph=True)
    gxr, wr = gx.double().requires_grad_(), w_hh.double().requires_grad_()
    href = _rnn64_identity(torch.nn.LSTM, gxr.view(T, B, 4 * H), wr)
    (href * dh.double()).sum().backward()
    _close(h.detach(), href, "h_all", 2e-5)
    _close(gxd.grad, gxr.grad, "d gx", 1e-4)
    if T == 1:
        assert float(wd.grad.abs().max()) == 0.0 and float(wr.grad.abs().max()) == 0.0
    else:
        _close(wd.grad, wr.grad, "dW_hh", 1e-4)
    with pytest.raises(RuntimeError):
        h.backward(dh.to(DEV))
    first = (h.detach().clone(), gxd.grad.clone(), wd.grad.clone())
    gxd.grad = wd.grad = None
    h2 = A.lstm_layer(gxd, wd, T, B)
    h2.backward(dh.to(DEV))
    assert torch.equal(h2.detach(), first[0]) and torch.equal(gxd.grad, first[1]) and torch.equal(wd.grad, first[2])


# --------------------------------------------------------------------------------------------------- d / e. whole models
FROB = 1e-5       # TOL['x3'] = TOL['fp32'] of test_gpu_grad_release.py: both GEMM modes are fp32-equivalent


def _batch(B, L, Fd, V, seed):
    """feats [B, L, Fd] and captions [B, L] from <sos> on, word ids over the whole vocabulary (0, Att_Baseline's padding row,
    included); any L >= 2"""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, L, Fd, generator=g)
    caps = torch.randint(0, V, (B, L), generator=g)
    caps[:, 0] = 3
    caps[0, L - 1] = 0
    return feats.to(DEV), caps.to(DEV)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _check_model(what, logits, ref_logits, m, P, n_params):
    """logits within 2e-5 max|ref| and every parameter's gradient within 1e-4 max|ref| (test_gpu_stack._check_train), and each of
    them within a relative Frobenius error of 1e-5 (test_gpu_grad_release); a reference gradient that is exactly zero must be an
    exactly-zero tensor, not None."""
    names = [k for k, _ in m.named_parameters()]
    assert len(names) == n_params and sorted(names) == sorted(P)
    report = {}
    err, top, fro = _err(logits.detach(), ref_logits.detach())
    report["logits"] = (err / top, fro)
    bad = []
    if err > 2e-5 * top or fro > FROB:
        bad.append("logits")
    for k, p in m.named_parameters():
        assert p.grad is not None and P[k].grad is not None, k
        err, top, fro = _err(p.grad, P[k].grad)
        if top == 0.0:
            assert err == 0.0, k
            report[k] = (0.0, 0.0)
            continue
        report[k] = (err / top, fro)
        if err > 1e-4 * top or fro > FROB:
            bad.append(k)
    print("%s: worst max-error / max|ref| %.3g (%s), worst relative Frobenius error %.3g (%s)" % (
        what, max(v[0] for v in report.values()), max(report, key=lambda k: report[k][0]),
        max(v[1] for v in report.values()), max(report, key=lambda k: report[k][1])))
    assert not bad, (what, {k: report[k] for k in bad})
    return report


def _gru_model(B, L, Fd, H, E, V, seed=0, **kw):
    import S2VTModel
    torch.manual_seed(seed)
    m = S2VTModel.S2VT(V, Fd, L, dim_hid=H, dim_embed=E, rnn_type="gru", **kw).to(DEV)
    feats, caps = _batch(B, L, Fd, V, 77 + seed)
    return m, feats, caps


def _upstream(shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(3))


# (B, L, F, H, E, V); (70, 5, 40, 128, 100, 97): more than one 64-row block, L*B and (L-1)*B off the blocks
GRU_MODEL_CASES = [(5, 6, 48, 30, 26, 37), (16, 6, 48, 64, 56, 37), (70, 5, 40, 128, 100, 97), (64, 8, 64, 256, 128, 300)]


@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("dims", GRU_MODEL_CASES)
def test_gru_model_against_fp64_composite(lib, mode, dims):
    """S2VT(rnn_type='gru').forward(mode='train') under a random upstream gradient: the logits and all 13 gradients, whole,
    against the fp64 composite, in the plane mode and on s2vt_gemm_f32.  Measured over the cases and both modes: max error at
    most 1.2e-6 of max|ref|, relative Frobenius error at most 7.4e-7 (vid_rnn.weight_hh_l0 at B=64, H=256, mode 0) against the
    bound of 1e-5."""
    m, feats, caps = _gru_model(*dims)
    R_up = _upstream((dims[0], dims[1] - 1, dims[5]))
    with _gemm_mode(lib, mode):
        logits = m(feats, targets=caps[:, :-1], mode="train")
        (logits * R_up.to(DEV)).sum().backward()
    P = R.leaves64(m.named_parameters())
    ref = R.gru_model64(P, feats, caps[:, :-1])
    (ref * R_up.double()).sum().backward()
    _check_model("gru %s mode %d" % (dims, mode), logits, ref, m, P, 13)


@pytest.mark.parametrize("mode", [3, 0])
def test_gru_model_with_injected_out_mask(lib, mode):
    """gru_functional.train_forward with an out_drop mask of {0, 1/(1-p)} entries: outputs and gradients against the composite
    with the same mask; a second run returns the same bits."""
    from s2vt_video_caption_amd import gru_functional as G
    B, L, Fd, H, E, V = 9, 6, 40, 36, 26, 41
    m, feats, caps = _gru_model(B, L, Fd, H, E, V, seed=1)
    g = torch.Generator().manual_seed(11)
    out_mask = ((torch.rand(B, L - 1, H, generator=g) > 0.3).float() / 0.7).to(DEV)
    R_up = _upstream((B, L - 1, V))
    runs = []
    with _gemm_mode(lib, mode):
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            logits = G.train_forward(m, feats, caps[:, :-1], out_mask=out_mask)
            (logits * R_up.to(DEV)).sum().backward()
            runs.append((logits.detach().clone(), _grads(m)))
    P = R.leaves64(m.named_parameters())
    ref = R.gru_model64(P, feats, caps[:, :-1], out_mask=out_mask)
    (ref * R_up.double()).sum().backward()
    _check_model("gru out_mask mode %d" % mode, logits, ref, m, P, 13)
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("mode", [3, 0])
def test_gru_model_through_mask_criterion_on_a_ragged_batch(lib, mode):
    """Training on real captions with their mask, a batch off every block size (B = 70), with out_dropout > 0 in train mode (the
    mask is the model's own draw, replayed as test_gpu_grad_release replays it): utils.MaskCriterion's loss and all 13 gradients
    against the composite under the reference's MaskCriterion arithmetic."""
    import utils
    from s2vt_video_caption_amd import synth
    B, L, Fd, H, E, V, p, seed = 70, 8, 40, 64, 56, 97, 0.25, 5
    m, _, _ = _gru_model(B, L, Fd, H, E, V, seed=2, out_dropout=p)
    feats, caps, mask = (t.to(DEV) for t in synth.make_batch(B, L, Fd, V, seed=99))
    m.train()
    with _gemm_mode(lib, mode):
        torch.manual_seed(seed)
        logits = m(feats, targets=caps[:, :-1], mode="train")
        loss = utils.MaskCriterion()(logits, caps, mask)
        loss.backward()
    torch.manual_seed(seed)
    out_mask = torch.nn.Dropout(p)(torch.ones(B, L - 1, H, device=DEV))
    assert 0.0 < float((out_mask == 0).float().mean()) < 1.0
    P = R.leaves64(m.named_parameters())
    ref = R.gru_model64(P, feats, caps[:, :-1], out_mask=out_mask)
    ref_loss = R.reference_criterion64(ref, caps, mask)
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-5     # (test_att_baseline_train_step_against_reference's)
    _check_model("gru criterion mode %d" % mode, logits, ref, m, P, 13)


def _att_model(B, L, Fd, H, E, V, seed=0, **kw):
    import attention_baseline
    torch.manual_seed(seed)
    m = attention_baseline.Att_Baseline(V, Fd, L, dim_hid=H, dim_embed=E, **kw).to(DEV)
    feats, caps = _batch(B, L, Fd, V, 55 + seed)
    return m, feats, caps


# (B, L, F, H, E, V); (6, 2, 40, 32, 24, 37): the decoder runs T = 1 step
ATT_MODEL_CASES = [(5, 8, 48, 32, 24, 60), (16, 6, 40, 64, 56, 37), (70, 5, 40, 128, 100, 97), (6, 2, 40, 32, 24, 37)]
ATT_ZERO = ("att_enc.weight", "att_enc.bias", "att_prev_hid.weight", "att_prev_hid.bias", "att_apply.weight")


@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("dims", ATT_MODEL_CASES)
def test_att_baseline_against_fp64_composite(lib, mode, dims):
    """Att_Baseline.forward(mode='train') under a random upstream gradient: the logits and all 22 gradients, whole, against the
    fp64 composite (bidirectional encoder, context = the sum over the frames, decoder over [Emb | context]); the attention
    layers' gradients are zero tensors, not None.  Measured over the cases and both modes: max error at most 1.2e-6 of max|ref|,
    relative Frobenius error at most 6.8e-7 (feat_linear.weight at B=70, mode 0) against the bound of 1e-5."""
    m, feats, caps = _att_model(*dims)
    R_up = _upstream((dims[0], dims[1] - 1, dims[5]))
    with _gemm_mode(lib, mode):
        logits = m(feats, targets=caps[:, :-1], mode="train")
        (logits * R_up.to(DEV)).sum().backward()
    P = R.leaves64(m.named_parameters())
    ref = R.att_model64(P, feats, caps[:, :-1])
    (ref * R_up.double()).sum().backward()
    for k in ATT_ZERO:
        g = dict(m.named_parameters())[k].grad
        assert g is not None and float(g.abs().max()) == 0.0, k
    _check_model("att %s mode %d" % (dims, mode), logits, ref, m, P, 22)


@pytest.mark.parametrize("mode", [3, 0])
def test_att_baseline_with_dropout_in_train_mode(lib, mode):
    """feat_dropout = 0.2 and out_dropout = 0.3 in train mode.  The masks are the model's own draws, replayed from the same seed
    in its order and shapes: nn.Dropout on [B, L, F] ones (the frames), then on [(L-1)*B, H] ones (the decoder's outputs,
    time-major).  Outputs and gradients against the composite with those masks; a second seeded run returns the same bits, and
    eval mode is the model without dropout."""
    B, L, Fd, H, E, V, seed = 9, 6, 40, 36, 28, 41, 17
    m, feats, caps = _att_model(B, L, Fd, H, E, V, seed=1, feat_dropout=0.2, out_dropout=0.3)
    R_up = _upstream((B, L - 1, V))
    m.train()
    runs = []
    with _gemm_mode(lib, mode):
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            torch.manual_seed(seed)
            logits = m(feats, targets=caps[:, :-1], mode="train")
            (logits * R_up.to(DEV)).sum().backward()
            runs.append((logits.detach().clone(), _grads(m)))
        m.eval()
        with torch.no_grad():
            plain = m(feats, targets=caps[:, :-1], mode="train")
        m.train()
    torch.manual_seed(seed)
    feat_mask = torch.nn.Dropout(0.2)(torch.ones(B, L, Fd, device=DEV))
    out_tm = torch.nn.Dropout(0.3)(torch.ones((L - 1) * B, H, device=DEV))
    out_mask = out_tm.view(L - 1, B, H).transpose(0, 1)
    assert 0.0 < float((feat_mask == 0).float().mean()) < 1.0 and 0.0 < float((out_tm == 0).float().mean()) < 1.0
    P = R.leaves64(m.named_parameters())
    ref = R.att_model64(P, feats, caps[:, :-1], feat_mask=feat_mask, out_mask=out_mask)
    (ref * R_up.double()).sum().backward()
    _check_model("att dropout mode %d" % mode, logits, ref, m, P, 22)
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    P0 = R.leaves64(m.named_parameters())
    _close(plain, R.att_model64(P0, feats, caps[:, :-1]).detach(), "eval-mode logits", 2e-5)
