"""GPU: the two kernel families that share csrc/step_frame.h with the LSTM step kernels - the layer-wavefront chain kernels
(csrc/lstm_stack.hip through s2vt_lstm_chain_fwd / _bwd) and the GRU step kernels (csrc/gru.hip) - against the fp64 restatements of
tests/step_family_ref.py, at the places where such kernels break and the rest of the suite does not go:

  a  chain forward, then backward on its own outputs (T = 3, n = 3: gx on one step, a zero-state layer under a mask, a bias-only
     layer): the 32-row tile with a ragged third row block and the 16 x 16 backward tile ragged both ways under the mask (70, 40);
     nine column tiles (130, 72); tiles wider than the matrix and K below one chunk (17, 8), (3, 4); the scalar kernels (3, 5).
     Outputs prefilled with NaN, inputs bit-unchanged, a second call bit-equal.
  b  the scalar 16-row form at B > 16 with H % 4 == 0, reached through w_hh 4 bytes past a 16-byte boundary, through w_in as a
     column block of a wider tensor, and in the backward through such a dG: against fp64 and against the aligned launch.
  c  the chain's token segment (T = 1 word chains): 32-row vector tile, scalar, all three segments on a ragged tile, the smallest.
  d  the backward's forms: dG aliased to the stash, T = 1, dh_t0 == T, dh_ext below the top, no mask, a chain of one layer.
  e  the GRU forward (zero state with b_ih alone, a state), the stash and the BPTT step from H = 4 to nine column tiles.
  f  the GRU scalar kernels through misaligned w_hh / h_prev and dgh_next / W_hh^T.
  g  the GRU backward's forms: the last step with a NaN-filled dh buffer, no h_prev, no dh_out, nothing flowing.
  h  the GRU token variant past B = 64 on ragged tiles, vector and scalar, int32 tokens and packed words; the zero state.
  i  an LSTM token step at B = 5, H = 2564, E = 2560 under option gemv = 2: the GEMV kernel would stage 163968 bytes of rows, more
     LDS than a CU has; the step has to run (on the tile kernel).

Bounds are the project's, relative to max|reference| (step_family_ref.REL_*: test_gpu_gru._close, test_gpu_stack._close);
tests/test_step_family_ref_host.py shows on the host that fp32 arithmetic stays under half of them and that zeroing the last row
or column block of any output of any case here moves it by at least 10 bounds.  (Tried once on the device: with the mask's row
map in chain_bwd_body transposed, and with gru_step_bwd_kernel reading r for z of the next step, every chain case under a mask
and every GRU backward case with a successor failed, the others passed.)  Every test prints its worst error / bound.
Seen on an MI355X (worst error / bound over the cases of a group):
  a  forward 0.051 (70, 40), dG 0.017 (3, 4)
  b  forward 0.054, dG 0.013; every misaligned launch bit-equal to the aligned one (the scalar loads change no summation order)
  c  0.068 (70, 40, 36) constant token
  d  forward 0.053, dG 0.032 ((17, 8) at T = 1)
  e  zero state 0.089 (130, 136), from a state 0.022, BPTT step 0.014
  f  forward 0.020, backward 0.014; bit-equal to the aligned launches
  g  0.013                                       h  0.021
  i  before lstm_step_fwd_gemv_ok counted the LDS: hipFuncSetAttribute refused the 163968 bytes (invalid argument) and the step
     failed; now on the tile kernel h 1.0e-6, c 1.3e-6 (4e-6)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_family_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731
_TENSORS = ("w_hh", "bias", "w_in", "h0", "c0", "gx", "x_in", "mask", "emb", "dh_ext")


def _off4(t):
    """a contiguous device copy of t whose first element lies 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _column_block(t):
    """a device copy of t [N, K] as the column block [:, 1:1+K] of a wider tensor full of NaN: rows a multiple of 16 bytes apart,
    every one of them 4 bytes past a 16-byte boundary"""
    wide = torch.full((t.shape[0], t.shape[1] + 4 - t.shape[1] % 4), NAN, device=DEV)
    v = wide[:, 1:1 + t.shape[1]]
    v.copy_(t)
    assert v.stride(0) % 4 == 0 or t.shape[1] % 4, v.stride()
    assert v.data_ptr() % 16 == 4 and v.stride(1) == 1
    return v


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _frac(what, got, ref, rel):
    """error / bound of a device result, which must be finite and within the bound"""
    e, b = R.err(got, ref), R.bound(ref, rel)
    assert bool(torch.isfinite(got).all()), what
    assert e <= b, (what, e, b)
    return e / b


# ---------------------------------------------------------------------------------------------------------------- chain helpers
def _device_layers(layers, T, B, H, off=None):
    """device dicts of a chain's host layers for ops.lstm_chain_fwd, every output prefilled with NaN.  off: 'w_hh' / 'w_in' puts
    that operand of every layer 4 bytes past a 16-byte boundary.  A layer with `w0` (token segment) gets x_in's weight and W_e as
    column blocks of it."""
    out = []
    for l in layers:
        d = {k: l[k].to(DEV) for k in _TENSORS if l.get(k) is not None and k != "dh_ext"}
        d.update({k: l[k] for k in ("gx_t0", "n_gx") if k in l})
        if off == "w_hh":
            d["w_hh"] = _off4(l["w_hh"])
        if off == "w_in":
            d["w_in"] = _column_block(l["w_in"])
        if l.get("w0") is not None:
            w0 = l["w0"].to(DEV)
            E = l["emb"].shape[1]
            d.update(w_in=w0[:, E:], w_e=w0, E=E, V=l["emb"].shape[0])
        d.update(h=_nan(T * B, H), c=_nan(T * B, H), stash=_nan(T * B, 4 * H))
        if l.get("mask") is not None:
            d["hm"] = _nan(T * B, H)
        out.append(d)
    return out


def _inputs_unchanged(dev_layers, layers):
    for d, l in zip(dev_layers, layers):
        for k in _TENSORS:
            if l.get(k) is not None and k in d:
                assert torch.equal(d[k].cpu(), l[k]), k
        if l.get("w0") is not None:
            assert torch.equal(d["w_e"].cpu(), l["w0"])


def _forward(layers, T, B, H, off=None, **token):
    """the device forward, run twice on NaN-prefilled outputs: inputs untouched, the second call bit-equal.  Returns the layers."""
    from s2vt_video_caption_amd import ops
    runs = []
    for _ in range(2):
        dev = _device_layers(layers, T, B, H, off)
        dev[0].update(token)
        ops.lstm_chain_fwd(T, B, H, dev)
        torch.cuda.synchronize()
        _inputs_unchanged(dev, layers)
        runs.append(dev)
    for a, b in zip(*runs):
        for k in ("h", "c", "stash", "hm"):
            assert (k in a) == (k in b) and (k not in a or torch.equal(a[k], b[k])), k
    return runs[0]


def _check_forward(what, dev, ref):
    worst = 0.0
    for j, (d, r) in enumerate(zip(dev, ref)):
        for k, want in zip(("h", "c", "stash", "hm"), r):
            assert (want is None) == (k not in d)
            if want is not None:
                worst = max(worst, _frac("%s layer %d %s" % (what, j, k), d[k], want, R.REL_CHAIN))
    return worst


def _backward(dev, layers, T, B, H, alias=False, off_dg=False):
    """the device backward on the forward's own outputs `dev`; returns per layer dG.  alias: dG written over the stash."""
    from s2vt_video_caption_amd import ops
    bw = []
    for j, (d, l) in enumerate(zip(dev, layers)):
        b = {k: v for k, v in d.items() if k not in ("x_in", "gx", "gx_t0", "n_gx")}
        if j == 0:
            b.pop("w_in", None)                  # no backward through an external input
        b.update(stash=d["stash"].clone(), c=d["c"].clone())
        b["dg"] = b["stash"] if alias else (_off4(torch.full((T * B, 4 * H), NAN)) if off_dg else _nan(T * B, 4 * H))
        if l.get("dh_ext") is not None:
            b.update(dh_ext=l["dh_ext"].to(DEV), dh_t0=l["dh_t0"])
        bw.append(b)
    ops.lstm_chain_bwd(T, B, H, bw)
    torch.cuda.synchronize()
    for b, d, l in zip(bw, dev, layers):
        assert torch.equal(b["c"], d["c"]) and (alias or torch.equal(b["stash"], d["stash"]))
        for k in ("w_hh", "w_in", "mask", "h0", "c0", "dh_ext"):
            if k in b and not (k == "dh_ext" and l["dh_t0"] == T):
                assert torch.equal(b[k].cpu(), l[k]), k
    return [b["dg"] for b in bw]


def _check_backward(what, dgs, ref):
    return max(_frac("%s layer %d dG" % (what, j), dg, r, R.REL_CHAIN_DG) for j, (dg, r) in enumerate(zip(dgs, ref)))


# ------------------------------------------------------------------------------------ a: chain forward, backward on its outputs
@pytest.mark.parametrize("B,H", R.CHAIN_SHAPES)
def test_chain_forward_then_backward_at_tile_edges(lib, B, H):
    c = R.chain_case(B, H)
    fwd, dg_ref = R.chain_ref(B, H)
    dev = _forward(c["layers"], c["T"], B, H)
    wf = _check_forward("a %s" % ((B, H),), dev, fwd)
    wb = _check_backward("a %s" % ((B, H),), _backward(dev, c["layers"], c["T"], B, H), dg_ref)
    print("a", (B, H), "forward %.3g of its bound, dG %.3g" % (wf, wb))


# ---------------------------------------------------------------------------------- b: the scalar 16-row form at H % 4 == 0
@pytest.mark.parametrize("operand", R.MISALIGNED_OPERANDS + ["dg"])
def test_chain_scalar_form_through_a_misaligned_operand(lib, operand):
    """lstm_chain_fwd_launch / _bwd_launch test every operand for 16-byte alignment and launch <1, false> / <false> when one fails.
    w_hh and w_in reach the forward (the backward works on transposed copies of its own); a misaligned dG reaches the backward."""
    B, H = R.CHAIN_MISALIGNED
    c = R.chain_case(B, H)
    T, layers = c["T"], c["layers"]
    fwd, dg_ref = R.chain_ref(B, H)
    aligned = _forward(layers, T, B, H)
    dg_aligned = _backward(aligned, layers, T, B, H)
    dev = _forward(layers, T, B, H, off=None if operand == "dg" else operand)
    dgs = _backward(dev, layers, T, B, H, off_dg=(operand == "dg"))
    wf, wb = _check_forward("b %s" % operand, dev, fwd), _check_backward("b %s" % operand, dgs, dg_ref)
    wa = 0.0
    for j in range(len(layers)):
        for k, r in zip(("h", "c", "stash", "hm"), fwd[j]):
            if r is not None:
                wa = max(wa, R.err(dev[j][k], aligned[j][k].cpu()) / (2 * R.bound(r, R.REL_CHAIN)))
        wa = max(wa, R.err(dgs[j], dg_aligned[j].cpu()) / (2 * R.bound(dg_ref[j], R.REL_CHAIN_DG)))
    print("b", operand, "forward %.3g of its bound, dG %.3g, to the aligned launch %.3g of twice the bound" % (wf, wb, wa))
    assert wa <= 1.0


# ------------------------------------------------------------------------------------------------------ c: chain token segment
@pytest.mark.parametrize("B,H,E", R.CHAIN_TOKEN)
def test_chain_token_segment_at_tile_edges(lib, B, H, E):
    from s2vt_video_caption_amd import capi
    c = R.token_case(B, H, E)
    for source in ("const", "packed"):
        tok = dict(tok_const=c["tok_const"]) if source == "const" else dict(tok_const=0, tok_packed=c["packed"].to(DEV))
        dev = _forward(c["layers"], 1, B, H, **tok)
        w = _check_forward("c %s %s" % ((B, H, E), source), dev, R.token_ref(B, H, E, source))
        capi.check_async_error()
        print("c", (B, H, E), source, "%.3g of its bound" % w)


# ------------------------------------------------------------------------------------------------------ d: chain backward forms
@pytest.mark.parametrize("form", ["alias"] + R.CHAIN_BWD_FORMS)
@pytest.mark.parametrize("B,H", R.CHAIN_BWD_SHAPES)
def test_chain_backward_forms(lib, B, H, form):
    name = "main" if form == "alias" else form
    c = R.chain_case(B, H, name)
    T, layers = c["T"], c["layers"]
    fwd, dg_ref = R.chain_ref(B, H, name)
    dev = _forward(layers, T, B, H)
    wf = _check_forward("d %s %s" % ((B, H), form), dev, fwd)
    dgs = _backward(dev, layers, T, B, H, alias=(form == "alias"))
    if form == "nothing_flows":
        assert all(float(dg.abs().max()) == 0.0 for dg in dgs)        # (and not NaN: the prefill is gone, dh_ext was not read)
        print("d", (B, H), form, "forward %.3g of its bound, dG exactly 0" % wf)
        return
    wb = _check_backward("d %s %s" % ((B, H), form), dgs, dg_ref)
    if form == "alias":
        for a, b in zip(dgs, _backward(dev, layers, T, B, H)):
            assert torch.equal(a, b)
    print("d", (B, H), form, "forward %.3g of its bound, dG %.3g" % (wf, wb))


# -------------------------------------------------------------------------------------------------------- GRU helpers
def _dev(t):
    return None if t is None else t.to(DEV)


def _gru_bwd(a, off_dgh=False, off_wt=False):
    """the device's (dgx, dgh, dh) of gru_bwd_args; both stash buffers must come back bit-unchanged"""
    from s2vt_video_caption_amd import ops
    B, H = a["stash"].shape[0], a["w_hh"].shape[1]
    last = a["dgh_next"] is None
    wt = a["w_hh"].t().contiguous()
    wt = None if last else (_off4(wt) if off_wt else wt.to(DEV))
    dgh_next = None if last else (_off4(a["dgh_next"]) if off_dgh else a["dgh_next"].to(DEV))
    dh = _nan(B, H) if last else a["dh_in"].to(DEV).clone()      # (the last step must not read it)
    stash, stash_next = a["stash"].to(DEV), _dev(a["stash_next"])
    dgx, dgh = ops.gru_step_bwd(dgh_next, wt, stash_next, _dev(a["dh_out"]), stash, _dev(a["h_prev"]), dh)
    torch.cuda.synchronize()
    assert torch.equal(stash.cpu(), a["stash"]) and (last or torch.equal(stash_next.cpu(), a["stash_next"]))
    return dgx, dgh, dh


def _check_gru(what, got, ref):
    return max(_frac("%s %s" % (what, n), g, r, R.REL_GRU) for n, g, r in zip(("dgx / h", "dgh / stash", "dh"), got, ref))


# ------------------------------------------------------------------------------------ e: GRU forward, stash and BPTT step
@pytest.mark.parametrize("B,H", R.GRU_SHAPES)
def test_gru_step_kernels_at_tile_edges(lib, B, H):
    from s2vt_video_caption_amd import ops
    d = R.gru_inputs(B, H)
    w, bh = d["w_hh"].to(DEV), d["b_hh"].to(DEV)
    z = _check_gru("e zero state", ops.gru_step_fwd(None, d["b_ih"].to(DEV), w, bh, None, want_stash=True, B=B), R.gru_fwd_ref(B, H, 0, "zero_state"))
    s = _check_gru("e state", ops.gru_step_fwd(d["gx"].to(DEV), None, w, bh, d["h_prev"].to(DEV), want_stash=True), R.gru_fwd_ref(B, H, 0, "state"))
    b = _check_gru("e bptt", _gru_bwd(R.gru_bwd_args(B, H)), R.gru_bwd_ref(B, H))
    print("e", (B, H), "zero state %.3g of its bound, from a state %.3g, BPTT step %.3g" % (z, s, b))


# ---------------------------------------------------------------------------------------------- f: GRU scalar instantiations
@pytest.mark.parametrize("which", ["w_hh", "h_prev", "dgh_next", "w_hh_t"])
def test_gru_scalar_kernels_through_a_misaligned_operand(lib, which):
    from s2vt_video_caption_amd import ops
    B, H = R.GRU_MISALIGNED
    d = R.gru_inputs(B, H)
    if which in ("w_hh", "h_prev"):
        ref = R.gru_fwd_ref(B, H, 0, "state")
        run = lambda w, h: ops.gru_step_fwd(d["gx"].to(DEV), None, w, d["b_hh"].to(DEV), h, want_stash=True)  # noqa: E731
        got = run(_off4(d["w_hh"]) if which == "w_hh" else d["w_hh"].to(DEV), _off4(d["h_prev"]) if which == "h_prev" else d["h_prev"].to(DEV))
        aligned = run(d["w_hh"].to(DEV), d["h_prev"].to(DEV))
    else:
        ref = R.gru_bwd_ref(B, H)
        got = _gru_bwd(R.gru_bwd_args(B, H), off_dgh=(which == "dgh_next"), off_wt=(which == "w_hh_t"))
        aligned = _gru_bwd(R.gru_bwd_args(B, H))
    w = _check_gru("f %s" % which, got, ref)
    wa = max(R.err(g, a.cpu()) / (2 * R.bound(r, R.REL_GRU)) for g, a, r in zip(got, aligned, ref))
    print("f", which, "%.3g of its bound, to the aligned launch %.3g of twice the bound" % (w, wa))
    assert wa <= 1.0


# ----------------------------------------------------------------------------------------------------- g: GRU backward forms
@pytest.mark.parametrize("form", R.GRU_BWD_FORMS)
@pytest.mark.parametrize("B,H", R.GRU_BWD_SHAPES)
def test_gru_backward_forms(lib, B, H, form):
    got = _gru_bwd(R.gru_bwd_args(B, H, form))
    ref = R.gru_bwd_ref(B, H, form)
    if form == "last_no_dh_out":
        assert all(float(t.abs().max()) == 0.0 for t in got)          # (dh came in as NaN: it was not read)
        print("g", (B, H), form, "exactly 0")
        return
    print("g", (B, H), form, "%.3g of its bound" % _check_gru("g %s" % form, got, ref))


# ----------------------------------------------------------------------------------------------------- h: GRU token variant
@pytest.mark.parametrize("B,H,E", R.GRU_TOKEN + [R.GRU_TOKEN_ZERO_STATE])
def test_gru_token_variant_on_ragged_tiles(lib, B, H, E):
    from s2vt_video_caption_amd import capi, ops
    d = R.gru_inputs(B, H, E)
    zero = (B, H, E) == R.GRU_TOKEN_ZERO_STATE
    ref = R.gru_fwd_ref(B, H, E, "token_zero_state" if zero else "token")[0]
    args = (d["gx"].to(DEV), d["w_hh"].to(DEV), d["b_hh"].to(DEV), None if zero else d["h_prev"].to(DEV), d["emb"].to(DEV), d["w_ih"].to(DEV))
    w = 0.0
    for name, tok in (("int32", dict(tok=d["tok"].int().to(DEV))), ("packed", dict(tok_packed=d["packed"].to(DEV)))):
        out = _nan(B, H)
        h = ops.gru_step_fwd_token(*args, out=out, **tok)
        w = max(w, _frac("h %s %s" % ((B, H, E), name), h, ref, R.REL_GRU))
    torch.cuda.synchronize()
    capi.check_async_error()
    print("h", (B, H, E), "%.3g of its bound" % w)


# ------------------------------------------------------------------- i: the GEMV step's staged rows against the LDS of a CU
def test_lstm_token_step_whose_staged_rows_exceed_the_lds(lib):
    """(last in the file: were the launch refused, the error must not be met by another test's launch check)"""
    from s2vt_video_caption_amd import capi, ops
    d, h_ref, c_ref = R.gemv_lds_inputs()
    prev = lib.s2vt_set_option(b"gemv", -1)
    try:
        lib.s2vt_set_option(b"gemv", 2)
        h, c = ops.lstm_step_fwd_token(*(d[k].to(DEV) for k in ("gx", "w_hh", "h_prev", "c_prev", "emb", "w_ih")), tok=d["tok"].to(DEV))
        torch.cuda.synchronize()
        capi.check_async_error()
    finally:
        lib.s2vt_set_option(b"gemv", prev)
    e = (R.err(h, h_ref), R.err(c, c_ref))
    print("i", R.GEMV_LDS_CASE, "h %.3g c %.3g (bound %.3g)" % (e[0], e[1], R.TOL_GEMV))
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all())
    assert e[0] < R.TOL_GEMV and e[1] < R.TOL_GEMV
