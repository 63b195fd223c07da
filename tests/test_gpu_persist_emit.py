"""GPU: what the persistent split-precision kernels (csrc/lstm_persist_x3.hip) write BESIDE the recurrence in the train and decode
drivers, through the test-support entry points s2vt_lstm_seq_{fwd,bwd}_x3_persist_emit, a few launches at T <= 4 per case:

  forward   SeqFwdX3Args::hblk - h_t as the blocked 3-plane row image that the batched GEMMs read - and no_stash;
  BPTT      SeqBwdX3Args::dgp (dG_t as such an image, through the XOR-swizzled LDS tile), colpart (the bias gradient's 32-row
            column sums per chain) and skip_dg.

Whole images are pinned by BIT equality with ops.split_planes (tested on its own, against a host split, in test_gpu_plane_split.py) of the fp32 output of the
run without emission - which test_persistent_split_precision_recurrence / _bptt pin against fp64 - and by a sentinel pre-fill of an
image with a wider row stride and 64 more rows: nothing outside the documented elements may change.  Column sums are pinned against
the fp64 sum of the same fp32 dG: (n - 1) * 2^-24 * sum|x| bounds an n-term fp32 sum in ANY fixed order (every one of the n - 1
additions rounds a partial sum of magnitude <= sum|x| by at most 2^-24 of it, to first order), n = 32 for a chain, n = T * B for
the total.  Every case prints observed / bound.

Chain plans (lstm_persist_frame.h: plan_chains, plan_xcd; restated in _plan below, checked in test_shapes_reach_the_planned_forms).
One workgroup per compute unit, so 256 resident workgroups; nC = ceil(H / 16) column slices; B / 32 row groups are merged two by
two while (row groups) * nC exceeds the limit: the whole capacity (256) for a forward launch with ONE layer, half of it (128) for a
layer of a pair and for every BPTT launch.
  B = 64:  2 row groups; 2 * nC <= 128 for every H <= 1024: one chain per workgroup, G = 2 groups dealt over the XCDs.
  B = 128, H = 520: nC = 33, 4 * 33 = 132 > 128 -> 2 row groups of TWO chains (66 workgroups) wherever the limit is 128: the BPTT
           and the forward pair; H = 504 (nC = 32, 128 workgroups) still has one.  A one-layer forward launch has 132 <= 256
           workgroups with one chain, so the forward list runs this shape as a pair too (added to the issue's list).
  B = 192, H = 520: 6 * 33 = 198: one chain in a one-layer forward launch (G = 6: grid in plain order); the BPTT merges to 3 row
           groups of two chains (99 workgroups, G = 3: plain order).
  B = 128, H = 1000 pair: nC = 63, 4 * 63 = 252 > 128 -> two chains, 126 workgroups per layer, G = 4, grid padded to 8 * 32 = 256:
           XCD-dealt with two chains per workgroup."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_decode_forms import PLANE_SENT  # noqa: E402
from test_gpu_kernels import _bptt_inputs, _r  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTF = -777.25                      # a float no launch may write over (or, with no_stash / skip_dg, at all)
U = 2.0 ** -24                       # unit roundoff of fp32


def _row_plane_index(rows, K, ld):
    """flat element index of (row, k, plane) in a blocked 3-plane ROW image of row stride ld (include/s2vt_hip.h, s2vt_split_planes;
    _plane_index of test_gpu_decode_forms.py with time-major rows r = t * B + b)"""
    r, k, pl = torch.arange(rows)[:, None, None], torch.arange(K)[None, :, None], torch.arange(3)[None, None, :]
    return (r // 64) * (64 * ld) + (k // 16) * 3072 + (pl * 2 + (k // 8) % 2) * 512 + (r % 64) * 8 + k % 8


def _plan(B, H, layers, bptt):
    """(chains per workgroup, workgroups per layer, XCD groups or 0) as plan_chains / plan_xcd (XCD_PADDED) compute them"""
    cap = min(256, torch.cuda.get_device_properties(0).multi_processor_count)
    nC = (H + 15) // 16
    if B % 32 or not 8 <= H <= 1024:
        return 0, 0, 0

    def chains(lim):
        R, ns = B // 32, 1
        while R * nC > lim and ns < 4 and R % 2 == 0:
            R, ns = R // 2, ns * 2
        return ns if R * nC <= lim and R <= 64 else 0
    ns = chains(cap // 2)
    if ns and layers == 1 and not bptt:
        ns = chains(cap)
    if not ns:
        return 0, 0, 0
    na = B // (32 * ns) * nC
    G = na * layers // nC
    xg = G if G in (1, 2, 4, 8) and 8 * -(-nC // (8 // G)) <= cap else 0
    return ns, na, xg


def _bits(t):
    return t.detach().cpu().contiguous()


def _check_image(tag, img, ld, rows, K, Kw, ref_planes, ld0):
    """img (int16, row stride ld, pre-filled with PLANE_SENT): elements (row < rows, k < K) have the bits of ref_planes (row stride
    ld0), (row < rows, K <= k < Kw) are zero, every other element still holds the sentinel"""
    flat, ref = _bits(img).flatten(), _bits(ref_planes).flatten()
    idx, idx0 = _row_plane_index(rows, Kw, ld), _row_plane_index(rows, K, ld0)
    assert int(idx.max()) < flat.numel() and int(idx0.max()) < ref.numel()
    outside = torch.ones(flat.numel(), dtype=torch.bool)
    outside[idx.flatten()] = False
    wrote = outside & (flat != PLANE_SENT)
    assert not wrote.any(), "%s: %d elements written outside rows < %d, k < %d; first flat index %d (row stride %d)" % (
        tag, int(wrote.sum()), rows, Kw, int(wrote.nonzero()[0]), ld)
    got, want = flat[idx[:, :K].flatten()], ref[idx0.flatten()]
    assert (want != PLANE_SENT).all()
    bad = (got != want).reshape(rows, K, 3)
    assert not bad.any(), "%s: %d image elements differ from split_planes, first (row, k, plane) = %s" % (
        tag, int(bad.sum()), bad.nonzero()[0].tolist())
    if Kw > K:
        pad = flat[idx[:, K:].flatten()].reshape(rows, Kw - K, 3)
        assert (pad == 0).all(), "%s: k padding [%d, %d) of a written record is not zero bits, first (row, k - K, plane) = %s" % (
            tag, K, Kw, (pad != 0).nonzero()[0].tolist())


# ------------------------------------------------------------------------------------------------------------ forward
# (T, B, H, n_gx, block, layers)
FWD_SHAPES = [
    (3, 64, 8, 3, 0, 1),          # one column slice; k16 records 1..3 of the 64-wide k block stay untouched
    (4, 64, 37, 2, 2, 1),         # H % 8 != 0: units 37..47 are pad inside the last record; two launches
    (3, 64, 72, 1, 0, 1),         # H % 16 == 8
    (4, 192, 520, 2, 3, 1),       # three 64-row blocks per step; launches of 3 + 1 steps
    (3, 128, 520, 3, 0, 1),       # 132 workgroups of one chain (see the module comment) ...
    (3, 128, 520, 3, 0, 2),       # ... and as a pair: the smallest shape with two chains per workgroup
    (3, 64, 1000, 1, 0, 1),       # config 2's 63 slices; units 1000..1007 are pad; record 63 untouched
    (2, 64, 1024, 0, 0, 1),       # no k padding at all; bias-only input
    (4, 128, 1000, 2, 2, 2),      # two layers per launch, distinct weights, both images; XCD-dealt grid, two chains per workgroup
]


def _fwd_inputs(T, B, H, n_gx, layer):
    s = 300 + 10 * layer
    return (_r(n_gx * B, 4 * H, seed=s + 1).to(DEV), _r(4 * H, seed=s + 2, scale=0.3).to(DEV),
            _r(4 * H, H, seed=s + 3, scale=H ** -0.5).to(DEV))


def _planted_stash(T, B, H, n_gx, gx):
    st = torch.full((T * B, 4 * H), SENTF, device=DEV)
    if n_gx:
        st[:n_gx * B].copy_(gx)
    return st


@functools.lru_cache(maxsize=None)
def _fwd_runs(T, B, H, n_gx, block, layers):
    """per layer: the run without emission (h, c, gates), the run with the image (h, c, stash, image, ld), the no_stash run with
    the image (h, c, stash, image) and the stash as it was handed in - each run is made ONCE"""
    from s2vt_video_caption_amd import capi, ops
    ins = [_fwd_inputs(T, B, H, n_gx, k) for k in range(layers)]
    keep = ops.lstm_seq_fwd_persist(T, B, ins[0][0], n_gx, ins[0][1], ins[0][2], block=block, second=ins[1] if layers == 2 else None)
    keep = keep if layers == 2 else (keep,)
    out = {"keep": keep, "ins": ins}
    for name, no_stash in (("emit", False), ("nostash", True)):
        st = [_planted_stash(T, B, H, n_gx, ins[k][0]) for k in range(layers)]
        im = [ops.row_plane_image(T * B, H, DEV, fill=PLANE_SENT, extra_ld=8, extra_rows=64) for _ in range(layers)]
        got = ops.lstm_seq_fwd_persist_emit(T, B, st[0], n_gx, ins[0][1], ins[0][2], hblk=im[0], no_stash=no_stash, block=block,
                                            second=(st[1], ins[1][1], ins[1][2], im[1]) if layers == 2 else None)
        got = got if layers == 2 else (got,)
        out[name] = [(got[k][0], got[k][1], st[k], im[k][0], im[k][1]) for k in range(layers)]
    torch.cuda.synchronize()
    capi.check_async_error()
    return out


@pytest.mark.parametrize("T,B,H,n_gx,block,layers", FWD_SHAPES)
def test_forward_row_image_by_bits(lib, T, B, H, n_gx, block, layers):
    """hblk set: h_all / c_all / gates unchanged; the image restricted to (row < T*B, unit < H) bit-equal to split_planes(h_all);
    units [H, 16 * ceil(H / 16)) of written rows zero in all three planes; everything else - the k16 records past them, the 8 extra
    elements per row, the 64 extra rows - still the sentinel.  With block > 0 each launch writes its own steps' rows: seen through
    the final image."""
    from s2vt_video_caption_amd import ops
    runs = _fwd_runs(T, B, H, n_gx, block, layers)
    kpad, Hw = (H + 63) // 64 * 64, (H + 15) // 16 * 16
    for k in range(layers):
        h0, c0, g0 = runs["keep"][k]
        h1, c1, st1, img, ld = runs["emit"][k]
        assert ld == 3 * kpad + 8 and img.shape[0] == T * B + 64
        assert torch.equal(h1, h0) and torch.equal(c1, c0) and torch.equal(st1, g0), "layer %d: emission changed the recurrence" % k
        ref, ld0, _ = ops.split_planes(h0)
        _check_image("fwd T=%d B=%d H=%d layer %d" % (T, B, H, k), img, ld, T * B, H, Hw, ref, ld0)
    ns, na, xg = _plan(B, H, layers, False)
    print("fwd T=%d B=%d H=%d x%d: %d chain(s) per workgroup, %d workgroups per layer, XCD groups %d; images bit-equal" % (
        T, B, H, layers, ns, na, xg))


@pytest.mark.parametrize("T,B,H,n_gx,block,layers", FWD_SHAPES)
def test_forward_no_stash_leaves_the_gate_buffer_alone(lib, T, B, H, n_gx, block, layers):
    """no_stash = 1 (greedy decode): h_all, c_all and the row image have the bits of the stash run; gx_stash is bitwise what was
    handed in - the gate inputs in its first n_gx * B rows, the planted sentinel in the rest."""
    runs = _fwd_runs(T, B, H, n_gx, block, layers)
    for k in range(layers):
        h1, c1, _, img1, _ = runs["emit"][k]
        h2, c2, st2, img2, _ = runs["nostash"][k]
        assert torch.equal(h2, h1) and torch.equal(c2, c1)
        assert torch.equal(img2, img1)
        want = _planted_stash(T, B, H, n_gx, runs["ins"][k][0])
        assert torch.equal(st2.view(torch.int32), want.view(torch.int32)), "layer %d: no_stash wrote into gx_stash" % k
        assert (st2[n_gx * B:] == SENTF).all()


# --------------------------------------------------------------------------------------------------------------- BPTT
# (T, B, H, dh_first, block, layers)
BWD_SHAPES = [
    (3, 64, 8, 0, 0, 1),
    (4, 64, 72, 1, 2, 1),         # H % 16 == 8: the last slice's second unit octet does not exist
    (4, 192, 520, 2, 3, 1),       # 3 row groups of two chains
    (3, 128, 520, 0, 0, 1),       # 2 row groups of two chains: the smallest such shape at B = 128
    (3, 64, 1000, 1, 0, 1),
    (2, 64, 1024, 0, 0, 1),       # 4H = 4096: no k padding
    (4, 128, 1000, 1, 2, 2),      # two layers per launch: two chains per workgroup on the XCD-dealt grid
]


@functools.lru_cache(maxsize=None)
def _bwd_runs(T, B, H, dh_first, block, layers):
    """per layer: K = dG of the run without emission; E / S = (stash_dg, image, ld, colpart) with dgp + colpart and skip_dg = 0 / 1"""
    from s2vt_video_caption_amd import capi, ops
    ins = []
    for k in range(layers):
        w, gates, c_all = _bptt_inputs(T, B, H, 400 + 10 * k)
        dh = _r((T - dh_first) * B, H, seed=409 + 10 * k, scale=0.1)
        ins.append((w.to(DEV), dh.to(DEV), c_all.to(DEV), gates.to(DEV)))
    keep = ops.lstm_seq_bwd_persist(T, B, ins[0][0], ins[0][1], dh_first, ins[0][2], ins[0][3], block=block,
                                    second=ins[1] if layers == 2 else None)
    out = {"K": keep if layers == 2 else (keep,), "gates": [i[3] for i in ins]}
    for name, skip in (("E", False), ("S", True)):
        st = [ins[k][3].clone() for k in range(layers)]
        im = [ops.row_plane_image(T * B, 4 * H, DEV, fill=PLANE_SENT, extra_ld=8, extra_rows=64) for _ in range(layers)]
        cp = [torch.full((T * B // 32 + 1, 4 * H), SENTF, device=DEV) for _ in range(layers)]
        ops.lstm_seq_bwd_persist_emit(T, B, ins[0][0], ins[0][1], dh_first, ins[0][2], st[0], dgp=im[0], colpart=cp[0], skip_dg=skip,
                                      block=block, second=ins[1][:3] + (st[1], im[1], cp[1]) if layers == 2 else None)
        out[name] = [(st[k], im[k][0], im[k][1], cp[k]) for k in range(layers)]
    torch.cuda.synchronize()
    capi.check_async_error()
    return out


@pytest.mark.parametrize("T,B,H,dh_first,block,layers", BWD_SHAPES)
def test_bptt_row_image_by_bits(lib, T, B, H, dh_first, block, layers):
    """dgp + colpart set: the fp32 dG unchanged; the images of the keep and the skip_dg run equal, and bit-equal to
    split_planes(dG) on (row < T*B, k < 4H); nothing else written - the k padding [4H, pad64(4H)) is the caller's to zero, so it
    too still holds the sentinel; with skip_dg the stash still holds the activated gates."""
    from s2vt_video_caption_amd import ops
    runs = _bwd_runs(T, B, H, dh_first, block, layers)
    K4, kpad = 4 * H, (4 * H + 63) // 64 * 64
    for k in range(layers):
        dg = runs["K"][k]
        st_e, img_e, ld, _ = runs["E"][k]
        st_s, img_s, _, _ = runs["S"][k]
        assert ld == 3 * kpad + 8 and img_e.shape[0] == T * B + 64
        assert torch.equal(st_e, dg), "layer %d: emission changed the fp32 dG" % k
        assert torch.equal(st_s.view(torch.int32), runs["gates"][k].view(torch.int32)), "layer %d: skip_dg wrote into the stash" % k
        ref, ld0, _ = ops.split_planes(dg)
        _check_image("bptt T=%d B=%d H=%d layer %d" % (T, B, H, k), img_e, ld, T * B, K4, K4, ref, ld0)
        assert torch.equal(img_s, img_e), "layer %d: the image depends on skip_dg" % k
    ns, na, xg = _plan(B, H, layers, True)
    print("bptt T=%d B=%d H=%d x%d: %d chain(s) per workgroup, %d workgroups per layer, XCD groups %d; images bit-equal" % (
        T, B, H, layers, ns, na, xg))


@pytest.mark.parametrize("T,B,H,dh_first,block,layers", BWD_SHAPES)
def test_bptt_column_sums(lib, T, B, H, dh_first, block, layers):
    """colpart[t * (B / 32) + chain] against the fp64 sum of that chain's 32 fp32 dG rows, within 31 * 2^-24 * sum|x| per entry;
    ops.colsum_finish over it against the fp64 column sum of dG within (T*B - 1) * 2^-24 * sum|x|; the same bits with skip_dg; the
    row past the last chain untouched."""
    from s2vt_video_caption_amd import ops
    runs = _bwd_runs(T, B, H, dh_first, block, layers)
    nch = T * B // 32
    for k in range(layers):
        dg = runs["K"][k].cpu().double()
        cp_e, cp_s = runs["E"][k][3], runs["S"][k][3]
        assert torch.equal(cp_e.view(torch.int32), cp_s.view(torch.int32)), "layer %d: colpart depends on skip_dg" % k
        assert (cp_e[nch:] == SENTF).all(), "layer %d: colpart written past row T * B / 32" % k
        chains = dg.view(nch, 32, 4 * H)                # rows t * B + 32 * chain + i  <->  [t * (B / 32) + chain][i]
        err = (cp_e[:nch].cpu().double() - chains.sum(1)).abs()
        bound = 31 * U * chains.abs().sum(1)
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        total = ops.colsum_finish(cp_e[:nch]).cpu().double()
        terr = (total - dg.sum(0)).abs()
        tbound = (T * B - 1) * U * dg.abs().sum(0)
        tratio = (terr / tbound.clamp_min(1e-300)).max().item()
        print("bptt T=%d B=%d H=%d layer %d: colpart max err %.3g, observed / bound %.3f; column total max err %.3g, observed / bound %.4f"
              % (T, B, H, k, err.max().item(), ratio, terr.max().item(), tratio))
        # (<=: the forget gate's dG at t = 0 is dc * c_{-1} * f (1 - f) with c_{-1} = 0 - those sums are zero and must come out as zero)
        assert (bound[:B // 32, H:2 * H] == 0).all() and (tbound > 0).all()
        assert (err <= bound).all(), (k, ratio, (err > bound).nonzero()[0].tolist())
        assert (terr <= tbound).all(), (k, tratio, (terr > tbound).nonzero()[0].tolist())


@pytest.mark.parametrize("B,H", [(64, 72), (128, 520)])
def test_bptt_column_sums_exact_on_integers(lib, B, H):
    """The last step of a BPTT has no recurrent term and no carried dL/dc, so its dG is cell arithmetic alone.  With every
    activated gate 0.5, c_T-1 = 0 (tanh 0 = 0 exactly) and dh = 64 n: dc = dh o = 32 n, dG_i = dc g i (1 - i) = 4 n,
    dG_f = dc c_T-2 f (1 - f) = 8 n c_T-2, dG_g = dc i (1 - g^2) = 12 n, dG_o = 0 - every factor a dyadic rational, every product
    exact, |n| <= 4 and integer |c_T-2| <= 3.  The step's dG rows are then these integers, and its colpart rows their integer
    sums (|sum| <= 32 * 96), exact in fp32 in any order: torch.equal.  (Step 0 of the T = 2 run has tanh(c_0) in it and is not
    looked at here.)"""
    from s2vt_video_caption_amd import ops
    T = 2
    g = torch.Generator().manual_seed(77)
    n = torch.randint(-4, 5, (B, H), generator=g)
    c0 = torch.randint(-3, 4, (B, H), generator=g)
    w = _r(4 * H, H, seed=78, scale=H ** -0.5).to(DEV)
    c_all = torch.cat([c0.float(), torch.zeros(B, H)]).to(DEV)
    stash = torch.full((T * B, 4 * H), 0.5, device=DEV)
    dgp = ops.row_plane_image(T * B, 4 * H, DEV, fill=0)          # (k padding zero, as split_planes leaves it)
    colpart = torch.full((T * B // 32, 4 * H), SENTF, device=DEV)
    ops.lstm_seq_bwd_persist_emit(T, B, w, (64 * n).float().to(DEV), 1, c_all, stash, dgp=dgp, colpart=colpart)
    want = torch.cat([4 * n, 8 * n * c0, 12 * n, torch.zeros_like(n)], dim=1)
    got = stash[B:].cpu()
    assert torch.equal(got, want.float()), "the last step's dG is not the integers the cell arithmetic gives"
    sums = want.view(B // 32, 32, 4 * H).sum(1)
    assert int(sums.abs().max()) <= 32 * 96
    assert torch.equal(colpart[B // 32:].cpu(), sums.float())
    assert torch.equal(ops.split_planes(stash)[0], dgp[0])
    print("bptt integers B=%d H=%d: dG and colpart of the last step exact (max |sum| %d)" % (B, H, int(sums.abs().max())))


def test_shapes_reach_the_planned_forms(lib):
    """The plans the module comment derives from plan_chains / plan_xcd hold on this device (256 resident workgroups): which cases
    run two chains per workgroup and which the XCD-dealt grid.  On a device where this fails the shapes above need another H: the
    smallest that still gives two chains at B = 128."""
    assert lib.s2vt_lstm_seq_x3_workspace_bytes(3, 128, 520) > 0
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 256
    assert _plan(128, 520, 1, False) == (1, 132, 4)
    assert _plan(128, 520, 2, False) == (2, 66, 4)
    assert _plan(128, 504, 2, False)[0] == 1                    # one slice fewer: 128 workgroups fit the half
    assert _plan(128, 1000, 2, False) == (2, 126, 4)
    assert _plan(192, 520, 1, False) == (1, 198, 0)
    assert _plan(64, 1000, 1, False) == (1, 126, 2)
    assert _plan(192, 520, 1, True) == (2, 99, 0)
    assert _plan(128, 520, 1, True) == (2, 66, 2)
    assert _plan(128, 504, 1, True)[0] == 1
    assert _plan(128, 1000, 2, True) == (2, 126, 4)
    assert _plan(64, 8, 1, True) == (1, 2, 2) and _plan(64, 1024, 1, True) == (1, 128, 2)
