"""GPU: which of the nine bf16 plane products each split-precision kernel sums, pinned by value.

An operand is three planes p0 + p1 + p2; the kernels sum the six products (i, j) with i + j <= 2 (plane_ref.KEPT).  Five places
hand-write that list (gemm_x3_kernel NT and TT, logits_argmax_x3_kernel, the persistent forward and BPTT kernels).  Integer operands
in [-4, 4] fill plane 0 only and random data hides a lost third-order product inside the fp32-level tolerances, so:

(a) the GEMM-type kernels read HAND-BUILT images (plane_ref.build_image): any bf16-exact integers in any plane.
      one-hot    plane i of A and plane j of B hold integer matrices, the other four planes zero bits: the result is A_i B_j^T (+ bias,
                 + c0 under accumulate) exactly where (i, j) is kept and exactly the bias / c0 where it is not - all nine (i, j);
      all planes six different integer matrices at once: exactly the sum over KEPT of A_i B_j^T (|sum| <= 6 * 16 * K < 2^24).
(b) the persistent recurrences make their planes inside the launch, so W_hh is made SPARSE instead: every contraction output is one
    product of two full-precision numbers (all three planes of both non-zero), compared with the fp64 product at 2^-21 relative.
    tests/test_plane_ref_host.py proves on the same operand generators that the six products in the kernels' order stay at 0.16 of
    that bound (2^-23.6) while any dropped or mis-paired third-order product leaves it on 59 to 83 % of the elements.

Device figures (MI355X; every bounded case prints observed / bound): (a) is exact everywhere; (b) reaches 0.26 (forward, tanh gate),
0.19 (forward, sigmoid gates) and 0.31 (BPTT) of its bounds - details in the docstrings of the two recurrence tests."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25
PAIRS = [(i, j) for i in range(3) for j in range(3)]


def _ints(g, *shape, lim=4):
    return torch.from_numpy(g.integers(-lim, lim + 1, shape).astype(np.float32))


def _bits(m):
    """bf16 bits of an integer matrix (exact: |m| <= 256)"""
    b = m.bfloat16()
    assert torch.equal(b.float(), m)
    return b.view(torch.int16).numpy().view(np.uint16)


def _image(mats):
    """device image (tensor, ld, kpad) of three [rows, K] integer matrices (None: a plane of zero bits)"""
    rows, K = next(m for m in mats if m is not None).shape
    zero = np.zeros((rows, K), dtype=np.uint16)
    img = P.build_image([zero if m is None else _bits(m) for m in mats])
    return img.to(DEV), img.shape[1], P.pad64(K)


def _one_hot(m, pl):
    return _image([m if q == pl else None for q in range(3)])


def _kept_sum(a, b, mm):
    """sum over KEPT of mm(a[i], b[j]), factored: a0 (b0 + b1 + b2) + a1 (b0 + b1) + a2 b0 - exact in fp32, every partial sum an
    integer below 2^24"""
    return mm(a[0], b[0] + b[1] + b[2]) + mm(a[1], b[0] + b[1]) + mm(a[2], b[0])


# ------------------------------------------------------------------------------------------------------------ gemm_x3, NT form
# (M, N, K, nsplit, one-hot cases too): three k stages with the deferred hi*hi group crossing a stage; the prologue alone; split-K;
# a persistent launch whose workgroups walk several tiles, the deferred group crossing a tile boundary (all-planes case only)
NT_SHAPES = [(300, 77, 192, 0, True), (333, 77, 64, 0, True), (4100, 1000, 2048, 3, True), (6001, 2900, 192, 0, False)]


@pytest.mark.parametrize("M,N,K,ns,one_hot", NT_SHAPES)
def test_gemm_x3_nt_sums_exactly_the_six_kept_products(lib, M, N, K, ns, one_hot):
    """ops.gemm_planes on hand-built images under s2vt_gemm_tune(3, tile_rows, nsplit) for every tile height (0: the launcher's
    choice), with bias and with accumulate: torch.equal against the integer reference."""
    from s2vt_video_caption_amd import capi, ops
    g = np.random.default_rng(M + N + K)
    a, b = [_ints(g, M, K) for _ in range(3)], [_ints(g, N, K) for _ in range(3)]
    bias, c0 = _ints(g, N, lim=8), _ints(g, M, N, lim=8)
    mm = lambda x, y: x @ y.t()
    cases = [("all planes", _image(a), _image(b), _kept_sum(a, b, mm))]
    if one_hot:
        prod = mm(a[0], b[0])
        ia, ib = [_one_hot(a[0], i) for i in range(3)], [_one_hot(b[0], j) for j in range(3)]
        cases += [("plane %d x plane %d" % (i, j), ia[i], ib[j], prod if P.KEPT[(i, j)] else torch.zeros(M, N)) for i, j in PAIRS]
    assert all(c[3].abs().max() < 2 ** 24 for c in cases)
    bias_d, c0_d = bias.to(DEV), c0.to(DEV)
    ws = torch.empty(4 * M * N + 1, device=DEV)
    try:
        for tile_rows in (0, 128, 192, 256):
            lib.s2vt_gemm_tune(3, tile_rows, ns)
            for tag, pa, pb, ref in cases:
                ref_d = ref.to(DEV)
                got = ops.gemm_planes(pa, pb, M, N, bias=bias_d, splitk_ws=ws)
                assert torch.equal(got, ref_d + bias_d), (tag, tile_rows, "bias", int((got != ref_d + bias_d).sum()))
                out = c0_d.clone()
                ops.gemm_planes(pa, pb, M, N, out=out, accumulate=True, splitk_ws=ws)
                assert torch.equal(out, ref_d + c0_d), (tag, tile_rows, "accumulate", int((out != ref_d + c0_d).sum()))
        torch.cuda.synchronize()
        capi.check_async_error()
    finally:
        lib.s2vt_gemm_tune(3, 0, 0)


# ------------------------------------------------------------------------------------------------------------ gemm_x3, TT form
@pytest.mark.parametrize("K,M,N", [(192, 300, 77), (640, 1003, 517)])
def test_gemm_x3_tt_sums_exactly_the_six_kept_products(lib, K, M, N):
    """ops.gemm_planes_tt: C = X_A^T X_B from hand-built ROW images of X_A [K + 64, M] and X_B [K + 64, N], read transposed, for
    tile_rows 0 / 128 / 256: rows [0, K) with bias, and rows [64, 64 + K) - the operand pointers advanced by one 64-row block - with
    accumulate."""
    from s2vt_video_caption_amd import capi, ops
    g = np.random.default_rng(K + M)
    xa, xb = [_ints(g, K + 64, M) for _ in range(3)], [_ints(g, K + 64, N) for _ in range(3)]
    bias, c0 = _ints(g, N, lim=8), _ints(g, M, N, lim=8)
    bias_d, c0_d = bias.to(DEV), c0.to(DEV)
    runs = ((0, dict(bias=bias_d), bias_d), (64, dict(accumulate=True), c0_d))

    def wants(ma, mb):
        """expected results of the two runs (k rows [0, K) + bias, k rows [64, 64 + K) + c0), on the device"""
        refs = [_kept_sum([m[off:off + K] for m in ma], [m[off:off + K] for m in mb], lambda x, y: x.t() @ y) for off, _, _ in runs]
        assert all(r.abs().max() < 2 ** 24 for r in refs)
        return [r.to(DEV) + add for r, (_, _, add) in zip(refs, runs)]
    cases = [("all planes", _image(xa), _image(xb), wants(xa, xb))]
    ia, ib = [_one_hot(xa[0], i) for i in range(3)], [_one_hot(xb[0], j) for j in range(3)]
    # one-hot: X_A[0] in plane i, X_B[0] in plane j - one product where (i, j) is kept, nothing but the bias / c0 where it is not
    kept = wants([xa[0]] + [torch.zeros_like(xa[0])] * 2, [xb[0]] + [torch.zeros_like(xb[0])] * 2)
    lost = [bias_d.expand(M, N), c0_d]
    for i, j in PAIRS:
        cases.append(("plane %d x plane %d" % (i, j), ia[i], ib[j], kept if P.KEPT[(i, j)] else lost))
    ws = torch.empty(8 * M * N + 1, device=DEV)
    try:
        for tile_rows in (0, 128, 256):
            lib.s2vt_gemm_tune(3, tile_rows, 0)
            for tag, pa, pb, want2 in cases:
                for (off, kw, _), want in zip(runs, want2):
                    out = c0_d.clone() if off else None
                    got = ops.gemm_planes_tt((pa[0][off:], pa[1], pa[2]), (pb[0][off:], pb[1], pb[2]), M, N, K, out=out, splitk_ws=ws, **kw)
                    assert torch.equal(got, want), (tag, tile_rows, off, int((got != want).sum()))
        torch.cuda.synchronize()
        capi.check_async_error()
    finally:
        lib.s2vt_gemm_tune(3, 0, 0)


# ------------------------------------------------------------------------------------------------------------ logits_argmax_x3
def _first_max(ref):
    best = ref.max(dim=1, keepdim=True).values
    col = torch.arange(ref.shape[1]).expand_as(ref)
    return best[:, 0], torch.where(ref == best, col, ref.shape[1]).min(dim=1).values


# the 2, 4, 6 and 10 k32-stage forms of test_gpu_decode_forms.py (pad64(H) = 64 / 128 / 192 / 320)
@pytest.mark.parametrize("H,B,M2,V", [(44, 37, 61, 61), (100, 130, 400, 61), (192, 65, 61, 130), (300, 64, 176, 130)])
def test_argmax_x3_sums_exactly_the_six_kept_products(lib, H, B, M2, V):
    """ops.argmax_x3_planes on hand-built images of h [B, H], W [V, H] and W2 [M2, H], both roles in one launch: z = h W2^T as a full
    matrix, exact; the packed score equal to the row maximum of h W^T + bias and the id the LOWEST index that attains it.  Where
    (i, j) is not kept the logits are exactly the bias (integers in [-8, 8]: ties in every row) and z is exactly zero."""
    from s2vt_video_caption_amd import capi, ops
    g = np.random.default_rng(H + B)
    h, w, w2 = ([_ints(g, r, H) for _ in range(3)] for r in (B, V, M2))
    bias = _ints(g, V, lim=8)
    mm = lambda x, y: x @ y.t()
    cases = [("all planes", _image(h), _image(w), _image(w2), _kept_sum(h, w, mm), _kept_sum(h, w2, mm))]
    ih, iw, iw2 = ([_one_hot(m[0], q) for q in range(3)] for m in (h, w, w2))
    for i, j in PAIRS:
        kept = P.KEPT[(i, j)]
        cases.append(("plane %d x plane %d" % (i, j), ih[i], iw[j], iw2[j], mm(h[0], w[0]) if kept else torch.zeros(B, V),
                      mm(h[0], w2[0]) if kept else torch.zeros(B, M2)))
    bias_d = bias.to(DEV)
    ldz = (M2 + 3) // 4 * 4 + 4
    for tag, ph, pw, pw2, lref, zref in cases:
        z = torch.full((B + 3, ldz), SENT, device=DEV)
        packed, _ = ops.argmax_x3_planes(pw, ph, B, V, bias=bias_d, pw2=pw2, M2=M2, z=z)
        torch.cuda.synchronize()
        zc, packed = z.cpu(), packed.cpu()
        assert (zc[B:] == SENT).all() and (zc[:, M2:] == SENT).all(), tag
        assert torch.equal(zc[:B, :M2], zref), (tag, int((zc[:B, :M2] != zref).sum()))
        best, first = _first_max(lref + bias)
        assert torch.equal(ops.packed_score(packed), best), tag
        assert torch.equal(0xFFFFFFFF - (packed & 0xFFFFFFFF), first), tag
    capi.check_async_error()


# ------------------------------------------------------------------------------------------------------------ persistent forward
def _sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-v))


@pytest.mark.parametrize("B,H", [(64, 72), (64, 520), (64, 1024)])
def test_persistent_forward_single_term_contraction(lib, B, H):
    """ops.lstm_seq_fwd_persist, T = 2, n_gx = 2.  Row col of W_hh has ONE non-zero w (|w| in [4, 16], three non-zero planes) at
    k(col) = (col % 64 + 64 s) % H, s = 0 .. ceil(H / 64) - 1, so every column slice meets every k (H = 1024: all four k quarters and
    the hand-written k16 step 15).  A first run with gx_1 = 0 gives h_0 (dense; bitwise repeatable).  With p = h_0[b][k(col)] * w in
    fp64 and gx_1 = -fp32(p) the second run's pre-activation gx_1 + acc (one fp32 add; the other three waves' partial sums are exact
    zeros) is the contraction's own error, seen through the activations at 0:
        |g - tanh(ref)| <= 2^-21 |p| + a   on the tanh gate,    |gate - sigmoid(ref)| <= 2^-23 |p| + a   on i, f, o,
    ref = fp64(gx_1) + p, a = 4e-7 for the activations' absolute error (common.h claims ~1.5e-7).  Host emulation of the six
    products: <= 0.15 of these bounds; a lost third-order product: 59 to 73 % of the elements over them (test_plane_ref_host.py).
    Observed on an MI355X (worst observed / bound over all shifts): tanh gate 0.198 / 0.242 / 0.256 and sigmoid gates 0.162 / 0.191 /
    0.190 at H = 72 / 520 / 1024.  The bounds stand as first set: neither a nor the 2^-21 was raised."""
    from s2vt_video_caption_amd import capi, ops
    T = 2
    bias = torch.zeros(4 * H, device=DEV)
    tanh_cols = np.zeros(4 * H, dtype=bool)
    tanh_cols[2 * H:3 * H] = True
    h0 = None
    worst_t = worst_s = 0.0
    for s in range(-(-H // 64)):
        gx0, W, w, k = P.fwd_single_term(B, H, s)
        assert all(((p & 0x7FFF) != 0).all() for p in P.split3(w)) and ((W != 0).sum(axis=1) == 1).all()
        Wd = torch.from_numpy(W).to(DEV)
        gx = torch.zeros(T * B, 4 * H)
        gx[:B] = torch.from_numpy(gx0)
        if h0 is None:
            h0 = ops.lstm_seq_fwd_persist(T, B, gx.to(DEV), 2, bias, Wd)[0][:B].cpu()
            assert (h0 != 0).all()
        p = h0.numpy()[:, k].astype(np.float64) * w.astype(np.float64)
        gx1 = (-p).astype(np.float32)
        gx[B:] = torch.from_numpy(gx1)
        h_all, _, gates = ops.lstm_seq_fwd_persist(T, B, gx.to(DEV), 2, bias, Wd)
        assert torch.equal(h_all[:B].cpu(), h0)
        got = gates[B:].cpu().numpy().astype(np.float64)
        ref = gx1.astype(np.float64) + p
        et = (np.abs(got - np.tanh(ref)) / (2.0 ** -21 * np.abs(p) + P.ACT_ABS))[:, tanh_cols]
        es = (np.abs(got - _sigmoid64(ref)) / (2.0 ** -23 * np.abs(p) + P.ACT_ABS))[:, ~tanh_cols]
        print("forward B=%d H=%d shift %d: tanh gate observed/bound max %.3f; sigmoid gates %.3f; max |p| %.3g" % (
            B, H, s, et.max(), es.max(), np.abs(p).max()))
        worst_t, worst_s = max(worst_t, et.max()), max(worst_s, es.max())
        assert et.max() <= 1.0, (s, np.argwhere(et > 1)[:4].tolist())
        assert es.max() <= 1.0, (s, np.argwhere(es > 1)[:4].tolist())
    print("forward B=%d H=%d: worst observed/bound: tanh %.3f, sigmoid %.3f" % (B, H, worst_t, worst_s))
    capi.check_async_error()


# ------------------------------------------------------------------------------------------------------------ persistent BPTT
@pytest.mark.parametrize("B,H", [(64, 72), (64, 520), (128, 520)])
def test_persistent_bptt_single_term_contraction(lib, B, H):
    """ops.lstm_seq_bwd_persist, T = 2, dh_first = 1.  Column j of W_hh has ONE non-zero w (|w| in [0.5, 2], three non-zero planes) at
    row col(j); step 1 has a dense random dh_out, random gates and c_1, and its dG_1 - read back from the result - is the operand:
    dh_0[b][j] = dG_1[b][col(j)] * w, one product (the other producers' partial blocks are exact zeros).  Step 0 is an exact gadget:
    c_0 = 20 makes tanhf_(20) = 1 - 2 / (1 + __expf(40)) = 1.0f exactly and o_0 = 0.5 gives dG_0[b][3H + j] = 0.25 * dh_0[b][j] bit for
    bit, whatever dc carries.  Asserted: |4 dG_0[b][3H + j] - dG_1[b][col(j)] w| <= 2^-21 |product| over 16 shifts of col(j), which
    between them use every one of the 4H gate columns (asserted).  (128, 520): two chains per workgroup.  Host emulation: 2^-23.6,
    0.16 of the bound; a lost third-order product: 75 to 83 % of the elements over it (test_plane_ref_host.py).
    Observed on an MI355X (worst observed / bound over the 16 shifts): 0.283 at (64, 72), 0.311 at (64, 520), 0.307 at (128, 520),
    i.e. a relative error of at most 2^-22.7 - the emulation's 2^-23.6 plus the matrix core's own accumulate rounding.  The bound
    stands at 2^-21: the fall-back to 2^-19 was not used."""
    from s2vt_video_caption_amd import capi, ops
    T = 2
    g = torch.Generator().manual_seed(90 + H)
    r = lambda *shape: torch.randn(*shape, generator=g)
    gates = torch.sigmoid(r(T * B, 4 * H))
    gates[:, 2 * H:3 * H] = torch.tanh(r(T * B, H))
    gates[:B, 3 * H:] = 0.5
    c_all = r(T * B, H) * 0.7
    c_all[:B] = 20.0
    dh = r(B, H) * 0.1
    gates_d, c_d, dh_d = gates.to(DEV), c_all.to(DEV), dh.to(DEV)
    used = np.zeros(4 * H, dtype=int)
    worst, dg1_first = 0.0, None
    for s in range(P.bwd_nshifts(H)):
        W, w, col = P.bwd_single_term(H, s)
        assert all(((p & 0x7FFF) != 0).all() for p in P.split3(w)) and ((W != 0).sum(axis=0) == 1).all()
        used[col] += 1
        dG = ops.lstm_seq_bwd_persist(T, B, torch.from_numpy(W).to(DEV), dh_d, 1, c_d, gates_d).cpu().numpy()
        dg1, dgo0 = dG[B:], dG[:B, 3 * H:]
        if dg1_first is None:
            dg1_first = dg1.copy()
            assert (dg1 != 0).mean() > 0.99
        assert np.array_equal(dg1, dg1_first)                              # step 1 takes nothing from W_hh
        prod = dg1[:, col].astype(np.float64) * w.astype(np.float64)
        err = np.abs(4.0 * dgo0.astype(np.float64) - prod)
        ratio = np.divide(err, P.BOUND_REL * np.abs(prod), out=np.where(err > 0, np.inf, 0.0), where=prod != 0)
        print("bptt B=%d H=%d shift %d: observed/bound max %.3f (max relative error 2^%.1f)" % (
            B, H, s, ratio.max(), np.log2(max(ratio.max() * P.BOUND_REL, 1e-300))))
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1.0, (s, np.argwhere(ratio > 1)[:4].tolist())
    assert used.min() >= 1 and all(used[q * H:(q + 1) * H].min() >= 1 for q in range(4))
    print("bptt B=%d H=%d: worst observed/bound %.3f" % (B, H, worst))
    capi.check_async_error()
