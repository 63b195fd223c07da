"""GPU: the forms of the step and arg-max kernels that only the decode drivers and the beam plane-path step fill in
(api_decode.hip: decode_fused, decode_two_chains; api_beam.hip), one launch at a time and by VALUE - whole decodes assert token ids,
which a shifted pre-activation rarely moves:

  the fused step with a per-token gate table, shared gate-input rows (gx_idx) and h_t written as blocked bf16 planes
      (lstm_step_fwd_kernel / lstm_step_fwd_gemv_kernel with StepFwdArgs::gx_tab / gx_idx / h_planes);
  the contraction-only step (z_out) followed by lstm_cell_pointwise_kernel<4> / <1>;
  the second role of logits_argmax_x3_kernel (W2 / M2 / z / v_off), alone and beside the logits;
  the beam plane-path depth step (s2vt_beam_step_cached) through its existing entry point.

References are int64 / fp64 torch on the CPU.  Integer-valued data where a sum is exact in any order (torch.equal); otherwise the
project's own tolerances and nothing wider - the tile step's 2e-6 (h, stash) / 4e-6 (c) of test_lstm_step_fwd_matches_cell, the
GEMV step's 4e-6, the split-precision contraction's 4e-6 * max|ref| + 1e-6 of test_split_precision_gemm_blocked_planes - and sums
of them where two of those kernels run in a row.  Every case prints its observed maximum against its bound."""
import contextlib
import ctypes
import functools

import pytest
import torch

from oracle import s2vt_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25                       # z rows / columns no launch may write
PLANE_SENT = 0x7FFF                  # a bf16 NaN pattern: split3 never produces it


def _ints(*shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _x3_bound(ref):
    """the split-precision contraction's bound (test_split_precision_gemm_blocked_planes)"""
    return 4e-6 * ref.abs().max().item() + 1e-6


def _ids(packed):
    return 0xFFFFFFFF - (packed & 0xFFFFFFFF)


def _first_max(ref):
    """(row maximum, lowest index that attains it)"""
    best = ref.max(dim=1, keepdim=True).values
    col = torch.arange(ref.shape[1]).expand_as(ref)
    return best[:, 0], torch.where(ref == best, col, ref.shape[1]).min(dim=1).values


@contextlib.contextmanager
def _options(lib, **kv):
    prev = {k: lib.s2vt_set_option(k.encode(), v) for k, v in kv.items()}
    assert all(v != -(2 ** 31) for v in prev.values()), "unknown option"
    try:
        yield
    finally:
        for k, v in prev.items():
            lib.s2vt_set_option(k.encode(), v)


# ------------------------------------------------------------------------------------------------ (a), (b): the z role of argmax_x3
# (H, B, M2, V).  pad64(H) = 64 / 128 / 192 / 320: 2, 4, 6 and 10 k32 stages - the ring's prologue alone, the tail loop alone, one
# and three trips of the steady loop.  B = 37 / 64: NB = 1; 65 / 130: NB = 2 with two batch tiles at 130 (the second: 2 rows and a
# clamped h block).  M2 = 61: the scalar tail of the 16-byte z store; 176 / 400: a partial last 64-row block.  V: the logits' blocks.
Z_SHAPES = [(44, 37, 61, 61), (44, 65, 176, 130), (100, 64, 64, 64), (100, 130, 400, 61), (192, 37, 400, 130), (192, 130, 61, 64),
            (300, 65, 64, 61), (300, 64, 176, 130), (300, 130, 400, 64), (44, 64, 400, 64), (100, 37, 176, 61), (192, 65, 61, 130)]


@functools.lru_cache(maxsize=None)
def _z_case(H, B, M2, V, integers, hmax=64):
    """(h, W2, W, bias) on the CPU and the int64 / fp64 references (z, logits) as fp64"""
    if integers:
        # |h| <= 64 and |W| <= 512 fit two bf16 planes, so every kept plane product is exact; |sum| <= 64 * 512 * 320 + 100 < 2^24
        # (hmax = 512 at K = 64: h needs its second plane too, and 512 * 512 * 44 + 100 is still below 2^24)
        h, w2 = _ints(B, H, seed=1, lo=-hmax, hi=hmax), _ints(M2, H, seed=2, lo=-512, hi=512)
        w, bias = _ints(V, H, seed=3, lo=-512, hi=512), _ints(V, seed=4, lo=-100, hi=100)
        # planted ties: vocabulary row V // 2 + i repeats row i, so EVERY batch row's maximum is attained twice (for V = 130 in two
        # different 64-row blocks, i.e. by two workgroups' atomics) unless it falls on an unpaired last row
        half = V // 2
        w[half:2 * half] = w[:half]
        bias[half:2 * half] = bias[:half]
        zref = (h.long() @ w2.long().t()).double()
        lref = (h.long() @ w.long().t() + bias.long()).double()
        assert zref.abs().max() < 2 ** 24 and lref.abs().max() < 2 ** 24
    else:
        h, w2 = _r(B, H, seed=1, scale=0.5), _r(M2, H, seed=2, scale=H ** -0.5)
        w, bias = _r(V, H, seed=3, scale=H ** -0.5), _r(V, seed=4)
        zref = h.double() @ w2.double().t()
        lref = h.double() @ w.double().t() + bias.double()
    return h, w2, w, bias, zref, lref


def _z_launches(H, B, M2, V, integers, sample=None, hmax=64):
    """The three launches of one shape: the z role alone, the logits alone (M2 = 0), both.  Asserts what must hold bit for bit between
    them and returns (z [B, M2], packed of the logits-only launch), both on the CPU."""
    from s2vt_video_caption_amd import ops
    h, w2, w, bias, _, _ = _z_case(H, B, M2, V, integers, hmax)
    pw, ph, pw2 = ops.split_planes(w.to(DEV)), ops.split_planes(h.to(DEV)), ops.split_planes(w2.to(DEV))
    assert pw[2] == ph[2] == pw2[2] == (H + 63) // 64 * 64
    bias_d = bias.to(DEV)
    ldz = (M2 + 3) // 4 * 4 + 4                                         # > M2, rows 16-byte aligned
    pattern = (torch.arange(B, dtype=torch.int64) * 0x0123456789AB + 0x7E57).to(DEV)
    # the z role alone: packed must come back untouched
    z_only = torch.full((B + 3, ldz), SENT, device=DEV)
    packed = pattern.clone()
    ops.argmax_x3_planes(pw, ph, B, V, bias=bias_d, packed=packed, pw2=pw2, M2=M2, z=z_only, with_logits=False)
    assert torch.equal(packed, pattern), "the z role wrote packed words"
    z_only = z_only.cpu()
    assert (z_only[B:] == SENT).all(), "z rows past B were written"
    assert (z_only[:, M2:] == SENT).all(), "z columns past M2 were written"
    # the logits alone, then both roles in one launch: ids and scores bit-equal, z bit-equal (sentinels included)
    packed0, _ = ops.argmax_x3_planes(pw, ph, B, V, bias=bias_d, sample=sample)
    z_both = torch.full((B + 3, ldz), SENT, device=DEV)
    packed1, _ = ops.argmax_x3_planes(pw, ph, B, V, bias=bias_d, pw2=pw2, M2=M2, z=z_both, sample=sample)
    assert torch.equal(packed1, packed0), "the logits differ beside the z role"
    assert torch.equal(z_both.cpu(), z_only), "z differs beside the logits"
    return z_only[:B, :M2], packed0.cpu()


@pytest.mark.parametrize("H,B,M2,V", Z_SHAPES)
def test_argmax_x3_z_role_exact_on_integers(lib, H, B, M2, V):
    """(a) z = h·W2^T and the logits on integer data: every sum is exact, so z equals the int64 product, the packed score equals the
    int64 row maximum and the id is the LOWEST index that attains it (every maximum is planted twice)."""
    from s2vt_video_caption_amd import ops
    _, _, _, _, zref, lref = _z_case(H, B, M2, V, True)
    z, packed = _z_launches(H, B, M2, V, True)
    assert torch.equal(z, zref.float())
    best, first = _first_max(lref)
    tied = ((lref == best[:, None]).sum(dim=1) > 1).sum().item()
    assert tied >= B // 2, tied                                         # (an unpaired last row may win some batch rows)
    assert torch.equal(_ids(packed), first)
    assert torch.equal(ops.packed_score(packed), best.float())
    print("z role, integers H=%d B=%d M2=%d V=%d: exact; %d of %d rows tied at the maximum" % (H, B, M2, V, tied, B))


@pytest.mark.parametrize("H,B,M2,V", [s for s in Z_SHAPES if s[0] == 44])
def test_argmax_x3_z_role_exact_with_two_planes_of_h(lib, H, B, M2, V):
    """Beyond (a): with |h| <= 64 the second plane of h is zero and the products W plane x h plane 1 never count.  At K = 64 the sums
    stay exact with |h| <= 512 too, where both operands need two planes: all four products of planes 0 and 1 are pinned."""
    from s2vt_video_caption_amd import ops
    h, _, _, _, zref, lref = _z_case(H, B, M2, V, True, 512)
    assert (h.bfloat16().float() != h).any()                            # (the first plane alone does not hold h)
    z, packed = _z_launches(H, B, M2, V, True, hmax=512)
    assert torch.equal(z, zref.float())
    best, first = _first_max(lref)
    assert torch.equal(_ids(packed), first)
    assert torch.equal(ops.packed_score(packed), best.float())


@pytest.mark.parametrize("H,B,M2,V", Z_SHAPES)
def test_argmax_x3_z_role_random_against_fp64(lib, H, B, M2, V):
    """(b) the same launches on random data against fp64 at the split-precision contraction's bound; the packed score is the row
    maximum of the logits within the same bound (a maximum moves by no more than its operands), the id is fp64's wherever the top-2
    margin exceeds twice that bound."""
    from s2vt_video_caption_amd import ops
    _, _, _, _, zref, lref = _z_case(H, B, M2, V, False)
    z, packed = _z_launches(H, B, M2, V, False)
    zerr, ztol = (z.double() - zref).abs().max().item(), _x3_bound(zref)
    top2 = lref.topk(2, dim=1).values
    serr, stol = (ops.packed_score(packed).double() - top2[:, 0]).abs().max().item(), _x3_bound(lref)
    print("z role, random H=%d B=%d M2=%d V=%d: max |z - fp64| = %.3g of %.3g (%.2f); score %.3g of %.3g (%.2f)" %
          (H, B, M2, V, zerr, ztol, zerr / ztol, serr, stol, serr / stol))
    assert zerr < ztol
    assert serr < stol
    safe = (top2[:, 0] - top2[:, 1]) > 2 * stol
    assert safe.sum() > B // 2
    assert torch.equal(_ids(packed)[safe], lref.argmax(dim=1)[safe])


@pytest.mark.parametrize("H,B,M2,V", [(100, 37, 176, 61), (44, 65, 176, 130)])
def test_argmax_x3_z_role_beside_a_draw(lib, H, B, M2, V):
    """The sampling instantiations (NB = 1 / 2) carry the second role too: beside a draw z is the z-only launch's, bit for bit, and
    the drawn words are those of the launch without a second image (both asserted inside _z_launches)."""
    _, _, _, _, zref, _ = _z_case(H, B, M2, V, False)
    z, packed = _z_launches(H, B, M2, V, False, sample=(0.7, 20261, 3, 0))
    assert (z.double() - zref).abs().max().item() < _x3_bound(zref)
    assert ((_ids(packed) >= 0) & (_ids(packed) < V)).all()


# ------------------------------------------------------------------------------------------------ (c), (d): the table step
STEP_V, STEP_G = 50, 3
# (B, H): the 16-row tile; the 16-row tile with two row tiles; the ragged 32-row tile (33 = 32 + 1) over two k blocks of planes;
# exactly one 64-row block of the image; two 64-row blocks (70).  H = 44, 36, 100: H % 8 = 4, a partly filled 16-byte slot.
STEP_SHAPES = [(5, 44), (17, 36), (33, 100), (64, 64), (70, 44)]


@functools.lru_cache(maxsize=None)
def _step_case(B, H):
    """inputs of one table step on the CPU: w_hh, gx [G, 4H], gx_idx (every row of gx used, rows repeated), gtab as the left 4H
    columns of a wider tensor, h0, c0 with |c0| <= 1, tok (both ends of the table)"""
    g = torch.Generator().manual_seed(100 * B + H)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5
    gx = _r(STEP_G, 4 * H, seed=2)
    gx_idx = torch.randint(0, STEP_G, (B,), generator=g, dtype=torch.int32)
    gx_idx[:3] = torch.tensor([2, 0, 1], dtype=torch.int32)
    gtab_wide = _r(STEP_V, 4 * H + 8, seed=3, scale=0.5)
    h0, c0 = _r(B, H, seed=4, scale=0.5), _r(B, H, seed=5).clamp_(-1.0, 1.0)
    tok = torch.randint(0, STEP_V, (B,), generator=g, dtype=torch.int32)
    tok[0], tok[1] = STEP_V - 1, 0
    return dict(w_hh=w_hh, gx=gx, gx_idx=gx_idx, gtab_wide=gtab_wide, h0=h0, c0=c0, tok=tok)


def _cell64(pre, c_prev):
    i, f, g, o = pre.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], dim=1)


def _step_ref(case, tok, z=None, c_prev=None):
    """fp64 (h, c, stash) of the step for the tokens `tok`; z: the recurrent half if it is not h0·W_hh^T"""
    H = case["w_hh"].shape[1]
    z = case["h0"].double() @ case["w_hh"].double().t() if z is None else z
    pre = case["gx"].double()[case["gx_idx"].long()] + case["gtab_wide"].double()[tok.long(), :4 * H] + z
    return _cell64(pre, (case["c0"] if c_prev is None else c_prev).double())


def _to_dev(case, c_offset=0):
    d = {k: v.to(DEV) for k, v in case.items()}
    H = case["w_hh"].shape[1]
    d["gtab"] = d["gtab_wide"][:, :4 * H]
    if c_offset:                          # c_prev as a view `c_offset` floats into its storage: rows no longer 16-byte aligned
        B = case["c0"].shape[0]
        store = torch.zeros(B * H + c_offset, device=DEV)
        store[c_offset:] = d["c0"].reshape(-1)
        d["c0"] = store[c_offset:].view(B, H)
        assert d["c0"].data_ptr() % 16 != 0
    return d


def _token_sources(tok):
    """the three token sources of TokenSrc with the ids they name"""
    packed = ((torch.arange(tok.numel(), dtype=torch.int64) + 1234) << 32) | (0xFFFFFFFF - tok.long())
    return (("tok", dict(tok=tok.to(DEV)), tok), ("packed", dict(tok_packed=packed.to(DEV)), tok),
            ("const", dict(tok_const=9), torch.full_like(tok, 9)))


def _plane_index(B, H, ld):
    """flat element index of (b, unit, plane) in a blocked 3-plane image of row stride ld (step_frame.h: store_h_planes)"""
    b, u, pl = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None], torch.arange(3)[None, None, :]
    return (b // 64) * (64 * ld) + (u // 16) * 3072 + (pl * 2 + (u // 8) % 2) * 512 + (b % 64) * 8 + u % 8


def _fused(d, src, fill=0, extra_ld=0):
    from s2vt_video_caption_amd import ops
    B, H = d["h0"].shape
    img = ops.h_plane_image(B, H, DEV, fill=fill, extra_ld=extra_ld)
    h, c, st = ops.lstm_step_fwd_table(d["w_hh"], d["h0"], d["c0"], gx=d["gx"], gx_idx=d["gx_idx"], gtab=d["gtab"], want_stash=True,
                                       h_planes=img, **src)
    return h, c, st, img[0]


def _two_launches(d, src, z=None):
    """the contraction-only step, then the stand-alone cell update on its z"""
    from s2vt_video_caption_amd import ops
    B, H = d["h0"].shape
    if z is None:
        z = torch.full((B + 2, 4 * H + 4), SENT, device=DEV)
        ops.lstm_step_contract(d["w_hh"], d["h0"], z=z)
    img = ops.h_plane_image(B, H, DEV, fill=0)
    h, c, st = ops.lstm_cell_pointwise(z, H, d["c0"], gx=d["gx"], gx_idx=d["gx_idx"], gtab=d["gtab"], want_stash=True, h_planes=img, B=B,
                                       **src)
    return h, c, st, img[0], z


def _check_step(tag, got, want, tols):
    from s2vt_video_caption_amd import capi
    torch.cuda.synchronize()
    capi.check_async_error()
    for name, g, w, tol in zip(("h", "c", "stash"), got, want, tols):
        err = (g.cpu().double() - w).abs().max().item()
        print("%s: max |%s - fp64| = %.3g of %.3g (%.2f)" % (tag, name, err, tol, err / tol))
        assert err < tol, (tag, name, err)


@pytest.mark.parametrize("B,H,gemv", [(b, h, 0) for b, h in STEP_SHAPES] + [(5, 44, 2)])
def test_table_step_against_the_fp64_cell_and_its_plane_image(lib, B, H, gemv):
    """(c) lstm_step_fwd with gx_tab + gx_idx + h_planes - the 16- and 32-row MFMA tiles, and for B <= 8 the GEMV kernel (option gemv
    = 2: lstm_step_fwd_gemv_ok holds at B = 5, H = 44) - against the fp64 cell for every token source; an id == V raises IndexError and its row runs with table row 0.  The plane
    image: bit-equal to ops.split_planes of the kernel's own h_out (the split itself against a host split: test_gpu_plane_split.py), and into a sentinel-filled image of a wider row stride exactly
    the elements of (b < B, unit < H) are written, with the same bits."""
    from s2vt_video_caption_amd import capi, ops
    case = _step_case(B, H)
    d = _to_dev(case)
    tols = (4e-6, 4e-6, 4e-6) if gemv else (2e-6, 4e-6, 2e-6)
    kpad = (H + 63) // 64 * 64
    with _options(lib, gemv=gemv):
        for name, src, ids in _token_sources(case["tok"]):
            h, c, st, img = _fused(d, src)
            _check_step("table step B=%d H=%d gemv=%d %s" % (B, H, gemv, name), (h, c, st), _step_ref(case, ids), tols)
            assert torch.equal(img, ops.split_planes(h)[0]), name
            h2, c2, st2, img2 = _fused(d, src, fill=PLANE_SENT, extra_ld=8)
            assert torch.equal(h2, h) and torch.equal(c2, c) and torch.equal(st2, st)
            inside, inside0 = _plane_index(B, H, 3 * kpad + 8).flatten(), _plane_index(B, H, 3 * kpad).flatten()
            flat = img2.cpu().flatten()
            assert torch.equal(flat[inside], img.cpu().flatten()[inside0]), name
            outside = torch.ones(flat.numel(), dtype=torch.bool)
            outside[inside] = False
            assert (flat[outside] == PLANE_SENT).all(), "%s: the step wrote plane elements outside (b < B, unit < H)" % name
        # an id beyond the table: flagged, and the row is computed with table row 0
        bad = case["tok"].clone()
        bad[2] = STEP_V
        hb, cb, stb, _ = _fused(d, dict(tok=bad.to(DEV)))
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
        bad[2] = 0
        _check_step("table step B=%d H=%d gemv=%d id == V" % (B, H, gemv), (hb, cb, stb), _step_ref(case, bad), tols)
        h4, _, _, _ = _fused(d, dict(tok=case["tok"].to(DEV)))            # the flag does not stick
        torch.cuda.synchronize()
        capi.check_async_error()


def _ulps(a, b):
    ia, ib = a.cpu().contiguous().view(torch.int32).long(), b.cpu().contiguous().view(torch.int32).long()
    key = lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(ia) - key(ib)).abs().max().item()


# (B, H, c_prev offset in floats): lstm_cell_pointwise_kernel<4> wherever H % 4 == 0 and every row is 16-byte aligned; <1> at H = 30
# (H % 4 != 0) and at H = 44 with c_prev one float into its storage.  Threads: B * H / 4 = 55, 153, 825, 1024, 770 (one launch
# with a whole number of 256-thread blocks, four without); B * H = 990 and 3080 for <1>.
POINTWISE_SHAPES = [(b, h, 0) for b, h in STEP_SHAPES] + [(33, 30, 0), (70, 44, 1)]


@pytest.mark.parametrize("B,H,c_offset", POINTWISE_SHAPES)
def test_contraction_then_pointwise_is_the_fused_step_in_bits(lib, B, H, c_offset):
    """(d) kernels.h: the contraction-only step followed by lstm_cell_pointwise performs "the same additions in the same order" as
    the fused step - h, c, the gate stash and the plane image must be torch.equal, for every token source and for a flagged id.  The
    contraction writes z [B, 4H] and nothing around it; z itself against fp64 at the tile step's 2e-6."""
    from s2vt_video_caption_amd import capi
    case = _step_case(B, H)
    d = _to_dev(case, c_offset)
    with _options(lib, gemv=0):
        z = None
        for name, src, _ in _token_sources(case["tok"]):
            fused = _fused(d, src)
            *pair, z = _two_launches(d, src, z)
            torch.cuda.synchronize()
            capi.check_async_error()
            for what, a, b in zip(("h", "c", "stash", "planes"), fused, pair):
                assert torch.equal(a, b), "B=%d H=%d %s: %s differs from the fused step by up to %s ulp" % (
                    B, H, name, what, _ulps(a, b) if a.dtype == torch.float32 else "?")
        zc = z.cpu()
        assert (zc[B:] == SENT).all() and (zc[:, 4 * H:] == SENT).all(), "the contraction wrote outside z [B, 4H]"
        zref = case["h0"].double() @ case["w_hh"].double().t()
        zerr = (zc[:B, :4 * H].double() - zref).abs().max().item()
        print("contraction B=%d H=%d: max |z - fp64| = %.3g of 2e-06 (%.2f)" % (B, H, zerr, zerr / 2e-6))
        assert zerr < 2e-6
        bad = case["tok"].clone()
        bad[B - 1] = STEP_V
        fused = _fused(d, dict(tok=bad.to(DEV)))
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
        *pair, _ = _two_launches(d, dict(tok=bad.to(DEV)), z)
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
        assert all(torch.equal(a, b) for a, b in zip(fused, pair))


@pytest.mark.parametrize("B,H", [(33, 100), (70, 44)])
def test_pointwise_on_the_z_of_the_argmax_launch(lib, B, H):
    """(d) the product's pairing (decode_fused): the step writes h_t as planes, the arg-max launch's second role multiplies those
    planes with the W_hh image into z, the cell update finishes step t + 1 from z.  z against fp64 at the split-precision bound; h
    and c of step t + 1 against the fp64 cell at the tile step's tolerances plus that bound (with |c_prev| <= 1 no derivative of the
    cell with respect to a pre-activation exceeds 1).  NB = 1 at B = 33, NB = 2 at B = 70."""
    from s2vt_video_caption_amd import capi, ops
    case = _step_case(B, H)
    d = _to_dev(case)
    kpad = (H + 63) // 64 * 64
    with _options(lib, gemv=0):
        h1, _, _, img = _fused(d, dict(tok=case["tok"].to(DEV)))                 # step t: h_t and its planes
        pwhh = ops.split_planes(d["w_hh"])
        z = torch.full((B + 1, 4 * H), SENT, device=DEV)
        ops.argmax_x3_planes(pwhh, (img, 3 * kpad, kpad), B, 4 * H, pw2=pwhh, M2=4 * H, z=z, with_logits=False)
        tok2 = case["tok"].flip(0).contiguous()
        h2, c2, _ = ops.lstm_cell_pointwise(z, H, d["c0"], gx=d["gx"], gx_idx=d["gx_idx"], gtab=d["gtab"], tok=tok2.to(DEV), B=B)
        torch.cuda.synchronize()
        capi.check_async_error()
    zref = h1.cpu().double() @ case["w_hh"].double().t()
    zc = z.cpu()
    assert (zc[B:] == SENT).all()
    zerr, ztol = (zc[:B].double() - zref).abs().max().item(), _x3_bound(zref)
    href, cref, _ = _step_ref(case, tok2, z=zref)
    herr, cerr = (h2.cpu().double() - href).abs().max().item(), (c2.cpu().double() - cref).abs().max().item()
    print("argmax z + pointwise B=%d H=%d: z %.3g of %.3g (%.2f); h %.3g of %.3g (%.2f); c %.3g of %.3g (%.2f)" %
          (B, H, zerr, ztol, zerr / ztol, herr, 2e-6 + ztol, herr / (2e-6 + ztol), cerr, 4e-6 + ztol, cerr / (4e-6 + ztol)))
    assert zerr < ztol
    assert herr < 2e-6 + ztol and cerr < 4e-6 + ztol


# ------------------------------------------------------------------------------------------------ (e): the beam plane-path step
BEAM_DIMS = (5, 8, 64, 40, 24, 300)          # B, L, F, H, E, V of test_beam_step_matches_cell_and_topk
BEAM_R, BEAM_SEED = 11, 9


@functools.lru_cache(maxsize=None)
def _beam_case(seed):
    """inputs of one depth step and its fp64 restatement (S2VTModel.py:208-219): states, gate input, logits, log-probs"""
    from s2vt_video_caption_amd import capi, synth
    B, L, F, H, E, V = BEAM_DIMS
    sd = synth.make_state_dict(V, F, H, E, seed=seed)
    g = torch.Generator().manual_seed(3)
    row_b = torch.randint(0, B, (BEAM_R,), generator=g, dtype=torch.int32)
    row_state = torch.randint(0, 7, (BEAM_R,), generator=g, dtype=torch.int32)
    tok = torch.randint(0, V, (BEAM_R,), generator=g, dtype=torch.int32)
    vid_h, vid_c = _r(B, H, seed=1, scale=0.5), _r(B, H, seed=2, scale=0.5)
    word_h, word_c = _r(7, H, seed=3, scale=0.5), _r(7, H, seed=4, scale=0.5)
    w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_f, b_f, w_o, b_o, emb = [sd[k].double() for k in capi.PARAM_KEYS]
    rvh, rvc = orc.lstm_cell(None, vid_h.double(), vid_c.double(), w_ih1, w_hh1, b_ih1, b_hh1)
    x = torch.cat([emb[tok.long()], rvh[row_b.long()]], dim=1)
    gate_in = x @ w_ih2.t() + b_ih2 + b_hh2                                  # what the plane path contracts: gtab row + vid_out half
    rwh, rwc = orc.lstm_cell(x, word_h.double()[row_state.long()], word_c.double()[row_state.long()], w_ih2, w_hh2, b_ih2, b_hh2)
    logits = rwh @ w_o.t() + b_o
    logp = torch.log_softmax(logits, dim=1)
    return dict(sd=sd, row_b=row_b, row_state=row_state, tok=tok, vid_h=vid_h, vid_c=vid_c, word_h=word_h, word_c=word_c, rvh=rvh,
                rvc=rvc, rwh=rwh, rwc=rwc, gate_in=gate_in, logits=logits, logp=logp)


def test_beam_plane_path_step_by_value(lib):
    """(e) s2vt_beam_step_cached on the plane path (s2vt_decode_plan says so) with the cache filled as beam.py fills it - one decode
    of the same weights - against the fp64 restatement of the depth step: vid_rnn's states at the tile step's 2e-6; word_rnn's at
    2e-6 plus the contraction bound on its gate input (gate table + plane GEMM); the log-probs at the sibling's 5e-6 plus the
    contraction bound on the logits; the 20 ids of EVERY row equal - the seed is one where each row's 20th / 21st log-probs are at
    least 10 tolerances apart, asserted first."""
    import S2VTModel
    from s2vt_video_caption_amd import capi, functional, synth
    from s2vt_video_caption_amd.functional import _params_struct, _ptr, _stream
    B, L, F, H, E, V = BEAM_DIMS
    R = BEAM_R
    k = _beam_case(BEAM_SEED)
    tol_w = 2e-6 + _x3_bound(k["gate_in"])
    tol_lp = 5e-6 + _x3_bound(k["logits"])
    top21 = k["logp"].topk(21, dim=1)
    gap = (top21.values[:, 19] - top21.values[:, 20]).min().item()
    assert gap >= 10 * tol_lp, (gap, tol_lp)
    rix = top21.indices[:, :20].sort(dim=1).values
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E)
    m.load_state_dict(k["sd"])
    m.to(DEV).eval()
    plist = tuple(m.state_dict()[key] for key in capi.PARAM_KEYS)
    d = capi.Dims(*BEAM_DIMS)
    dev = torch.device(DEV)
    with _options(lib, persist=1, persist_x3_fwd=1, pipe_block=32, gemm_mode=3, decode_fused=1, pad_min_batch=33):
        assert lib.s2vt_set_gemm_mode(-1) != 0 and capi.decode_plan(BEAM_DIMS, encode_only=True)[0] % 64 == 0      # DecodePlan::planes
        # the cache of this model's weights, filled by one decode (a batch of 64: at most 16 clips decode without the images)
        functional.clear_decode_cache(m)
        cache, valid = functional.decode_cache_entry(m, plist, d, dev, lib)
        assert cache is not None and not valid
        functional.greedy_decode(synth.make_batch(64, L, F, V, seed=12)[0].to(DEV), plist, 0, owner=m)
        cache, valid = functional.decode_cache_entry(m, plist, d, dev, lib)
        assert valid and cache.numel() >= lib.s2vt_decode_cache_bytes(ctypes.byref(d))
        ps = _params_struct(capi.Params, plist)
        nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(d), R)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        ins = [k[n].to(DEV) for n in ("row_b", "row_state", "tok", "vid_h", "vid_c")]
        vh, vc = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
        wh, wc = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV)
        tix, tlp = torch.empty(R, 20, dtype=torch.int32, device=DEV), torch.empty(R, 20, device=DEV)
        word_h, word_c = k["word_h"].to(DEV), k["word_c"].to(DEV)
        capi.check(lib.s2vt_beam_step_cached(ctypes.byref(d), ctypes.byref(ps), R, *[_ptr(t) for t in ins], _ptr(vh), _ptr(vc),
                                             _ptr(word_h), _ptr(word_c), _ptr(wh), _ptr(wc), _ptr(tix), _ptr(tlp), _ptr(ws), nbytes,
                                             _ptr(cache), cache.numel(), _stream(dev)), "s2vt_beam_step_cached")
        torch.cuda.synchronize()
        capi.check_async_error()
    errs = {n: (got.cpu().double() - k[ref]).abs().max().item() for n, got, ref in
            (("vh", vh, "rvh"), ("vc", vc, "rvc"), ("wh", wh, "rwh"), ("wc", wc, "rwc"))}
    lp_err = (tlp.cpu().double() - k["logp"].gather(1, rix)).abs().max().item()
    print("beam plane step: vh %.3g vc %.3g of 2e-06; wh %.3g wc %.3g of %.3g; top_lp %.3g of %.3g; 20/21 gap %.3g" %
          (errs["vh"], errs["vc"], errs["wh"], errs["wc"], tol_w, lp_err, tol_lp, gap))
    assert errs["vh"] < 2e-6 and errs["vc"] < 2e-6
    assert errs["wh"] < tol_w and errs["wc"] < tol_w
    assert torch.equal(tix.cpu().long(), rix)
    assert lp_err < tol_lp
