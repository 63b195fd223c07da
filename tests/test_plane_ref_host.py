"""CPU only: the host restatement of the split-precision contract (tests/plane_ref.py) against torch's own bf16 rounding, the
layout's bijection, and the proof that the bounds of test_gpu_plane_products.py tell a correct accumulation of the six plane products
from one that lost or mis-paired a third-order product - on the very operand generators the GPU tests import.  That proof stands in
for running an edited kernel: the kernels' product lists carry hand-counted waits and are never mutated on a device.

Emulation results (fp32 accumulation in each kernel's order, one rounding per add; printed by the tests):
  all six products: max relative error 2^-23.6 on the BPTT's single-term operands, 0.16 of the 2^-21 bound; the forward's gates
  reach 0.15 of their bounds;
  any one of (1,1), (0,2), (2,0) dropped or read from a wrong plane: BPTT 75 to 83 % of the elements over the bound, max 11 to 27
  times the bound; forward gates (the activations' absolute allowance is in their bounds) 59 to 73 % over, max 9 to 23 times."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref as P  # noqa: E402


def _chain(x):
    """the split through torch's own fp32 -> bf16 conversion"""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    r2 = r1 - p1.float()
    p2 = r2.bfloat16()
    return [p.view(torch.int16).numpy().view(np.uint16) for p in (p0, p1, p2)]


def test_split3_is_torchs_bf16_chain_and_sums_back_exactly():
    """1e6 values randn * 2^U[-100, 100): split3's bits are those of x.bfloat16() applied three times, and p0 + p1 + p2 == x exactly
    (summed in fp64, and in fp32 from the small end) for every |x| >= 2^-100."""
    g = np.random.default_rng(1)
    x = (g.standard_normal(1_000_000) * np.exp2(g.uniform(-100.0, 100.0, 1_000_000))).astype(np.float32)
    got, want = P.split3(x), _chain(x)
    for pl in range(3):
        assert np.array_equal(got[pl], want[pl]), pl
    big = np.abs(x) >= 2.0 ** -100
    assert big.sum() > 990_000
    v = [P.bits_f32(p).astype(np.float64) for p in got]
    assert np.array_equal((v[0] + v[1] + v[2])[big], x.astype(np.float64)[big])
    f = [P.bits_f32(p) for p in got]
    assert np.array_equal(((f[2] + f[1]) + f[0])[big], x[big])
    # the generator of the GPU tests keeps to that range (or 0) and still spans it
    y = P.full_range(100_000, 3)
    assert ((np.abs(y) >= 2.0 ** -100) | (y == 0)).all() and np.abs(y).max() > 2.0 ** 90 and np.abs(y[y != 0]).min() < 2.0 ** -90
    assert not (np.array(P.split3(y)) == P.PLANE_SENT).any()


def test_split3_edges_by_bits():
    one = 0x3F80
    f = lambda v: [int(p[0]) for p in P.split3(np.array([v], dtype=np.float32))]
    # 1 + 2^-8: half an ulp of bf16 at 1, a tie -> the even neighbour 1.0; the residual 2^-8 is exact in p1
    assert f(1 + 2.0 ** -8) == [one, 0x3B80, 0]
    # 1 + 3*2^-8: a tie between 1 + 2^-7 (odd) and 1 + 2^-6 (even) -> up; the residual -2^-8 is negative
    assert f(1 + 3 * 2.0 ** -8) == [0x3F82, 0xBB80, 0]
    # all mantissa bits set: the rounding carries into the exponent
    x = np.array([0x3F7FFFFF], dtype=np.uint32).view(np.float32)[0]
    p = f(x)
    assert p[0] == one and p[1] == 0xB380 and p[2] == 0                     # 1.0 - 2^-24
    assert f(-0.0) == [0x8000, 0, 0] and f(0.0) == [0, 0, 0]
    for v in (1.0, -2.5, 4.0, 3.0 * 2.0 ** -90, 2.0 ** 100, -0.0078125):
        p = f(v)
        assert p[1] == 0 and p[2] == 0 and P.bits_f32(np.array([p[0]], dtype=np.uint16))[0] == np.float32(v)
    assert int(P.bf16_rn_bits(np.array([np.nan], dtype=np.float32))[0]) & 0x7FC0 == 0x7FC0
    snan = np.array([0x7F800001], dtype=np.uint32).view(np.float32)
    assert int(P.bf16_rn_bits(snan)[0]) == 0x7FC0                           # (u >> 16) | 0x40: not rounded to infinity
    assert int(P.bf16_rn_bits(np.array([np.inf], dtype=np.float32))[0]) == 0x7F80
    # every edge the GPU test feeds the kernels agrees with torch's chain too
    for a, b in zip(P.split3(P.EDGES), _chain(P.EDGES)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rows,K,extra", [(1, 1, 0), (64, 64, 0), (130, 70, 8), (200, 129, 40), (65, 16, 24)])
def test_plane_index_is_a_bijection_onto_the_image(rows, K, extra):
    """Over (row < ceil64(rows), k < pad64(K), plane) the index is injective, stays inside the image, and covers it exactly when
    ld == 3*pad64(K); a wider ld leaves exactly 64*(ld - 3*pad64(K)) elements per 64-row block unaddressed."""
    rp, kp = P.pad64(rows), P.pad64(K)
    ld = 3 * kp + extra
    idx = P.plane_index(rp, kp, ld).reshape(-1)
    assert idx.min() == 0 and idx.max() < rp * ld
    assert np.unique(idx).size == idx.size == rp * 3 * kp
    hit = np.zeros(rp * ld, dtype=bool)
    hit[idx] = True
    per_block = (~hit).reshape(rp // 64, 64 * ld).sum(axis=1)
    assert (per_block == 64 * extra).all()
    ridx = P.row_index(rp, kp, kp + extra).reshape(-1)
    assert np.unique(ridx).size == ridx.size and ridx.max() < rp * (kp + extra)


@pytest.mark.parametrize("rows,K,extra", [(1, 1, 0), (130, 70, 8), (200, 129, 0)])
def test_build_image_is_the_scatter_by_plane_index(rows, K, extra):
    g = np.random.default_rng(rows)
    planes = [g.integers(1, 0x7000, (rows, K)).astype(np.uint16) for _ in range(3)]
    kp = P.pad64(K)
    ld = 3 * kp + extra
    img = P.build_image(planes, ld=ld, extra_rows=64, fill=P.PLANE_SENT)
    assert tuple(img.shape) == (P.pad64(rows) + 64, ld) and img.dtype == torch.int16
    want = np.full(img.numel(), P.PLANE_SENT, dtype=np.uint16)
    want[P.plane_index(P.pad64(rows), kp, ld).reshape(-1)] = 0
    want[P.plane_index(rows, K, ld)] = np.stack(planes, axis=2)
    assert np.array_equal(img.numpy().view(np.uint16).reshape(-1), want)
    for a, b in zip(P.read_image(img, rows, K), planes):
        assert np.array_equal(a, b)
    row = P.build_row_image(planes[0], ld=kp + extra, extra_rows=3, fill=P.PLANE_SENT, rows_pad=rows + 2).numpy().view(np.uint16)
    assert np.array_equal(row[:rows, :K], planes[0]) and (row[:rows + 2, K:kp] == 0).all() and (row[rows:rows + 2, :kp] == 0).all()
    assert (row[rows + 2:] == P.PLANE_SENT).all() and (row[:, kp:] == P.PLANE_SENT).all()


def test_kept_products_and_orders():
    assert sorted(k for k, v in P.KEPT.items() if v) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]
    assert len(P.KEPT) == 9
    for name, order in P.ORDERS.items():
        assert sorted(order) == sorted(k for k, v in P.KEPT.items() if v), name
        assert order[-1] == (0, 0), name                                   # small terms first


def _rel(acc, x, y):
    p = x.astype(np.float64) * y.astype(np.float64)
    return np.abs(acc.astype(np.float64) - p) / np.abs(p)


def _report(tag, rel, bound):
    over = float((rel > bound).mean())
    print("%s: max %.3g = 2^%.1f (%.2f of the bound), %.0f %% of the elements over it" % (
        tag, rel.max(), np.log2(rel.max()), rel.max() / bound, 100 * over))
    return over


@pytest.mark.parametrize("H", [72, 520])
def test_bptt_bound_discriminates_on_its_own_operands(H):
    """The BPTT case of test_gpu_plane_products.py asserts |dh - dG * w| <= 2^-21 |dG * w|.  dG-like operands (products of gate
    derivatives: a wide range of magnitudes) against the generator's weights, in the kernel's order."""
    g = np.random.default_rng(5)
    _, w, _ = P.bwd_single_term(H, 1)
    dg = (0.1 * g.standard_normal((64, H)) * g.uniform(0.0, 0.25, (64, H)) * g.uniform(0.0, 1.0, (64, H))).astype(np.float32)
    dg[dg == 0] = 1e-3
    xp, yp = P.planes_f32(dg), P.planes_f32(np.broadcast_to(w, dg.shape).copy())
    order = P.ORDERS["bwd_persist"]
    good = _rel(P.six_products(xp, yp, order), dg, w)
    assert _report("bptt H=%d all six" % H, good, P.BOUND_REL) == 0.0 and good.max() <= 0.25 * P.BOUND_REL
    for d in P.THIRD_ORDER:
        assert _report("bptt H=%d drop %s" % (H, d), _rel(P.six_products(xp, yp, order, drop=d), dg, w), P.BOUND_REL) >= 0.30
    for a, b in P.MISPAIRS:
        assert _report("bptt H=%d %s read as %s" % (H, a, b), _rel(P.six_products(xp, yp, order, swap={a: b}), dg, w),
                       P.BOUND_REL) >= 0.30


@pytest.mark.parametrize("H", [72, 520])
def test_forward_gate_bounds_discriminate_on_their_own_operands(H):
    """The forward case asserts on the activated gates of step 1 with pre = gx_1 + acc, gx_1 = -fp32(p): |tanh(pre) - tanh(ref)| <=
    2^-21 |p| + a and |sigmoid(pre) - sigmoid(ref)| <= 2^-23 |p| + a, ref = fp64(gx_1) + p.  Here with exact activations (a is the
    kernel's activation error and is only ever in the bound): the accumulation alone must stay inside, every mutation must leave."""
    B = 64
    gx0, _, w, k = P.fwd_single_term(B, H, 1)
    h0 = P.host_h0(gx0)
    assert np.median(np.abs(h0)) > 0.2
    x, y = h0[:, k], np.broadcast_to(w, (B, 4 * H)).copy()                   # [B, 4H] single terms
    p = x.astype(np.float64) * y.astype(np.float64)
    gx1 = (-p).astype(np.float32)
    ref = gx1.astype(np.float64) + p
    xp, yp = P.planes_f32(x), P.planes_f32(y)
    order = P.ORDERS["fwd_persist"]
    tanh_cols = np.zeros(4 * H, dtype=bool)
    tanh_cols[2 * H:3 * H] = True
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))

    def over(acc, tag):
        pre = (gx1 + acc).astype(np.float64)                               # one fp32 add (exact here: the two nearly cancel)
        assert np.array_equal(pre, gx1.astype(np.float64) + acc.astype(np.float64))
        et = np.abs(np.tanh(pre) - np.tanh(ref))[:, tanh_cols] / (2.0 ** -21 * np.abs(p) + P.ACT_ABS)[:, tanh_cols]
        es = np.abs(sig(pre) - sig(ref))[:, ~tanh_cols] / (2.0 ** -23 * np.abs(p) + P.ACT_ABS)[:, ~tanh_cols]
        print("forward H=%d %s: tanh gate max %.2f of its bound, %.0f %% over; sigmoid gates max %.2f, %.0f %% over" % (
            H, tag, et.max(), 100 * (et > 1).mean(), es.max(), 100 * (es > 1).mean()))
        return et, es
    et, es = over(P.six_products(xp, yp, order), "all six")
    assert et.max() <= 0.25 and es.max() <= 0.25
    for d in P.THIRD_ORDER:
        et, es = over(P.six_products(xp, yp, order, drop=d), "drop %s" % (d,))
        assert (et > 1).mean() >= 0.30 and (es > 1).mean() >= 0.30
    for a, b in P.MISPAIRS:
        et, es = over(P.six_products(xp, yp, order, swap={a: b}), "%s read as %s" % (a, b))
        assert (et > 1).mean() >= 0.30 and (es > 1).mean() >= 0.30


def test_single_term_generators_cover_what_they_claim():
    for H in (72, 520, 1024):
        seen = np.zeros((4 * H, H), dtype=bool)
        for s in range(-(-H // 64)):
            _, W, w, k = P.fwd_single_term(2, H, s)
            assert ((W != 0).sum(axis=1) == 1).all() and np.array_equal(W[np.arange(4 * H), k], w)
            assert (np.abs(w) >= 4).all() and (np.abs(w) <= 16).all()
            assert all(((p & 0x7FFF) != 0).all() for p in P.split3(w))
            seen[np.arange(4 * H), k] = True
        # every 64-column slice of the gate columns meets every k
        assert seen.reshape(-1, 64, H).any(axis=1).all() if H % 64 == 0 else seen.any(axis=0).all()
    for H in (72, 520):
        assert P.bwd_nshifts(H) == 16
        used = np.zeros(4 * H, dtype=int)
        for s in range(P.bwd_nshifts(H)):
            W, w, col = P.bwd_single_term(H, s)
            assert ((W != 0).sum(axis=0) == 1).all() and np.array_equal(W[col, np.arange(H)], w)
            assert (np.abs(w) >= 0.5).all() and (np.abs(w) <= 2).all()
            used[col] += 1
        assert used.min() >= 1 and all(used[g * H:(g + 1) * H].min() >= 1 for g in range(4))
