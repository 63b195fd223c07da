"""Host restatement of the split-precision contract (include/s2vt_hip.h, csrc/common.h, csrc/split.hip), written from the header's
words and not from the library's code - nothing here imports the package:

  bf16_rn_bits / split3     fp32 -> bf16 round-to-nearest-even (NaN kept NaN), x = p0 + p1 + p2 with residuals taken in fp32;
  plane_index / row_index   element offsets of the blocked three-plane image and of the one-plane row image;
  build_image / read_image  scatter / gather of whole images;
  KEPT, ORDERS, six_products  which of the nine plane products a kernel sums, the order each kernel sums them in, and an fp32
                            emulation of that accumulation (one rounding per add) with a product dropped or read from a wrong plane;
  full_range, EDGES, fwd_single_term, bwd_single_term   the operand generators the GPU tests and the host proofs share.

Bits travel as numpy uint16; images as torch int16 (what ops.split_planes returns)."""
import numpy as np
import torch

PLANE_SENT = 0x7FFF                  # a bf16 NaN pattern: split3 produces it from no finite input
KEPT = {(i, j): i + j <= 2 for i in range(3) for j in range(3)}
# the order in which each kernel adds its six products into the fp32 accumulator, as (plane of the activations, plane of the weights)
ORDERS = {
    "gemm_x3": [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)],            # X3_GROUP list, the hi*hi group deferred to the end
    "fwd_persist": [(2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)],        # X_MM2, X_MM1N, X_MM0: h plane x W plane
    "bwd_persist": [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)],        # Y_PROD(W plane, dG plane) restated as (dG, W)
}


def pad64(n):
    return (n + 63) // 64 * 64


# ----------------------------------------------------------------------------------------------------------- the split
def _f32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def bf16_rn_bits(x):
    """uint16 bits of bf16(x), round to nearest even: u += 0x7fff + ((u >> 16) & 1); u >> 16.  NaN -> (u >> 16) | 0x40."""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bits_f32(bits):
    """the fp32 value of bf16 bits"""
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """(p0, p1, p2) as uint16 bits: p0 = rn(x), r1 = x - p0, p1 = rn(r1), r2 = r1 - p1, p2 = rn(r2); residuals in fp32"""
    x = _f32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        p0 = bf16_rn_bits(x)
        r1 = x - bits_f32(p0)
        p1 = bf16_rn_bits(r1)
        r2 = r1 - bits_f32(p1)
        p2 = bf16_rn_bits(r2)
    return p0, p1, p2


# ----------------------------------------------------------------------------------------------------------- the layouts
def plane_index(rows, K, ld):
    """int64 [rows, K, 3]: offset of (r, k, plane) in a blocked three-plane image of row stride ld:
    (r/64)*(64*ld) + (k/16)*3072 + (pl*2 + (k%16)/8)*512 + (r%64)*8 + k%8"""
    r = np.arange(rows, dtype=np.int64)[:, None, None]
    k = np.arange(K, dtype=np.int64)[None, :, None]
    pl = np.arange(3, dtype=np.int64)[None, None, :]
    return (r // 64) * (64 * ld) + (k // 16) * 3072 + (pl * 2 + (k % 16) // 8) * 512 + (r % 64) * 8 + k % 8


def row_index(rows, K, ld):
    """int64 [rows, K]: offset of (r, k) in a one-plane row image: r*ld + k"""
    return np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(K, dtype=np.int64)[None, :]


def _as_u16(p):
    if isinstance(p, torch.Tensor):
        p = p.detach().cpu().numpy()
    p = np.asarray(p)
    return p.view(np.uint16) if p.dtype == np.int16 else p.astype(np.uint16)


def build_image(planes, ld=None, extra_rows=0, fill=0):
    """Three [rows, K] bit arrays -> int16 image [ceil64(rows) + extra_rows, ld] in the blocked layout, ld >= 3*pad64(K) (default:
    equal).  The k padding and the rows up to the 64-row block are zero bits; `fill` is everything no (row < ceil64(rows),
    k < pad64(K)) element maps to.  A 64-row block with ld == 3*pad64(K) is the contiguous array [k/16][plane][k half][64 rows][8]:
    whole images are made by one transposition (test_plane_ref_host.py checks it against plane_index element by element)."""
    planes = [_as_u16(p) for p in planes]
    rows, K = planes[0].shape
    rp, kp = pad64(rows), pad64(K)
    ld = 3 * kp if ld is None else ld
    assert ld >= 3 * kp and len(planes) == 3 and all(p.shape == (rows, K) for p in planes)
    full = np.zeros((3, rp, kp), dtype=np.uint16)
    for pl in range(3):
        full[pl, :rows, :K] = planes[pl]
    blocks = full.reshape(3, rp // 64, 64, kp // 16, 2, 8).transpose(1, 3, 0, 4, 2, 5).reshape(rp // 64, 192 * kp)
    img = np.full((rp // 64 + (extra_rows + 63) // 64, 64 * ld), fill, dtype=np.uint16)
    img[:rp // 64, :192 * kp] = blocks
    img = img.reshape(-1, ld)[:rp + extra_rows]
    return torch.from_numpy(np.ascontiguousarray(img).view(np.int16))


def read_image(img, rows, K, ld=None):
    """the three [rows, K] uint16 bit arrays of a blocked image (row stride ld, default: the tensor's width)"""
    flat = _as_u16(img).reshape(-1)
    ld = img.shape[1] if ld is None else ld
    got = flat[plane_index(rows, K, ld)]
    return got[:, :, 0], got[:, :, 1], got[:, :, 2]


def build_row_image(bits, ld=None, extra_rows=0, fill=0, rows_pad=None):
    """[rows, K] bits -> int16 one-plane row image [rows_pad + extra_rows, ld]: element (r, k) at r*ld + k, zero bits in the k
    padding and in the rows [rows, rows_pad), `fill` elsewhere"""
    bits = _as_u16(bits)
    rows, K = bits.shape
    rp, kp = pad64(rows) if rows_pad is None else rows_pad, pad64(K)
    ld = kp if ld is None else ld
    img = np.full((rp + extra_rows, ld), fill, dtype=np.uint16)
    img[:rp, :kp] = 0
    img[:rows, :K] = bits
    return torch.from_numpy(img.view(np.int16))


# ----------------------------------------------------------------------------------------------------------- the products
def six_products(xp, yp, order, drop=None, swap=None):
    """fp32 emulation of one contraction term: acc = 0; for (i, j) in order: acc = fp32(acc + xp[i] * yp[j]) (a product of two bf16
    values is exact in fp32; one rounding per add).  xp / yp: the three planes as fp32 arrays.  drop = (i, j): that product is left
    out.  swap = {(i, j): (i', j')}: that product reads planes (i', j') instead."""
    acc = np.zeros(np.broadcast(xp[0], yp[0]).shape, dtype=np.float32)
    for (i, j) in order:
        if drop is not None and (i, j) == tuple(drop):
            continue
        a, b = (swap or {}).get((i, j), (i, j))
        acc = (acc + (xp[a].astype(np.float32) * yp[b].astype(np.float32)).astype(np.float32)).astype(np.float32)
    return acc


def planes_f32(x):
    """the three planes of x as fp32 value arrays"""
    return tuple(bits_f32(p) for p in split3(x))


# the single-product mutations the bounds of test_gpu_plane_products.py must notice: each third-order product dropped, and each read
# with one operand from the plane below (the error is then a fourth-order term short of the dropped one's)
THIRD_ORDER = [(1, 1), (0, 2), (2, 0)]
MISPAIRS = [((0, 2), (2, 2)), ((2, 0), (2, 2)), ((1, 1), (1, 2)), ((1, 1), (2, 1)), ((0, 2), (1, 2)), ((2, 0), (2, 1))]
BOUND_REL = 2.0 ** -21               # the recurrences' contraction bound, relative to the single product (host emulation: 2^-23.6)
ACT_ABS = 4e-7                       # absolute allowance for the forward's activations (common.h claims ~1.5e-7 each)


# ----------------------------------------------------------------------------------------------------------- generators
def full_range(n, seed):
    """n fp32 values randn * 2^U[-100, 100); anything below 2^-100 in magnitude is replaced by 0 (below ~2^-110 the third residual
    goes subnormal and p0 + p1 + p2 = x no longer holds exactly)"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * np.exp2(g.uniform(-100.0, 100.0, n))).astype(np.float32)
    x[np.abs(x) < 2.0 ** -100] = 0.0
    return x


def _from_bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


# ties to even (down / up), the carry into the exponent, signed zeros, bf16-exact values, the same at both ends of the range
EDGES = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, _from_bits(0x3F7FFFFF), -0.0, 0.0, 1.0, -2.5, 3.0 * 2.0 ** -90, -(1 + 2.0 ** -8),
                  -(1 + 3 * 2.0 ** -8), (1 + 2.0 ** -8) * 2.0 ** 99, (1 + 3 * 2.0 ** -8) * 2.0 ** -99, 1 + 2.0 ** -16, 1 + 3 * 2.0 ** -16,
                  1 + 2.0 ** -23, 2 - 2.0 ** -23, 4.0, -4.0, 2.0 ** -100, -(2.0 ** 100)], dtype=np.float32)


def split_values(rows, cols, seed):
    """[rows, cols] fp32: the full-range generator with the edge list at the start (as far as it fits)"""
    x = full_range(rows * cols, seed)
    n = min(x.size, EDGES.size)
    x[:n] = EDGES[:n]
    return x.reshape(rows, cols)


def _three_plane_weights(g, n, lo, hi):
    """n fp32 values, random sign, |w| uniform in [lo, hi], every one with three non-zero planes"""
    w = (g.uniform(lo, hi, n) * g.choice([-1.0, 1.0], n)).astype(np.float32)
    for _ in range(100):
        bad = np.zeros(n, dtype=bool)
        for p in split3(w):
            bad |= (p & 0x7FFF) == 0
        if not bad.any():
            return w
        w[bad] = (g.uniform(lo, hi, int(bad.sum())) * g.choice([-1.0, 1.0], int(bad.sum()))).astype(np.float32)
    raise AssertionError("no three-plane weights")


def fwd_k_of_col(H, s):
    """k(col) of shift s: (col % 64 + 64*s) % H for the 4H gate columns"""
    col = np.arange(4 * H)
    return (col % 64 + 64 * s) % H


def fwd_single_term(B, H, s, seed=0):
    """The forward recurrence's single-term case: (gx0 [B, 4H], W_hh [4H, H] with one non-zero per row at k(col), w [4H], k [4H]).
    |w| in [4, 16]; gx0 = randn with the input and output gates' columns shifted by +2 and the cell input's doubled: h_0 is dense
    and |h_0| is mostly 0.2 to 0.6, so that |p| = |h_0 w| stands well above the activations' absolute allowance in the bounds."""
    g = np.random.default_rng(1000 * H + 10 * s + seed)
    gx0 = np.random.default_rng(7 * H + seed).standard_normal((B, 4, H))
    gx0 = (gx0 * np.array([1.0, 1.0, 2.0, 1.0])[None, :, None] + np.array([2.0, 0.0, 0.0, 2.0])[None, :, None]).reshape(B, 4 * H).astype(np.float32)
    w = _three_plane_weights(g, 4 * H, 4.0, 16.0)
    k = fwd_k_of_col(H, s)
    W = np.zeros((4 * H, H), dtype=np.float32)
    W[np.arange(4 * H), k] = w
    return gx0, W, w, k


def host_h0(gx0):
    """h_0 of the cell from c_{-1} = h_{-1} = 0 in fp64, rounded to fp32 (what the kernel's step 0 gives up to its activations)"""
    i, f, gg, o = np.split(gx0.astype(np.float64), 4, axis=1)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    return (sig(o) * np.tanh(sig(i) * np.tanh(gg))).astype(np.float32)


def bwd_nshifts(H):
    return 4 * -(-4 * H // H)


def bwd_col_of_j(H, s):
    """col(j) of shift s in [0, bwd_nshifts(H)): (j + s * ceil(4H / nshifts)) % 4H - the runs' windows of H gate columns overlap and
    walk once round the 4H, so every gate column is col(j) of about four different j"""
    step = -(-4 * H // bwd_nshifts(H))
    return (np.arange(H) + s * step) % (4 * H)


def bwd_single_term(H, s, seed=0):
    """The BPTT's single-term case: (W_hh [4H, H] with one non-zero per column j at row col(j), w [H], col [H]); |w| in [0.5, 2]"""
    g = np.random.default_rng(2000 * H + 10 * s + seed)
    w = _three_plane_weights(g, H, 0.5, 2.0)
    col = bwd_col_of_j(H, s)
    W = np.zeros((4 * H, H), dtype=np.float32)
    W[col, np.arange(H)] = w
    return W, w, col
