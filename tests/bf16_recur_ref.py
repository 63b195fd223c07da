"""Plain restatements on the CPU of the bf16-operand (config 3) LSTM recurrence kernels - csrc/lstm_bf16.hip (one launch per timestep)
and the bf16 half of csrc/lstm_persist.hip (persistent forward and BPTT) - with the kernels' operand rounding, the inputs the tests
feed them, the bounds, and the case lists the host test (test_bf16_recur_ref_host.py) and the GPU test
(test_gpu_bf16_recurrence_edges.py) both iterate.

What the kernels compute: the recurrent contraction reads bf16 operands - bf16(W_hh) and the bf16 image of the fp32 h_{t-1} (forward)
or of the fp32 dG_{t+1} (backward) the step before wrote - and accumulates in fp32; the cell, its state and every output stay fp32.

  bf16r         fp32 -> bf16 (round to nearest even, as f2bf / f2bf_rn) -> fp64
  fwd_step / bwd_step     one step from the operands the kernel saw, evaluated in `dtype`
  fwd_chain / bwd_chain   a layer running on its own outputs, as the device does: in float64 without rounding it is
                lstm_step_ref.layer_fwd / layer_bwd; in float32 with rounding it is a host emulation of the device, the stand-in for
                device results in the host test.  `mutate` plants one structural mistake (MUTATIONS_*).
  fwd_teacher_forced / bwd_teacher_forced   every step of given results checked on its own, in fp64, from what the device itself
                wrote for the step before: bf16r(device h_{t-1}) and the device's fp32 c_{t-1}; bf16r(device fp32 dG_{t+1}).  The
                device emits no dc per step, so the backward reference carries its own fp64 dc chain, fed by these teacher-forced
                dh.  What then separates device and reference is fp32 rounding alone - no bf16 re-rounding flip - so no element is
                left out of a comparison and the bound is an fp32-level one.

Bounds.  Forward: the project's 2e-5 absolute on h, c and the gates (test_gpu_kernels._check_seq_bf16_teacher_forced), unchanged.
Backward: BWD_REL * max|ref| + BWD_ABS on dG, where BWD_REL starts at lstm_step_ref.TOL_DG (5e-6) and is kept because the fp32
emulation stays under half of it for every case (test_bf16_recur_ref_host.py records the measured worst); free-running against its
own fp64 chain the old bound was 2e-3 * max|ref|."""
import functools

import torch

import lstm_step_ref as sref

F64 = torch.float64
F32 = torch.float32

TOL_FWD = 2e-5                 # absolute: h, c, activated gates of a teacher-forced forward step
BWD_REL = sref.TOL_DG          # 5e-6, relative to max|ref dG| of the case (old free-running bound: 2e-3)
BWD_ABS = 1e-9
BWD_REL_CEILING = 2e-5         # the relative part may in no case exceed this

# ------------------------------------------------------------------------------------------------------------------ case lists
# a. per-timestep forward (T, B, H, n_gx): n_gx = 0 (bias alone), in between, T (gx alone)
STEP_FWD_CASES = ([(3, B, 37, n) for B, n in ((1, 0), (31, 1), (32, 3), (33, 2), (64, 0), (65, 3))] +
                  [(3, 33, H, n) for H, n in ((3, 1), (15, 3), (16, 0), (17, 2), (64, 1), (130, 3))] + [(3, 5, 1000, 2)])
# b. per-timestep backward (T, B, H, dh_first); dh_first None: dh_out = None.  H = 3 and 16: Kp = 64, one k chunk
STEP_BWD_CASES = ([(3, B, 37, f) for B, f in ((1, 0), (32, 1), (33, 0), (65, 2))] +
                  [(3, 33, H, f) for H, f in ((3, 0), (16, 1), (31, 0), (32, 2), (33, 1), (130, 0))] +
                  [(3, 33, 37, 3), (3, 33, 37, None), (1, 33, 37, 0), (1, 65, 16, 0)])
# c. persistent forward (T, B, H, n_gx, block).  H = 5 and 8 are shapes the kernel is meant to run: lstm_seq_fwd_bf16_persist_supported
# asks only B % 32 and Kp <= 1024, plan_chains gives one workgroup (one column slice, one row group), and in seq_fwd_body Kp = 64
# means nch = half = 1 - the second k-half wave gets cbeg = cend = 1, zero W registers, and joins every barrier without a chunk
PERSIST_FWD_CASES = [(5, 32, 8, 5, 2), (4, 32, 37, 1, 2), (5, 64, 70, 3, 2), (3, 32, 999, 1, 0), (5, 64, 1024, 2, 0), (4, 32, 5, 4, 3)]
PERSIST_FWD_PAIR = (4, 32, 37, 1, 2)
# d. persistent BPTT (T, B, H, dh_first, block), each under bptt_units 0, 16 and 32.  (4, 64, 40, 4, 0) has dh_first == T: nothing flows,
# every dG is zero; (4, 64, 40, 1, 0) is the same ragged shape with a gradient
PERSIST_BWD_CASES = [(5, 32, 8, 0, 2), (4, 32, 72, 1, 2), (4, 64, 40, 4, 0), (3, 32, 1000, 1, 0), (5, 64, 1024, 2, 0), (4, 64, 40, 1, 0)]
PERSIST_BWD_PAIR = (4, 32, 72, 1, 2)
BPTT_UNITS = [0, 16, 32]
# e. refusals of the persistent entry points (B, H)
REFUSE_FWD = [(33, 37), (32, 1032)]          # B % 32; Kp = 1088 > 1024
REFUSE_BWD = [(32, 36), (32, 1032)]          # H % 8; 4H = 4128 > 4096
# g. ragged cases of each kernel whose row image is read back (the persistent forward stores whole 16-unit tiles: every ragged width)
IMAGE_STEP_FWD = (3, 33, 37, 2)
IMAGE_STEP_BWD = (3, 33, 37, 1)
IMAGE_PERSIST_FWD = [(4, 32, 37, 1, 2), (4, 32, 5, 4, 3), (3, 32, 999, 1, 0)]
IMAGE_PERSIST_BWD = (4, 32, 72, 1, 2)

FWD_CASES_ALL = sorted(set(STEP_FWD_CASES + [c[:4] for c in PERSIST_FWD_CASES]))
BWD_CASES_ALL = sorted(set(STEP_BWD_CASES + [c[:4] for c in PERSIST_BWD_CASES]), key=str)

# the mistakes the bounds must see (test_bf16_recur_ref_host.py): name -> what is planted
MUTATIONS_FWD = ["zero_last_rows", "zero_last_cols", "drop_last_k", "stale_c"]
MUTATIONS_BWD = ["zero_last_rows", "zero_last_cols", "drop_last_k", "c_for_c_prev", "drop_dc", "shift_dh_out"]
FWD_TILE = (32, 16)            # (rows, hidden units) of an output tile: the last one is what "last block" means
BWD_TILE = (32, 32)
KCH = 64                       # k chunk of every kernel


def pad64(n):
    return (n + 63) // 64 * 64


def _r(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bf16r(x, rounding=True):
    """fp32 tensor -> the fp64 value of its bf16 rounding (nearest even); rounding=False: the fp64 value of x itself"""
    if not rounding:
        return x.to(F64)
    assert x.dtype == F32, x.dtype
    return x.to(torch.bfloat16).to(F64)


# ---------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def fwd_inputs(T, B, H, seed=11):
    """fp32 (gx [T*B, 4H], bias [4H], w_hh [4H, H]) at the scales of test_gpu_kernels.test_bf16_step_kernels_h1000_odd_batch; never modified"""
    return _r(T * B, 4 * H, seed=seed), _r(4 * H, seed=seed + 1, scale=0.3), _r(4 * H, H, seed=seed + 2, scale=H ** -0.5)


@functools.lru_cache(maxsize=None)
def bwd_inputs(T, B, H, dh_first, seed=50):
    """fp32 (w_hh, gates [T*B, 4H], c_all [T*B, H], dh_out [(T - dh_first)*B, H] or None): test_gpu_kernels._bptt_inputs and its dh_out
    (scale 0.1); never modified"""
    w = _r(4 * H, H, seed=seed, scale=H ** -0.5)
    gates = torch.sigmoid(_r(T * B, 4 * H, seed=seed + 1))
    gates[:, 2 * H:3 * H] = torch.tanh(_r(T * B, H, seed=seed + 2))
    c_all = _r(T * B, H, seed=seed + 3, scale=0.7)
    dh = None if dh_first is None else _r((T - dh_first) * B, H, seed=seed + 9, scale=0.1)
    return w, gates, c_all, dh


def has_gradient(T, dh_first):
    """does any gradient arrive in a backward case (else every dG is zero and no mutation of the arithmetic can show)"""
    return dh_first is not None and dh_first < T


# -------------------------------------------------------------------------------------------------------------------- the steps
def _drop_k(a, K):
    """a [.., K] with its last k chunk zeroed: the contraction without it"""
    a = a.clone()
    a[..., (K - 1) // KCH * KCH:] = 0
    return a


def fwd_step(g, h_prev, c_prev, w_hh, dtype=F64, rounding=True, drop_last_k=False):
    """One forward step.  g [B, 4H] (fp32: gx rows or the bias on every row), h_prev / c_prev fp32 [B, H] as the step before wrote them (None:
    zero state), w_hh fp32.  Returns (h, c, gates) in dtype."""
    H = w_hh.shape[1]
    hp = None
    if h_prev is not None:
        hp = bf16r(h_prev, rounding)
        if drop_last_k:
            hp = _drop_k(hp, H)
    return sref.cell_fwd(g, bf16r(w_hh, rounding), hp, c_prev, dtype)


def bwd_step(dg_next, w_hh, dh_out, stash, c, c_prev, dc_in, dtype=F64, rounding=True, drop_last_k=False):
    """One BPTT step: dg_next fp32 [B, 4H] as the step after wrote it (None at T - 1), dc_in in any dtype (None: zero).
    Returns (dg, dc_prev) in dtype."""
    dgn = None
    if dg_next is not None:
        dgn = bf16r(dg_next, rounding)
        if drop_last_k:
            dgn = _drop_k(dgn, dgn.shape[1])
    return sref.step_bwd(dgn, bf16r(w_hh, rounding), dh_out, stash, c, c_prev, dc_in, dtype)


def _zero_last_block(x, B, cols, tile, what, ngroups=1):
    """x [B, ngroups * cols] with the last row block / the last column block (of every gate group) zeroed"""
    x = x.clone()
    tr, tc = tile
    if what == "zero_last_rows":
        x[(B - 1) // tr * tr:] = 0
    else:
        for g in range(ngroups):
            x[:, g * cols + (cols - 1) // tc * tc:(g + 1) * cols] = 0
    return x


# ------------------------------------------------------------------------------------------------------------------- the chains
def fwd_chain(gx, n_gx, bias, w_hh, T, B, H, dtype=F64, rounding=True, mutate=None):
    """The layer from the zero state on its own outputs: what each step wrote (fp32 when rounding, as the device stores it) feeds the
    next.  Returns fp32 (rounding) or dtype (h_all, c_all, gates)."""
    assert mutate is None or mutate in MUTATIONS_FWD
    store = (lambda x: x.to(F32)) if rounding else (lambda x: x)
    hs, cs, ss = [], [], []
    for t in range(T):
        g = gx[t * B:(t + 1) * B] if t < n_gx else bias.expand(B, -1)
        cp = cs[-1] if t else None
        if mutate == "stale_c" and t:
            cp = cs[-2] if t > 1 else torch.zeros_like(cs[-1])
        h, c, s = fwd_step(g, hs[-1] if t else None, cp, w_hh, dtype, rounding, drop_last_k=(mutate == "drop_last_k"))
        if mutate in ("zero_last_rows", "zero_last_cols"):
            h = _zero_last_block(h, B, H, FWD_TILE, mutate)
        hs.append(store(h)), cs.append(store(c)), ss.append(store(s))
    return torch.cat(hs), torch.cat(cs), torch.cat(ss)


def bwd_chain(w_hh, dh_out, dh_first, c_all, gates, T, B, H, dtype=F64, rounding=True, mutate=None):
    """The BPTT on its own outputs: dG_{t+1} as stored (fp32 when rounding) feeds step t, dc is carried in dtype.  Returns dG [T*B, 4H]."""
    assert mutate is None or mutate in MUTATIONS_BWD
    store = (lambda x: x.to(F32)) if rounding else (lambda x: x)
    dgs = [None] * T
    dc = None
    first = dh_first if dh_first is not None else 0
    for t in range(T - 1, -1, -1):
        rows = slice(t * B, (t + 1) * B)
        k = t - first + (1 if mutate == "shift_dh_out" else 0)          # the block of dh_out rows step t takes
        dho = dh_out[k * B:(k + 1) * B] if dh_out is not None and 0 <= k < T - first else None
        cp = c_all[(t - 1) * B:t * B] if t else None
        if mutate == "c_for_c_prev":
            cp = c_all[rows]
        dgn = dgs[t + 1] if t < T - 1 else None
        dg, dc = bwd_step(dgn, w_hh, dho, gates[rows], c_all[rows], cp, None if mutate == "drop_dc" else dc, dtype, rounding,
                          drop_last_k=(mutate == "drop_last_k"))
        if mutate in ("zero_last_rows", "zero_last_cols"):
            dg = _zero_last_block(dg, B, H, BWD_TILE, mutate, ngroups=4)
        dgs[t] = store(dg)
    return torch.cat(dgs)


# -------------------------------------------------------------------------------------------------------------- teacher forcing
def fwd_teacher_forced(h_all, c_all, gates, gx, n_gx, bias, w_hh, T, B, H):
    """Every step of fp32 results (h_all, c_all [T*B, H], gates [T*B, 4H]) against fp64 math on the operands the kernel itself saw.
    Returns {"h", "c", "gates", "worst"}: the largest absolute errors.  A wrong k mapping, a stale or torn hand-off of h_{t-1}, a lost
    row or column shows as an O(0.1) error; fp32 accumulation order as ~1e-6."""
    h_all, c_all, gates = (x.detach().cpu().to(F32) for x in (h_all, c_all, gates))
    gx, w_hh = gx.detach().cpu().to(F32), w_hh.detach().cpu().to(F32)
    bias = None if bias is None else bias.detach().cpu().to(F32)
    err = {"h": 0.0, "c": 0.0, "gates": 0.0}
    for t in range(T):
        rows = slice(t * B, (t + 1) * B)
        prev = slice((t - 1) * B, t * B)
        g = gx[rows] if t < n_gx else bias.expand(B, -1)
        h, c, s = fwd_step(g, h_all[prev] if t else None, c_all[prev] if t else None, w_hh)
        for name, got, ref in (("h", h_all[rows], h), ("c", c_all[rows], c), ("gates", gates[rows], s)):
            d = (got.to(F64) - ref).abs()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)          # an unwritten (NaN) element is an error
            err[name] = max(err[name], d.max().item())
    err["worst"] = max(err.values())
    return err


def bwd_teacher_forced(dg_all, w_hh, dh_out, dh_first, c_all, gates, T, B, H):
    """Every step of fp32 dG results [T*B, 4H] against fp64 math from bf16r(dG_{t+1} of the results themselves); the reference's own fp64
    dc chain.  Returns {"worst": largest absolute error, "ref_max": max|ref|, "bound": bwd_bound(ref_max)}."""
    dg_all = dg_all.detach().cpu().to(F32)
    w_hh, c_all, gates = (x.detach().cpu().to(F32) for x in (w_hh, c_all, gates))
    dh_out = None if dh_out is None else dh_out.detach().cpu().to(F32)
    first = dh_first if dh_first is not None else 0
    dc = None
    worst = ref_max = 0.0
    for t in range(T - 1, -1, -1):
        rows = slice(t * B, (t + 1) * B)
        dho = dh_out[(t - first) * B:(t - first + 1) * B] if dh_out is not None and t >= first else None
        ref, dc = bwd_step(dg_all[(t + 1) * B:(t + 2) * B] if t < T - 1 else None, w_hh, dho, gates[rows], c_all[rows],
                           c_all[(t - 1) * B:t * B] if t else None, dc)
        d = (dg_all[rows].to(F64) - ref).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        worst = max(worst, d.max().item())
        ref_max = max(ref_max, ref.abs().max().item())
    return {"worst": worst, "ref_max": ref_max, "bound": bwd_bound(ref_max)}


def bwd_bound(ref_max):
    return BWD_REL * ref_max + BWD_ABS


# ----------------------------------------------------------------------------------------------------------------- the row images
def image_view(ws, layout, rows, which="rows", base=0):
    """the int16 view [rows, ld] of an image inside a workspace (uint8 tensor): layout from ops.seq_bf16_layout, base = byte offset of
    the workspace of a pair's second layer"""
    off, ld, kpad = layout[which]
    img = ws[base + off:base + off + rows * ld * 2].view(torch.int16).view(rows, ld)
    return img, kpad


def bf16_bits(x):
    """the int16 bit patterns of bf16(x), x fp32"""
    return x.detach().to(F32).to(torch.bfloat16).view(torch.int16)
