"""The sampled decode's noise, restated in numpy (host side; float64).

`mode='sample'` draws a token from softmax(logit / temperature) as the arg-max of `logit / temperature + g` with g i.i.d.
standard Gumbel noise (Gumbel-max).  The device generates g inside the arg-max kernels' epilogues (csrc/philox.h); this module is
the same definition written a second time - what the tests compare the device against, and the documentation of the mapping:

    one draw per (seed, decode step, batch row, vocabulary index v)
    key     = (seed & 0xFFFFFFFF, seed >> 32)
    counter = (v // 4, batch row, decode step, STREAM_TAG)
    x       = word v % 4 of philox4x32_10(counter, key)
    u       = ((x >> 9) + 0.5) * 2**-23           (exact in fp32, strictly inside (0, 1))
    g       = -log(-log(u))                       (in [-2.82, 16.64])

Nothing of a kernel's tiling, of the batch padding or of the launch enters.

Top-k / nucleus truncation ahead of the draw (`top_k`, `top_p` of S2VT.sample_truncated; csrc/truncate.hip,
include/s2vt_hip.h "truncated draw") is restated here as well - `truncation_mask`.  For a logits row x, inv_t = 1 / temperature:

    1. scores   s_v = x_v * inv_t in fp32 (the heads' expression)
    2. top-k    (k = 0 or k >= V: off)  tau = the k-th largest s, counted with multiplicity; survivors {v : s_v >= tau} - equal
                values at the k-th place all stay, so at least k elements survive
    3. nucleus  (p >= 1: off, not evaluated) over the survivors of 2:  m = max s, e_v = exp(s_v - m), Z = sum e_v;  v stays iff
                A(s_v) < p * Z with A(y) = sum of e_u over {u : s_u > y}: the shortest descending prefix whose mass reaches p,
                renormalised over the top-k set ("top-k, then top-p"); equal values stay or go together, the maximum always stays
    4. draw     token = argmax over the kept v of (s_v + g_v), lowest index on a tie, g the noise above - with nothing truncated,
                today's draw
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
STREAM_TAG = 0x47554D42                  # "GUMB": counter word 3 of the sampler's stream (GUMBEL_STREAM_TAG of csrc/philox.h)
SS_STREAM_TAG = 0x53534D58               # "SSMX": counter word 3 of the scheduled-sampling coins (SS_STREAM_TAG of csrc/philox.h)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other);
    returns uint32 [..., 4]."""
    counter = np.asarray(counter, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., i], shape).astype(np.uint64) for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(W0)) & _MASK32, (k[1] + np.uint64(W1)) & _MASK32]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform_from_bits(x):
    """u = ((x >> 9) + 0.5) * 2^-23 in float64 (the value is exact in fp32 as well)"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_from_bits(x):
    u = uniform_from_bits(x)
    return -np.log(-np.log1p(-(1.0 - u)))    # 1 - u is exact; log1p keeps -log(u) accurate next to u = 1


def gumbel_noise(seed, step, rows, V):
    """float64 [len(rows), V]: the noise of decode step `step` for the batch rows `rows` (an int n means rows 0..n-1)."""
    rows = np.arange(rows, dtype=np.uint32) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint32)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    nblk = (int(V) + 3) // 4
    counter = np.empty((rows.shape[0], nblk, 4), dtype=np.uint32)
    counter[..., 0] = np.arange(nblk, dtype=np.uint32)[None, :]
    counter[..., 1] = rows[:, None]
    counter[..., 2] = np.uint32(step)
    counter[..., 3] = np.uint32(STREAM_TAG)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    bits = philox4x32_10(counter, key).reshape(rows.shape[0], nblk * 4)[:, :int(V)]
    return gumbel_from_bits(bits)


def ss_coin(seed, step, rows):
    """float32 [len(rows)]: the scheduled-sampling coins of decode step `step` for the batch rows `rows` (an int n means rows
    0..n-1): u = ((x >> 9) + 0.5) * 2^-23 with x = word 0 of philox4x32_10((0, row, step, SS_STREAM_TAG), seed halves) - exact
    in fp32, strictly inside (0, 1).  The step is fed the model's own previous word where coin < np.float32(p)."""
    rows = np.arange(rows, dtype=np.uint32) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint32)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    counter = np.zeros((rows.shape[0], 4), dtype=np.uint32)
    counter[:, 1] = rows
    counter[:, 2] = np.uint32(step)
    counter[:, 3] = np.uint32(SS_STREAM_TAG)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return uniform_from_bits(philox4x32_10(counter, key)[:, 0]).astype(np.float32)


def ss_used(targets, draws, p, seed, row0=0):
    """int64 [B, T]: the words a scheduled pass feeds - targets[:, 0], then draws[:, j-1] where ss_coin < float32(p), targets[:, j]
    otherwise (numpy arrays; the definition the device is compared against)."""
    targets, draws = np.asarray(targets, dtype=np.int64), np.asarray(draws, dtype=np.int64)
    used = targets.copy()
    rows = np.arange(targets.shape[0], dtype=np.uint32) + np.uint32(row0)
    for j in range(1, targets.shape[1]):
        own = ss_coin(seed, j, rows) < np.float32(p)
        used[own, j] = draws[own, j - 1]
    return used


def draw_seed(generator=None):
    """A 63-bit seed from torch's default (CPU) generator: `torch.manual_seed` makes a run of seed=None calls reproducible."""
    import torch
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=generator).item())


def check_sample_args(temperature, seed):
    """(temperature as float, seed as int in [0, 2^64)) or ValueError - before anything reaches the library"""
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    seed = draw_seed() if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64), got %r" % (seed,))
    return t, seed


def check_n_samples(n_samples):
    """n_samples as an int >= 1 or ValueError (2.5, '3', True and 0 are refused) - before anything reaches the library"""
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or int(n_samples) < 1:
        raise ValueError("n_samples must be an integer >= 1, got %r" % (n_samples,))
    return int(n_samples)


def check_truncation(top_k, top_p, V):
    """(top_k as int in [0, V], top_p as float in (0, 1]) or ValueError (top_k: ints only - True, 2.5 and '3' are refused; top_p:
    NaN is refused) - before anything reaches the library.  0 / 1.0 are 'off'."""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 0 <= int(top_k) <= int(V):
        raise ValueError("top_k must be an integer in [0, vocab_size = %d] (0: off), got %r" % (int(V), top_k))
    if isinstance(top_p, (bool, str)) or not isinstance(top_p, (int, float, np.integer, np.floating)) or not 0.0 < float(top_p) <= 1.0:
        raise ValueError("top_p must be a number in (0, 1] (1: off), got %r" % (top_p,))
    return int(top_k), float(top_p)


def truncates(top_k, top_p, V):
    """whether (top_k, top_p) of check_truncation cut anything off a row of V scores"""
    return 0 < top_k < V or top_p < 1.0


def truncation_mask(scores, top_k, top_p):
    """bool [rows, V]: the elements that steps 2-3 of the definition above keep, in float64 on a [rows, V] score array (scores =
    logits * inv_t; what the device's `kept` counts and its draws stay inside)."""
    s = np.asarray(scores, dtype=np.float64)
    rows, V = s.shape
    keep = np.ones((rows, V), dtype=bool)
    if 0 < top_k < V:
        tau = np.sort(s, axis=1)[:, V - top_k]                        # the k-th largest, with multiplicity
        keep = s >= tau[:, None]
    if top_p < 1.0:
        e = np.where(keep, np.exp(s - s.max(axis=1, keepdims=True)), 0.0)
        Z = e.sum(axis=1)
        order = np.argsort(-s, axis=1, kind="stable")
        ss, es = np.take_along_axis(s, order, 1), np.take_along_axis(e, order, 1)
        before = np.cumsum(es, axis=1) - es                           # the mass in front of each element of the descending order ...
        first = np.ones((rows, V), dtype=bool)
        first[:, 1:] = ss[:, 1:] != ss[:, :-1]
        # ... and in front of its run of equal values: A(s_v), the mass of the strictly larger scores
        A_sorted = np.maximum.accumulate(np.where(first, before, 0.0), axis=1)
        A = np.empty_like(A_sorted)
        np.put_along_axis(A, order, A_sorted, 1)
        keep = keep & (A < top_p * Z[:, None])
    return keep


def sample_rows(model, feats, params, K, temperature, seed, top_k=0, top_p=1.0):
    """ids int64 [B, K, L-1]: K draws per clip on ONE encode - s2vt_sample_decode_rows; with a truncating (top_k, top_p) (already
    through check_truncation) s2vt_sample_decode_rows_trunc: the same driver with the logits GEMM and the truncated draw as head.  Row b*K + k draws with the noise of
    (seed, decode step, batch row b*K + k, v): the draw of mode='sample' on feats.repeat_interleave(K, 0).  With the model's decode
    cache where a decode of the batch takes the plane path's persistent encode (filled here on fresh weights), on the fp32-input
    MFMA path otherwise.  On the device, no host synchronisation, no gradient."""
    import ctypes

    import torch

    from . import capi
    from . import functional as F
    with torch.no_grad():
        lib = capi.load()
        F.require_hip(feats, "feats")
        feats = F._f32c(feats, "feats")
        raw = params
        params = tuple(F._f32c(p.detach(), "parameter") for p in params)
        d = F._dims(feats, params)
        trunc = truncates(top_k, top_p, d.V)
        nbytes = (lib.s2vt_sample_rows_trunc_workspace_bytes if trunc else lib.s2vt_sample_rows_workspace_bytes)(ctypes.byref(d), K)
        if nbytes <= 0:
            raise ValueError("sample: %d clips x %d samples is not a shape the library serves" % (d.B, K))
        dev = feats.device
        with torch.cuda.device(dev):
            cache, valid = None, False
            # (the plane path where a greedy decode of this batch takes it: fewer than 24 clips run as they are on the
            # launch-per-timestep path - api_internal.h, batch_pads)
            if capi.decode_plan(d, encode_only=False)[1]:
                cache, valid = F.decode_cache_entry(model, raw, d, dev, lib)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            ids = torch.empty(d.B, K, d.L - 1, dtype=torch.int64, device=dev)
            ps = F._params_struct(capi.Params, params)
            tail = (F._ptr(ids), F._ptr(ws), nbytes, F._ptr(cache), cache.numel() if cache is not None else 0, 1 if valid else 0,
                    F._stream(dev))
            if trunc:
                capi.check(lib.s2vt_sample_decode_rows_trunc(ctypes.byref(d), ctypes.byref(ps), F._ptr(feats), K, int(model.sos_ix),
                                                             temperature, seed, top_k, top_p, *tail), "s2vt_sample_decode_rows_trunc")
            else:
                capi.check(lib.s2vt_sample_decode_rows(ctypes.byref(d), ctypes.byref(ps), F._ptr(feats), K, int(model.sos_ix),
                                                       temperature, seed, *tail), "s2vt_sample_decode_rows")
            if cache is not None:
                entry = F._DECODE_CACHES.get(model)
                if entry is not None and entry[1] is cache:
                    entry[2] = True                 # (stream-ordered, as in functional.greedy_decode: the call wrote every image)
    return ids
