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

Constrained decoding (S2VT.decode_constrained; csrc/truncate.hip, include/s2vt_hip.h "constrained draw") is restated here too -
`constrain_logits`.  For one row at decode step t (t words generated after <sos>, history h[0..t)), on the RAW logits x, in order:

    1. repetition penalty theta >= 1 (1: off): once per DISTINCT v of h, x_v <- x_v * r if x_v > 0 else x_v * theta, with
       r = fp32(1.0 / (double)theta) - multiplications, so the fp32 restatement is bitwise
    2. no-repeat n-gram n >= 0 (0: off): if t >= n - 1, every i in [0, t - n] with h[i .. i+n-2] == h[t-n+1 .. t-1] sets
       x[h[i+n-1]] <- -inf (n = 1 bans every word of h)
    3. banned ids: x_v <- -inf
    4. minimum length m: if t < m, x[eos_ix] <- -inf

A ban wins over a penalty.  Then the arg-max (greedy; lowest index on a tie) or steps 1-4 of the truncated draw above.
"""
import collections

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


MAX_BANNED = 32                          # banned ids of one call (they travel in the row kernel's launch arguments)
MAX_HISTORY = 1023                       # the longest history a row kernel stages: length - 1 <= 1024
ConstraintSpec = collections.namedtuple("ConstraintSpec", "no_repeat_ngram repetition_penalty min_length eos_ix banned")


def _is_int(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def check_constraints(no_repeat_ngram_size, repetition_penalty, min_length, banned_ids, V, eos_ix, length=None):
    """A ConstraintSpec (repetition_penalty as the fp32 value the library gets, banned as a tuple of distinct ints) or ValueError -
    before anything reaches the library.  length: the model's L, for the drivers' rule that no step may ban a whole row,
    V > (L - 1) + n_banned + 1, and for the history bound L - 1 <= 1024."""
    V = int(V)
    if not _is_int(no_repeat_ngram_size) or int(no_repeat_ngram_size) < 0:
        raise ValueError("no_repeat_ngram_size must be an integer >= 0 (0: off), got %r" % (no_repeat_ngram_size,))
    if isinstance(repetition_penalty, (bool, str)) or not isinstance(repetition_penalty, (int, float, np.integer, np.floating)):
        raise ValueError("repetition_penalty must be a finite number >= 1 (1: off), got %r" % (repetition_penalty,))
    with np.errstate(over="ignore"):
        theta = float(np.float32(repetition_penalty))
    if not 1.0 <= theta < float("inf"):
        raise ValueError("repetition_penalty must be a finite number >= 1 (1: off), got %r" % (repetition_penalty,))
    if not _is_int(min_length) or int(min_length) < 0:
        raise ValueError("min_length must be an integer >= 0, got %r" % (min_length,))
    banned = [] if banned_ids is None else list(banned_ids)
    if any(not _is_int(b) or not 0 <= int(b) < V for b in banned):
        raise ValueError("banned_ids must be integers in [0, vocab_size = %d), got %r" % (V, banned_ids))
    banned = tuple(sorted(set(int(b) for b in banned)))
    if len(banned) > MAX_BANNED:
        raise ValueError("banned_ids: at most %d distinct ids, got %d" % (MAX_BANNED, len(banned)))
    if not _is_int(eos_ix) or not 0 <= int(eos_ix) < V:
        raise ValueError("eos_ix must be an integer in [0, vocab_size = %d), got %r" % (V, eos_ix))
    if length is not None:
        if int(length) - 1 > MAX_HISTORY + 1:
            raise ValueError("length %d: constrained decoding keeps at most %d words of history" % (int(length), MAX_HISTORY))
        if not V > (int(length) - 1) + len(banned) + 1:
            raise ValueError("vocab_size %d <= (length - 1) + banned ids + 1 = %d: the constraints could ban a whole row"
                             % (V, int(length) - 1 + len(banned) + 1))
    return ConstraintSpec(int(no_repeat_ngram_size), theta, int(min_length), int(eos_ix), banned)


def constrains(spec):
    """whether a ConstraintSpec of check_constraints changes any logit at any step"""
    return spec.no_repeat_ngram > 0 or spec.repetition_penalty != 1.0 or spec.min_length > 0 or len(spec.banned) > 0


def constraints_struct(spec):
    """(capi.Constraints, keep-alive): the spec as the library's s2vt_constraints (the banned ids in host memory)"""
    import ctypes

    from . import capi
    arr = (ctypes.c_int32 * max(1, len(spec.banned)))(*spec.banned)
    c = capi.Constraints(spec.no_repeat_ngram, spec.repetition_penalty, spec.min_length, spec.eos_ix, len(spec.banned),
                         ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)))
    return c, arr


def constrain_logits(x, hist_ids, t, spec):
    """The constrained logits of decode step t (rules 1-4 of the definition above): x float32 or float64 [rows, V] (or [V]), hist_ids
    ints [rows, >= t] (or [>= t]) - row r's history is hist_ids[r, :t].  A new array of x's dtype: in float32 bit for bit what the
    row kernel leaves in its logits buffer; in float64 the same rules with the same fp32 factors (theta and r as the device holds
    them).  History ids outside [0, V) are matched like any other and never written."""
    x = np.array(x, copy=True)
    if x.dtype not in (np.float32, np.float64):
        raise ValueError("x must be float32 or float64")
    out = x.reshape(1, -1) if x.ndim == 1 else x
    rows, V = out.shape
    t = int(t)
    h = np.asarray(hist_ids, dtype=np.int64).reshape(rows, -1)[:, :t] if t > 0 else np.zeros((rows, 0), dtype=np.int64)
    if h.shape[1] != t:
        raise ValueError("hist_ids holds fewer than t = %d words" % t)
    theta = x.dtype.type(np.float32(spec.repetition_penalty))
    r = x.dtype.type(np.float32(1.0 / float(np.float32(spec.repetition_penalty))))
    n = spec.no_repeat_ngram
    for row in range(rows):
        hr = h[row].tolist()
        if theta != 1:
            for v in sorted(set(hr)):
                if 0 <= v < V:
                    out[row, v] = out[row, v] * r if out[row, v] > 0 else out[row, v] * theta
        if n > 0 and t >= n - 1:
            suffix = hr[t - n + 1:t]
            for i in range(0, t - n + 1):
                if hr[i:i + n - 1] == suffix and 0 <= hr[i + n - 1] < V:
                    out[row, hr[i + n - 1]] = -np.inf
        for v in spec.banned:
            out[row, v] = -np.inf
        if t < spec.min_length:
            out[row, spec.eos_ix] = -np.inf
    return x


def sample_rows(model, feats, params, K, temperature, seed, top_k=0, top_p=1.0, constraints=None):
    """ids int64 [B, K, L-1]: K draws per clip on ONE encode - s2vt_sample_decode_rows; with a truncating (top_k, top_p) (already
    through check_truncation) s2vt_sample_decode_rows_trunc: the same driver with the logits GEMM and the truncated draw as head.  Row b*K + k draws with the noise of
    (seed, decode step, batch row b*K + k, v): the draw of mode='sample' on feats.repeat_interleave(K, 0).  With the model's decode
    cache where a decode of the batch takes the plane path's persistent encode (filled here on fresh weights), on the fp32-input
    MFMA path otherwise.  On the device, no host synchronisation, no gradient.
    constraints = (ConstraintSpec, greedy): s2vt_decode_rows_constrained - the same driver with the constrained draw as head (greedy:
    the arg-max of the constrained row, temperature 1 / top_k 0 / top_p 1; else the truncated draw on it)."""
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
        size = lib.s2vt_decode_rows_constrained_workspace_bytes if constraints is not None else (
            lib.s2vt_sample_rows_trunc_workspace_bytes if trunc else lib.s2vt_sample_rows_workspace_bytes)
        nbytes = size(ctypes.byref(d), K)
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
            if constraints is not None:
                cs, keep = constraints_struct(constraints[0])
                capi.check(lib.s2vt_decode_rows_constrained(ctypes.byref(d), ctypes.byref(ps), F._ptr(feats), K, int(model.sos_ix),
                                                            1 if constraints[1] else 0, temperature, seed, top_k, top_p, ctypes.byref(cs),
                                                            *tail), "s2vt_decode_rows_constrained")
            elif trunc:
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
