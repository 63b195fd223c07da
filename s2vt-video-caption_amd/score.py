"""Caption scoring, `S2VT.forward(mode='score')` (not in the reference): the log-likelihood of given captions under the model,
K candidates per clip, computed on the device by s2vt_score_captions (include/s2vt_hip.h).

    scores, lengths, token_logprobs = model(feats, targets=captions, mode='score', length_alpha=0.0)

`check_score_args` is pure (no library call except the workspace-size query, which needs no GPU) and runs before anything reaches
the library; `score_captions` is the binding: it hands the caption tensor's strides over and copies nothing.
"""
import ctypes
import math

import torch

from . import capi


def check_score_args(captions, B, L, dims, length_alpha):
    """(K, T, squeeze, alpha) of a mode='score' call or ValueError: captions int64 [B, T] (squeeze = True, K = 1) or [B, K, T] with
    2 <= T <= L, a unit token stride and non-negative batch / candidate strides (a stride of 0 - an expanded view - is fine);
    length_alpha finite and >= 0; and a shape the library serves (s2vt_score_workspace_bytes(dims, K, T) > 0)."""
    if not isinstance(captions, torch.Tensor):
        raise ValueError("mode='score': targets must be an int64 tensor [B, T] or [B, K, T], got %r" % (type(captions),))
    if captions.dtype != torch.int64:
        raise ValueError("mode='score': targets must be int64, got %s" % (captions.dtype,))
    if captions.dim() not in (2, 3):
        raise ValueError("mode='score': targets must be [B, T] or [B, K, T], got %s" % (tuple(captions.shape),))
    squeeze = captions.dim() == 2
    K = 1 if squeeze else int(captions.shape[1])
    T = int(captions.shape[-1])
    if int(captions.shape[0]) != int(B):
        raise ValueError("mode='score': targets' first dimension %d != the %d clips of feats" % (captions.shape[0], B))
    if K < 1:
        raise ValueError("mode='score': targets [B, K, T] needs K >= 1, got %s" % (tuple(captions.shape),))
    if not 2 <= T <= int(L):
        raise ValueError("mode='score': captions need 2 <= T <= length = %d tokens, got T = %d" % (L, T))
    if captions.stride(-1) != 1 or any(s < 0 for s in captions.stride()):
        raise ValueError("mode='score': targets need a unit token stride and non-negative strides, got %s" % (captions.stride(),))
    try:
        alpha = float(length_alpha)
    except (TypeError, ValueError):
        raise ValueError("mode='score': length_alpha must be a number, got %r" % (length_alpha,))
    if not math.isfinite(alpha) or alpha < 0:
        raise ValueError("mode='score': length_alpha must be finite and >= 0, got %r" % (length_alpha,))
    if dims is not None and capi.load().s2vt_score_workspace_bytes(ctypes.byref(dims), K, T) <= 0:
        raise ValueError("mode='score': %d clips x %d candidates x %d tokens is not a shape the library serves" % (B, K, T))
    return K, T, squeeze, alpha


@torch.no_grad()
def score_captions(model, feats, captions, params, length_alpha=0.7):
    """(scores fp32 [B(, K)], lengths int64 [B(, K)], token_logprobs fp32 [B(, K), T-1]) of `captions` (<sos>, words, <eos>,
    padding) for the clips `feats`: see s2vt_score_captions.  The K candidates of a clip share one encode; inference arithmetic
    (no dropout); on the device, no host synchronisation, no gradient.  With the model's decode cache where a decode of the batch
    takes the plane path's persistent encode (filled here on fresh weights), on the fp32-input MFMA path otherwise."""
    from . import functional as F
    lib = capi.load()
    F.require_hip(feats, "feats")
    feats = F._f32c(feats, "feats")
    raw = params
    params = tuple(F._f32c(p.detach(), "parameter") for p in params)
    d = F._dims(feats, params)
    K, T, squeeze, alpha = check_score_args(captions, d.B, d.L, d, length_alpha)
    F.require_hip(captions, "targets")
    dev = feats.device
    sb = captions.stride(0)
    sk = 0 if squeeze else captions.stride(1)
    with torch.cuda.device(dev):
        cache, valid = None, False
        # (the plane path where a greedy decode of this batch takes it: fewer than 24 clips run as they are on the launch-per-timestep
        # path, which is faster there than 64 padded rows - api_internal.h, batch_pads)
        if capi.decode_plan(d, encode_only=False)[1]:
            cache, valid = F.decode_cache_entry(model, raw, d, dev, lib)
        nbytes = lib.s2vt_score_workspace_bytes(ctypes.byref(d), K, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        shape = (d.B,) if squeeze else (d.B, K)
        token_lp = torch.empty(shape + (T - 1,), dtype=torch.float32, device=dev)
        scores = torch.empty(shape, dtype=torch.float32, device=dev)
        lengths = torch.empty(shape, dtype=torch.int64, device=dev)
        ps = F._params_struct(capi.Params, params)
        capi.check(lib.s2vt_score_captions(ctypes.byref(d), ctypes.byref(ps), F._ptr(feats), F._ptr(captions), sb, sk, K, T,
                                           int(model.eos_ix), alpha, F._ptr(token_lp), F._ptr(scores), F._ptr(lengths), F._ptr(ws),
                                           nbytes, F._ptr(cache), cache.numel() if cache is not None else 0, 1 if valid else 0,
                                           F._stream(dev)), "s2vt_score_captions")
        if cache is not None:
            entry = F._DECODE_CACHES.get(model)
            if entry is not None and entry[1] is cache:
                entry[2] = True                     # (stream-ordered, as in functional.greedy_decode: the call wrote every image)
    return scores, lengths, token_lp

