"""Every entry point of the decode driver on every path it can take (tools, GPU box): greedy, greedy with the weight cache, sampled,
scheduled, the encode hand-out and the beam depth step (cached / precomputed vid_rnn half / plain), each under the five option sets
that select the driver's paths (fused, two chains, and the two-lane loop through persist = 0, pipe_block = 0 and gemm mode 0), at two
small ragged shapes and at c5 with B = 128.  Seeded inputs; every line carries the first argument as a tag, the sha1 of every output,
the launch counts s2vt_prof_read reports for kinds 0 (GEMM), 1 (forward steps) and 4 (argmax) of ONE call, the median time of 5 calls
(HIP events) and the median host time of a call up to the point before the synchronisation: two library builds on one box
(S2VT_LIB, interleaved processes) compare for bit-equal results, equal launch sequences and speed.
usage: [S2VT_LIB=<library>] python tools/bench_decode_paths.py [TAG]"""
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2vt_video_caption_amd  # noqa
from s2vt_video_caption_amd import build, capi, functional, ops, synth
from bench_sha import sha, show

TAG = sys.argv[1] if len(sys.argv) > 1 else "-"
if not os.environ.get("S2VT_LIB"):
    build.build()
try:
    lib = capi.load()
except AttributeError:      # a build from before s2vt_decode_plan: everything else here is older than that
    del capi.SIGNATURES["s2vt_decode_plan"]
    lib = capi.load()
DEV = "cuda:0"
DEFAULTS = dict(gemm_mode=3, persist=1, persist_x3_fwd=1, pipe_block=32, decode_fused=1, pad_min_batch=33)
PATHS = (("fused", {}), ("two_chains", dict(decode_fused=0)), ("persist0", dict(persist=0)), ("pipe_block0", dict(pipe_block=0)),
         ("gemm_mode0", dict(gemm_mode=0)))
c5 = synth.CONFIGS["c5"]
SHAPES = ((64, 5, 70, 44, 28, 61), (128, 4, 36, 100, 52, 333), (128, c5["L"], c5["F"], c5["H"], c5["E"], c5["V"]))
_ptr, _stream = functional._ptr, functional._stream


def measure(name, fn):
    """one warm-up, one profiled call (launch counts), 5 timed calls (sha1 of each one's outputs)"""
    out = fn()
    torch.cuda.synchronize()
    if out is None:
        print("%s %s: not taken by this path" % (TAG, name), flush=True)
        return
    lib.s2vt_prof_enable(1)
    lib.s2vt_prof_reset()
    fn()
    torch.cuda.synchronize()
    counts = [capi.prof_read(k)[1] for k in (0, 1, 4)]
    lib.s2vt_prof_enable(0)
    ms, host, shas = [], [], []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        shas.append(sha(out))
    show(TAG, "%s: launches %d/%d/%d median %.4f ms (min %.4f, max %.4f) host %.4f ms" %
         (name, counts[0], counts[1], counts[2], statistics.median(ms), min(ms), max(ms), statistics.median(host)), shas)


for dims in SHAPES:
    B, L, F, H, E, V = dims
    sd = synth.make_state_dict(V, F, H, E, seed=11)
    import S2VTModel
    m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E)
    m.load_state_dict(sd)
    m.to(DEV).eval()
    plist = tuple(m.state_dict()[k] for k in capi.PARAM_KEYS)
    feats, caps, _ = synth.make_batch(B, L, F, V, seed=12)
    feats, targets = feats.to(DEV), caps[:, :-1].contiguous().to(DEV)
    g = torch.Generator().manual_seed(13)
    R = 5 * B
    row_b = torch.arange(B, dtype=torch.int32).repeat_interleave(5).to(DEV)
    row_state = torch.randperm(R, generator=g).to(torch.int32).to(DEV)
    tok = torch.randint(0, V, (R,), generator=g, dtype=torch.int32).to(DEV)
    vid_h, vid_c, word_h, word_c = [(torch.randn(n, H, generator=g) * 0.5).to(DEV) for n in (B, B, R, R)]
    gx_vid = torch.randn(B, 4 * H, generator=g).to(DEV)
    d = capi.Dims(*dims)
    ps = functional._params_struct(capi.Params, plist)
    nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(d), R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def beam_cached(gx):
        """s2vt_beam_step_cached / s2vt_beam_step_gx on the model's decode cache (None: no cache in this mode)"""
        cache, valid = functional.decode_cache_entry(m, plist, d, feats.device, lib)
        if cache is None or not valid:
            return None
        vh, vc = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
        wh, wc = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV)
        tix, tlp = torch.empty(R, 20, dtype=torch.int32, device=DEV), torch.empty(R, 20, device=DEV)
        tail = (_ptr(word_h), _ptr(word_c), _ptr(wh), _ptr(wc), _ptr(tix), _ptr(tlp), _ptr(ws), nbytes, _ptr(cache), cache.numel(), _stream(feats.device))
        if gx:
            capi.check(lib.s2vt_beam_step_gx(ctypes.byref(d), ctypes.byref(ps), R, _ptr(row_b), _ptr(row_state), _ptr(tok), _ptr(gx_vid), *tail),
                       "s2vt_beam_step_gx")
            return wh, wc, tix, tlp
        capi.check(lib.s2vt_beam_step_cached(ctypes.byref(d), ctypes.byref(ps), R, _ptr(row_b), _ptr(row_state), _ptr(tok), _ptr(vid_h), _ptr(vid_c),
                                             _ptr(vh), _ptr(vc), *tail), "s2vt_beam_step_cached")
        return vh, vc, wh, wc, tix, tlp

    entries = (
        ("greedy", lambda: functional.greedy_decode(feats, plist, 0)),
        ("greedy_cached", lambda: functional.greedy_decode(feats, plist, 0, owner=m)),
        ("sample", lambda: functional.greedy_decode(feats, plist, 0, owner=m, sample=(0.5, 20261))),
        ("scheduled", lambda: functional.scheduled_inputs(feats, targets, plist, 0.5, seed=7, owner=m, return_draws=True)),
        ("encode_hand_out", lambda: functional.decode_encode(feats, plist, m, depth=min(6, L - 1))),
        ("beam_step_cached", lambda: beam_cached(False)),
        ("beam_step_gx", lambda: beam_cached(True)),
        ("beam_step", lambda: ops.beam_step(plist, dims, row_b, row_state, tok, vid_h, vid_c, word_h, word_c)),
    )
    for path, kv in PATHS:
        prev = {k: lib.s2vt_set_option(k.encode(), v) for k, v in dict(DEFAULTS, **kv).items()}
        functional.clear_decode_cache(m)
        plan = capi.decode_plan(dims) if "s2vt_decode_plan" in capi.SIGNATURES else None
        for name, fn in entries:
            measure("B=%d L=%d H=%d V=%d %s %s" % (B, L, H, V, path, name), fn)
        print("%s B=%d L=%d H=%d V=%d %s plan %s" % (TAG, B, L, H, V, path, plan), flush=True)
        for k, v in prev.items():
            lib.s2vt_set_option(k.encode(), v)
    capi.check_async_error()
