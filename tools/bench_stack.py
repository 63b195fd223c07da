"""Stacked-LSTM S2VT (num_layers = 2) on one GPU, in one process, the cases alternating round by round after their warm-up:
the train step (forward, MaskCriterion, backward, torch.optim.Adam) at BASELINE configs[1] (B=64, L=80, F=4096, H=E=1000,
V=12000) on the layer-wavefront chain kernels and on the layer-by-layer path (stack_functional.reference_layerwise), the
greedy decode at B = 64 and B = 128, and the train step at the reference defaults (B=16, H=E=512).  Prints one JSON line of
medians in ms.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_stack.py --rounds 1`.

--kernels: the recurrences alone: one N = 2 chain (4 layers, T = 2L-1) forward and backward through s2vt_lstm_chain_fwd / _bwd
against the same four layers through s2vt_lstm_seq_fwd / _bwd one after the other; microseconds per diagonal and per
layer-step.

  python tools/bench_stack.py [--steps 5] [--warmup 2] [--rounds 3] [--kernels]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(cases, a):
    from s2vt_video_caption_amd import capi
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    capi.check_async_error()
    for _ in range(a.rounds):
        for k, fn in cases.items():
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
    capi.check_async_error()
    return {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        return bench_kernels(a)
    import S2VTModel
    import utils
    from s2vt_video_caption_amd import build, synth
    from s2vt_video_caption_amd import stack_functional as S
    build.build()
    dev = "cuda:0"
    crit = utils.MaskCriterion()
    cases = {}

    def model(B, L, F, H, E, V):
        torch.manual_seed(7)
        m = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, num_layers=2).to(dev)
        feats, caps, mask = (t.to(dev) for t in synth.make_batch(B, L, F, V, seed=1241))
        return m, torch.optim.Adam(m.parameters(), lr=1e-4), feats, caps, mask

    def train(m, opt, feats, caps, mask, fn):
        def step():
            opt.zero_grad()
            m.train()
            crit(fn(m, feats, caps[:, :-1]), caps, mask).backward()
            opt.step()
        return step

    def decode(m, feats):
        def run():
            m.eval()
            with torch.no_grad():
                m(feats, mode="test")
        return run
    d = synth.CONFIGS["c2"]
    B, L, F, H, E, V = (d[k] for k in "BLFHEV")
    c2 = model(B, L, F, H, E, V)
    cases["c2_train_step_wavefront_ms"] = train(*c2, S.train_forward)
    cases["c2_train_step_layerwise_ms"] = train(*c2, S.reference_layerwise)
    cases["c2_greedy_decode_B64_ms"] = decode(c2[0], c2[2])
    feats128 = synth.make_batch(128, L, F, V, seed=1242)[0].to(dev)
    cases["c2_greedy_decode_B128_ms"] = decode(c2[0], feats128)
    ref = model(16, L, F, 512, 512, V)
    cases["refdefault_train_step_wavefront_ms"] = train(*ref, S.train_forward)
    cases["refdefault_train_step_layerwise_ms"] = train(*ref, S.reference_layerwise)
    out = {"config": "num_layers=2; c2: B=64 L=80 F=4096 H=E=1000 V=12000; refdefault: B=16 H=E=512",
           "steps_per_round": a.steps, "rounds": a.rounds}
    out.update(_timed(cases, a))
    print(json.dumps(out))


def bench_kernels(a):
    from s2vt_video_caption_amd import build, capi, ops, synth
    from s2vt_video_caption_amd.functional import _ptr, _stream
    build.build()
    lib = capi.load()
    dev = "cuda:0"
    d = synth.CONFIGS["c2"]
    B, H, L = d["B"], d["H"], d["L"]
    T, n = 2 * L - 1, 4
    g = torch.Generator().manual_seed(0)
    k = H ** -0.5

    def u(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * k).to(dev)
    layers = [dict(w_hh=u(4 * H, H), w_in=u(4 * H, H) if j else None, bias=u(4 * H), h=torch.empty(T * B, H, device=dev),
                   c=torch.empty(T * B, H, device=dev), stash=torch.empty(T * B, 4 * H, device=dev)) for j in range(n)]
    layers[0].update(gx=torch.randn(L * B, 4 * H, generator=g).to(dev), gx_t0=0, n_gx=L)
    layers[-1].update(dh_ext=torch.randn(T * B, H, generator=g).to(dev), dh_t0=0)
    for lay in layers:
        lay["dg"] = torch.empty(T * B, 4 * H, device=dev)
    seq = dict(stash=torch.randn(T * B, 4 * H, generator=g).to(dev), wt=torch.empty(H, 4 * H, device=dev), dc=torch.empty(B, H, device=dev))
    st = _stream(dev)

    def chain_fwd():
        ops.lstm_chain_fwd(T, B, H, layers)

    def chain_bwd():
        ops.lstm_chain_bwd(T, B, H, layers)

    def seq_fwd():          # four layers one after the other (gate inputs in place in the stash; the GEMMs are not timed)
        for lay in layers:
            capi.check(lib.s2vt_lstm_seq_fwd(T, B, H, _ptr(seq["stash"]), T, _ptr(lay["bias"]), _ptr(lay["w_hh"]), _ptr(lay["h"]),
                                             _ptr(lay["c"]), _ptr(seq["stash"]), st), "s2vt_lstm_seq_fwd")

    def seq_bwd():
        for lay in layers:
            capi.check(lib.s2vt_lstm_seq_bwd(T, B, H, _ptr(lay["w_hh"]), _ptr(layers[-1]["dh_ext"]), 0, _ptr(lay["c"]),
                                             _ptr(lay["dg"]), _ptr(seq["wt"]), _ptr(seq["dc"]), st), "s2vt_lstm_seq_bwd")
    chain_fwd()
    a.steps = max(1, a.steps)
    res = _timed({"chain_fwd": chain_fwd, "seq_fwd": seq_fwd, "chain_bwd": chain_bwd, "seq_bwd": seq_bwd}, a)
    diag = T + n - 1
    out = {"config": "chain of %d layers, T=%d, B=%d, H=%d, alone on the device" % (n, T, B, H),
           "chain_fwd_us_per_diagonal": round(res["chain_fwd"] * 1000 / diag, 2),
           "seq_fwd_us_per_layer_step": round(res["seq_fwd"] * 1000 / (n * T), 2),
           "chain_bwd_us_per_diagonal": round(res["chain_bwd"] * 1000 / diag, 2),
           "seq_bwd_us_per_layer_step": round(res["seq_bwd"] * 1000 / (n * T), 2),
           "chain_fwd_ms": res["chain_fwd"], "seq_fwd_ms": res["seq_fwd"], "chain_bwd_ms": res["chain_bwd"], "seq_bwd_ms": res["seq_bwd"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
