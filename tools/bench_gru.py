"""GRU S2VT at BASELINE configs[1] (B=64, L=80, F=4096, H=E=1000, V=12000), in one process, the cases alternating round by round
after their warm-up: the GRU train step (forward, MaskCriterion, backward, torch.optim.Adam), the GRU greedy decode per call, and
for comparison the LSTM model's train step with option persist=0 (its launch-per-timestep recurrence).  Prints one JSON line
of medians in ms.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_gru.py --rounds 1`.

--kernels: the recurrences alone instead, for a controlled per-timestep comparison of the two cells at the same (B, H): one
layer of T = 2L-1 steps through the per-op entry points s2vt_{gru,lstm}_seq_fwd / _seq_bwd (launch per timestep, one stream,
nothing else on the device, buffers allocated outside the timed region), alternating GRU and LSTM; microseconds per timestep.

  python tools/bench_gru.py [--steps 10] [--warmup 3] [--rounds 3] [--kernels]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="time the recurrences alone (per-op seq entries), not the model")
    a = ap.parse_args()
    if a.kernels:
        return bench_kernels(a)
    import S2VTModel
    import utils
    from s2vt_video_caption_amd import build, capi, synth
    from s2vt_video_caption_amd.optim import FlatAdam
    build.build()
    lib = capi.load()
    dev = "cuda:0"
    d = synth.CONFIGS["c2"]
    B, L, F, H, E, V = (d[k] for k in "BLFHEV")
    feats, caps, mask = (t.to(dev) for t in synth.make_batch(B, L, F, V, seed=1241))
    crit = utils.MaskCriterion()

    gru = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E, rnn_type="gru")
    gru.load_state_dict(synth.make_gru_state_dict(V, F, H, E, seed=7))
    gru.to(dev)
    gopt = torch.optim.Adam(gru.parameters(), lr=1e-4)
    lstm = S2VTModel.S2VT(V, F, L, dim_hid=H, dim_embed=E)
    lstm.load_state_dict(synth.make_state_dict(V, F, H, E, seed=7))
    lstm.to(dev)
    lopt = FlatAdam(lstm, lr=1e-4)

    def gru_train():
        gopt.zero_grad()
        gru.train()
        crit(gru(feats, targets=caps[:, :-1], mode="train"), caps, mask).backward()
        gopt.step()

    def gru_decode():
        gru.eval()
        with torch.no_grad():
            gru(feats, mode="test")

    def lstm_train():
        prev = lib.s2vt_set_option(b"persist", 0)
        try:
            lopt.zero_grad()
            lstm.train()
            crit(lstm(feats, targets=caps[:, :-1], mode="train"), caps, mask).backward()
            lopt.step()
        finally:
            lib.s2vt_set_option(b"persist", prev)

    cases = {"gru_train_step_ms": gru_train, "gru_greedy_decode_ms": gru_decode, "lstm_persist0_train_step_ms": lstm_train}
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
    out = {"config": "configs[1] B=64 L=80 F=4096 H=E=1000 V=12000", "steps_per_round": a.steps, "rounds": a.rounds}
    for k, v in times.items():
        v = sorted(v)
        out[k] = round(v[len(v) // 2], 3)
    print(json.dumps(out))


def bench_kernels(a):
    from s2vt_video_caption_amd import build, capi, synth
    from s2vt_video_caption_amd.functional import _ptr, _stream
    build.build()
    lib = capi.load()
    dev = "cuda:0"
    d = synth.CONFIGS["c2"]
    B, H, T = d["B"], d["H"], 2 * d["L"] - 1
    g = torch.Generator().manual_seed(0)
    k = H ** -0.5

    def u(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * k).to(dev)
    st = _stream(dev)
    bufs = {}
    for cell, G in (("gru", 3), ("lstm", 4)):
        bufs[cell] = dict(w=u(G * H, H), b=u(G * H), b2=u(G * H), gx=torch.randn(T * B, G * H, generator=g).to(dev),
                          dh=torch.randn(T * B, H, generator=g).to(dev), h=torch.empty(T * B, H, device=dev),
                          c=torch.empty(T * B, H, device=dev), stash=torch.empty(T * B, 4 * H, device=dev),
                          wt=torch.empty(H, G * H, device=dev), dcarry=torch.empty(B, H, device=dev),
                          dgx=torch.empty(T * B, 3 * H, device=dev), dgh=torch.empty(T * B, 3 * H, device=dev))

    def gru_fwd():
        q = bufs["gru"]
        capi.check(lib.s2vt_gru_seq_fwd(T, B, H, _ptr(q["gx"]), T, _ptr(q["b2"]), _ptr(q["w"]), _ptr(q["b"]), _ptr(q["h"]),
                                        _ptr(q["stash"]), st), "s2vt_gru_seq_fwd")

    def gru_bwd():
        q = bufs["gru"]
        capi.check(lib.s2vt_gru_seq_bwd(T, B, H, _ptr(q["w"]), _ptr(q["dh"]), 0, _ptr(q["h"]), _ptr(q["stash"]), _ptr(q["wt"]),
                                        _ptr(q["dcarry"]), _ptr(q["dgx"]), _ptr(q["dgh"]), st), "s2vt_gru_seq_bwd")

    def lstm_fwd():         # the gate input is the stash buffer (in place), refreshed before the call (untimed)
        q = bufs["lstm"]
        capi.check(lib.s2vt_lstm_seq_fwd(T, B, H, _ptr(q["stash"]), T, _ptr(q["b"]), _ptr(q["w"]), _ptr(q["h"]), _ptr(q["c"]),
                                         _ptr(q["stash"]), st), "s2vt_lstm_seq_fwd")

    def lstm_bwd():         # consumes the stash in place: the forward before it (untimed) writes a fresh one
        q = bufs["lstm"]
        capi.check(lib.s2vt_lstm_seq_bwd(T, B, H, _ptr(q["w"]), _ptr(q["dh"]), 0, _ptr(q["c"]), _ptr(q["stash"]), _ptr(q["wt"]),
                                         _ptr(q["dcarry"]), st), "s2vt_lstm_seq_bwd")

    def lstm_prep_fwd():
        bufs["lstm"]["stash"].copy_(bufs["lstm"]["gx"])

    def lstm_prep_bwd():
        lstm_prep_fwd()
        lstm_fwd()
    gru_fwd()
    cases = {"gru_fwd_us_per_step": (None, gru_fwd), "lstm_fwd_us_per_step": (lstm_prep_fwd, lstm_fwd),
             "gru_bwd_us_per_step": (None, gru_bwd), "lstm_bwd_us_per_step": (lstm_prep_bwd, lstm_bwd)}
    times = {n: [] for n in cases}
    for r in range(a.warmup + a.rounds * a.steps):
        for n, (prep, fn) in cases.items():
            if prep:
                prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[n].append(e0.elapsed_time(e1) * 1000.0 / T)
    capi.check_async_error()
    out = {"config": "one layer, T=%d steps, B=%d, H=%d, launch per timestep, alone on the device" % (T, B, H),
           "calls": a.rounds * a.steps}
    for n, v in times.items():
        v = sorted(v)
        out[n] = round(v[len(v) // 2], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
