"""Cost of the ensemble beam search (S2VTModel.Ensemble; csrc/ensemble.hip) beside the cumulative-score search (mode='beam') of
ONE of its members, in one process on one MI355X.
Whole search: config 5 dims (L=80, F=4096, H=E=1000, V=12000), B = 128, width 5, depth 30; M = 3 members (three seeds of the seeded
weights), uniform weights.  Per depth the ensemble runs one policy launch, M depth steps up to their logits and one ensemble head;
mode='beam' runs one policy launch and one depth step with its own head - so about M times a member's depth minus M - 1 policy
launches is what to expect, a ratio to M x single near 1.  The legs ALTERNATE call by call; a call is timed with HIP events on the
stream (the encode phases included: M of them in an ensemble call), and its time per depth is the call time / the depths that call
actually ran (beam.LAST_DEPTHS).  Median and spread over --calls calls per leg after --warmup calls of each.
The head alone: s2vt_ensemble_top20 on 640 rows x 12000 words for M = 2, 3, 4 against s2vt_top20_logprob on 640 rows: --reps
launches between two HIP events (host enqueue included), legs alternating.
Appends what it prints to profiles/beam_ensemble.txt (or --out).

  python tools/bench_beam_ensemble.py [--calls 20] [--warmup 3] [--reps 20] [--batch 128] [--width 5] [--depth 30] [--members 3]
                                      [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import S2VTModel
from s2vt_video_caption_amd import beam, capi, synth

SOS, EOS = 3, 4
HEAD_ROWS, HEAD_V = 640, 12000


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def search_legs(a, d, dev, lines):
    feats = synth.make_batch(a.batch, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    models = []
    for i in range(a.members):
        m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
        m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=100 * i))
        models.append(m.to(dev).eval())
    ens = S2VTModel.Ensemble(models)
    legs = (("mode='beam'", lambda: models[0](feats, mode="beam", beam_width=a.width, max_beam_depth=a.depth)),
            ("Ensemble.beam", lambda: ens.beam(feats, beam_width=a.width, max_beam_depth=a.depth)))
    ms = {k: [] for k, _ in legs}
    per_depth = {k: [] for k, _ in legs}
    depths = {k: [] for k, _ in legs}
    paths = {}
    with torch.no_grad():
        for i in range(a.warmup + a.calls):
            for name, fn in legs:
                t, _ = _timed(fn, dev)
                paths[name] = beam.LAST_PATH
                if i >= a.warmup:
                    ms[name].append(t)
                    depths[name].append(beam.LAST_DEPTHS)
                    per_depth[name].append(t / beam.LAST_DEPTHS)
    med = {k: statistics.median(v) for k, v in per_depth.items()}
    call = {k: statistics.median(v) for k, v in ms.items()}
    lines.append("  the whole search: config 5 dims, B=%d, width %d, depth %d; Ensemble of %d members (seeds 0, 100, ..), uniform weights, "
                 "against mode='beam' of member 0; the two legs alternate in one process; HIP events around a call (encode phases "
                 "included); median of %d calls per leg after %d warm-up (min .. max):" % (
                     a.batch, a.width, a.depth, a.members, a.calls, a.warmup))
    for k, _ in legs:
        lines.append("  %-13s %8.3f ms per call, %2d..%2d depths run, %7.3f ms per depth (%.3f .. %.3f), %8.0f clips/s  [%s]" % (
            k, call[k], min(depths[k]), max(depths[k]), med[k], min(per_depth[k]), max(per_depth[k]), 1e3 * a.batch / call[k], paths[k]))
    M = a.members
    lines.append("  ratio Ensemble / (%d x mode='beam'): %.3f per depth, %.3f per call" % (
        M, med["Ensemble.beam"] / (M * med["mode='beam'"]), call["Ensemble.beam"] / (M * call["mode='beam'"])))
    capi.check_async_error()


def head_legs(a, dev, lines):
    lib = capi.load()
    rng = np.random.RandomState(3)
    x = torch.from_numpy((3.0 * rng.randn(4, HEAD_ROWS, HEAD_V)).astype(np.float32)).to(dev)
    ix = torch.empty(HEAD_ROWS, 20, dtype=torch.int32, device=dev)
    lp = torch.empty(HEAD_ROWS, 20, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def single():
        capi.check(lib.s2vt_top20_logprob(x.data_ptr(), x.stride(1), HEAD_ROWS, HEAD_V, ix.data_ptr(), lp.data_ptr(), st), "s2vt_top20_logprob")

    def head(fn, M):
        lw = (ctypes.c_float * M)(*([float(np.log(1.0 / M))] * M))

        def run():
            rc = fn(x.data_ptr(), x.stride(0), x.stride(1), M, HEAD_ROWS, HEAD_V, lw, ix.data_ptr(), lp.data_ptr(), st)
            assert rc == 0, rc
        return run
    legs = [("s2vt_top20_logprob", single)] + [("s2vt_ensemble_top20 M=%d" % M, head(lib.s2vt_ensemble_top20, M)) for M in (2, 3, 4)]
    us = {leg: [] for leg, _ in legs}
    for i in range(a.warmup + a.calls):
        for leg, fn in legs:
            def group():
                for _ in range(a.reps):
                    fn()
            t, _ = _timed(group, dev)
            if i >= a.warmup:
                us[leg].append(1000.0 * t / a.reps)
    base = statistics.median(us[legs[0][0]])
    lines.append("  the head alone, %d rows x %d words, uniform weights; %d launches between two HIP events (host enqueue included), legs "
                 "alternating, median of %d groups after %d warm-up (min .. max):" % (HEAD_ROWS, HEAD_V, a.reps, a.calls, a.warmup))
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %-30s %8.1f us per launch (%.1f .. %.1f)  %.2f x s2vt_top20_logprob" % (leg, med, min(us[leg]), max(us[leg]), med / base))
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=5)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_ensemble.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_ensemble.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    lines = ["", "tools/bench_beam_ensemble.py:"]
    search_legs(a, d, dev, lines)
    head_legs(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
