"""Cost of diverse (group) beam search (S2VT.beam_diverse; csrc/beam_policy.hip) beside the cumulative-score search (mode='beam') at
the same width in one process on one MI355X.
Whole search: config 5 dims (L=80, F=4096, H=E=1000, V=12000), B = 128, depth 30, one seeded model; beam_diverse(beam_width=6,
num_groups=3, diversity_lambda=0.5) against mode='beam' at beam_width=6.  The two share the encoder, the depth loop and every launch
of a depth, the policy kernel included (one group against three).  The legs ALTERNATE call by call; a call is timed with HIP events on the stream, and its time per
depth is the call time / the depths that call actually ran (beam.LAST_DEPTHS).  The diverse search runs until the SLOWEST group of a
sample has settled, so it may run more depths than mode='beam': the depths run are printed beside the times.  Median and spread
over --calls calls per leg after --warmup calls of each.
The policy launch alone: s2vt_beam_div_step against s2vt_beam_cum_step on the same random top-20 arrays ([B*W][20], log-probs
uniform in [-3, 0], no <eos>: no sample freezes): every timed group initialises its state (depth 1, not timed) and then steps
min(--reps, depth - 2) consecutive depths of one search between two HIP events (host enqueue included).
Appends what it prints to profiles/beam_diverse.txt (or --out).

  python tools/bench_beam_diverse.py [--calls 20] [--warmup 3] [--reps 20] [--batch 128] [--width 6] [--groups 3] [--lam 0.5]
                                     [--depth 30] [--out FILE]"""
import argparse
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
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev).eval()
    legs = (("mode='beam'", lambda: m(feats, mode="beam", beam_width=a.width, max_beam_depth=a.depth)),
            ("beam_diverse", lambda: m.beam_diverse(feats, beam_width=a.width, num_groups=a.groups, diversity_lambda=a.lam,
                                                    max_beam_depth=a.depth)))
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
    lines.append("  the whole search: config 5 dims, B=%d, width %d, depth %d; beam_diverse(num_groups=%d, diversity_lambda=%g); the two legs "
                 "alternate in one process; HIP events around a call; median of %d calls per leg after %d warm-up (min .. max):" % (
                     a.batch, a.width, a.depth, a.groups, a.lam, a.calls, a.warmup))
    for k, _ in legs:
        lines.append("  %-13s %8.3f ms per call, %2d..%2d depths run, %7.3f ms per depth (%.3f .. %.3f), %8.0f clips/s  [%s]" % (
            k, call[k], min(depths[k]), max(depths[k]), med[k], min(per_depth[k]), max(per_depth[k]), 1e3 * a.batch / call[k], paths[k]))
    lines.append("  ratio beam_diverse / beam: %.3f per depth, %.3f per call" % (med["beam_diverse"] / med["mode='beam'"],
                                                                                call["beam_diverse"] / call["mode='beam'"]))
    capi.check_async_error()


def policy_legs(a, dev, lines):
    lib = capi.load()
    B, W, G, D = a.batch, a.width, a.groups, a.depth
    R = B * W
    rng = np.random.RandomState(3)
    ix = np.stack([np.sort(rng.choice(np.arange(EOS + 1, 12000), 20, replace=False)) for _ in range(R)]).astype(np.int32)
    ix_d = torch.from_numpy(ix).to(dev)
    lp_d = torch.from_numpy((-3.0 * rng.rand(R, 20)).astype(np.float32)).to(dev)
    rows = torch.zeros(3, R, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()
    nb_c, nb_d = lib.s2vt_beam_cum_bytes(B, W, D), lib.s2vt_beam_div_bytes(B, W, G, D, 0)
    qc = torch.empty(nb_c, dtype=torch.uint8, device=dev)
    qd = torch.empty(nb_d, dtype=torch.uint8, device=dev)

    def cum(depth):
        capi.check(lib.s2vt_beam_cum_step(B, W, D, SOS, EOS, 0.7, depth, p(qc), nb_c, p(ix_d), p(lp_d), p(rows[0]), p(rows[1]), p(rows[2]),
                                          st), "s2vt_beam_cum_step")

    def div(depth):
        capi.check(lib.s2vt_beam_div_step(B, W, G, D, SOS, EOS, 0.7, a.lam, depth, p(qd), nb_d, p(ix_d), p(lp_d), p(rows[0]), p(rows[1]),
                                          p(rows[2]), None, None, st), "s2vt_beam_div_step")
    legs = (("s2vt_beam_cum_step", cum), ("s2vt_beam_div_step", div))
    us = {leg: [] for leg, _ in legs}
    reps = min(a.reps, D - 2)                       # (every launch is one more depth of the same search: stay below max_depth)
    for i in range(a.warmup + a.calls):
        for leg, fn in legs:
            fn(1)

            def group():
                for r in range(reps):
                    fn(2 + r)
            t, _ = _timed(group, dev)
            if i >= a.warmup:
                us[leg].append(1000.0 * t / reps)
    base = statistics.median(us[legs[0][0]])
    lines.append("  the policy launch alone, B=%d, width %d (%d groups), random top-20 arrays without <eos>; %d launches (depths 2..%d of one "
                 "search) between two HIP events (host enqueue included), legs alternating, median of %d groups after %d warm-up "
                 "(min .. max):" % (B, W, G, reps, reps + 1, a.calls, a.warmup))
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %-20s %8.1f us per launch (%.1f .. %.1f)  %.2f x s2vt_beam_cum_step" % (leg, med, min(us[leg]), max(us[leg]), med / base))
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=6)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_diverse.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_diverse.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    lines = ["", "tools/bench_beam_diverse.py:"]
    search_legs(a, d, dev, lines)
    policy_legs(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
