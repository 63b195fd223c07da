"""Cost of a depth of the cumulative-score beam search (mode='beam', csrc/beam_policy.hip) beside the reference's search
(mode='beam_search', csrc/beam_queue.hip), in one process on one MI355X: config 5 dims (L=80, F=4096, H=E=1000, V=12000), B = 128,
width 5, depth 30, one seeded model.  The two share the encoder, the depth step and the depth loop, so the ratio of their times
per depth isolates the policy kernel and the driver.  The legs ALTERNATE call by call; a call is timed with HIP events on the
stream, and its time per depth is the call time / the depths that call actually ran (beam.LAST_DEPTHS: either search stops once
every sample is frozen).  Median and spread over --calls calls per leg after --warmup calls of each.
Appends what it prints to profiles/beam_cum.txt (or --out).

  python tools/bench_beam_cum.py [--calls 20] [--warmup 3] [--batch 128] [--width 5] [--depth 30] [--out-scale 1.0] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import beam, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=5)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--out-scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_cum.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_cum.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    feats = synth.make_batch(a.batch, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0, out_scale=a.out_scale))
    m.to(dev).eval()
    legs = {"beam_search": dict(mode="beam_search"), "beam": dict(mode="beam")}
    ms = {k: [] for k in legs}
    per_depth = {k: [] for k in legs}
    depths = {k: [] for k in legs}
    paths = {}
    with torch.no_grad():
        for i in range(a.warmup + a.calls):
            for name, kw in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                m(feats, beam_width=a.width, max_beam_depth=a.depth, **kw)
                e1.record()
                torch.cuda.synchronize(dev)
                paths[name] = beam.LAST_PATH
                if i >= a.warmup:
                    t = e0.elapsed_time(e1)
                    ms[name].append(t)
                    depths[name].append(beam.LAST_DEPTHS)
                    per_depth[name].append(t / beam.LAST_DEPTHS)
    med = {k: statistics.median(v) for k, v in per_depth.items()}
    lines = ["", "tools/bench_beam_cum.py: config 5 dims, B=%d, width %d, depth %d, out_scale %g; the two legs alternate in one process; "
             "HIP events around a call; median of %d calls per leg after %d warm-up (min .. max):" % (
                 a.batch, a.width, a.depth, a.out_scale, a.calls, a.warmup)]
    for k in legs:
        call = statistics.median(ms[k])
        lines.append("  mode='%s'%s %8.3f ms per call, %2d..%2d depths run, %7.3f ms per depth (%.3f .. %.3f), %8.0f captions/s  [%s]" % (
            k, " " * (11 - len(k)), call, min(depths[k]), max(depths[k]), med[k], min(per_depth[k]), max(per_depth[k]),
            1e3 * a.batch / call, paths[k]))
    lines.append("  per-depth ratio beam / beam_search: %.3f" % (med["beam"] / med["beam_search"]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
