"""Cost of scheduled sampling on the train step, in one process on one MI355X: BASELINE configs[1] (B=64, L=80, F=4096, H=E=1000,
V=12000), one seeded model, FlatAdam, utils.MaskCriterion, dp.train_step with the synchronising error check train.py uses.  Two
legs on the same model, ALTERNATING step by step so that both see the same machine state: ss_prob = 0 (the plain teacher-forced
step: no keyword reaches the model) and ss_prob = 0.25 (one scheduled decode pass in front of it; the optimiser moves the weights
every step, so every pass rebuilds the decode's weight images, as mode='sample' does under --self-critical).  Wall clock around
steps that end in a device synchronisation; median and spread of --steps steps per leg after --warmup steps of each.
Appends what it prints to profiles/scheduled_sampling_step.txt (or --out).

  python tools/bench_scheduled.py [--steps 30] [--warmup 5] [--ss-prob 0.25] [--ss-temperature T] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
import utils
from s2vt_video_caption_amd import capi, dp, functional, synth
from s2vt_video_caption_amd.optim import FlatAdam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ss-prob", type=float, default=0.25)
    ap.add_argument("--ss-temperature", type=float, default=None)
    ap.add_argument("--config", default="c2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scheduled_sampling_step.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scheduled.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS[a.config]
    feats, caps, mask = (t.to(dev) for t in synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5))
    torch.manual_seed(0)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev)
    opt = FlatAdam(m, lr=1e-4, reducer=None)
    crit = utils.MaskCriterion()
    legs = {"ss_prob = 0": None, "ss_prob = %g" % a.ss_prob: dict(ss_prob=a.ss_prob, ss_temperature=a.ss_temperature)}
    times = {k: [] for k in legs}
    for i in range(a.warmup + a.steps):
        for name, kw in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loss = dp.train_step(m, crit, opt, feats, caps, mask, None, check_errors=True, forward_kwargs=kw)
            torch.cuda.synchronize(dev)
            dt = 1e3 * (time.perf_counter() - t0)
            assert torch.isfinite(loss)
            if i >= a.warmup:
                times[name].append(dt)
    capi.check_async_error()
    # the scheduled pass alone while the weights stand (the decode's weight images stay cached)
    tg = caps[:, :-1]
    alone = []
    for _ in range(a.warmup + a.steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        functional.scheduled_inputs(feats, tg, m._hip_params(), a.ss_prob, temperature=a.ss_temperature, owner=m)
        torch.cuda.synchronize(dev)
        alone.append(1e3 * (time.perf_counter() - t0))
    alone = alone[a.warmup:]
    med = {k: statistics.median(v) for k, v in times.items()}
    (n0, t0_), (n1, t1_) = med.items()
    lines = ["", "tools/bench_scheduled.py: train step at %s (B=%d, L=%d, H=E=%d, V=%d), draw = %s; the two legs alternate in one "
             "process; median of %d steps per leg after %d warm-up (min .. max):" % (
                 a.config, d["B"], d["L"], d["H"], d["V"], "arg-max" if a.ss_temperature is None else "sample at T = %g" % a.ss_temperature,
                 a.steps, a.warmup)]
    for k, v in times.items():
        lines.append("  %-16s %8.2f ms  (%.2f .. %.2f)" % (k, med[k], min(v), max(v)))
    lines.append("  difference       %8.2f ms  (%.1f %% of the plain step)" % (t1_ - t0_, 100.0 * (t1_ - t0_) / t0_))
    lines.append("  scheduled pass alone, weights standing (decode images cached): %.2f ms  (%.2f .. %.2f)" % (
        statistics.median(alone), min(alone), max(alone)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
