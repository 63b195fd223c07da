"""Time split of a train.py --self-critical step with the host and with the device rewarder, in one process on one MI355X: the
recipe in the header of profiles/self_critical_split.txt - BASELINE configs[1] (B=64, L=80, F=4096, H=E=1000, V=12000), 20 synthetic
references of 6-12 words per clip, median of 10 steps after 3 warm-up per leg.  Both legs run train.make_self_critical_step (the
`host` leg is the code path of --sc-reward host, unchanged) on their own copy of the same seeded model, the host leg first.
Appends what it prints to profiles/self_critical_split.txt (or --out).

  python tools/bench_self_critical.py [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import S2VTModel
import train
import utils
from s2vt_video_caption_amd import capi, synth
from s2vt_video_caption_amd.optim import FlatAdam
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder

PHASES = ("sample", "greedy", "scoring", "train")
SOS, EOS = 3, 4


def leg(where, d, feats, vids, caps, steps, warmup, dev):
    torch.manual_seed(0)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev)
    opt = FlatAdam(m, lr=1e-4, reducer=None)
    t0 = time.perf_counter()
    if where == "device":
        rewarder = DeviceCiderRewarder(caps, vids, SOS, EOS, device=dev, vocab_size=d["V"])
    else:
        rewarder = CiderRewarder(caps, vids, SOS, EOS)
    build_ms = 1e3 * (time.perf_counter() - t0)
    hist = {"sc_split_ms": {k: 0.0 for k in PHASES}, "reward_sample": [], "reward_greedy": []}
    hist["sc_split_ms"]["steps"] = 0
    step = train.make_self_critical_step(m, opt, utils.RewardCriterion(), rewarder, hist, SOS, EOS, dev, 1.0, where, None)
    per_step = []
    for _ in range(warmup + steps):
        before = dict(hist["sc_split_ms"])
        loss = step(feats, vids)
        assert torch.isfinite(loss)
        per_step.append({k: hist["sc_split_ms"][k] - before[k] for k in PHASES})
    capi.check_async_error()
    timed = per_step[warmup:]
    med = {k: statistics.median(s[k] for s in timed) for k in PHASES}
    med["total"] = statistics.median(sum(s.values()) for s in timed)
    return med, build_ms, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_critical_split.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_self_critical.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c2"]
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    rng = np.random.RandomState(0)
    vids = ["clip%03d" % i for i in range(d["B"])]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(20)] for v in vids}
    lines = ["", "tools/bench_self_critical.py: host and device rewarder (train.py --sc-reward) in one process, the recipe above "
             "(B=%d, L=%d, H=E=%d, V=%d, 20 references of 6-12 words per clip); median of %d steps after %d warm-up:" % (
                 d["B"], d["L"], d["H"], d["V"], a.steps, a.warmup)]
    got = {}
    for where in ("host", "device"):
        med, build_ms, hist = leg(where, d, feats, vids, caps, a.steps, a.warmup, dev)
        got[where] = (med, hist)
        lines.append("  --sc-reward %s (rewarder built in %.0f ms)" % (where, build_ms))
        for k in PHASES:
            lines.append("    %-8s %8.2f ms  (%4.1f %%)" % (k, med[k], 100.0 * med[k] / med["total"]))
        lines.append("    %-8s %8.2f ms" % ("total", med["total"]))
    (mh, hh), (md, hd) = got["host"], got["device"]
    lines.append("  first step's mean rewards (same seeds, same ids): sampled host %.12f device %.12f, greedy host %.12f device %.12f" % (
        hh["reward_sample"][0], hd["reward_sample"][0], hh["reward_greedy"][0], hd["reward_greedy"][0]))
    saved, drop = mh["scoring"] - md["scoring"], mh["total"] - md["total"]
    lines.append("  bar: device scoring %.2f ms %s its train phase %.2f ms; step total dropped by %.2f ms, scoring by %.2f ms (%s the "
                 "scoring difference minus 1 ms)" % (md["scoring"], "<" if md["scoring"] < md["train"] else ">= (MISSED)", md["train"], drop,
                                                     saved, ">=" if drop >= saved - 1.0 else "< (MISSED)"))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
