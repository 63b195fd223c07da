"""Cost of K sampled captions per clip with S2VT.sample (csrc/api_sample_rows.hip: one encode per clip) beside the only route there
was before it - mode='sample' on the clips repeated K times, which is the existing code and so the yardstick - in one process on one
MI355X.  Dims: config 5 (L=80, F=4096, H=E=1000, V=12000) at B = 128 clips, and train.py's defaults (B=16, L=80, F=4096, H=E=512,
V=3000); K = 1 and K = 5; one seeded model per (dims, K).  The legs ALTERNATE call by call; a call is timed with HIP events on the
stream; median over --calls calls per leg after --warmup calls of each (min .. max).  "cold" is a leg's first call on freshly built
weights (weight images of the decode cache, workspace and encode scratch allocations).  Every warm pair is also compared: with the
same seed the two legs draw the same ids except where two scores are closer than the paths' logit rounding (counted).

Then the split of a self-critical step (train.make_self_critical_step, --sc-reward device) at the train defaults with 20 synthetic
references of 6-12 words per clip: --sc-samples 5 --sc-baseline mean against --sc-samples 1 (greedy baseline), median of --steps
steps after --warmup.  The `train` share of the K = 5 step is what a K-captions-per-clip train pass would attack: it still encodes
every clip K times.  Appends what it prints to profiles/sample_rows.txt (or --out).

  python tools/bench_sample_rows.py [--calls 20] [--warmup 3] [--steps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import S2VTModel
import train
import utils
from s2vt_video_caption_amd import capi, synth
from s2vt_video_caption_amd.optim import FlatAdam
from s2vt_video_caption_amd.self_critical import DeviceCiderRewarder

PHASES = ("sample", "greedy", "scoring", "train")
SOS, EOS = 3, 4
DIMS = (("config 5 dims, B=128", dict(synth.CONFIGS["c5"], B=128)),
        ("train.py defaults, B=16", dict(B=16, L=80, F=4096, H=512, E=512, V=3000)))


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def _fresh(d, sd, dev):
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def decode_legs(name, d, calls, warmup, dev, lines):
    B = d["B"]
    feats = synth.make_batch(B, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    ratios = {}
    with torch.no_grad():
        for K in (1, 5):
            rep = feats.repeat_interleave(K, 0) if K > 1 else feats
            m_rows, m_rep = _fresh(d, sd, dev), _fresh(d, sd, dev)
            cold_rows, _ = _timed(lambda: m_rows.sample(feats, K, seed=1), dev)
            cold_rep, _ = _timed(lambda: m_rep(rep, mode="sample", seed=1), dev)
            ms = {"rows": [], "rep": []}
            differ = 0
            for i in range(warmup + calls):
                t_rows, a = _timed(lambda: m_rows.sample(feats, K, seed=100 + i), dev)
                t_rep, b = _timed(lambda: m_rep(rep, mode="sample", seed=100 + i), dev)
                differ += int((a.view(B * K, -1) != b).any(1).sum())
                if i >= warmup:
                    ms["rows"].append(t_rows)
                    ms["rep"].append(t_rep)
            med = {k: statistics.median(v) for k, v in ms.items()}
            ratios[K] = med["rows"] / med["rep"]
            lines.append("  %s, K=%d  model.sample(feats, K)                %8.3f ms per call (%.3f .. %.3f), cold %8.3f ms" % (
                name, K, med["rows"], min(ms["rows"]), max(ms["rows"]), cold_rows))
            lines.append("  %s, K=%d  mode='sample' on the repeated clips   %8.3f ms per call (%.3f .. %.3f), cold %8.3f ms" % (
                name, K, med["rep"], min(ms["rep"]), max(ms["rep"]), cold_rep))
            lines.append("  %s, K=%d  ratio warm %.3f, cold %.3f; rows whose ids differ between the legs (same seed): %d of %d" % (
                name, K, ratios[K], cold_rows / cold_rep, differ, (warmup + calls) * B * K))
            del m_rows, m_rep
            torch.cuda.empty_cache()
    capi.check_async_error()
    return ratios


def sc_leg(samples, baseline, d, feats, vids, caps, steps, warmup, dev):
    torch.manual_seed(0)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev)
    opt = FlatAdam(m, lr=1e-4, reducer=None)
    rewarder = DeviceCiderRewarder(caps, vids, SOS, EOS, device=dev, vocab_size=d["V"])
    hist = {"sc_split_ms": {k: 0.0 for k in PHASES}, "reward_sample": [], "reward_greedy": [], "reward_baseline": []}
    hist["sc_split_ms"]["steps"] = 0
    step = train.make_self_critical_step(m, opt, utils.RewardCriterion(), rewarder, hist, SOS, EOS, dev, 1.0, "device", None,
                                         samples=samples, baseline=baseline)
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
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rows.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample_rows.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["", "tools/bench_sample_rows.py: K draws per clip, S2VT.sample (one encode per clip) against mode='sample' on the clips "
             "repeated K times; the legs alternate in one process; HIP events around a call; median of %d calls per leg after %d "
             "warm-up (min .. max):" % (a.calls, a.warmup)]
    ratios = {}
    for name, d in DIMS:
        ratios[name] = decode_legs(name, d, a.calls, a.warmup, dev, lines)
    ok = all(r[5] < 1.0 for r in ratios.values())
    lines.append("  condition: at K = 5 the new call is faster than the repeated-clips call at both dims: %s (%s)" % (
        "met" if ok else "MISSED", ", ".join("%s: %.3f" % (n, r[5]) for n, r in ratios.items())))
    d = DIMS[1][1]
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    rng = np.random.RandomState(0)
    vids = ["clip%03d" % i for i in range(d["B"])]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(20)] for v in vids}
    lines.append("  self-critical step split, --sc-reward device, train.py defaults (B=%d, L=%d, H=E=%d, V=%d), 20 references of 6-12 words "
                 "per clip; median of %d steps after %d warm-up:" % (d["B"], d["L"], d["H"], d["V"], a.steps, a.warmup))
    for samples, baseline in ((1, "greedy"), (5, "mean")):
        med = sc_leg(samples, baseline, d, feats, vids, caps, a.steps, a.warmup, dev)
        lines.append("    --sc-samples %d --sc-baseline %s" % (samples, baseline))
        for k in PHASES:
            lines.append("      %-8s %8.2f ms  (%4.1f %%)" % (k, med[k], 100.0 * med[k] / med["total"]))
        lines.append("      %-8s %8.2f ms" % ("total", med["total"]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
