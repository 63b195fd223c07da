"""Cost and effect of self-critical training on stochastic-beam samples (train.py --sc-distinct: S2VT.sample_distinct +
s2vt_sc_weights_swor) beside the step it stands next to (--sc-samples K with S2VT.sample + s2vt_sc_weights_group), in one process on
one MI355X.  Dims: train.py's defaults (B=16, L=80, F=4096, H=E=512, V=3000) and config 5 (L=80, F=4096, H=E=1000, V=12000) at
B = 128 clips; K = 5; 20 synthetic references of 6-12 words per clip.  The legs ALTERNATE step by step (call by call).

  (a) a whole --sc-samples 5 --sc-baseline mean --sc-shared-encode --sc-reward device step (train.make_self_critical_step) with and
      without --sc-distinct, split into sample / scoring / train as hist["sc_split_ms"] does; median of --steps steps after --warmup
  (b) the weight launch alone, ops.sc_weights_swor against ops.sc_weights_group on the same rows: HIP events around --burst calls
      back to back, median over --calls bursts per leg, per call (both allocate their two outputs per call)
  (c) on seeded weights made peaked - out_scale doubled until S2VT.sample returns fewer than 2 distinct captions of 5 per clip on
      average - the share of clips whose K rows all get weight 0 under each sampler, mean baseline, over --draws draws.  The
      references of (c) are each clip's 8 sample_distinct captions at a fixed seed plus 12 random ones, so that rewards differ
      between captions at all (random references alone share almost no n-gram with a caption).

Appends what it prints to profiles/sc_swor.txt (or --out).

  python tools/bench_sc_swor.py [--steps 20] [--warmup 3] [--calls 20] [--burst 50] [--draws 10] [--out FILE]"""
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
from s2vt_video_caption_amd import capi, ops, synth
from s2vt_video_caption_amd.optim import FlatAdam
from s2vt_video_caption_amd.self_critical import DeviceCiderRewarder

PHASES = ("sample", "greedy", "scoring", "train")
SOS, EOS, K = 3, 4, 5
DIMS = (("train.py defaults, B=16", dict(B=16, L=80, F=4096, H=512, E=512, V=3000)),
        ("config 5 dims, B=128", dict(synth.CONFIGS["c5"], B=128)))


def _model(d, dev, out_scale=1.0):
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0, out_scale=out_scale))
    return m.to(dev)


def _random_refs(d, vids, n):
    rng = np.random.RandomState(0)
    return {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(n)] for v in vids}


def _cut(row):
    return row[:row.index(EOS) + 1] if EOS in row else row


def _distinct_per_clip(ids):
    """mean number of different captions per clip of ids [B, K, T], each cut behind its first <eos>"""
    return float(np.mean([len(set(tuple(_cut(r)) for r in rows)) for rows in ids.cpu().tolist()]))


def step_legs(d, feats, vids, steps, warmup, dev):
    """(a): {distinct: median ms per phase and in total}"""
    refs = _random_refs(d, vids, 20)
    legs = {}
    for distinct in (False, True):
        m = _model(d, dev)
        hist = {"sc_split_ms": dict({k: 0.0 for k in PHASES}, steps=0), "reward_sample": [], "reward_greedy": [], "reward_baseline": []}
        step = train.make_self_critical_step(m, FlatAdam(m, lr=1e-4, reducer=None), utils.RewardCriterion(),
                                             DeviceCiderRewarder(refs, vids, SOS, EOS, device=dev, vocab_size=d["V"]), hist, SOS, EOS, dev,
                                             1.0, "device", None, shared_encode=True, distinct=distinct, samples=K, baseline="mean")
        legs[distinct] = (step, hist, [])
    for _ in range(warmup + steps):
        for distinct in (False, True):
            step, hist, per_step = legs[distinct]
            before = dict(hist["sc_split_ms"])
            loss = step(feats, vids)
            assert torch.isfinite(loss)
            per_step.append({k: hist["sc_split_ms"][k] - before[k] for k in PHASES})
    capi.check_async_error()
    out = {}
    for distinct, (_, _, per_step) in legs.items():
        timed = per_step[warmup:]
        out[distinct] = dict({k: statistics.median(s[k] for s in timed) for k in PHASES},
                             total=statistics.median(sum(s.values()) for s in timed))
    return out


def weight_legs(d, calls, burst, dev):
    """(b): median us per call of the two weight launches on B*K rows of L-1 ids"""
    B, T = d["B"], d["L"] - 1
    rng = np.random.RandomState(1)
    sampled = torch.tensor(rng.randint(5, d["V"], size=(B * K, T)), device=dev)
    phi = torch.tensor(-40.0 * rng.rand(B * K), dtype=torch.float32, device=dev)
    kappa = torch.tensor(-45.0 - rng.rand(B), dtype=torch.float32, device=dev)
    r = torch.tensor(rng.rand(B * K) * 3, device=dev)
    fns = {"swor": lambda: ops.sc_weights_swor(sampled, phi, kappa, r, None, K, SOS, EOS),
           "group": lambda: ops.sc_weights_group(sampled, r, None, K, SOS, EOS)}
    us = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(calls + 2):
        for k, fn in fns.items():
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if i >= 2:
                us[k].append(1e3 * e0.elapsed_time(e1) / burst)
    capi.check_async_error()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def zero_share(d, feats, vids, draws, dev):
    """(c): (out_scale, distinct captions per clip of S2VT.sample, {sampler: (share of clips whose rows all get weight 0, distinct
    captions per clip)}) - or None when no out_scale up to 2^20 makes the seeded weights that peaked"""
    B, L = d["B"], d["L"]
    scale, m = 1.0, None
    with torch.no_grad():
        while scale <= 2.0 ** 20:
            m = _model(d, dev, scale).eval()
            n = float(np.mean([_distinct_per_clip(m.sample(feats, K, seed=100 + i)) for i in range(3)]))
            if n < 2.0:
                break
            scale, m = scale * 2.0, None
        if m is None:
            return None
        own = m.sample_distinct(feats, 8, temperature=1.0, seed=7, max_depth=L - 1)[0].cpu().tolist()
        refs = _random_refs(d, vids, 12)
        for b, v in enumerate(vids):
            refs[v] = refs[v] + [[SOS] + [t for t in _cut(row) if t != EOS] + [EOS] for row in own[b]]
        rewarder = DeviceCiderRewarder(refs, vids, SOS, EOS, device=dev, vocab_size=d["V"])
        row_ids = [v for v in vids for _ in range(K)]
        zero, kinds = {"sample": [], "sample_distinct": []}, {"sample": [], "sample_distinct": []}
        for i in range(draws):
            ids = m.sample(feats, K, seed=1000 + i)
            flat = ids.view(B * K, -1)
            w = ops.sc_weights_group(flat, rewarder.rewards(row_ids, flat), None, K, SOS, EOS)[1]
            zero["sample"].append(float((w.view(B, -1) == 0).all(1).double().mean()))
            kinds["sample"].append(_distinct_per_clip(ids))
            ids, _, lp, _, kappa = m.sample_distinct(feats, K, temperature=1.0, seed=1000 + i, max_depth=L - 1)
            flat = ids.view(B * K, -1)
            w = ops.sc_weights_swor(flat, lp.reshape(-1), kappa, rewarder.rewards(row_ids, flat), None, K, SOS, EOS)[1]
            zero["sample_distinct"].append(float((w.view(B, -1) == 0).all(1).double().mean()))
            kinds["sample_distinct"].append(_distinct_per_clip(ids))
    capi.check_async_error()
    return scale, n, {k: (float(np.mean(zero[k])), float(np.mean(kinds[k]))) for k in zero}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc_swor.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sc_swor.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["", "tools/bench_sc_swor.py: --self-critical --sc-samples %d --sc-baseline mean --sc-shared-encode --sc-reward device with and "
             "without --sc-distinct; the legs alternate in one process; seeded random weights, not a trained model:" % K]
    for name, d in DIMS:
        feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
        vids = ["clip%03d" % i for i in range(d["B"])]
        med = step_legs(d, feats, vids, a.steps, a.warmup, dev)
        lines.append("  %s (a) step split, wall clock with a synchronisation behind every phase, median of %d steps after %d warm-up:" % (
            name, a.steps, a.warmup))
        for distinct in (False, True):
            lines.append("      %-40s %s, total %8.2f ms" % (
                "--sc-distinct (S2VT.sample_distinct)" if distinct else "without (S2VT.sample)",
                ", ".join("%s %8.2f ms" % (k, med[distinct][k]) for k in PHASES if k != "greedy"), med[distinct]["total"]))
        lines.append("      ratio with / without: %s, total %.3f" % (
            ", ".join("%s %.3f" % (k, med[True][k] / med[False][k]) for k in PHASES if k != "greedy"),
            med[True]["total"] / med[False]["total"]))
        torch.cuda.empty_cache()
        us = weight_legs(d, a.calls, a.burst, dev)
        lines.append("  %s (b) weight launch alone on %d rows of %d ids, per call in bursts of %d, median of %d bursts (min .. max): "
                     "s2vt_sc_weights_swor %.2f us (%.2f .. %.2f), s2vt_sc_weights_group %.2f us (%.2f .. %.2f), ratio %.3f" % (
                         name, d["B"] * K, d["L"] - 1, a.burst, a.calls, us["swor"][0], us["swor"][1], us["swor"][2], us["group"][0],
                         us["group"][1], us["group"][2], us["swor"][0] / us["group"][0]))
        res = zero_share(d, feats, vids, a.draws, dev)
        if res is None:
            lines.append("  %s (c) no out_scale up to 2^20 makes S2VT.sample return fewer than 2 distinct captions of %d" % (name, K))
        else:
            scale, n, share = res
            lines.append("  %s (c) peaked weights (out_scale %g: S2VT.sample returns %.2f distinct captions of %d), mean baseline, %d draws: "
                         "clips whose %d rows all get weight 0 - S2VT.sample %.1f %% (%.2f distinct captions per clip), "
                         "S2VT.sample_distinct %.1f %% (%.2f distinct)" % (
                             name, scale, n, K, a.draws, K, 100 * share["sample"][0], share["sample"][1],
                             100 * share["sample_distinct"][0], share["sample_distinct"][1]))
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
