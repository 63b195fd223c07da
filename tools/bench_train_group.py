"""Cost of a train pass on K captions per clip with one encode per clip (S2VT.forward with 3-D targets; the grouped path of
csrc/api_train_f32.hip) beside the only route there was before it - mode='train' on the clips repeated K times, which is the existing code and so the
yardstick - in one process on one MI355X.  A pass = forward + MaskCriterion + backward (every parameter gradient; no optimiser step).
Dims: train.py's defaults (B=16, L=80, F=4096, H=E=512, V=3000) at K = 1 and K = 5, and config 5 (L=80, F=4096, H=E=1000, V=12000)
at B = 128 clips, K = 5 (B = 32 if the B = 128 pass does not fit the card).  The legs ALTERNATE pass by pass; a pass is timed with
HIP events on the stream; median over --calls passes per leg after --warmup passes of each (min .. max).  The two legs' losses and
gradients are compared at the timed sizes (largest gradient difference relative to the largest entry of that gradient).  Then the
grouped pass's split by launch kind (s2vt_prof_read: summed kernel-bracket time and wall-clock busy time per kind, one pass).

Then the split of a self-critical step (train.make_self_critical_step, --sc-reward device) at the train defaults with 20 synthetic
references of 6-12 words per clip: --sc-samples 5 --sc-baseline mean with and without --sc-shared-encode, median of --steps steps
after --warmup.  Appends what it prints to profiles/train_group.txt (or --out).

  python tools/bench_train_group.py [--calls 20] [--warmup 3] [--steps 20] [--out FILE]"""
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
KINDS = ((0, "GEMM"), (1, "forward steps"), (2, "BPTT steps"), (3, "criterion"))
SOS, EOS = 3, 4
DEFAULTS = dict(B=16, L=80, F=4096, H=512, E=512, V=3000)


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
    return m.to(dev).train()


def _pass(m, crit, feats, targets, caps, mask):
    m.zero_grad(set_to_none=True)
    logits = m(feats, targets=targets, mode="train")
    loss = crit(logits if logits.dim() == 3 else logits.flatten(0, 1), caps, mask)
    loss.backward()
    return loss.detach()


def train_legs(name, d, K, calls, warmup, dev, lines):
    B, L = d["B"], d["L"]
    feats, caps, mask = (t.to(dev) for t in synth.make_batch(B * K, L, d["F"], d["V"], seed=5))
    feats = feats[:B].contiguous()
    rep = feats.repeat_interleave(K, 0)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    crit = utils.MaskCriterion()
    m_grp, m_rep = _fresh(d, sd, dev), _fresh(d, sd, dev)
    t3 = caps[:, :-1].unflatten(0, (B, K))
    ms = {"grp": [], "rep": []}
    for i in range(warmup + calls):
        t_grp, l_grp = _timed(lambda: _pass(m_grp, crit, feats, t3, caps, mask), dev)
        t_rep, l_rep = _timed(lambda: _pass(m_rep, crit, rep, caps[:, :-1], caps, mask), dev)
        if i >= warmup:
            ms["grp"].append(t_grp)
            ms["rep"].append(t_rep)
    capi.check_async_error()
    worst, worst_name = max((((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30)).item(), n)
                            for (n, p), q in zip(m_grp.named_parameters(), m_rep.parameters()))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append("  %s, K=%d  3-D targets, one encode per clip         %8.3f ms per pass (%.3f .. %.3f)" % (
        name, K, med["grp"], min(ms["grp"]), max(ms["grp"])))
    lines.append("  %s, K=%d  mode='train' on the repeated clips       %8.3f ms per pass (%.3f .. %.3f)" % (
        name, K, med["rep"], min(ms["rep"]), max(ms["rep"])))
    lines.append("  %s, K=%d  ratio %.3f; loss %.7f against %.7f; largest gradient difference / largest entry of that gradient: %.2e (%s)" % (
        name, K, med["grp"] / med["rep"], float(l_grp), float(l_rep), worst, worst_name))
    lib = capi.load()
    lib.s2vt_prof_reset()
    lib.s2vt_prof_enable(1)
    _pass(m_grp, crit, feats, t3, caps, mask)
    torch.cuda.synchronize(dev)
    lib.s2vt_prof_enable(0)
    parts = []
    for kind, label in KINDS:
        total, n = capi.prof_read(kind)
        parts.append("%s %.3f ms in %d launches (busy %.3f ms)" % (label, total, n, capi.prof_read_busy(kind)))
    lib.s2vt_prof_reset()
    lines.append("  %s, K=%d  grouped pass by launch kind (brackets on; lanes overlap): %s" % (name, K, "; ".join(parts)))
    del m_grp, m_rep
    torch.cuda.empty_cache()
    return med["grp"] / med["rep"]


def sc_leg(shared, d, feats, vids, caps, steps, warmup, dev):
    torch.manual_seed(0)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev)
    opt = FlatAdam(m, lr=1e-4, reducer=None)
    rewarder = DeviceCiderRewarder(caps, vids, SOS, EOS, device=dev, vocab_size=d["V"])
    hist = {"sc_split_ms": {k: 0.0 for k in PHASES}, "reward_sample": [], "reward_greedy": [], "reward_baseline": []}
    hist["sc_split_ms"]["steps"] = 0
    step = train.make_self_critical_step(m, opt, utils.RewardCriterion(), rewarder, hist, SOS, EOS, dev, 1.0, "device", None,
                                         shared_encode=shared, samples=5, baseline="mean")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_group.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_group.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["", "tools/bench_train_group.py: train pass (forward + MaskCriterion + backward) on K captions per clip, 3-D targets (one "
             "encode per clip) against mode='train' on the clips repeated K times; the legs alternate in one process; HIP events around "
             "a pass; median of %d passes per leg after %d warm-up (min .. max):" % (a.calls, a.warmup)]
    ratios = []
    for K in (1, 5):
        ratios.append(("train.py defaults K=%d" % K, train_legs("train.py defaults, B=16", DEFAULTS, K, a.calls, a.warmup, dev, lines)))
    for B in (128, 32):
        d = dict(synth.CONFIGS["c5"], B=B)
        try:
            ratios.append(("config 5 dims B=%d K=5" % B, train_legs("config 5 dims, B=%d" % B, d, 5, a.calls, a.warmup, dev, lines)))
            break
        except torch.cuda.OutOfMemoryError:
            lines.append("  config 5 dims, B=%d, K=5: out of device memory" % B)
            torch.cuda.empty_cache()
    lines.append("  ratios grouped / repeated (below 1: the shared encode is faster): %s" % ", ".join("%s: %.3f" % r for r in ratios))
    d = DEFAULTS
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    rng = np.random.RandomState(0)
    vids = ["clip%03d" % i for i in range(d["B"])]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(20)] for v in vids}
    lines.append("  self-critical step split, --sc-reward device --sc-samples 5 --sc-baseline mean, train.py defaults (B=%d, L=%d, H=E=%d, "
                 "V=%d), 20 references of 6-12 words per clip; median of %d steps after %d warm-up:" % (
                     d["B"], d["L"], d["H"], d["V"], a.steps, a.warmup))
    for shared in (False, True):
        med = sc_leg(shared, d, feats, vids, caps, a.steps, a.warmup, dev)
        lines.append("    %s" % ("--sc-shared-encode" if shared else "(the clips repeated 5 times)"))
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
