"""Cost of stochastic beam search (S2VT.sample_distinct; csrc/gumbel_top.hip, csrc/sbs_policy.hip) beside the two things it stands
between, in one process on one MI355X.
Whole call: config 5 dims (L=80, F=4096, H=E=1000, V=12000), B = 128, K = 5, depth 30, one seeded model.  Three legs ALTERNATE call
by call: sample_distinct(n_samples=5, max_depth=30); mode='beam' at beam_width=5, n_best=5, max_beam_depth=30 - the same rows, the
same encoder, depth loop and launches of a depth, only the fan-out head and the policy differ; model.sample(n_samples=5) - the i.i.d.
alternative, which draws all L - 1 = 79 words of every row.  A call is timed with HIP events on the stream; the two searches also
report time per depth = call time / the depths that call ran (beam.LAST_DEPTHS).  For the two samplers the distinct captions per clip
(cut behind the first <eos>) of the last call are counted (the seeded random weights are not peaked: i.i.d. draws of 79 words do not
repeat themselves there).  Median and spread over --calls calls per leg after --warmup calls of each.
The head alone: s2vt_top20_gumbel against s2vt_top20_logprob on the same random logits [640, 12000], --reps launches between two
HIP events (host enqueue included), legs alternating.
The policy launch alone: s2vt_sbs_step against s2vt_beam_div_step (one group) on the same random top-20 arrays ([B*W][20], no <eos>:
no clip freezes): every timed group initialises its state (depth 1, not timed) and then steps min(--reps, depth - 2) consecutive
depths of one search between two HIP events.
Appends what it prints to profiles/sbs.txt (or --out).

  python tools/bench_sbs.py [--calls 20] [--warmup 3] [--reps 20] [--batch 128] [--samples 5] [--depth 30] [--temperature 1.0]
                            [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import S2VTModel
from s2vt_video_caption_amd import beam, capi, ops, synth

SOS, EOS = 3, 4


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def _distinct_per_clip(ids):
    """mean number of different captions per clip of ids [B, K, T], each cut behind its first <eos>"""
    n = []
    for rows in ids.cpu().tolist():
        n.append(len(set(tuple(r[:r.index(EOS) + 1] if EOS in r else r) for r in rows)))
    return sum(n) / float(len(n))


def search_legs(a, d, dev, lines):
    feats = synth.make_batch(a.batch, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m.to(dev).eval()
    K, D, t = a.samples, a.depth, a.temperature
    legs = (("sample_distinct", lambda: m.sample_distinct(feats, n_samples=K, temperature=t, seed=11, max_depth=D)[0]),
            ("mode='beam'", lambda: m(feats, mode="beam", beam_width=K, max_beam_depth=D, n_best=K)[0]),
            ("sample", lambda: m.sample(feats, K, t, 11)))
    ms = {k: [] for k, _ in legs}
    per_depth = {k: [] for k, _ in legs}
    depths = {k: [] for k, _ in legs}
    paths, last = {}, {}
    with torch.no_grad():
        for i in range(a.warmup + a.calls):
            for name, fn in legs:
                tm, out = _timed(fn, dev)
                last[name] = out
                if name != "sample":
                    paths[name] = beam.LAST_PATH
                if i >= a.warmup:
                    ms[name].append(tm)
                    if name != "sample":
                        depths[name].append(beam.LAST_DEPTHS)
                        per_depth[name].append(tm / beam.LAST_DEPTHS)
    call = {k: statistics.median(v) for k, v in ms.items()}
    lines.append("  the whole call: config 5 dims, B=%d, K=%d, depth %d, temperature %g; the three legs alternate in one process; HIP events "
                 "around a call; median of %d calls per leg after %d warm-up (min .. max):" % (a.batch, K, D, t, a.calls, a.warmup))
    for k in ("sample_distinct", "mode='beam'"):
        lines.append("  %-16s %8.3f ms per call (%.3f .. %.3f), %2d..%2d depths run, %7.3f ms per depth (%.3f .. %.3f), %8.0f clips/s  [%s]" % (
            k, call[k], min(ms[k]), max(ms[k]), min(depths[k]), max(depths[k]), statistics.median(per_depth[k]), min(per_depth[k]),
            max(per_depth[k]), 1e3 * a.batch / call[k], paths[k]))
    lines.append("  %-16s %8.3f ms per call (%.3f .. %.3f), %d word steps, %8.0f clips/s" % (
        "sample", call["sample"], min(ms["sample"]), max(ms["sample"]), d["L"] - 1, 1e3 * a.batch / call["sample"]))
    lines.append("  ratio sample_distinct / beam: %.3f per depth, %.3f per call; sample_distinct / sample: %.3f per call" % (
        statistics.median(per_depth["sample_distinct"]) / statistics.median(per_depth["mode='beam'"]),
        call["sample_distinct"] / call["mode='beam'"], call["sample_distinct"] / call["sample"]))
    lines.append("  distinct captions per clip (of %d; seeded random weights, not a trained model): sample_distinct %.2f, sample %.2f" % (
        K, _distinct_per_clip(last["sample_distinct"]), _distinct_per_clip(last["sample"])))
    capi.check_async_error()


def head_legs(a, dev, lines):
    rows, V = 640, 12000
    x = torch.from_numpy(np.random.RandomState(2).randn(rows, V).astype(np.float32)).to(dev)
    legs = (("s2vt_top20_logprob", lambda: ops.top20_logprob(x)), ("s2vt_top20_gumbel", lambda: ops.top20_gumbel(x, 1.0, 7, 3, 0)))
    us = {leg: [] for leg, _ in legs}
    for i in range(a.warmup + a.calls):
        for leg, fn in legs:
            def group():
                for _ in range(a.reps):
                    fn()
            tm, _ = _timed(group, dev)
            if i >= a.warmup:
                us[leg].append(1000.0 * tm / a.reps)
    base = statistics.median(us[legs[0][0]])
    lines.append("  the head alone on logits [%d, %d]: %d launches between two HIP events (host enqueue and the output allocations included), "
                 "legs alternating, median of %d groups after %d warm-up (min .. max):" % (rows, V, a.reps, a.calls, a.warmup))
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %-20s %8.1f us per launch (%.1f .. %.1f)  %.2f x s2vt_top20_logprob" % (leg, med, min(us[leg]), max(us[leg]), med / base))


def policy_legs(a, dev, lines):
    lib = capi.load()
    B, W, D = a.batch, a.samples, a.depth
    R = B * W
    rng = np.random.RandomState(3)
    ix = np.stack([rng.choice(np.arange(EOS + 1, 12000), 20, replace=False) for _ in range(R)]).astype(np.int32)
    ix_s = torch.from_numpy(np.sort(ix, axis=1)).to(dev)                 # (the cumulative policy's rows are in ascending token order)
    ix_d = torch.from_numpy(ix).to(dev)
    lp_d = torch.from_numpy((-3.0 * rng.rand(R, 20)).astype(np.float32)).to(dev)
    g_d = torch.from_numpy(-np.sort(-rng.gumbel(size=(R, 20)).astype(np.float32), axis=1)).to(dev)
    rows = torch.zeros(3, R, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()                                           # noqa: E731
    nb_d = lib.s2vt_beam_div_bytes(B, W, 1, D, 0)
    qd = torch.empty(nb_d, dtype=torch.uint8, device=dev)
    qs, srows = ops.sbs_state(B, W, D, dev)

    def div(depth):
        capi.check(lib.s2vt_beam_div_step(B, W, 1, D, SOS, EOS, 0.7, 0.0, depth, p(qd), nb_d, p(ix_s), p(lp_d), p(rows[0]), p(rows[1]),
                                          p(rows[2]), None, None, st), "s2vt_beam_div_step")

    def sbs(depth):
        capi.check(lib.s2vt_sbs_step(B, W, D, SOS, EOS, depth, p(qs), qs.numel(), p(ix_d), p(lp_d), p(g_d), p(srows[0]), p(srows[1]),
                                     p(srows[2]), st), "s2vt_sbs_step")
    legs = (("s2vt_beam_div_step", div), ("s2vt_sbs_step", sbs))
    us = {leg: [] for leg, _ in legs}
    reps = min(a.reps, D - 2)                       # (every launch is one more depth of the same search: stay below max_depth)
    for i in range(a.warmup + a.calls):
        for leg, fn in legs:
            fn(1)

            def group():
                for r in range(reps):
                    fn(2 + r)
            tm, _ = _timed(group, dev)
            if i >= a.warmup:
                us[leg].append(1000.0 * tm / reps)
    base = statistics.median(us[legs[0][0]])
    lines.append("  the policy launch alone, B=%d, width %d, random top-20 arrays without <eos>; %d launches (depths 2..%d of one search) between "
                 "two HIP events (host enqueue included), legs alternating, median of %d groups after %d warm-up (min .. max):" % (
                     B, W, reps, reps + 1, a.calls, a.warmup))
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %-20s %8.1f us per launch (%.1f .. %.1f)  %.2f x s2vt_beam_div_step" % (leg, med, min(us[leg]), max(us[leg]), med / base))
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sbs.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sbs.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    lines = ["", "tools/bench_sbs.py:"]
    search_legs(a, d, dev, lines)
    head_legs(a, dev, lines)
    policy_legs(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
