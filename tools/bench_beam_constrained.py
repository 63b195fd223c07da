"""Cost of the constraints inside the cumulative-score beam search (S2VT.beam_constrained; csrc/beam_policy.hip with per-slot
histories, csrc/ce.hip's constrained top-20 fan-out) beside the unconstrained search (mode='beam') in one process on one MI355X.
Whole search: config 5 dims (L=80, F=4096, H=E=1000, V=12000), B = 128, width 5, depth 30, one seeded model;
beam_constrained(no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=5, 2 banned ids) against mode='beam'.  The two share
the encoder, the depth loop and every launch of a depth but the policy kernel and the fan-out head.  The legs ALTERNATE call by
call; a call is timed with HIP events on the stream, and its time per depth is the call time / the depths that call actually ran
(beam.LAST_DEPTHS; the constraints change the captions, so the two legs may run different depths).  Median and spread over --calls
calls per leg after --warmup calls of each.
The head alone: s2vt_top20_logprob_constrained against s2vt_top20_logprob on 640 rows x 12 000 words at t = 15 (the middle of a
depth-30 search), --reps launches between two HIP events (host enqueue included).  The constrained head edits its buffer, so every
timed group starts from a fresh copy of the logits (the copy is not timed).
Appends what it prints to profiles/beam_constrained.txt (or --out).

  python tools/bench_beam_constrained.py [--calls 20] [--warmup 3] [--reps 20] [--batch 128] [--width 5] [--depth 30] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import beam, capi, ops, sampling, synth

SOS, EOS = 3, 4
NGRAM, THETA, MIN_LEN, BANNED = 3, 1.2, 5, (1, 2)
HEAD_ROWS, HEAD_T = 640, 15


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
    con = dict(no_repeat_ngram_size=NGRAM, repetition_penalty=THETA, min_length=MIN_LEN, banned_ids=list(BANNED))
    legs = (("mode='beam'", lambda: m(feats, mode="beam", beam_width=a.width, max_beam_depth=a.depth)),
            ("beam_constrained", lambda: m.beam_constrained(feats, beam_width=a.width, max_beam_depth=a.depth, **con)))
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
    lines.append("  the whole search: config 5 dims, B=%d, width %d, depth %d; beam_constrained(n=%d, theta=%g, m=%d, %d banned ids); the two "
                 "legs alternate in one process; HIP events around a call; median of %d calls per leg after %d warm-up (min .. max):" % (
                     a.batch, a.width, a.depth, NGRAM, THETA, MIN_LEN, len(BANNED), a.calls, a.warmup))
    for k, _ in legs:
        call = statistics.median(ms[k])
        lines.append("  %-17s %8.3f ms per call, %2d..%2d depths run, %7.3f ms per depth (%.3f .. %.3f), %8.0f captions/s  [%s]" % (
            k, call, min(depths[k]), max(depths[k]), med[k], min(per_depth[k]), max(per_depth[k]), 1e3 * a.batch / call, paths[k]))
    lines.append("  per-depth ratio beam_constrained / beam: %.3f" % (med["beam_constrained"] / med["mode='beam'"]))
    capi.check_async_error()


def head_legs(a, d, dev, lines):
    R, H, V = HEAD_ROWS, d["H"], d["V"]
    g = torch.Generator().manual_seed(7)
    h = torch.tanh(torch.randn(R, H, generator=g)).to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    master = ops.gemm(h, sd["out_linear.weight"].to(dev).contiguous(), sd["out_linear.bias"].to(dev).contiguous())
    logits = master.clone()
    hist = torch.randint(5, 55, (R, 32), generator=g).to(torch.int32).to(dev)       # words of a small set: repeats and n-gram matches
    spec = sampling.check_constraints(NGRAM, THETA, MIN_LEN, list(BANNED), V, EOS)
    legs = (("s2vt_top20_logprob", lambda: ops.top20_logprob(logits)),
            ("s2vt_top20_logprob_constrained", lambda: ops.top20_logprob_constrained(logits, hist, HEAD_T, spec)))
    us = {leg: [] for leg, _ in legs}
    for i in range(a.warmup + a.calls):
        for leg, fn in legs:
            def group():
                for _ in range(a.reps):
                    fn()
            logits.copy_(master)
            t, _ = _timed(group, dev)
            if i >= a.warmup:
                us[leg].append(1000.0 * t / a.reps)
    base = statistics.median(us[legs[0][0]])
    lines.append("  the fan-out head alone on one logits buffer, %d rows x V=%d, t = %d; %d launches between two HIP events (host enqueue "
                 "and the two output allocations included), legs alternating, median of %d groups after %d warm-up (min .. max):" % (
                     R, V, HEAD_T, a.reps, a.calls, a.warmup))
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %-32s %8.1f us per launch (%.1f .. %.1f)  %.2f x the unconstrained head" % (leg, med, min(us[leg]), max(us[leg]),
                                                                                                   med / base))
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=5)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_constrained.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_constrained.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    lines = ["", "tools/bench_beam_constrained.py:"]
    search_legs(a, d, dev, lines)
    head_legs(a, d, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
