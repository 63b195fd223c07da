"""Cost of constrained decoding (csrc/truncate.hip "constrained draw": repetition penalty, no-repeat n-gram, banned ids, minimum
length inside the row kernel) beside the existing calls - the yardsticks - in one process on one MI355X.

1. The row kernel alone on one logits buffer: 640 rows x 12 000 words and 80 rows x 3000 words (out_linear of seeded hidden states), a
history of t = 40 words per row drawn from 50 distinct words, n = 3, theta = 1.2, m = 5 and 2 banned ids.  Legs: s2vt_truncated_draw
with top_k=0, top_p=1 (the baseline: the same frame without the constraint phase), s2vt_constrained_draw sampled, and greedy.  The
constrained draw edits its buffer, so every timed group starts from a fresh copy of the logits (the copy is not timed); --reps
launches back to back between two HIP events, the legs alternating, median of --calls such groups.

2. The whole decode, dims as tools/bench_sample_trunc.py: config 5 (L=80, F=4096, H=E=1000, V=12000) at B = 128 and train.py's defaults
(B=16, L=80, F=4096, H=E=512, V=3000).  Legs: mode='test' against greedy S2VT.decode_constrained(no_repeat_ngram_size=3) (per step
the logits GEMM + the row kernel instead of the fused arg-max head), and S2VT.sample_truncated(top_k=50) against sampled
decode_constrained(top_k=50, no_repeat_ngram_size=3) (the same two launches per step, the row kernel with its constraint phase).
The legs ALTERNATE call by call; HIP events around a call; median over --calls calls per leg after --warmup calls of each.
Appends what it prints to profiles/decode_constrained.txt (or --out).

  python tools/bench_decode_constrained.py [--calls 20] [--warmup 3] [--reps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import capi, ops, sampling, synth

SOS, EOS = 3, 4
DIMS = (("config 5 dims, B=128", dict(synth.CONFIGS["c5"], B=128)),
        ("train.py defaults, B=16", dict(B=16, L=80, F=4096, H=512, E=512, V=3000)))
T_HIST, NGRAM, THETA, MIN_LEN, BANNED = 40, 3, 1.2, 5, (1, 2)


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def kernel_legs(name, d, K, calls, warmup, reps, dev, lines):
    R, H, V = d["B"] * K, d["H"], d["V"]
    g = torch.Generator().manual_seed(7)
    h = torch.tanh(torch.randn(R, H, generator=g)).to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    master = ops.gemm(h, sd["out_linear.weight"].to(dev).contiguous(), sd["out_linear.bias"].to(dev).contiguous())
    logits = master.clone()
    words = torch.randint(5, 55, (T_HIST, R), generator=g)
    hist = ((0x3F800000 << 32) | (0xFFFFFFFF - words)).to(torch.int64).to(dev)
    spec = sampling.check_constraints(NGRAM, THETA, MIN_LEN, list(BANNED), V, EOS)
    packed = torch.empty(R, dtype=torch.int64, device=dev)
    legs = (("s2vt_truncated_draw top_k=0, top_p=1", lambda: ops.truncated_draw(logits, seed=1, packed=packed)),
            ("s2vt_constrained_draw sampled", lambda: ops.constrained_draw(logits, hist, T_HIST, spec, seed=1, packed=packed)),
            ("s2vt_constrained_draw greedy", lambda: ops.constrained_draw(logits, hist, T_HIST, spec, greedy=True, packed=packed)))
    us = {leg: [] for leg, _ in legs}
    for i in range(warmup + calls):
        for leg, fn in legs:
            def group():
                for _ in range(reps):
                    fn()
            logits.copy_(master)
            t, _ = _timed(group, dev)
            if i >= warmup:
                us[leg].append(1000.0 * t / reps)
    base = statistics.median(us[legs[0][0]])
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %s, %d rows x V=%d  %-38s %8.1f us per launch (%.1f .. %.1f)  %.2f x the unconstrained draw" % (
            name, R, V, leg, med, min(us[leg]), max(us[leg]), med / base))
    capi.check_async_error()


def decode_legs(name, d, calls, warmup, dev, lines):
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    with torch.no_grad():
        m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        legs = (("mode='test'", lambda i: m(feats, mode="test")),
                ("decode_constrained(n=3) greedy", lambda i: m.decode_constrained(feats, no_repeat_ngram_size=NGRAM)),
                ("sample_truncated(top_k=50)", lambda i: m.sample_truncated(feats, 1, seed=100 + i, top_k=50)),
                ("decode_constrained(n=3, top_k=50)", lambda i: m.decode_constrained(feats, 1, temperature=1.0, seed=100 + i, top_k=50,
                                                                                     no_repeat_ngram_size=NGRAM)))
        ms = {leg: [] for leg, _ in legs}
        for i in range(warmup + calls):
            for leg, fn in legs:
                t, _ = _timed(lambda: fn(i), dev)
                if i >= warmup:
                    ms[leg].append(t)
        med = {leg: statistics.median(v) for leg, v in ms.items()}
        for (leg, _), base in zip(legs, (legs[0][0], legs[0][0], legs[2][0], legs[2][0])):
            lines.append("  %s  %-34s %8.3f ms per call (%.3f .. %.3f)  %.3f x %s" % (
                name, leg, med[leg], min(ms[leg]), max(ms[leg]), med[leg] / med[base], base))
        del m
        torch.cuda.empty_cache()
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_constrained.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode_constrained.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["", "tools/bench_decode_constrained.py: the row kernel alone on one logits buffer (t = %d, n = %d, theta = %g, m = %d, %d banned "
             "ids), %d launches between two HIP events (host enqueue included), legs alternating, median of %d groups after %d warm-up "
             "(min .. max):" % (T_HIST, NGRAM, THETA, MIN_LEN, len(BANNED), a.reps, a.calls, a.warmup)]
    for name, d in DIMS:
        kernel_legs(name, d, 5, a.calls, a.warmup, a.reps, dev, lines)
    lines.append("  the whole decode, K = 1; the legs alternate in one process; HIP events around a call; median of %d calls per leg after %d "
                 "warm-up (min .. max):" % (a.calls, a.warmup))
    for name, d in DIMS:
        decode_legs(name, d, a.calls, a.warmup, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
