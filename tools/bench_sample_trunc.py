"""Cost of top-k / nucleus truncation in the sampled decode (csrc/truncate.hip) beside the untruncated call - the existing code and so
the yardstick - in one process on one MI355X.  Dims as tools/bench_sample_rows.py: config 5 (L=80, F=4096, H=E=1000, V=12000) at
B = 128 clips with K = 1 and K = 5, and train.py's defaults (B=16, L=80, F=4096, H=E=512, V=3000, K = 1 and 5); one seeded model per
(dims, K).  Legs: S2VT.sample(feats, K) (the fused Gumbel arg-max heads), S2VT.sample_truncated with top_k=50, with top_p=0.9 (per step the
logits GEMM + the row kernel instead of the fused head).  The legs ALTERNATE call by call; a call is timed with HIP events on the
stream; median over --calls calls per leg after --warmup calls of each (min .. max).

Then the row kernel alone on one logits buffer [B*K rows, V] (out_linear of seeded hidden states): s2vt_truncated_draw with top_k=50,
with top_p=0.9, with both, beside s2vt_top20_logprob - the existing kernel of the same frame (one 256-thread workgroup per row, the
row in registers) - and beside the fp32-input logits GEMM that stands in front of either in the step.  --reps launches back to back
between two HIP events, the legs alternating, median of --calls such groups.  Appends what it prints to profiles/sample_trunc.txt
(or --out).

  python tools/bench_sample_trunc.py [--calls 20] [--warmup 3] [--reps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import capi, ops, synth

SOS, EOS = 3, 4
DIMS = (("config 5 dims, B=128", dict(synth.CONFIGS["c5"], B=128)),
        ("train.py defaults, B=16", dict(B=16, L=80, F=4096, H=512, E=512, V=3000)))
LEGS = (("untruncated", {}), ("top_k=50", dict(top_k=50)), ("top_p=0.9", dict(top_p=0.9)))


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def decode_legs(name, d, calls, warmup, dev, lines):
    feats = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    with torch.no_grad():
        for K in (1, 5):
            m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
            m.load_state_dict(sd)
            m = m.to(dev).eval()
            ms = {leg: [] for leg, _ in LEGS}
            for i in range(warmup + calls):
                for leg, kw in LEGS:
                    t, _ = _timed(lambda: (m.sample_truncated(feats, K, seed=100 + i, **kw) if kw else m.sample(feats, K, seed=100 + i)), dev)
                    if i >= warmup:
                        ms[leg].append(t)
            med = {leg: statistics.median(v) for leg, v in ms.items()}
            for leg, _ in LEGS:
                lines.append("  %s, K=%d  model.sample(feats, K, %-11s)  %8.3f ms per call (%.3f .. %.3f)  %.3f x untruncated" % (
                    name, K, leg if leg != "untruncated" else "", med[leg], min(ms[leg]), max(ms[leg]), med[leg] / med["untruncated"]))
            del m
            torch.cuda.empty_cache()
    capi.check_async_error()


def kernel_legs(name, d, K, calls, warmup, reps, dev, lines):
    R, H, V = d["B"] * K, d["H"], d["V"]
    g = torch.Generator().manual_seed(7)
    h = torch.tanh(torch.randn(R, H, generator=g)).to(dev)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0)
    w, b = sd["out_linear.weight"].to(dev).contiguous(), sd["out_linear.bias"].to(dev).contiguous()
    logits = ops.gemm(h, w, b)
    out = torch.empty_like(logits)
    packed = torch.empty(R, dtype=torch.int64, device=dev)
    legs = (("s2vt_top20_logprob", lambda: ops.top20_logprob(logits)),
            ("s2vt_truncated_draw top_k=50", lambda: ops.truncated_draw(logits, top_k=50, seed=1, packed=packed)),
            ("s2vt_truncated_draw top_p=0.9", lambda: ops.truncated_draw(logits, top_p=0.9, seed=1, packed=packed)),
            ("s2vt_truncated_draw top_k=50, top_p=0.9", lambda: ops.truncated_draw(logits, top_k=50, top_p=0.9, seed=1, packed=packed)),
            ("logits GEMM (s2vt_gemm_f32 + bias)", lambda: ops.gemm(h, w, b, out=out)))
    us = {leg: [] for leg, _ in legs}
    for i in range(warmup + calls):
        for leg, fn in legs:
            def group():
                for _ in range(reps):
                    fn()
            t, _ = _timed(group, dev)
            if i >= warmup:
                us[leg].append(1000.0 * t / reps)
    base = statistics.median(us["s2vt_top20_logprob"])
    for leg, _ in legs:
        med = statistics.median(us[leg])
        lines.append("  %s, %d rows x V=%d  %-42s %8.1f us per launch (%.1f .. %.1f)  %.2f x top20_logprob" % (
            name, R, V, leg, med, min(us[leg]), max(us[leg]), med / base))
    capi.check_async_error()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_trunc.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample_trunc.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = ["", "tools/bench_sample_trunc.py: S2VT.sample_truncated with top_k=50 / top_p=0.9 against S2VT.sample; the legs alternate in "
             "one process; HIP events around a call; median of %d calls per leg after %d warm-up (min .. max):" % (a.calls, a.warmup)]
    for name, d in DIMS:
        decode_legs(name, d, a.calls, a.warmup, dev, lines)
    lines.append("  the row kernel alone on one logits buffer, %d launches between two HIP events (host enqueue included), legs "
                 "alternating, median of %d groups after %d warm-up:" % (a.reps, a.calls, a.warmup))
    for name, d in DIMS:
        kernel_legs(name, d, 5, a.calls, a.warmup, a.reps, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
