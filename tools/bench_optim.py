"""Cost of optim.FlatAdam.step() with gradient clipping / weight decay / the non-finite guard (s2vt_grad_norm + s2vt_adam_step_clipped,
csrc/optim.hip) beside the plain step (s2vt_adam_step: the existing code and so the yardstick), in one process on one MI355X.
Dims: config 2 (the bench's model: F=4096, H=E=1000, V=12000) and train.py's defaults (F=4096, H=E=512, V=3000).  ONE model and ONE
optimizer per size; a leg is a setting of param_groups[0], so every leg steps the same buffers.  The legs ALTERNATE window by window; a
window is --steps steps timed with HIP events on the stream; median over --windows windows per leg after --warmup windows of each
(min .. max).  Then the norm's two launches alone.  Achieved bytes/s from shape-computed bytes: 28 B / parameter for a step kernel
(p, m, v read and written, g read), 4 B / parameter for the norm.  Appends what it prints to profiles/optim_clip.txt (or --out).

  python tools/bench_optim.py [--windows 20] [--steps 50] [--warmup 2] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import capi
from s2vt_video_caption_amd.optim import CLIP_DEFAULTS, FlatAdam

SIZES = (("config 2", dict(L=80, F=4096, H=1000, E=1000, V=12000)), ("train.py defaults", dict(L=80, F=4096, H=512, E=512, V=3000)))
LEGS = (("plain step (defaults)", {}),
        ("weight_decay=5e-5 (the clipped kernel alone)", dict(weight_decay=5e-5)),
        ("max_grad_norm=1.0", dict(max_grad_norm=1.0)),
        ("max_grad_norm=1.0, weight_decay=5e-5", dict(max_grad_norm=1.0, weight_decay=5e-5)),
        ("max_grad_norm=1.0, weight_decay=5e-5, skip_nonfinite", dict(max_grad_norm=1.0, weight_decay=5e-5, skip_nonfinite=True)))
BOUNDARY_US = 0.93      # profiles/round2_launch_boundary_microbench.txt: one launch boundary behind a kernel of >= 4 us


def _window(fn, steps, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return 1e3 * e0.elapsed_time(e1) / steps          # us per step


def run_size(name, d, args, dev, say):
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"]).to(dev)
    opt = FlatAdam(m, lr=1e-4)
    n = opt.n
    opt.flat_g.copy_(torch.randn(n, device=dev) * 1e-3)          # norm ~ 1e-3 sqrt(n) > 1: the clip is active
    lib = capi.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def leg(kw):
        def fn():
            g = opt.param_groups[0]
            g.update(CLIP_DEFAULTS)
            g.update(kw)
            opt.step()
        return fn

    def norm_alone():
        capi.check(lib.s2vt_grad_norm(ptr(opt.flat_g), n, 1.0, 0, ptr(opt._norm_ws), opt._norm_ws.numel() * 8, ptr(opt._record), None),
                   "s2vt_grad_norm")
    fns = [(label, leg(kw)) for label, kw in LEGS] + [("s2vt_grad_norm alone (two launches)", norm_alone)]
    times = {label: [] for label, _ in fns}
    for w in range(args.warmup + args.windows):
        for label, fn in fns:
            t = _window(fn, args.steps, dev)
            if w >= args.warmup:
                times[label].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    plain = med[LEGS[0][0]]
    say("%s: %d parameters (%.1f MB per buffer); %d windows of %d steps per leg, legs alternating" % (name, n, 4e-6 * n, args.windows, args.steps))
    say("  grad norm %.4f, clip scale %.4f, skipped steps %d" % (float(opt.grad_norm), float(opt.clip_scale), opt.skipped_steps))
    for label, _ in fns:
        t = times[label]
        nbytes = 4 * n if "alone (two" in label else 28 * n if "norm" not in label else 32 * n
        say("  %-58s %8.2f us (%.2f .. %.2f)  x%.3f of the plain step  %6.2f TB/s over %d B/parameter" % (
            label, med[label], min(t), max(t), med[label] / plain, 1e-6 * nbytes / med[label], nbytes // n))
    est = plain * 32.0 / 28.0 + 2 * BOUNDARY_US
    full = med[LEGS[3][0]]
    say("  estimate for norm + clipped step: 32/28 of the plain step + two launch boundaries of %.2f us = %.2f us (x%.3f); measured x%.3f "
        "of the plain step = %+.1f %% against the estimate (explained below where above +15 %%)" % (
            BOUNDARY_US, est, est / plain, full / plain, 100.0 * (full / est - 1.0)))
    del opt, m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_clip.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("tools/bench_optim.py on %s" % torch.cuda.get_device_name(dev))
    for name, d in SIZES:
        run_size(name, d, args, dev, say)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
