"""Per-shape MEDIAN of 15 single-call timings (after 3 warm calls) of the persistent plane GEMMs - gemm_x3 (planes = 3) or gemm_b1
(planes = 1), in the k-major form (nn) or with both operands read transposed from their row images (tt) - on the batched GEMM shapes
of a config-2 step, one line per shape tagged with the first argument: time and the sha1 of the output.  Inputs are seeded, so two
library builds on one box (S2VT_LIB, interleaved processes) can be compared for speed AND for bit-equal results (the best-of-4 of
tools/bench_gemm_shapes.py moves by up to 10 % between two runs of one build on the small shapes).
usage: S2VT_LIB=<library> python tools/bench_gemm_shapes_ab.py TAG [planes = 3] [nn | tt]   (GPU box)"""
import hashlib, os, sys, statistics
sys.path.insert(0, os.getcwd())
import torch
from s2vt_video_caption_amd import capi, ops
capi.load()
B, L, F, H, V, BLK = 64, 80, 4096, 1000, 12000, 32
R, T = B * (L - 1), 2 * L - 1
SHAPES = [("x1", B * L, H, F), ("gx1", B * L, 4 * H, H), ("gx2blk", BLK * B, 4 * H, H), ("gxe", R, 4 * H, H), ("logits", R, V, H),
          ("dh2", R, H, V), ("dWo", V, H, R), ("dh1blk", BLK * B, H, 4 * H), ("dWhh", 4 * H, H, T * B), ("dWe", 4 * H, H, R),
          ("demb", R, H, 4 * H), ("dx1", B * L, H, 4 * H), ("dWih1", 4 * H, H, B * L), ("dWf", H, F, B * L)]
dev = "cuda:0"
ws = torch.empty(256 << 20, device=dev)
tag = sys.argv[1]
NP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
form = sys.argv[3] if len(sys.argv) > 3 else "nn"
assert NP in (1, 3) and form in ("nn", "tt"), "planes: 1 or 3, form: nn or tt"
tot = 0.0
out = []
for i, (name, M, N, K) in enumerate(SHAPES):
    gen = torch.Generator(device=dev).manual_seed(1000 + i)
    if form == "tt":    # row images of X_A [K, M], X_B [K, N]; the image rows K..pad64(K) are zero
        pa, pb = (ops.split_planes(torch.randn(K, D, device=dev, generator=gen), NP) for D in (M, N))
        Kp = (K + 63) // 64 * 64
        run = lambda: ops.gemm_planes_tt(pa, pb, M, N, Kp, out=c, splitk_ws=ws, nplanes=NP)
    else:
        pa, pb = (ops.split_planes(torch.randn(D, K, device=dev, generator=gen), NP) for D in (M, N))
        run = lambda: ops.gemm_planes(pa, pb, M, N, nplanes=NP, out=c, splitk_ws=ws)
    c = torch.empty(M, N, device=dev)
    ts = []
    for it in range(18):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3)
    med = statistics.median(ts)
    tot += med
    out.append("%s %s %.1f %s" % (tag, name, med, hashlib.sha1(c.cpu().numpy().tobytes()).hexdigest()[:16]))
    del pa, pb, c
print("\n".join(out))
print("%s SUM %.1f" % (tag, tot), flush=True)
