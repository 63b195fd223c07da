"""Per-shape MEDIAN of 15 single-call timings (after 3 warm calls) of gemm_x3 on the batched GEMM shapes of a config-2 step, one
line per shape tagged with the first argument - for A/B of two library builds on one box (S2VT_LIB, interleaved processes; the
best-of-4 of tools/bench_gemm_shapes.py moves by up to 10 % between two runs of one build on the small shapes).
usage: S2VT_LIB=<library> python tools/bench_gemm_shapes_ab.py TAG   (GPU box)"""
import os, sys, statistics
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
tot = 0.0
out = []
for name, M, N, K in SHAPES:
    pa, pb = ops.split_planes(torch.randn(M, K, device=dev), 3), ops.split_planes(torch.randn(N, K, device=dev), 3)
    c = torch.empty(M, N, device=dev)
    ts = []
    for it in range(18):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.gemm_planes(pa, pb, M, N, nplanes=3, out=c, splitk_ws=ws); e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3)
    med = statistics.median(ts)
    tot += med
    out.append("%s %s %.1f" % (tag, name, med))
    del pa, pb, c
print("\n".join(out))
print("%s SUM %.1f" % (tag, tot), flush=True)
