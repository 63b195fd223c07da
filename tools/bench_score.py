"""Cost of scoring captions with mode='score' (csrc/api_score.hip) beside the only route there was before it - mode='train' on
features repeated K times, then torch log_softmax + gather - in one process on one MI355X: config 5 dims (L=80, F=4096, H=E=1000,
V=12000), B = 128 clips, captions of T = 31 tokens, K = 1 and K = 5 candidates per clip, one seeded model.  The baseline feeds
captions[:, :-1] padded to L-1 words (mode='train' takes nothing shorter) and reads the first T-1 logits rows.  The legs ALTERNATE
call by call; a call is timed with HIP events on the stream; median over --calls calls per leg after --warmup calls of each
(min .. max).  "cold" is the first mode='score' call on freshly built weights: it builds the weight images of the decode cache and
allocates the encode scratch.  Also prints the head kernel's largest error against fp64 log_softmax over the inputs of
tests/test_gpu_score.py.  Appends what it prints to profiles/score.txt (or --out).

  python tools/bench_score.py [--calls 20] [--warmup 3] [--batch 128] [--tokens 31] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import S2VTModel
from s2vt_video_caption_amd import ops, synth


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def head_error(dev):
    """largest |s2vt_pick_logprob - fp64 log_softmax| over the head-kernel inputs of tests/test_gpu_score.py"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_score as t
    worst = 0.0
    for V, ld in ((1, 1), (50, 50), (257, 259), (1000, 1004), (12001, 12001)):
        x, tgt = t._head_inputs(V, ld, seed=100 + V)
        lp, _ = ops.pick_logprob(x.to(dev)[:, :V], tgt.to(dev))
        want = torch.log_softmax(x[:, :V].double(), dim=1).gather(1, tgt.long()[:, None])[:, 0]
        worst = max(worst, float((lp.cpu().double() - want).abs().max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_score.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = synth.CONFIGS["c5"]
    B, T, L, V = a.batch, a.tokens, d["L"], d["V"]
    feats = synth.make_batch(B, L, d["F"], V, seed=5)[0].to(dev)
    sd = synth.make_state_dict(V, d["F"], d["H"], d["E"], seed=0)

    def fresh():
        m = S2VTModel.S2VT(V, d["F"], L, dim_hid=d["H"], dim_embed=d["E"])
        m.load_state_dict(sd)
        return m.to(dev).eval()
    lines = ["", "tools/bench_score.py: config 5 dims, B=%d clips, T=%d tokens per caption; the legs alternate in one process; HIP events "
             "around a call; median of %d calls per leg after %d warm-up (min .. max):" % (B, T, a.calls, a.warmup)]
    with torch.no_grad():
        for K in (1, 5):
            g = torch.Generator().manual_seed(7 + K)
            caps = torch.randint(5, V, (B, K, T), generator=g)
            caps[..., 0], caps[..., T - 1] = 3, 4
            caps = caps.to(dev)
            m = fresh()
            cold, _ = _timed(lambda: m(feats, targets=caps, mode="score", length_alpha=0.0), dev)
            inp = torch.full((B * K, L - 1), 4, dtype=torch.long, device=dev)
            inp[:, :T - 1] = caps.reshape(B * K, T)[:, :-1]
            tgt = caps.reshape(B * K, T)[:, 1:, None]

            def score():
                return m(feats, targets=caps, mode="score", length_alpha=0.0)

            def baseline():
                logits = m(feats.repeat_interleave(K, dim=0) if K > 1 else feats, targets=inp, mode="train")[:, :T - 1]
                return torch.log_softmax(logits, dim=-1).gather(2, tgt)[..., 0].sum(-1)
            ms = {"score": [], "train": []}
            diff = 0.0
            for i in range(a.warmup + a.calls):
                ts, out = _timed(score, dev)
                tb, ll = _timed(baseline, dev)
                diff = max(diff, float((out[0].reshape(-1) - ll).abs().max()))
                if i >= a.warmup:
                    ms["score"].append(ts)
                    ms["train"].append(tb)
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines.append("  K=%d  mode='score'                 %8.3f ms per call (%.3f .. %.3f), cold %8.3f ms, %8.0f captions/s" % (
                K, med["score"], min(ms["score"]), max(ms["score"]), cold, 1e3 * B * K / med["score"]))
            lines.append("  K=%d  mode='train' + log_softmax    %8.3f ms per call (%.3f .. %.3f), %8.0f captions/s" % (
                K, med["train"], min(ms["train"]), max(ms["train"]), 1e3 * B * K / med["train"]))
            lines.append("  K=%d  score / baseline time ratio %.3f; largest difference of the two log-likelihoods %.3g" % (
                K, med["score"] / med["train"], diff))
            del m
            torch.cuda.empty_cache()
    lines.append("  head kernel (s2vt_pick_logprob) against fp64 log_softmax, inputs of tests/test_gpu_score.py: largest error %.3g"
                 % head_error(dev))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
