"""Cost of consensus (MBR) caption selection on the device (consensus.select -> s2vt_cider_consensus, csrc/cider.hip) beside the two
things a user compares it with, in one process on one MI355X: the host path on the same ids (ids.cpu() + CiderRewarder.consensus -
what choosing among the candidates cost before the kernel) and the S2VT.sample call that produced the candidates.  Dims: config 5
(L=80, F=4096, H=E=1000, V=12000) at B = 128 clips, T = L - 1 = 79 ids per candidate, K = 5, 10 and 20 candidates per clip drawn by
S2VT.sample of the seeded model (which never stops at <eos>: nearly every row is 79 words long, the longest a candidate of these
dims can be); the idf table is of 256 synthetic clips with 20 references of 6-12 words each.  The legs ALTERNATE call by call.  The
device call and the producer are timed with HIP events on the stream, median of --calls calls after --warmup (min .. max); the host
path with a host clock, median of --host-calls calls (it takes seconds).  Every device result is compared with the host's.  Appends
what it prints to profiles/consensus.txt (or --out).

  python tools/bench_consensus.py [--calls 20] [--warmup 3] [--host-calls 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import S2VTModel
from s2vt_video_caption_amd import capi, consensus, synth
from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder

SOS, EOS = 3, 4
KS = (5, 10, 20)


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_consensus.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = dict(synth.CONFIGS["c5"], B=a.batch)
    B, T = d["B"], d["L"] - 1
    rng = np.random.RandomState(0)
    vids = ["clip%03d" % i for i in range(256)]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(20)] for v in vids}
    host = CiderRewarder(caps, vids, SOS, EOS)
    rew = DeviceCiderRewarder(caps, vids, SOS, EOS, device=dev, vocab_size=d["V"])
    feats = synth.make_batch(B, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m = m.to(dev).eval()
    lines = ["", "tools/bench_consensus.py: consensus.select among K sampled candidates per clip, config 5 dims, B = %d, T = %d; legs "
             "alternate in one process; device call and producer: HIP events, median of %d calls after %d warm-up (min .. max); host "
             "path: host clock, median of %d calls:" % (B, T, a.calls, a.warmup, a.host_calls)]
    with torch.no_grad():
        for K in KS:
            ms = {"device": [], "host": [], "producer": []}
            worst = 0.0
            for i in range(a.warmup + a.calls):
                t_prod, ids = _timed(lambda: m.sample(feats, K, seed=100 + i), dev)
                t_dev, (chosen, best, util) = _timed(lambda: consensus.select(rew, ids), dev)
                if i >= a.warmup:
                    ms["producer"].append(t_prod)
                    ms["device"].append(t_dev)
                if i >= a.warmup and len(ms["host"]) < a.host_calls:
                    t0 = time.perf_counter()
                    hb, hu = host.consensus(ids.cpu())
                    ms["host"].append(1e3 * (time.perf_counter() - t0))
                    got = util.cpu().numpy()
                    worst = max(worst, float(np.abs(got - hu).max()))
                    np.testing.assert_allclose(got, hu, rtol=1e-10, atol=1e-12)
                    assert np.array_equal(best.cpu().numpy(), np.argmax(got, 1))
            capi.check_async_error()
            med = {k: statistics.median(v) for k, v in ms.items()}
            words = float((ids != EOS).long().cumprod(2).sum(2).double().mean())
            for k, what in (("device", "consensus.select on the device"), ("host", ".cpu() + CiderRewarder.consensus"),
                            ("producer", "S2VT.sample(feats, K), the producer")):
                lines.append("  K=%-2d  %-38s %10.3f ms per call (%.3f .. %.3f)" % (K, what, med[k], min(ms[k]), max(ms[k])))
            lines.append("  K=%-2d  device / host %.5f, device / producer %.4f; mean words per candidate %.1f; max |device - host| utility %.2e" % (
                K, med["device"] / med["host"], med["device"] / med["producer"], words, worst))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
