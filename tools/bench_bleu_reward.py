"""Cost of the mixed CIDEr / sentence BLEU-4 reward on the device (self_critical.DeviceMixedRewarder -> s2vt_mixed_rewards /
s2vt_mixed_consensus, csrc/cider.hip) beside the CIDEr-only calls it extends, in one process on one MI355X, the legs ALTERNATING call
by call on the same ids:

  rewards    640 rows x T = 79 (config 5 dims, B = 128 clips, K = 5 captions each from S2VT.sample): ops.mixed_rewards (mix and both
             parts) against ops.cider_rewards, beside the S2VT.sample call that feeds them and the host MixedRewarder on the same ids
  consensus  B = 128, K = 5 and 20: ops.mixed_consensus against ops.cider_consensus

Dims: config 5 (L=80, F=4096, H=E=1000, V=12000); the seeded model never stops at <eos>, so nearly every row is 79 words long, the
longest a row of these dims can be; the tables are of 256 synthetic clips with 20 references of 6-12 words each.  Device calls are
timed with HIP events on the stream, median of --calls calls after --warmup (min .. max); the host path with a host clock, median of
--host-calls calls.  The CIDEr parts are compared bit for bit with the CIDEr-only calls, BLEU-4 with the host's.  Appends what it prints
to profiles/bleu_reward.txt (or --out).

  python tools/bench_bleu_reward.py [--calls 30] [--warmup 5] [--host-calls 2] [--out FILE]"""
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
from s2vt_video_caption_amd import capi, ops, synth
from s2vt_video_caption_amd.self_critical import DeviceMixedRewarder, MixedRewarder

SOS, EOS = 3, 4
WC, WB = 1.0, 0.5
KS = (5, 20)


def _timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def _line(what, v):
    return "  %-44s %10.3f ms per call (%.3f .. %.3f)" % (what, statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bleu_reward.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bleu_reward.py measures on a GPU"
    dev = torch.device("cuda", 0)
    d = dict(synth.CONFIGS["c5"], B=a.batch)
    B, T = d["B"], d["L"] - 1
    rng = np.random.RandomState(0)
    vids = ["clip%03d" % i for i in range(256)]
    caps = {v: [[SOS] + [int(x) for x in rng.randint(5, d["V"], size=rng.randint(6, 13))] + [EOS] for _ in range(20)] for v in vids}
    host = MixedRewarder(caps, vids, SOS, EOS, WC, WB)
    rew = DeviceMixedRewarder(caps, vids, SOS, EOS, WC, WB, device=dev, vocab_size=d["V"])
    feats = synth.make_batch(B, d["L"], d["F"], d["V"], seed=5)[0].to(dev)
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], sos_ix=SOS, eos_ix=EOS)
    m.load_state_dict(synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=0))
    m = m.to(dev).eval()
    lines = ["", "tools/bench_bleu_reward.py: w_cider %.2f, w_bleu %.2f; config 5 dims, B = %d clips, T = %d; legs alternate in one process; "
             "device calls: HIP events, median of %d calls after %d warm-up (min .. max); host: host clock, median of %d calls:" % (
                 WC, WB, B, T, a.calls, a.warmup, a.host_calls)]
    with torch.no_grad():
        # ---- rewards: K = 5 captions per clip, the rows of a --sc-samples 5 step
        K = 5
        row_vids = [vids[b % len(vids)] for b in range(B) for _ in range(K)]
        clip_rows = torch.tensor([rew.row_of[v] for v in row_vids], dtype=torch.int32, device=dev)
        ms = {"mixed": [], "cider": [], "producer": [], "host": []}
        worst = 0.0
        for i in range(a.warmup + a.calls):
            t_prod, ids = _timed(lambda: m.sample(feats, K, seed=100 + i), dev)
            rows = ids.view(B * K, T)
            tb, bt = rew._tables(rows)
            t_mix, (mix, cider, bleu) = _timed(lambda: ops.mixed_rewards(tb, bt, clip_rows, rows, SOS, EOS, WC, WB, return_parts=True), dev)
            t_cid, plain = _timed(lambda: ops.cider_rewards(tb, clip_rows, rows, SOS, EOS), dev)
            assert torch.equal(cider.view(torch.int64), plain.view(torch.int64))
            if i >= a.warmup:
                ms["mixed"].append(t_mix)
                ms["cider"].append(t_cid)
                ms["producer"].append(t_prod)
            if i >= a.warmup and len(ms["host"]) < a.host_calls:
                t0 = time.perf_counter()
                want = host.rewards(row_vids, rows.cpu())
                ms["host"].append(1e3 * (time.perf_counter() - t0))
                assert (bleu.cpu().numpy() == host.last_parts[1]).all()
                worst = max(worst, float(np.abs(mix.cpu().numpy() - want).max()))
                np.testing.assert_allclose(mix.cpu().numpy(), want, rtol=1e-10, atol=1e-12)
        capi.check_async_error()
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append(" rewards, %d rows x T = %d (K = %d):" % (B * K, T, K))
        lines.append(_line("ops.mixed_rewards (mix, cider, bleu)", ms["mixed"]))
        lines.append(_line("ops.cider_rewards", ms["cider"]))
        lines.append(_line("S2VT.sample(feats, 5), the producer", ms["producer"]))
        lines.append(_line(".cpu() + MixedRewarder.rewards (host)", ms["host"]))
        lines.append("  mixed / cider-only %.3f, mixed / producer %.4f, mixed / host %.6f; mean bleu %.3e; max |device - host| reward %.2e" % (
            med["mixed"] / med["cider"], med["mixed"] / med["producer"], med["mixed"] / med["host"], float(bleu.mean()), worst))
        # ---- consensus
        for K in KS:
            ms = {"mixed": [], "cider": []}
            for i in range(a.warmup + a.calls):
                ids = m.sample(feats, K, seed=200 + i)
                tb, bt = rew._tables(ids)
                t_mix, (mb, mu) = _timed(lambda: ops.mixed_consensus(tb, bt, ids, SOS, EOS, WC, WB), dev)
                t_cid, (cb, cu) = _timed(lambda: ops.cider_consensus(tb, ids, SOS, EOS), dev)
                if i >= a.warmup:
                    ms["mixed"].append(t_mix)
                    ms["cider"].append(t_cid)
            capi.check_async_error()
            ones = ops.mixed_consensus(tb, bt, ids, SOS, EOS, 1.0, 0.0)[1]
            assert torch.equal(ones.view(torch.int64), cu.view(torch.int64))
            row0 = ids[0].cpu().tolist()
            walk = WC * cu[0].cpu().numpy() + WB * rew.bleu_consensus_walk(row0)
            assert (mu[0].cpu().numpy() == walk).all()
            lines.append(" consensus, B = %d, K = %d:" % (B, K))
            lines.append(_line("ops.mixed_consensus", ms["mixed"]))
            lines.append(_line("ops.cider_consensus", ms["cider"]))
            lines.append("  mixed / cider-only %.3f" % (statistics.median(ms["mixed"]) / statistics.median(ms["cider"])))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
