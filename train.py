"""Training harness for the MI355X S2VT path: the reference's loop (train.py:56-175) —
Adam(lr) + ReduceLROnPlateau(patience) + EarlyStopping(patience) + full-module checkpoints every `save_freq` epochs, at
the best validation loss and at the end — on top of the drop-in `S2VTModel.S2VT`, `utils.MaskCriterion`,
`dataloader.VideoDataset` and, with more than one process, data parallelism over RCCL (`s2vt_video_caption_amd.dp`).

  python train.py --caption-file data/captions.json --feats-path data/feats/vgg16_bn
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...

Differences from the reference script: it trains `S2VT` (the reference's committed script instantiates the unrelated
`Att_Baseline`, train.py:86), configuration comes from argparse with the reference's `Opt` defaults (train.py:20-48),
TensorBoard logging is optional (tensorboardX is not a dependency), and `ReduceLROnPlateau` is built without the
`verbose` argument that torch >= 2.6 removed.
"""
import argparse
import math
import os
import time

import torch
import torch.distributed as dist
from torch import optim


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--caption-file", default="./data/captions_server.json")
    ap.add_argument("--feats-path", default="./data/feats/vgg16_bn")
    ap.add_argument("--train-length", type=int, default=80)
    ap.add_argument("--dim-hidden", type=int, default=512)
    ap.add_argument("--dim-embed", type=int, default=512)
    ap.add_argument("--feat-dim", type=int, default=4096)
    ap.add_argument("--feat-dropout", type=float, default=0.0)
    ap.add_argument("--out-dropout", type=float, default=0.0)
    ap.add_argument("--rnn-dropout", type=float, default=0.0,
                    help="nn.LSTM's dropout between the layers of vid_rnn / word_rnn (the reference's Opt.rnn_dropout); no effect "
                         "with one layer")
    ap.add_argument("--num-layers", type=int, default=1,
                    help="layers of vid_rnn and word_rnn (the reference's Opt.num_layers): > 1 runs the stacked-LSTM chain "
                         "kernels with torch's Adam and, across processes, the plain bucketed all-reduce")
    ap.add_argument("--batch-size", type=int, default=16, help="per process")
    ap.add_argument("--workers", type=int, default=0,
                    help="DataLoader worker processes (0 = the reference's behaviour: items are loaded by the feed thread; "
                         "at B=64 a batch is 64 .npy files = 84 MB per 13-ms step, so real runs want a few workers)")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--save-freq", type=int, default=100)
    ap.add_argument("--save-path", default="./checkpoint")
    ap.add_argument("--early-stopping-patience", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--learning-rate-patience", type=int, default=20)
    # reproducibility switches (not in the reference, whose runs are unseeded): used by the harness parity test
    ap.add_argument("--no-shuffle", action="store_true", help="iterate the training set in file order")
    ap.add_argument("--seed", type=int, default=None, help="seed numpy's global RNG (caption sampling, dataloader.py:41)")
    ap.add_argument("--model", choices=("s2vt", "att_baseline"), default="s2vt",
                    help="s2vt: S2VTModel.S2VT (the hot path); att_baseline: attention_baseline.Att_Baseline, the network the "
                         "reference's committed train.py:86 instantiates")
    ap.add_argument("--rnn-type", choices=("lstm", "gru"), default="lstm",
                    help="S2VT's recurrent cell (the reference's Opt.rnn_type): gru runs the GRU timestep kernels with torch's Adam "
                         "and, with several processes, the plain bucketed all-reduce")
    ap.add_argument("--self-critical", action="store_true",
                    help="sequence-level training on CIDEr instead of cross-entropy: per batch a sampled (mode='sample') and a greedy "
                         "(mode='test') caption are scored against the clip's references (document frequencies of the training split), "
                         "and the sampled tokens' log-likelihood is weighted with reward(sampled) - reward(greedy) "
                         "(utils.RewardCriterion).  Start from a cross-entropy-trained --init-state.  Single process.")
    ap.add_argument("--sc-temperature", type=float, default=1.0, help="temperature of the sampled caption (--self-critical)")
    ap.add_argument("--sc-top-k", type=int, default=0, metavar="k",
                    help="--self-critical: the sampled captions draw every word among the k most probable of its step (S2VT.sample_truncated's top_k; "
                         "0, the default: off).  utils.RewardCriterion still weights the FULL-softmax log-prob of the drawn words")
    ap.add_argument("--sc-top-p", type=float, default=1.0, metavar="p",
                    help="--self-critical: ... from the nucleus, the smallest set of most probable words whose mass reaches p, taken "
                         "after --sc-top-k (its top_p; 1, the default: off).  The loss is on the full-softmax log-prob as well")
    ap.add_argument("--sc-reward", choices=("host", "device"), default="host",
                    help="where --self-critical scores the captions.  host: self_critical.CiderRewarder on the CPU, between two copies "
                         "of the ids.  device: self_critical.DeviceCiderRewarder - the reference table is built once and lives on the "
                         "card, the rewards, the <sos>-prefixed captions and the advantage weights come from HIP kernels "
                         "(s2vt_cider_rewards, s2vt_sc_weights) and the ids never leave the device")
    ap.add_argument("--sc-cider-weight", type=float, default=1.0, metavar="w",
                    help="--self-critical: the reward is w * CIDEr-D + (--sc-bleu-weight) * sentence BLEU-4 (the cider_reward_weight / "
                         "bleu_reward_weight mix of Luo's self-critical.pytorch).  1 and 0 (the defaults): CIDEr-D alone, today's rewarder")
    ap.add_argument("--sc-bleu-weight", type=float, default=0.0, metavar="w",
                    help="--self-critical: weight of the sentence BLEU-4 (caption_metrics.bleu's per-sentence BLEU_4 over token ids) in the "
                         "reward.  With --sc-reward device both scores come from one kernel call per batch (s2vt_mixed_rewards: "
                         "self_critical.DeviceMixedRewarder); on the host (MixedRewarder) the Python scorer costs hundreds of ms per batch")
    ap.add_argument("--sc-samples", type=int, default=1, metavar="K",
                    help="captions sampled per clip in a --self-critical step (S2VT.sample: one encode per clip, K rows of word "
                         "steps); the train step then runs on the B*K captions.  1 (default): today's step")
    ap.add_argument("--sc-baseline", choices=("greedy", "mean"), default="greedy",
                    help="what a sampled caption's reward is compared with.  greedy: the reward of the clip's greedy caption (SCST, "
                         "Rennie et al. 2017).  mean: the mean reward of the clip's other K - 1 samples (Luo 2020) - no greedy "
                         "decode runs; needs --sc-samples >= 2")
    ap.add_argument("--sc-distinct", action="store_true",
                    help="the K captions of a --self-critical step with --sc-samples K (2..8) are sampled WITHOUT replacement "
                         "(S2VT.sample_distinct: K pairwise distinct captions per clip) and weighted with the normalised "
                         "importance-weighted estimator of Kool et al. 2019 (s2vt_sc_weights_swor, self_critical.swor_advantages): a "
                         "peaked model no longer spends the step on K copies of one sentence.  --sc-baseline greedy compares with the "
                         "greedy reward, mean with the estimator's own estimate of the expected reward.  One-layer LSTM S2VT, "
                         "temperature 1, no truncation")
    ap.add_argument("--sc-shared-encode", action="store_true",
                    help="the train step of a --self-critical step with --sc-samples K encodes every clip once (S2VT.forward with "
                         "3-D targets: dp.train_step(group=K)) instead of running on the clips repeated K times.  Same loss and "
                         "gradients; which is faster depends on the shapes (profiles/train_group.txt), so it is opt-in")
    ap.add_argument("--captions-per-clip", type=int, default=1, metavar="K",
                    help="cross-entropy training on K reference captions of every clip per step (dataloader.VideoDataset("
                         "captions_per_clip=K)), the clip encoded once; the loss is MaskCriterion over the B*K captions.  1 "
                         "(default): the reference's one caption per clip.  Validation stays one caption")
    ap.add_argument("--init-state", default=None, help="state_dict file to start from instead of the seeded default init")
    ap.add_argument("--scheduled-sampling-start", type=int, default=-1, metavar="E",
                    help="scheduled sampling (Bengio et al., 2015) from epoch E on: each decode-step input of a training step is, with "
                         "the epoch's probability, the word the model itself chose at the previous step instead of the caption's "
                         "(S2VT.forward(ss_prob=...)); -1 (default): off.  The usual stage between cross-entropy and --self-critical "
                         "training.  Validation stays teacher-forced")
    ap.add_argument("--scheduled-sampling-increase-every", type=int, default=5, metavar="N",
                    help="the probability grows every N epochs after the start")
    ap.add_argument("--scheduled-sampling-increase-prob", type=float, default=0.05, metavar="d", help="by this much")
    ap.add_argument("--scheduled-sampling-max-prob", type=float, default=0.25, metavar="m", help="up to this value")
    ap.add_argument("--ss-temperature", type=float, default=None,
                    help="the model's own word is a draw from softmax(logit / temperature); absent: the arg-max")
    ap.add_argument("--grad-clip", type=float, default=0.0, metavar="c",
                    help="global-norm gradient clipping at c before every optimiser step (0, the default: off).  The one-layer LSTM "
                         "path clips inside the device step (optim.FlatAdam(max_grad_norm=c): the norm in fp64, no host read; p.grad "
                         "keeps the unclipped gradient); GRU, stacked and att_baseline use torch.nn.utils.clip_grad_norm_")
    ap.add_argument("--weight-decay", type=float, default=0.0, metavar="w",
                    help="weight decay (the reference's commented-out Opt.weight_decay = 5e-5): L2 added to the gradient, as "
                         "torch.optim.Adam(weight_decay=w); with --adamw decoupled, as torch.optim.AdamW.  0 (default): off")
    ap.add_argument("--adamw", action="store_true", help="decoupled weight decay (p *= 1 - lr * w before the update)")
    ap.add_argument("--no-decay-bias", action="store_true", help="leave the bias vectors out of the weight decay")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="a step whose gradient norm is inf or NaN leaves parameters and moments untouched (one-layer LSTM path only: "
                         "the guard sits in optim.FlatAdam's device step)")
    opt = ap.parse_args(argv)
    if not opt.grad_clip >= 0.0:
        ap.error("--grad-clip must be >= 0 (0: off)")
    if not 0.0 <= opt.weight_decay < float("inf"):
        ap.error("--weight-decay must be finite and >= 0")
    if (opt.adamw or opt.no_decay_bias) and opt.weight_decay == 0.0:
        ap.error("--adamw / --no-decay-bias need --weight-decay")
    if opt.skip_nonfinite and not (opt.model == "s2vt" and opt.rnn_type == "lstm" and opt.num_layers == 1):
        ap.error("--skip-nonfinite needs the one-layer LSTM S2VT (optim.FlatAdam's device step); torch's Adam, which trains GRU, "
                 "stacked and att_baseline models, has no such guard")
    if not (math.isfinite(opt.sc_cider_weight) and math.isfinite(opt.sc_bleu_weight)):
        ap.error("--sc-cider-weight / --sc-bleu-weight must be finite")
    if (opt.sc_cider_weight != 1.0 or opt.sc_bleu_weight != 0.0) and not opt.self_critical:
        ap.error("--sc-cider-weight / --sc-bleu-weight need --self-critical")
    if (opt.sc_samples != 1 or opt.sc_baseline != "greedy") and not opt.self_critical:
        ap.error("--sc-samples / --sc-baseline need --self-critical")
    if opt.sc_samples < 1:
        ap.error("--sc-samples must be at least 1")
    if (opt.sc_top_k != 0 or opt.sc_top_p != 1.0) and not opt.self_critical:
        ap.error("--sc-top-k / --sc-top-p need --self-critical")
    if opt.sc_top_k < 0 or not 0.0 < opt.sc_top_p <= 1.0:
        ap.error("--sc-top-k must be >= 0 and --sc-top-p in (0, 1]")
    if opt.sc_baseline == "mean" and opt.sc_samples < 2:
        ap.error("--sc-baseline mean needs --sc-samples >= 2 (the mean of the other K - 1 samples)")
    if opt.sc_distinct:
        if not opt.self_critical:
            ap.error("--sc-distinct needs --self-critical")
        if not 2 <= opt.sc_samples <= 8:
            ap.error("--sc-distinct needs --sc-samples K with 2 <= K <= 8 (S2VT.sample_distinct's widths; one caption has nothing to "
                     "be distinct from)")
        if opt.sc_top_k != 0 or opt.sc_top_p != 1.0 or opt.sc_temperature != 1.0:
            ap.error("--sc-distinct samples the distribution that is trained: not with --sc-top-k, --sc-top-p or an --sc-temperature "
                     "other than 1 (the inclusion probabilities would be those of another distribution)")
        if opt.model != "s2vt" or opt.rnn_type != "lstm" or opt.num_layers != 1:
            ap.error("--sc-distinct needs the one-layer LSTM S2VT (S2VT.sample_distinct refuses GRU and stacked models; Att_Baseline "
                     "has none)")
    if opt.sc_shared_encode and not opt.self_critical:
        ap.error("--sc-shared-encode needs --self-critical")
    if opt.captions_per_clip < 1:
        ap.error("--captions-per-clip must be at least 1")
    if opt.captions_per_clip > 1:
        if opt.self_critical:
            ap.error("--captions-per-clip applies to cross-entropy training (--self-critical samples its captions: --sc-samples)")
        if opt.model == "att_baseline":
            ap.error("--captions-per-clip needs --model s2vt (Att_Baseline takes one caption per clip)")
        if opt.scheduled_sampling_start >= 0:
            ap.error("--captions-per-clip cannot be combined with scheduled sampling (--scheduled-sampling-start)")
    if opt.scheduled_sampling_start >= 0:
        if opt.self_critical:
            ap.error("--scheduled-sampling-start cannot be combined with --self-critical (it is the stage before it)")
        if opt.model == "att_baseline":
            ap.error("--scheduled-sampling-start needs --model s2vt (Att_Baseline has no scheduled sampling)")
        if opt.scheduled_sampling_increase_every < 1:
            ap.error("--scheduled-sampling-increase-every must be at least 1")
        if not (0.0 <= opt.scheduled_sampling_max_prob <= 1.0 and opt.scheduled_sampling_increase_prob >= 0.0):
            ap.error("--scheduled-sampling-max-prob must be in [0, 1] and --scheduled-sampling-increase-prob >= 0")
        if opt.ss_temperature is not None and not 0.0 < opt.ss_temperature < float("inf"):
            ap.error("--ss-temperature must be finite and > 0")
    return opt


def ss_prob_for_epoch(epoch, start, every, inc, max_prob):
    """Scheduled-sampling probability of an epoch: 0 before `start` (or with start < 0: off), then inc * ((epoch - start) // every),
    capped at max_prob."""
    if start < 0 or epoch < start:
        return 0.0
    return min(inc * ((epoch - start) // every), max_prob)


def make_self_critical_step(model, optimizer, reward_criterion, rewarder, hist, sos, eos, dev, temperature=1.0, sc_reward="host",
                            reducer=None, shared_encode=False, max_grad_norm=None, top_k=0, top_p=1.0, distinct=False, samples=1,
                            baseline="greedy"):
    """step(feats, video_ids) -> loss of one --self-critical step: sample, decode greedily, score both against the clips' references,
    train on the sampled ids weighted with reward(sampled) - reward(greedy).  hist["sc_split_ms"] accumulates the wall-clock split
    (every phase ends with a device synchronisation), hist["reward_sample"] / ["reward_greedy"] the batch means.  sc_reward
    "host": rewarder is a CiderRewarder and the ids make a round trip through the host; "device": a DeviceCiderRewarder, and
    nothing but the two batch means leaves the card.
    samples = K > 1 (or baseline "mean"): K captions per clip from model.sample (one encode per clip), rewards over the B*K rows,
    each row's reward compared with its clip's greedy reward (baseline "greedy") or with the mean reward of the clip's other K - 1
    rows (baseline "mean": no greedy decode runs, sc_split_ms["greedy"] stays 0 and hist["reward_greedy"] empty), then the train step
    on the clips repeated K times with the B*K captions - or, with shared_encode, on the clips as they are with K captions each
    (dp.train_step(group=K): one encode per clip, same loss and gradients).  hist["reward_baseline"] gets the batch mean of the
    baselines.  top_k / top_p: the truncation of the sampled captions (S2VT.sample_truncated; 0 / 1.0: off) - the loss still
    weights the full-softmax log-prob of the drawn words.  max_grad_norm: dp.train_step's (clipping for torch's optimisers; an
    optim.FlatAdam carries its own).
    distinct (2 <= samples <= 8, temperature 1, no truncation): the K captions are sampled WITHOUT replacement, pairwise distinct
    (model.sample_distinct), and weighted with the normalised importance-weighted estimator of Kool et al. 2019 from their
    log-probs and the search's threshold kappa (ops.sc_weights_swor on the device, self_critical.swor_advantages on the host):
    baseline "greedy" compares with the greedy reward, "mean" with the estimator's own estimate N / W of the expected reward.
    Everything else - rewards, the train step, the history - is the K-sample step's.
    A rewarder that keeps `last_parts` (MixedRewarder / DeviceMixedRewarder: the CIDEr and BLEU-4 parts of its latest rewards() call)
    also gets the batch means of the sampled rows' two parts appended to the returned step's `part_means`."""
    from s2vt_video_caption_amd import dp, ops
    from s2vt_video_caption_amd.self_critical import advantage_weights, group_advantages, swor_advantages
    K = int(samples)
    if baseline not in ("greedy", "mean") or K < 1 or (baseline == "mean" and K < 2):
        raise ValueError("samples must be >= 1 and baseline 'greedy' or 'mean' (which needs samples >= 2), got %r, %r" % (samples, baseline))

    mixed = hasattr(rewarder, "last_parts")
    part_means = []

    def sampled_parts(on_device):
        """the parts of the rewards() call just made: as two more entries of the device step's one read (a list of tensors), or
        recorded at once from the host arrays"""
        if not mixed:
            return []
        cider, bleu = rewarder.last_parts
        if on_device:
            return [cider.mean(), bleu.mean()]
        part_means.append((float(cider.mean()), float(bleu.mean())))
        return []

    truncated = top_k != 0 or top_p != 1.0
    if distinct and (not 2 <= K <= 8 or truncated or temperature != 1.0):
        raise ValueError("distinct needs 2 <= samples <= 8, temperature 1 and no truncation (the inclusion probabilities are those of "
                         "the distribution that is trained), got samples %r, temperature %r, top_k %r, top_p %r" % (
                             samples, temperature, top_k, top_p))

    def draw_one(feats):
        """one sampled caption per clip: mode='sample'; where top_k / top_p are set, S2VT.sample_truncated's single sample
        (Att_Baseline takes the two as keywords of its forward)"""
        if not truncated:
            return model(feats, mode='sample', temperature=temperature)
        if hasattr(model, "sample_truncated"):
            return model.sample_truncated(feats, 1, temperature=temperature, top_k=top_k, top_p=top_p)[:, 0]
        return model(feats, mode='sample', temperature=temperature, top_k=top_k, top_p=top_p)

    def group_step(feats, ids):
        sp = hist["sc_split_ms"]
        on_device = sc_reward == "device"
        t0 = time.perf_counter()
        logprob = kappa = None
        if distinct:
            sampled, _, logprob, _, kappa = model.sample_distinct(feats, K, temperature=1.0, seed=None, max_depth=model.length - 1)
            sampled, logprob = sampled.view(feats.shape[0] * K, -1), logprob.reshape(-1)
            if not on_device:
                logprob, kappa = logprob.cpu().numpy(), kappa.cpu().numpy()
        elif truncated:
            sampled = model.sample_truncated(feats, K, temperature=temperature, top_k=top_k, top_p=top_p).view(feats.shape[0] * K, -1)
        else:
            sampled = model.sample(feats, K, temperature=temperature).view(feats.shape[0] * K, -1)
        if on_device:
            torch.cuda.synchronize(dev)
        else:
            sampled = sampled.cpu()
        t1 = time.perf_counter()
        greedy = None
        if baseline == "greedy":
            with torch.no_grad():
                greedy = model(feats, mode='test')
            if on_device:
                torch.cuda.synchronize(dev)
            else:
                greedy = greedy.cpu()
        t2 = time.perf_counter()
        row_ids = [v for v in ids for _ in range(K)]
        r_s = rewarder.rewards(row_ids, sampled)
        extra = sampled_parts(on_device)
        r_g = rewarder.rewards(ids, greedy) if greedy is not None else None
        if on_device:
            if distinct:
                caps, weight, _, base = ops.sc_weights_swor(sampled, logprob, kappa, r_s, r_g, K, sos, eos, return_extras=True)
            else:
                caps, weight, base = ops.sc_weights_group(sampled, r_s, r_g, K, sos, eos, return_baseline=True)
            means = torch.stack([r_s.mean(), base.mean()] + ([r_g.mean()] if r_g is not None else []) + extra).tolist()   # the phase's synchronisation
            if extra:
                part_means.append(tuple(means[-2:]))
        else:
            if distinct:
                adv, _, base = swor_advantages(logprob.reshape(-1, K), kappa, r_s.reshape(-1, K), r_g)
            else:
                adv, base = group_advantages(r_s.reshape(-1, K), r_g)
            weight = advantage_weights(sampled, adv.reshape(-1), eos).to(dev)
            caps = torch.cat([torch.full((sampled.shape[0], 1), sos, dtype=torch.long), sampled], 1).to(dev)
            means = [float(r_s.mean()), float(base.mean())] + ([float(r_g.mean())] if r_g is not None else [])
        t3 = time.perf_counter()
        if shared_encode:
            loss = dp.train_step(model, reward_criterion, optimizer, feats, caps, weight, reducer, check_errors=True, group=K,
                                 max_grad_norm=max_grad_norm)
        else:
            loss = dp.train_step(model, reward_criterion, optimizer, feats.repeat_interleave(K, 0), caps, weight, reducer, check_errors=True,
                                 max_grad_norm=max_grad_norm)
        t4 = time.perf_counter()
        for k, v in (("sample", t1 - t0), ("greedy", t2 - t1 if greedy is not None else 0.0), ("scoring", t3 - t2), ("train", t4 - t3)):
            sp[k] += 1e3 * v
        sp["steps"] += 1
        hist["reward_sample"].append(means[0])
        hist.setdefault("reward_baseline", []).append(means[1])
        if r_g is not None:
            hist["reward_greedy"].append(means[2])
        return loss

    if K > 1 or baseline == "mean":           # (K = 1: the steps below run on the clips as they are - nothing to share)
        group_step.part_means = part_means
        return group_step

    def host_step(feats, ids):
        sp = hist["sc_split_ms"]
        t0 = time.perf_counter()
        with torch.no_grad():
            sampled = draw_one(feats).cpu()
        t1 = time.perf_counter()
        with torch.no_grad():
            greedy = model(feats, mode='test').cpu()
        t2 = time.perf_counter()
        r_s = rewarder.rewards(ids, sampled)
        sampled_parts(False)
        r_g = rewarder.rewards(ids, greedy)
        weight = advantage_weights(sampled, r_s - r_g, eos).to(dev)
        caps = torch.cat([torch.full((sampled.shape[0], 1), sos, dtype=torch.long), sampled], 1).to(dev)
        t3 = time.perf_counter()
        loss = dp.train_step(model, reward_criterion, optimizer, feats, caps, weight, reducer, check_errors=True, max_grad_norm=max_grad_norm)
        t4 = time.perf_counter()
        for k, v in (("sample", t1 - t0), ("greedy", t2 - t1), ("scoring", t3 - t2), ("train", t4 - t3)):
            sp[k] += 1e3 * v
        sp["steps"] += 1
        hist["reward_sample"].append(float(r_s.mean()))
        hist["reward_greedy"].append(float(r_g.mean()))
        hist.setdefault("reward_baseline", []).append(float(r_g.mean()))
        return loss

    def device_step(feats, ids):
        sp = hist["sc_split_ms"]
        t0 = time.perf_counter()
        with torch.no_grad():
            sampled = draw_one(feats)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        with torch.no_grad():
            greedy = model(feats, mode='test')
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        r_s = rewarder.rewards(ids, sampled)
        extra = sampled_parts(True)
        r_g = rewarder.rewards(ids, greedy)
        caps, weight = ops.sc_weights(sampled, r_s, r_g, sos, eos)
        means = torch.stack([r_s.mean(), r_g.mean()] + extra).tolist()          # the phase's synchronisation
        if extra:
            part_means.append(tuple(means[-2:]))
        t3 = time.perf_counter()
        loss = dp.train_step(model, reward_criterion, optimizer, feats, caps, weight, reducer, check_errors=True, max_grad_norm=max_grad_norm)
        t4 = time.perf_counter()
        for k, v in (("sample", t1 - t0), ("greedy", t2 - t1), ("scoring", t3 - t2), ("train", t4 - t3)):
            sp[k] += 1e3 * v
        sp["steps"] += 1
        hist["reward_sample"].append(means[0])
        hist["reward_greedy"].append(means[1])
        hist.setdefault("reward_baseline", []).append(means[1])
        return loss

    step = device_step if sc_reward == "device" else host_step
    step.part_means = part_means
    return step


def run(opt):
    """The reference's training loop (train.py:108-168).  Returns the history it went through:
    {"train_loss": [...], "valid_loss": [...], "lr": [lr in force DURING each epoch], "stopped_at": epoch or None,
     "checkpoints": [file names in the order they were written]}."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import s2vt_video_caption_amd  # noqa: F401
        from s2vt_video_caption_amd import dp as _dp
        _dp.plan_for_collectives(world)      # RCCL's channel count and the GEMMs' compute-unit reserve, before the communicator exists
        dist.init_process_group(backend="nccl", device_id=dev)

    import numpy as np
    import dataloader
    from S2VTModel import S2VT
    from utils import EarlyStopping, MaskCriterion
    from s2vt_video_caption_amd import capi, dp

    if opt.seed is not None:
        np.random.seed(opt.seed + rank)
    start_time = time.strftime('%y_%m_%d_%H_%M_%S-', time.localtime())
    os.makedirs(opt.save_path, exist_ok=True)
    if rank == 0:                                           # the run's configuration beside its checkpoints (save_opt, train.py:51-53)
        with open(os.path.join(opt.save_path, start_time + 'opt.txt'), 'w+', encoding='utf-8') as f:
            f.write(str(vars(opt)))
    cpc = opt.captions_per_clip
    if cpc > 1:
        trainset = dataloader.VideoDataset(opt.caption_file, opt.feats_path, max_len=opt.train_length, captions_per_clip=cpc)
    else:
        trainset = dataloader.VideoDataset(opt.caption_file, opt.feats_path, max_len=opt.train_length)
    validset = dataloader.VideoDataset(opt.caption_file, opt.feats_path, max_len=opt.train_length, mode='valid')
    shuffle = not opt.no_shuffle
    sampler = torch.utils.data.distributed.DistributedSampler(trainset, shuffle=shuffle, drop_last=True) if world > 1 else None
    train_loader = torch.utils.data.DataLoader(trainset, batch_size=opt.batch_size, shuffle=shuffle and sampler is None,
                                               sampler=sampler, drop_last=world > 1, num_workers=opt.workers,
                                               persistent_workers=opt.workers > 0)
    # Validation is NOT sharded: every rank runs the whole split in the reference's batch composition (train.py:136-146), so
    # the number that drives ReduceLROnPlateau / EarlyStopping is the single-process one whatever the world size.  (A
    # DistributedSampler pads the split with duplicated samples and a mean of per-rank batch means weights the ragged last
    # batches differently: LR cuts and the stop epoch could then differ from a 1-GPU run.)  The split is small (MSVD: 100
    # videos); rank 0's value is broadcast so that every replica steps its schedulers on the same bits.
    valid_loader = torch.utils.data.DataLoader(validset, batch_size=opt.batch_size, shuffle=False,
                                               num_workers=opt.workers, persistent_workers=opt.workers > 0)
    word2ix = trainset.word2ix

    torch.manual_seed(0)        # identical replicas
    if opt.model == "att_baseline":
        from attention_baseline import Att_Baseline
        model = Att_Baseline(len(word2ix), opt.feat_dim, length=opt.train_length, dim_hid=opt.dim_hidden, dim_embed=opt.dim_embed,
                             feat_dropout=opt.feat_dropout, out_dropout=opt.out_dropout,
                             sos_ix=word2ix['<sos>'], eos_ix=word2ix['<eos>'])                      # train.py:86-87 upstream
    else:
        model = S2VT(len(word2ix), opt.feat_dim, length=opt.train_length, dim_hid=opt.dim_hidden, dim_embed=opt.dim_embed,
                     feat_dropout=opt.feat_dropout, rnn_dropout=opt.rnn_dropout, out_dropout=opt.out_dropout,
                     num_layers=opt.num_layers, rnn_type=opt.rnn_type, sos_ix=word2ix['<sos>'], eos_ix=word2ix['<eos>'])
    # the one-layer LSTM whole path: flat gradient buffer, FlatAdam
    flat = opt.model == "s2vt" and opt.rnn_type == "lstm" and opt.num_layers == 1
    if opt.init_state:
        model.load_state_dict(torch.load(opt.init_state))
    model.to(dev)
    reducer = None
    if world > 1:       # S2VT: gradients written straight into the flat buffer, all-reduce overlapped with the backward;
        reducer = dp.FlatGradAllReducer(model.parameters())            # Att_Baseline, GRU: plain bucketed all-reduce after it
        if flat:
            reducer.attach(model)
    if flat:                    # train.py:89-93's Adam, same arithmetic, as one launch over flat parameter / gradient / moment buffers
        from s2vt_video_caption_amd.optim import FlatAdam
        optimizer = FlatAdam(model, lr=opt.lr, reducer=reducer, max_grad_norm=opt.grad_clip or None, weight_decay=opt.weight_decay,
                             decoupled=opt.adamw, no_decay=("bias",) if opt.no_decay_bias else (), skip_nonfinite=opt.skip_nonfinite)
    elif opt.weight_decay == 0.0:
        optimizer = optim.Adam(model.parameters(), lr=opt.lr)                                       # train.py:89-93
    else:                       # the reference's commented-out weight_decay=opt.weight_decay; --no-decay-bias: two param groups
        from s2vt_video_caption_amd.optim import matches_no_decay
        named = list(model.named_parameters())
        bias = [p for n, p in named if opt.no_decay_bias and matches_no_decay(n, ("bias",))]
        groups = [{"params": [p for n, p in named if not any(p is b for b in bias)], "weight_decay": opt.weight_decay}]
        if bias:
            groups.append({"params": bias, "weight_decay": 0.0})
        optimizer = (optim.AdamW if opt.adamw else optim.Adam)(groups, lr=opt.lr)
    # --grad-clip on torch's optimisers: dp.train_step clips before optimizer.step() (FlatAdam clips inside its device step)
    clip = opt.grad_clip or None
    log_norm = opt.grad_clip > 0 or opt.skip_nonfinite
    lr_scheduler = optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=opt.learning_rate_patience)   # :95-97
    early_stopping = EarlyStopping(patience=opt.early_stopping_patience, verbose=rank == 0,
                                   path=os.path.join(opt.save_path, start_time + 'stop.pth'))        # :98-100
    criterion = MaskCriterion()
    hist = {"train_loss": [], "valid_loss": [], "lr": [], "stopped_at": None, "checkpoints": [], "ss_prob": []}
    if log_norm:                # (only then: the harness tests compare the keys of hist with the oracle's)
        hist["grad_norm"], hist["skipped_steps"] = [], []
    rewarder = None
    if opt.self_critical:
        if world > 1 or opt.model != "s2vt":
            raise NotImplementedError("--self-critical runs S2VT in a single process")
        from utils import RewardCriterion
        from s2vt_video_caption_amd.self_critical import CiderRewarder, DeviceCiderRewarder, DeviceMixedRewarder, MixedRewarder
        sos, eos = word2ix['<sos>'], word2ix['<eos>']
        sc_mixed = opt.sc_cider_weight != 1.0 or opt.sc_bleu_weight != 0.0
        if sc_mixed and opt.sc_reward == "device":
            rewarder = DeviceMixedRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos, opt.sc_cider_weight,
                                           opt.sc_bleu_weight, device=dev, vocab_size=len(word2ix))
        elif sc_mixed:
            rewarder = MixedRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos, opt.sc_cider_weight,
                                     opt.sc_bleu_weight)
        elif opt.sc_reward == "device":
            rewarder = DeviceCiderRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos, device=dev,
                                           vocab_size=len(word2ix))
        else:
            rewarder = CiderRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos)
        reward_criterion = RewardCriterion()
        # wall-clock split of the self-critical steps (ms, summed over the run; each phase ends with a device synchronisation)
        hist["sc_split_ms"] = {"sample": 0.0, "greedy": 0.0, "scoring": 0.0, "train": 0.0, "steps": 0}
        hist["reward_sample"], hist["reward_greedy"], hist["reward_baseline"] = [], [], []
        if sc_mixed:            # the epoch means of the sampled rows' two parts
            hist["reward_cider"], hist["reward_bleu"] = [], []

    if rewarder is not None:
        self_critical_step = make_self_critical_step(model, optimizer, reward_criterion, rewarder, hist, sos, eos, dev, opt.sc_temperature,
                                                     opt.sc_reward, reducer, samples=opt.sc_samples, baseline=opt.sc_baseline,
                                                     shared_encode=opt.sc_shared_encode, top_k=opt.sc_top_k, top_p=opt.sc_top_p, max_grad_norm=clip,
                                                     distinct=opt.sc_distinct)

    def save(name):
        if rank == 0:
            torch.save(model, os.path.join(opt.save_path, start_time + name))
            hist["checkpoints"].append(name)

    for epoch in range(opt.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        hist["lr"].append(optimizer.param_groups[0]['lr'])
        ss_prob = ss_prob_for_epoch(epoch, opt.scheduled_sampling_start, opt.scheduled_sampling_increase_every,
                                    opt.scheduled_sampling_increase_prob, opt.scheduled_sampling_max_prob)
        hist["ss_prob"].append(ss_prob)
        # (ss_prob == 0 passes no keyword at all: the plain teacher-forced step; every process draws its own seeds)
        ss_kwargs = dict(ss_prob=ss_prob, ss_temperature=opt.ss_temperature) if ss_prob > 0 else None
        running, count = 0.0, 0
        norm_acc = torch.zeros(2, dtype=torch.float64, device=dev)      # sum and count of the epoch's finite gradient norms, on the device
        sc_from = len(hist["reward_baseline"]) if rewarder is not None else 0
        for feats, targets, ids, masks in dataloader.feed_batches(train_loader, dev):
            # train.py:116-127; check_errors: a device-side error of this step (IndexError for a caption id outside the vocabulary)
            # is raised BEFORE optimizer.step(), as in the reference, whose nn.Embedding raises in the forward
            if rewarder is not None:
                loss = self_critical_step(feats, ids)
            elif cpc > 1:       # targets / masks [B, K, L]: row b*K + k of the step = caption k of clip b, the clip encoded once
                loss = dp.train_step(model, criterion, optimizer, feats, targets.flatten(0, 1), masks.flatten(0, 1), reducer,
                                     check_errors=True, group=cpc, max_grad_norm=clip)
            else:
                loss = dp.train_step(model, criterion, optimizer, feats, targets, masks, reducer, check_errors=True,
                                     forward_kwargs=ss_kwargs, max_grad_norm=clip)
            running += float(loss)
            count += 1
            if log_norm and getattr(optimizer, "grad_norm", None) is not None:       # no read here: once per epoch, below
                gn = optimizer.grad_norm.detach().to(torch.float64)
                ok = torch.isfinite(gn)
                norm_acc += torch.stack([torch.where(ok, gn, torch.zeros_like(gn)), ok.to(torch.float64)])
        train_loss = running / max(count, 1)
        norm_text = ""
        if log_norm:
            total, finite = norm_acc.tolist()
            hist["grad_norm"].append(total / max(finite, 1.0))
            hist["skipped_steps"].append(optimizer.skipped_steps if flat else 0)
            norm_text = " grad norm: {} skipped steps: {}".format(hist["grad_norm"][-1], hist["skipped_steps"][-1])
        running, count = 0.0, 0
        model.eval()
        with torch.no_grad():
            for feats, targets, ids, masks in dataloader.feed_batches(valid_loader, dev):
                probs = model(feats, targets=targets[:, :-1], mode='train')                    # train.py:141-143
                running += float(criterion(probs, targets, masks))
                count += 1
        valid_loss = running / max(count, 1)                                                   # train.py:147
        if world > 1:
            vl = torch.tensor([valid_loss], dtype=torch.float64, device=dev)
            dist.broadcast(vl, 0)
            valid_loss = float(vl[0])
        hist["train_loss"].append(train_loss)
        hist["valid_loss"].append(valid_loss)
        if rewarder is not None and self_critical_step.part_means:
            pm = self_critical_step.part_means
            hist["reward_cider"].append(sum(p[0] for p in pm) / len(pm))
            hist["reward_bleu"].append(sum(p[1] for p in pm) / len(pm))
            del pm[:]
        if rank == 0:
            sc_text = ""
            if rewarder is not None and len(hist["reward_baseline"]) > sc_from:      # the epoch's mean sampled reward and baseline
                n = len(hist["reward_baseline"]) - sc_from
                sc_text = " reward: {} baseline: {}".format(sum(hist["reward_sample"][sc_from:]) / n, sum(hist["reward_baseline"][sc_from:]) / n)
            print("epoch {} train loss:{} valid loss: {} lr: {}{}{}{}".format(
                epoch, train_loss, valid_loss, optimizer.param_groups[0]['lr'],
                " ss_prob: {}".format(ss_prob) if opt.scheduled_sampling_start >= 0 else "", sc_text, norm_text))
        lr_scheduler.step(valid_loss)                                                          # train.py:155
        n_before = early_stopping.val_loss_min
        if rank == 0:
            early_stopping(valid_loss, model)                                                  # train.py:158
            if early_stopping.val_loss_min != n_before:
                hist["checkpoints"].append('stop.pth')
        stop = torch.tensor([1 if (rank == 0 and early_stopping.early_stop) else 0], device=dev)
        if world > 1:
            dist.broadcast(stop, 0)
        if int(stop):                                                                          # train.py:159-161
            if rank == 0:
                print("Early stopping")
            hist["stopped_at"] = epoch
            break
        if epoch % opt.save_freq == 0:                                                         # train.py:164-167
            save(str(epoch) + '.pth')
    save('final.pth')                                                                          # train.py:175
    hist["start_time"] = start_time
    if world > 1:
        dist.destroy_process_group()
    return hist


def main():
    run(parse())


if __name__ == '__main__':
    main()
