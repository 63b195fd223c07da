"""Caption generation for the MI355X S2VT path: the decode loops of the reference's eval.py
(`eval()` eval.py:30-60, `beam_eval()` :63-99) on top of the drop-in model — load a full-module checkpoint, decode the
test split greedily or by beam search, map ids to words and cut at `<eos>` (eval.py:54-58, :90-96).  --beam-mode cumulative
decodes with the cumulative-score beam search instead (mode='beam', not in the reference), through the same post-processing.

`main()` writes the predictions as JSON ({video_id: caption}) and, with --gts, scores them as the reference's
`__main__` does (eval.py:222-236: gts.json -> pred_to_coco_samples_IDs -> COCOScorer.score) with caption_metrics.py:
BLEU-1..4, ROUGE-L, CIDEr.  METEOR and the Stanford tokenizer are Java jars the reference does not ship
(`.MISSING_LARGE_BLOBS`); see caption_metrics.py for what stands in for them.  --perplexity scores the split's reference captions
under the model instead (mode='score', not in the reference): per-word perplexity and per-reference log-likelihoods.
--sample K additionally writes K sampled captions per clip (S2VT.sample_truncated, not in the reference; --temperature, --top-k, --top-p,
--sample-seed) to <out>.samples.json; with --sample-distinct (K <= 8) they are the K pairwise distinct captions of S2VT.sample_distinct
(stochastic beam search, not in the reference; no truncation, no constraints).  --no-repeat-ngram / --repetition-penalty / --min-length / --ban-words constrain the greedy captions
and those of --sample (S2VT.decode_constrained, not in the reference) and the search of --beam N --beam-mode cumulative
(S2VT.beam_constrained); they are refused together with the reference's search (--beam N --beam-mode reference).
--beam-groups G [--diversity-lambda x] (with --beam N --beam-mode cumulative, N a multiple of G) decodes by diverse beam search
(S2VT.beam_diverse, not in the reference): the prediction of a clip is the best of its G group-best captions (the lowest group wins a
tie), and all G with their scores (null for one that is not finite) go to <out>.groups.json.  The constraint flags compose with it.
--ensemble PATH[,PATH...] [--ensemble-weights w0,w1,...] (with --beam N --beam-mode cumulative) decodes with --model-path and the
further checkpoints as ONE search over the weighted mean of their word distributions (S2VTModel.Ensemble, not in the reference); the
first weight is --model-path's.  The constraint flags and --n-best compose with it.
--consensus (with --sample K, K >= 2; --beam N --beam-mode cumulative --n-best n, n >= 2, also under --ensemble; or --beam-groups G,
G >= 2; not in the reference) chooses among a clip's candidates the one that agrees most with the others under CIDEr-D with the
training split's idf (consensus / minimum-Bayes-risk selection, consensus.select on the device) and writes {video_id: {"chosen",
"utility", "captions"}} to <out>.consensus.json: with a beam search the choice is the prediction, with --sample the greedy
predictions stay.  Without the flag every file is what it was.
"""
import argparse
import json
import math

import torch


def ids_to_caption(ids, ix2word, drop_sos=False):
    """[token ids] -> 'w1 w2 ...' cut at the first <eos> (eval.py:54-58); beam results start with <sos> (eval.py:92-95)."""
    words = [ix2word[str(int(i))] for i in ids]
    if '<eos>' in words:
        words = words[:words.index('<eos>')]
    if drop_sos and '<sos>' in words:
        words.remove('<sos>')
    return ' '.join(words)


def generate(model_path, caption_file, feats_path, batch_size=10, mode='test', beam_width=5, max_beam_depth=30,
             split='test', device=None, length_alpha=0.7, n_best=1, nbest=None, constraints=None, beam_groups=0, diversity_lambda=0.5,
             groups=None, ensemble_paths=None, ensemble_weights=None):
    """{video_id: caption} of a split.  mode: 'test' (greedy), 'beam_search' (the reference's search) or 'beam' (cumulative scores,
    length_alpha; with a dict `nbest`, that is filled with {video_id: [the n_best captions, best first]}).  constraints (modes 'test'
    and 'beam'): keyword arguments of S2VT.decode_constrained / S2VT.beam_constrained, with `ban_words` looked up in the split's
    word2ix.  beam_groups > 0 (mode 'beam'): diverse beam search, S2VT.beam_diverse with that many groups and diversity_lambda -
    the caption of a clip is the group-best caption with the highest score (the lowest group wins a tie), and a dict `groups` is filled
    with {video_id: [{"caption", "score"} of every group, in group order]} (a score that is not finite: None).
    ensemble_paths (mode 'beam' without groups): further checkpoints decoded together with model_path by S2VTModel.Ensemble,
    ensemble_weights: one weight per model, model_path's first (None: uniform)."""
    import math
    import dataloader
    dev = device or torch.device('cuda', 0)
    dataset = dataloader.VideoDataset(caption_file, feats_path, mode=split)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False)
    model = torch.load(model_path, weights_only=False).to(dev)          # full-module pickle (eval.py:41)
    model.eval()
    if mode in ('beam_search', 'beam'):                                 # old pickles lack these attrs (eval.py:84-86)
        model.rnn_type, model.sos_ix, model.eos_ix = 'lstm', dataset.word2ix.get('<sos>', 3), dataset.word2ix.get('<eos>', 4)
    con = constraint_kwargs(constraints, dataset.word2ix, model)
    ensemble = None
    if ensemble_paths:
        if mode != 'beam' or beam_groups > 0:
            raise ValueError("ensemble_paths apply to mode='beam' without beam_groups")
        import S2VTModel
        members = [model] + [torch.load(p, weights_only=False).to(dev).eval() for p in ensemble_paths]
        for m in members[1:]:
            m.rnn_type, m.sos_ix, m.eos_ix = model.rnn_type, model.sos_ix, model.eos_ix
        ensemble = S2VTModel.Ensemble(members, ensemble_weights)
    preds = {}
    with torch.no_grad():
        for feats, targets, ids, masks in dataloader.feed_batches(loader, dev):
            if mode == 'beam_search':
                out = model(feats, mode='beam_search', beam_width=beam_width, max_beam_depth=max_beam_depth)
                for vid, seq in zip(ids, out):
                    preds[vid] = ids_to_caption([int(t.item()) for t in seq], dataset.ix2word, drop_sos=True)
            elif mode == 'beam' and beam_groups > 0:
                out, lens, scores = model.beam_diverse(feats, beam_width=beam_width, num_groups=beam_groups,
                                                       diversity_lambda=diversity_lambda, max_beam_depth=max_beam_depth,
                                                       length_alpha=length_alpha, n_best=1, **con)
                out, lens, scores = out[:, :, 0].cpu().tolist(), lens[:, :, 0].cpu().tolist(), scores[:, :, 0].cpu().tolist()
                for vid, rows, ln, sc in zip(ids, out, lens, scores):
                    caps = [ids_to_caption(r[:n], dataset.ix2word) for r, n in zip(rows, ln)]
                    preds[vid] = caps[max(range(len(sc)), key=lambda g: (sc[g], -g))]
                    if groups is not None:
                        # (a score can be -inf - a hypothesis through a word of log-prob -inf: null in the file, JSON has no infinity)
                        groups[vid] = [{"caption": c, "score": x if math.isfinite(x) else None} for c, x in zip(caps, sc)]
            elif mode == 'beam':
                if ensemble is not None:
                    out, lens, _ = ensemble.beam(feats, beam_width=beam_width, max_beam_depth=max_beam_depth, length_alpha=length_alpha,
                                                 n_best=n_best, **con)
                elif con:
                    out, lens, _ = model.beam_constrained(feats, beam_width=beam_width, max_beam_depth=max_beam_depth,
                                                          length_alpha=length_alpha, n_best=n_best, **con)
                else:
                    out, lens, _ = model(feats, mode='beam', beam_width=beam_width, max_beam_depth=max_beam_depth,
                                         length_alpha=length_alpha, n_best=n_best)
                out, lens = out.cpu().tolist(), lens.cpu().tolist()
                for vid, rows, ln in zip(ids, out, lens):
                    caps = [ids_to_caption(r[:n], dataset.ix2word) for r, n in zip(rows, ln)]
                    preds[vid] = caps[0]
                    if nbest is not None:
                        nbest[vid] = caps
            else:
                out = (model.decode_constrained(feats, **con)[:, 0] if con else model(feats, mode='test')).cpu()
                for vid, seq in zip(ids, out):
                    preds[vid] = ids_to_caption(seq.tolist(), dataset.ix2word)
    return preds


def constraint_kwargs(constraints, word2ix, model):
    """The keyword arguments of S2VT.decode_constrained for the command line's constraints ({} where there are none): `ban_words`
    become banned_ids through word2ix (an unknown word is an error), and <eos> is the vocabulary's."""
    if not constraints:
        return {}
    con = dict(constraints)
    words = con.pop("ban_words", None) or []
    unknown = [w for w in words if w not in word2ix]
    if unknown:
        raise ValueError("--ban-words: not in the vocabulary: %s" % ", ".join(unknown))
    con["banned_ids"] = [int(word2ix[w]) for w in words]
    if not hasattr(model, "decode_constrained"):
        raise NotImplementedError("constrained decoding needs S2VT.decode_constrained; %s has none" % type(model).__name__)
    model.eos_ix = word2ix.get('<eos>', 4)                              # (old pickles lack the attribute, as for the beam modes)
    return con


def distinct_draw(model, word2ix):
    """the draw of --sample-distinct as a callable (feats, n_samples, temperature, seed) -> ids [B, n_samples, L-1]: the n_samples
    pairwise distinct captions of S2VT.sample_distinct (stochastic beam search), at most L-1 words each as the other draws"""
    if not hasattr(model, "sample_distinct"):
        raise NotImplementedError("--sample-distinct needs S2VT.sample_distinct; %s has none" % type(model).__name__)
    model.rnn_type, model.sos_ix, model.eos_ix = 'lstm', word2ix.get('<sos>', 3), word2ix.get('<eos>', 4)      # (as for the beam modes)
    return lambda feats, n_samples, temperature, seed: model.sample_distinct(feats, n_samples, temperature=temperature, seed=seed,
                                                                             max_depth=model.length - 1)[0]


def sample_captions(model_path, caption_file, feats_path, n_samples, batch_size=10, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                    split='test', device=None, constraints=None, distinct=False):
    """{video_id: [n_samples captions]} of a split, drawn by S2VT.sample_truncated (one encode per clip; top_k / top_p cut every step's
    distribution, 0 / 1.0: off), each cut at its first <eos> like a greedy caption.  Batch i draws with seed + i.  distinct: the
    n_samples pairwise distinct captions of S2VT.sample_distinct instead (no truncation, no constraints)."""
    import dataloader
    dev = device or torch.device('cuda', 0)
    dataset = dataloader.VideoDataset(caption_file, feats_path, mode=split)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False)
    model = torch.load(model_path, weights_only=False).to(dev)
    model.eval()
    con = constraint_kwargs(constraints, dataset.word2ix, model)
    draw = model.decode_constrained if con else model.sample_truncated
    pick = distinct_draw(model, dataset.word2ix) if distinct else None
    out = {}
    with torch.no_grad():
        for i, (feats, targets, ids, masks) in enumerate(dataloader.feed_batches(loader, dev)):
            if pick is not None:
                drawn = pick(feats, n_samples, temperature, int(seed) + i).cpu().tolist()
            else:
                drawn = draw(feats, n_samples, temperature=temperature, seed=int(seed) + i, top_k=top_k, top_p=top_p, **con).cpu().tolist()
            for vid, rows in zip(ids, drawn):
                out[vid] = [ids_to_caption(r, dataset.ix2word) for r in rows]
    return out


def consensus_captions(model_path, caption_file, feats_path, source, batch_size=10, split='test', device=None, constraints=None,
                       n_samples=0, temperature=1.0, top_k=0, top_p=1.0, seed=0, beam_width=5, max_beam_depth=30, length_alpha=0.7,
                       n_best=1, beam_groups=0, diversity_lambda=0.5, ensemble_paths=None, ensemble_weights=None, distinct=False,
                       weights=None):
    """--consensus: per clip of a split the candidate caption that agrees most with the clip's other candidates under CIDEr-D
    (consensus.select: one kernel call per batch, the ids never leave the device before the choice is made), with the document
    frequencies of the caption file's TRAINING split - a DeviceCiderRewarder built the way train.py builds --sc-reward device's.
    source names the candidates, produced exactly as sample_captions / generate produce them: 'sample' the n_samples draws of
    S2VT.sample_truncated (batch i with seed + i; distinct: the pairwise distinct captions of S2VT.sample_distinct), 'nbest' the n_best list of the cumulative beam search (plain, constrained or the
    ensemble's), 'groups' the group-best captions of S2VT.beam_diverse.  A candidate whose score is not finite is not a candidate.
    -> (preds {video_id: chosen caption}, detail {video_id: {"chosen": k, "utility": [...], "captions": [...]}} - the utility of a
    candidate that is not valid: null -, scores {video_id: [the candidates' search scores]}, None for 'sample').
    weights (cider, bleu), or None for (1, 0): the utility is cider * CIDEr-D + bleu * sentence BLEU-4 (a DeviceMixedRewarder)."""
    import dataloader
    from s2vt_video_caption_amd import consensus
    from s2vt_video_caption_amd.self_critical import DeviceCiderRewarder, DeviceMixedRewarder
    if source not in ('sample', 'nbest', 'groups'):
        raise ValueError("consensus_captions: source must be 'sample', 'nbest' or 'groups', got %r" % (source,))
    dev = device or torch.device('cuda', 0)
    dataset = dataloader.VideoDataset(caption_file, feats_path, mode=split)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False)
    trainset = dataloader.VideoDataset(caption_file, feats_path, mode='train')
    sos, eos = dataset.word2ix.get('<sos>', 3), dataset.word2ix.get('<eos>', 4)
    if weights is None:
        rewarder = DeviceCiderRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos, device=dev,
                                       vocab_size=len(dataset.word2ix))
    else:
        rewarder = DeviceMixedRewarder(trainset.captions, [p.stem for p in trainset.feat_paths], sos, eos, weights[0], weights[1],
                                       device=dev, vocab_size=len(dataset.word2ix))
    model = torch.load(model_path, weights_only=False).to(dev)
    model.eval()
    if source != 'sample':
        model.rnn_type, model.sos_ix, model.eos_ix = 'lstm', sos, eos
    con = constraint_kwargs(constraints, dataset.word2ix, model)
    ensemble = None
    if ensemble_paths:
        if source != 'nbest':
            raise ValueError("ensemble_paths apply to source 'nbest'")
        import S2VTModel
        members = [model] + [torch.load(p, weights_only=False).to(dev).eval() for p in ensemble_paths]
        for m in members[1:]:
            m.rnn_type, m.sos_ix, m.eos_ix = model.rnn_type, model.sos_ix, model.eos_ix
        ensemble = S2VTModel.Ensemble(members, ensemble_weights)
    preds, detail, all_scores = {}, {}, (None if source == 'sample' else {})
    with torch.no_grad():
        for i, (feats, targets, ids, masks) in enumerate(dataloader.feed_batches(loader, dev)):
            scores = None
            if source == 'sample' and distinct:
                cands = distinct_draw(model, dataset.word2ix)(feats, n_samples, temperature, int(seed) + i)
            elif source == 'sample':
                draw = model.decode_constrained if con else model.sample_truncated
                cands = draw(feats, n_samples, temperature=temperature, seed=int(seed) + i, top_k=top_k, top_p=top_p, **con)
            elif source == 'groups':
                cands, _, scores = model.beam_diverse(feats, beam_width=beam_width, num_groups=beam_groups, diversity_lambda=diversity_lambda,
                                                      max_beam_depth=max_beam_depth, length_alpha=length_alpha, n_best=1, **con)
                cands, scores = cands[:, :, 0], scores[:, :, 0]
            else:
                kw = dict(beam_width=beam_width, max_beam_depth=max_beam_depth, length_alpha=length_alpha, n_best=n_best)
                if ensemble is not None:
                    cands, _, scores = ensemble.beam(feats, **kw, **con)
                elif con:
                    cands, _, scores = model.beam_constrained(feats, **kw, **con)
                else:
                    cands, _, scores = model(feats, mode='beam', **kw)
            _, best, utility = consensus.select(rewarder, cands, scores)
            rows, best, utility = cands.cpu().tolist(), best.cpu().tolist(), utility.cpu().tolist()
            scores = None if scores is None else scores.cpu().tolist()
            for b, vid in enumerate(ids):
                caps = [ids_to_caption(r, dataset.ix2word) for r in rows[b]]
                preds[vid] = caps[best[b]]
                detail[vid] = {"chosen": best[b], "utility": [u if math.isfinite(u) else None for u in utility[b]], "captions": caps}
                if scores is not None:
                    all_scores[vid] = scores[b]
    return preds, detail, all_scores


def pack_references(ref_lists, eos_ix, max_len):
    """The reference captions of a batch of clips as ONE mode='score' input: ref_lists = per clip its token lists (<sos>, words,
    <eos>, as dataloader.VideoDataset.captions holds them), cut at max_len.  -> (int64 [B, K, T], counts): K = the most references
    any clip has (a clip with fewer repeats its first one; counts[b] says how many rows are real), T = the batch's longest caption
    (at least 2), shorter ones right-padded with <eos>."""
    refs = [[list(r)[:max_len] for r in rs] for rs in ref_lists]
    if not refs or any(not rs or any(len(r) < 2 for r in rs) for rs in refs):
        raise ValueError("every clip needs at least one reference caption of at least two tokens")
    K = max(len(rs) for rs in refs)
    T = max(len(r) for rs in refs for r in rs)
    caps = torch.full((len(refs), K, T), int(eos_ix), dtype=torch.long)
    for b, rs in enumerate(refs):
        for k in range(K):
            r = rs[k] if k < len(rs) else rs[0]
            caps[b, k, :len(r)] = torch.tensor(r, dtype=torch.long)
    return caps, [len(rs) for rs in refs]


def perplexity_summary(logliks, lengths):
    """{total_loglik, tokens, perplexity, mean_caption_loglik} of per-caption log-likelihoods and scored-token counts (the <eos>
    counts): per-word perplexity = exp(-sum of log-likelihoods / sum of tokens)."""
    import math
    total, tokens = float(sum(logliks)), int(sum(lengths))
    if not logliks or tokens <= 0:
        raise ValueError("no caption was scored")
    return {"total_loglik": total, "tokens": tokens, "perplexity": math.exp(-total / tokens),
            "mean_caption_loglik": total / len(logliks)}


def reference_logliks(model_path, caption_file, feats_path, batch_size=10, split='test', device=None):
    """({video_id: [log-likelihood of each reference caption]}, summary) of a split under the model: every reference of every clip
    scored by mode='score' (length_alpha = 0: plain sums), the references of a clip in one call."""
    import dataloader
    dev = device or torch.device('cuda', 0)
    dataset = dataloader.VideoDataset(caption_file, feats_path, mode=split)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=False)
    model = torch.load(model_path, weights_only=False).to(dev)
    model.eval()
    model.rnn_type, model.sos_ix, model.eos_ix = 'lstm', dataset.word2ix.get('<sos>', 3), dataset.word2ix.get('<eos>', 4)
    out, lls, ns = {}, [], []
    with torch.no_grad():
        for feats, targets, ids, masks in dataloader.feed_batches(loader, dev):
            caps, counts = pack_references([dataset.captions[v] for v in ids], model.eos_ix, model.length)
            scores, lengths, _ = model(feats, targets=caps.to(dev), mode='score', length_alpha=0.0)
            scores, lengths = scores.cpu().tolist(), lengths.cpu().tolist()
            for vid, sc, ln, c in zip(ids, scores, lengths, counts):
                out[vid] = sc[:c]
                lls.extend(sc[:c])
                ns.extend(ln[:c])
    return out, perplexity_summary(lls, ns)


def to_samples(prediction_dict, gts):
    """{video_id: caption} -> ({video_id: [{'image_id', 'caption'}]}, ids) for the ids that have ground truth
    (pred_to_coco_samples_IDs, eval.py:138-151)."""
    samples = {k: [{'image_id': k, 'caption': v}] for k, v in prediction_dict.items() if k in gts}
    return samples, list(samples.keys())


def score(prediction_dict, gts_file):
    """Metrics of a prediction dictionary against a gts.json ({'gts': {video_id: [{'caption': ...}, ...]}})."""
    import caption_metrics
    with open(gts_file, encoding='utf-8') as f:
        gts = json.load(f)['gts']
    samples, ids = to_samples(prediction_dict, gts)
    scorer = caption_metrics.CaptionScorer()
    scorer.score(gts, samples, ids)
    return scorer


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--caption-file", default="./data/captions_server.json")
    ap.add_argument("--feats-path", default="./data/feats/vgg16_bn")
    ap.add_argument("--batch-size", type=int, default=10)
    ap.add_argument("--beam", type=int, default=0, help="beam width (0: greedy)")
    ap.add_argument("--beam-mode", choices=("reference", "cumulative"), default="reference",
                    help="with --beam: the reference's search (last-token scores) or cumulative log-prob scores (width <= 8)")
    ap.add_argument("--length-alpha", type=float, default=0.7, help="cumulative: a finished caption scores sum / length**alpha")
    ap.add_argument("--n-best", type=int, default=1,
                    help="cumulative: captions kept per clip; more than one also writes {video_id: [captions]} to <out>.nbest.json")
    ap.add_argument("--beam-groups", type=int, default=0, metavar="G",
                    help="cumulative: diverse beam search (S2VT.beam_diverse) with G groups of --beam / G slots; the prediction is the "
                         "best group-best caption, all G with their scores go to <out>.groups.json (0: off)")
    ap.add_argument("--diversity-lambda", type=float, default=None, metavar="X",
                    help="--beam-groups: what a candidate loses per earlier group that chose its word at this depth (default 0.5)")
    ap.add_argument("--ensemble", default="", metavar="PATH[,PATH...]",
                    help="cumulative: further checkpoints decoded together with --model-path as one search over the weighted mean of "
                         "the models' word distributions (S2VTModel.Ensemble)")
    ap.add_argument("--ensemble-weights", default="", metavar="W0,W1,...",
                    help="--ensemble: one positive weight per model, --model-path's first (default: uniform)")
    ap.add_argument("--perplexity", action="store_true",
                    help="instead of decoding: score every reference caption of the split (mode='score'), print total "
                         "log-likelihood, tokens, per-word perplexity and mean per-caption log-likelihood, write "
                         "{video_id: [per-reference log-likelihoods]} to <out>.ll.json")
    ap.add_argument("--sample", type=int, default=0, metavar="K",
                    help="also draw K captions per clip (S2VT.sample_truncated) and write {video_id: [captions]} to <out>.samples.json")
    ap.add_argument("--temperature", type=float, default=1.0, help="--sample: draw from softmax(logit / temperature)")
    ap.add_argument("--top-k", type=int, default=0, help="--sample: draw among the k most probable words of a step (0: off)")
    ap.add_argument("--top-p", type=float, default=1.0,
                    help="--sample: draw from the smallest set of most probable words whose mass reaches p (1: off)")
    ap.add_argument("--sample-seed", type=int, default=0, help="--sample: batch i draws with this seed + i")
    ap.add_argument("--sample-distinct", action="store_true",
                    help="--sample K (K <= 8): the K captions are pairwise distinct - sampled without replacement by stochastic beam "
                         "search (S2VT.sample_distinct) at --temperature; not with --top-k, --top-p or the constraint flags")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, metavar="N",
                    help="greedy, --sample and --beam-mode cumulative: never complete an n-gram the caption already holds (0: off)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, metavar="THETA",
                    help="greedy, --sample and --beam-mode cumulative: divide the positive logits of the words generated so far by THETA, multiply the others (1: off)")
    ap.add_argument("--min-length", type=int, default=0, metavar="M", help="greedy, --sample and --beam-mode cumulative: no <eos> among the first M words")
    ap.add_argument("--ban-words", default="", metavar="W1,W2", help="greedy, --sample and --beam-mode cumulative: words that are never generated, e.g. \"<unk>,<pad>\"")
    ap.add_argument("--consensus", action="store_true",
                    help="with --sample K (K >= 2), --beam N --beam-mode cumulative --n-best n (n >= 2; also under --ensemble) or "
                         "--beam-groups G (G >= 2): choose among the clip's candidates the one that agrees most with the others under "
                         "CIDEr-D (consensus / minimum-Bayes-risk selection on the device, consensus.select; idf of the training split) "
                         "and write {video_id: {chosen, utility, captions}} to <out>.consensus.json.  With a beam search the choice is "
                         "the prediction; with --sample the greedy predictions stay as they are")
    ap.add_argument("--consensus-cider-weight", type=float, default=1.0, metavar="w",
                    help="--consensus: the utility is w * CIDEr-D + (--consensus-bleu-weight) * sentence BLEU-4, each against the clip's "
                         "other candidates (1 and 0, the defaults: CIDEr-D alone, every file as without the two flags)")
    ap.add_argument("--consensus-bleu-weight", type=float, default=0.0, metavar="w",
                    help="--consensus: weight of the sentence BLEU-4 in the utility (s2vt_mixed_consensus on the device; "
                         "<out>.consensus.json then records the two weights under \"_weights\")")
    ap.add_argument("--out", default="predictions.json")
    ap.add_argument("--gts", default=None, help="gts.json: also print BLEU / ROUGE-L / CIDEr of the predictions")
    return ap


def constraints_of(a):
    """the constraint flags of parsed arguments as a dict, or None where none is set"""
    words = [w for w in a.ban_words.split(",") if w]
    if a.no_repeat_ngram == 0 and a.repetition_penalty == 1.0 and a.min_length == 0 and not words:
        return None
    return dict(no_repeat_ngram_size=a.no_repeat_ngram, repetition_penalty=a.repetition_penalty, min_length=a.min_length, ban_words=words)


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    constraints = constraints_of(a)
    if constraints and a.beam and a.beam_mode != "cumulative":
        ap.error("--no-repeat-ngram / --repetition-penalty / --min-length / --ban-words apply to greedy decoding, --sample and "
                 "--beam N --beam-mode cumulative, not to the reference's search (--beam-mode reference)")
    if (a.beam_groups or a.diversity_lambda is not None) and not (a.beam and a.beam_mode == "cumulative"):
        ap.error("--beam-groups / --diversity-lambda apply to --beam N --beam-mode cumulative only")
    if a.diversity_lambda is not None and not a.beam_groups:
        ap.error("--diversity-lambda needs --beam-groups G")
    if a.beam_groups < 0 or (a.beam_groups and a.n_best > 1):
        ap.error("--beam-groups must be >= 1, and it keeps one caption per group (--n-best 1)")
    ens_paths = [p for p in a.ensemble.split(",") if p]
    ens_weights = None
    if a.ensemble_weights and not ens_paths:
        ap.error("--ensemble-weights needs --ensemble PATH[,PATH...]")
    if ens_paths:
        if not (a.beam and a.beam_mode == "cumulative") or a.beam_groups or a.sample or a.perplexity:
            ap.error("--ensemble applies to --beam N --beam-mode cumulative only, without --beam-groups, --sample or --perplexity")
        if a.ensemble_weights:
            try:
                ens_weights = [float(w) for w in a.ensemble_weights.split(",")]
            except ValueError:
                ap.error("--ensemble-weights: numbers separated by commas, got %r" % a.ensemble_weights)
            if len(ens_weights) != len(ens_paths) + 1:
                ap.error("--ensemble-weights: %d weights for %d models (--model-path's comes first)" % (len(ens_weights), len(ens_paths) + 1))
    if a.sample_distinct:
        if not 1 <= a.sample <= 8:
            ap.error("--sample-distinct needs --sample K with 1 <= K <= 8")
        if a.top_k != 0 or a.top_p != 1.0 or constraints:
            ap.error("--sample-distinct samples from the whole distribution: not with --top-k, --top-p, --no-repeat-ngram, "
                     "--repetition-penalty, --min-length or --ban-words")
    cons_source = None
    if not (math.isfinite(a.consensus_cider_weight) and math.isfinite(a.consensus_bleu_weight)):
        ap.error("--consensus-cider-weight / --consensus-bleu-weight must be finite")
    cons_weights = None
    if a.consensus_cider_weight != 1.0 or a.consensus_bleu_weight != 0.0:
        if not a.consensus:
            ap.error("--consensus-cider-weight / --consensus-bleu-weight need --consensus")
        cons_weights = (a.consensus_cider_weight, a.consensus_bleu_weight)
    if a.consensus:
        sources = [s for s, on in (("sample", a.sample >= 2), ("groups", a.beam_groups >= 2),
                                   ("nbest", bool(a.beam) and a.beam_mode == "cumulative" and not a.beam_groups and a.n_best >= 2)) if on]
        if len(sources) != 1 or a.perplexity:
            ap.error("--consensus chooses among the candidates of exactly one of --sample K (K >= 2), --beam N --beam-mode cumulative "
                     "--n-best n (n >= 2) and --beam-groups G (G >= 2), and not with --perplexity")
        cons_source = sources[0]
    if a.perplexity:
        per_clip, summary = reference_logliks(a.model_path, a.caption_file, a.feats_path, a.batch_size)
        print("total log-likelihood {total_loglik:.4f} over {tokens} tokens: per-word perplexity {perplexity:.4f}, "
              "mean per-caption log-likelihood {mean_caption_loglik:.4f}".format(**summary))
        with open(a.out + ".ll.json", 'w', encoding='utf-8') as f:
            json.dump(per_clip, f, ensure_ascii=False, indent=1)
        return summary
    cumulative = bool(a.beam) and a.beam_mode == "cumulative"
    nbest = {} if cumulative and a.n_best > 1 else None
    groups = {} if a.beam_groups else None
    diverse = dict(beam_groups=a.beam_groups, diversity_lambda=0.5 if a.diversity_lambda is None else a.diversity_lambda,
                   groups=groups) if a.beam_groups else {}
    cons = None
    if cons_source in ("nbest", "groups"):
        # the search's candidates, the consensus choice as the prediction; the n-best / groups files as without the flag
        preds, cons, cand_scores = consensus_captions(
            a.model_path, a.caption_file, a.feats_path, cons_source, a.batch_size, constraints=constraints, beam_width=a.beam,
            length_alpha=a.length_alpha, n_best=a.n_best, beam_groups=a.beam_groups,
            diversity_lambda=0.5 if a.diversity_lambda is None else a.diversity_lambda, ensemble_paths=ens_paths or None,
            ensemble_weights=ens_weights, weights=cons_weights)
        if nbest is not None:
            nbest.update({v: d["captions"] for v, d in cons.items()})
        if groups is not None:
            groups.update({v: [{"caption": c, "score": x if math.isfinite(x) else None} for c, x in zip(d["captions"], cand_scores[v])]
                           for v, d in cons.items()})
    else:
        preds = generate(a.model_path, a.caption_file, a.feats_path, a.batch_size,
                         ('beam' if cumulative else 'beam_search') if a.beam else 'test', beam_width=a.beam or 5,
                         length_alpha=a.length_alpha, n_best=a.n_best if cumulative else 1, nbest=nbest, constraints=constraints,
                         **diverse, **(dict(ensemble_paths=ens_paths, ensemble_weights=ens_weights) if ens_paths else {}))
    with open(a.out, 'w', encoding='utf-8') as f:
        json.dump(preds, f, ensure_ascii=False, indent=1)
    print("wrote {} captions to {}".format(len(preds), a.out))
    if nbest is not None:
        with open(a.out + ".nbest.json", 'w', encoding='utf-8') as f:
            json.dump(nbest, f, ensure_ascii=False, indent=1)
    if groups is not None:
        with open(a.out + ".groups.json", 'w', encoding='utf-8') as f:
            json.dump(groups, f, ensure_ascii=False, indent=1)
    if a.sample > 0:
        if cons_source == "sample":            # the same draws, kept on the device for the choice; the predictions above stay greedy
            _, cons, _ = consensus_captions(a.model_path, a.caption_file, a.feats_path, "sample", a.batch_size, constraints=constraints,
                                            n_samples=a.sample, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.sample_seed,
                                            distinct=a.sample_distinct, weights=cons_weights)
            samples = {v: d["captions"] for v, d in cons.items()}
        else:
            samples = sample_captions(a.model_path, a.caption_file, a.feats_path, a.sample, a.batch_size, a.temperature, a.top_k, a.top_p,
                                      a.sample_seed, constraints=constraints, distinct=a.sample_distinct)
        with open(a.out + ".samples.json", 'w', encoding='utf-8') as f:
            json.dump(samples, f, ensure_ascii=False, indent=1)
        print("wrote {} sampled captions per clip to {}".format(a.sample, a.out + ".samples.json"))
    if cons is not None:
        with open(a.out + ".consensus.json", 'w', encoding='utf-8') as f:
            json.dump(cons if cons_weights is None else dict(cons, _weights={"cider": cons_weights[0], "bleu": cons_weights[1]}), f,
                      ensure_ascii=False, indent=1)
        print("wrote the consensus choice among {} candidates per clip to {}".format(
            len(next(iter(cons.values()))["captions"]) if cons else 0, a.out + ".consensus.json"))
    if a.gts:
        scorer = score(preds, a.gts)
        print("***********************")
        print(scorer.eval)
        print("***********************")


if __name__ == '__main__':
    main()
