"""What the A/B bench tools (bench_persist.py, bench_step_kernels.py, bench_criterion.py) print per line: a tag and the sha1 of every output tensor of
every timed run, so that two library builds on one box can be compared for speed AND for bit-equal results."""
import hashlib

import torch


def sha(out):
    """sha1 (16 hex digits) of every tensor of a run's result, in order"""
    if torch.is_tensor(out):
        return [hashlib.sha1(out.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]]
    if isinstance(out, (tuple, list)):
        return [h for o in out for h in sha(o)]
    return []


def show(tag, line, shas):
    print("%s %s | sha1 %s" % (tag, line, " ".join("/".join(r) for r in shas)), flush=True)
