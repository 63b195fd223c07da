"""CPU: K captions per clip on one encode (S2VT.forward with 3-D targets; the grouped path of the fp32 train driver,
csrc/api_train_f32.hip) - the C ABI's surface, the size query without a device and its sizes against a table recorded from the build
before the grouped driver was merged into the fp32 train driver (tests/golden/group_workspace_layout.json), the argument checks that
come before any device call, the dataset's K-caption items and train.py's flags.

Recording the table (with the library whose layout is the reference):
    S2VT_LIB=<library> PYTHONPATH=. python tests/test_train_group_host.py tests/golden/group_workspace_layout.json"""
import ctypes
import inspect
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi

import test_decode_plan_host as plan  # noqa: E402  (the shapes of the recorded layout tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "group_workspace_layout.json")
GROUP_K = (1, 2, 5)
PIPE_BLOCKS = (0, 32)
NEW = ("s2vt_train_group_workspace_bytes", "s2vt_train_group_forward", "s2vt_train_group_backward", "s2vt_group_sum_rows")


def test_new_symbols_declared_exported_bound_and_abi_9(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in capi.SIGNATURES, name
    assert re.search(r"#define S2VT_ABI_VERSION 9\b", header)
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9


def test_workspace_query_without_a_device(lib):
    d = capi.Dims(16, 80, 4096, 512, 512, 3000)
    sizes = [lib.s2vt_train_group_workspace_bytes(ctypes.byref(d), K) for K in (0, 1, 2, 5)]
    assert sizes[0] == 0 and 0 < sizes[1] < sizes[2] < sizes[3]
    assert lib.s2vt_train_group_workspace_bytes(ctypes.byref(d), -1) == 0
    assert lib.s2vt_train_group_workspace_bytes(ctypes.byref(capi.Dims(0, 80, 4096, 512, 512, 3000)), 2) == 0
    assert lib.s2vt_train_group_workspace_bytes(ctypes.byref(capi.Dims(16, 1, 4096, 512, 512, 3000)), 2) == 0
    assert lib.s2vt_train_group_workspace_bytes(None, 2) == 0
    # L * B * K rows past what the column sums' 64-row chunks index (64 * 65535 rows)
    assert lib.s2vt_train_group_workspace_bytes(ctypes.byref(d), 64 * 65535 // (80 * 16) + 1) == 0
    # the decode images are the part that grows with K: K = 5 costs less than five K = 1 workspaces
    assert sizes[3] < 5 * sizes[1]


def group_layout_table(lib):
    """{"pipe_block": [[s2vt_train_group_workspace_bytes at K = 1, 2, 5] for every (L, F, E, V) x H x B of test_decode_plan_host.py, in
    that order]}; the option is put back afterwards"""
    before = lib.s2vt_set_option(b"pipe_block", -1)
    table = {}
    try:
        for blk in PIPE_BLOCKS:
            lib.s2vt_set_option(b"pipe_block", blk)
            table[str(blk)] = [[lib.s2vt_train_group_workspace_bytes(ctypes.byref(capi.Dims(B, L, F, H, E, V)), K) for K in GROUP_K]
                               for (L, F, E, V), H, B in itertools.product(plan.LFEV, plan.HIDDEN, plan.BATCHES)]
    finally:
        lib.s2vt_set_option(b"pipe_block", before)
    return table


def test_group_workspace_layouts_are_the_recorded_ones(lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = group_layout_table(lib)
    assert sorted(got) == sorted(want) == sorted(str(b) for b in PIPE_BLOCKS)
    shapes = list(itertools.product(plan.LFEV, plan.HIDDEN, plan.BATCHES))
    for key in want:
        assert len(got[key]) == len(want[key]) == len(shapes)
        for shape, g, w in zip(shapes, got[key], want[key]):
            assert g == w and len(g) == len(GROUP_K) and 0 < g[0] < g[1] < g[2], (key, shape, g, w)


def test_library_argument_errors_come_before_the_device(lib):
    """null pointers stand for device memory: every rejection happens before anything is enqueued"""
    d = capi.Dims(4, 6, 16, 8, 8, 30)
    p, g = capi.Params(), capi.Grads()
    one = ctypes.c_void_p(256)
    big = 1 << 40

    def fwd(K=2, sb=10, sk=5, ws=big, feats=one, dims=d):
        return lib.s2vt_train_group_forward(ctypes.byref(dims), ctypes.byref(p), feats, one, sb, sk, K, None, one, one, ws, None)
    for kw in (dict(K=0), dict(K=-2), dict(sb=-1), dict(sk=-5), dict(ws=16), dict(feats=None), dict(dims=capi.Dims(4, 1, 16, 8, 8, 30)),
               dict(K=64 * 65535)):
        assert fwd(**kw) == -1, kw
        assert b"s2vt_train_group_forward" in lib.s2vt_last_error()
    # a backward on a workspace no grouped forward filled
    assert lib.s2vt_train_group_backward(ctypes.byref(d), ctypes.byref(p), one, one, None, ctypes.byref(g), None, one, big, None) == -1
    assert b"no s2vt_train_group_forward has run on this workspace" in lib.s2vt_last_error()
    assert lib.s2vt_train_group_backward(ctypes.byref(d), ctypes.byref(p), one, None, None, ctypes.byref(g), None, one, big, None) == -1
    assert lib.s2vt_group_sum_rows(one, 8, None, 8, 4, 2, 8, None) == -1
    assert lib.s2vt_group_sum_rows(one, 8, ctypes.c_void_p(1 << 20), 8, 4, 2, 9, None) == -1       # cols > ld


def test_forward_refusals_come_before_the_device():
    import S2VTModel
    B, L, Fd, V = 2, 5, 16, 30
    x = torch.zeros(B, L, Fd)                        # CPU tensors: a bad argument is refused before the tensors are looked at
    good = torch.zeros(B, 3, L - 1, dtype=torch.long)
    for kw in ({}, dict(rnn_type="gru"), dict(num_layers=2)):
        m = S2VTModel.S2VT(V, Fd, L, dim_hid=8, dim_embed=8, **kw)
        for bad in (torch.zeros(B + 1, 3, L - 1, dtype=torch.long), torch.zeros(B, 3, L, dtype=torch.long),
                    torch.zeros(B, 3, L - 2, dtype=torch.long), torch.zeros(B, 0, L - 1, dtype=torch.long)):
            with pytest.raises(ValueError, match=r"targets must be \[B, K, L-1\]"):
                m(x, targets=bad, mode="train")
        with pytest.raises(ValueError, match="scheduled sampling"):
            m(x, targets=good, mode="train", ss_prob=0.25)
        with pytest.raises(capi.S2VTHipError, match="HIP"):      # good arguments: the CPU tensors fail loudly
            m(x, targets=good, mode="train")
    sig = inspect.signature(S2VTModel.S2VT.forward)
    assert list(sig.parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob", "ss_temperature",
                                    "length_alpha", "n_best", "temperature", "seed"]


def test_functional_checks_targets_on_the_host():
    from s2vt_video_caption_amd import functional
    with pytest.raises(capi.S2VTHipError, match="HIP"):
        functional.group_targets(torch.zeros(2, 3, 4, dtype=torch.long), 2, 4)
    sig = inspect.signature(functional.train_forward_group)
    assert list(sig.parameters) == ["feats", "targets", "params", "grad_sink", "out_mask"]
    assert sig.parameters["grad_sink"].default is None and sig.parameters["out_mask"].default is None


def test_dp_train_step_group_keyword():
    from s2vt_video_caption_amd import dp
    sig = inspect.signature(dp.train_step)
    assert list(sig.parameters)[-1] == "group" and sig.parameters["group"].default is None


def _make(tmp_path, n=6, L=8, F=16):
    rng = np.random.RandomState(0)
    caps, ids = {}, []
    os.makedirs(tmp_path / "feats")
    for i in range(n):
        vid = "vid%d" % i
        ids.append(vid)
        np.save(tmp_path / "feats" / (vid + ".npy"), rng.randn(L, F).astype(np.float32))
        caps[vid] = [[3] + [int(x) for x in rng.randint(5, 20, size=rng.randint(1, 12))] + [4] for _ in range(rng.randint(2, 5))]
    data = {"word2ix": {str(i): i for i in range(20)}, "ix2word": {str(i): str(i) for i in range(20)},
            "captions": caps, "splits": {"train": ids[:4], "valid": ids[4:5], "test": ids[5:]}}
    with open(tmp_path / "captions.json", "w") as f:
        json.dump(data, f)
    return data


def test_dataset_k_captions_per_clip(tmp_path):
    import dataloader
    data = _make(tmp_path)
    args = (str(tmp_path / "captions.json"), str(tmp_path / "feats"))
    today = dataloader.VideoDataset(*args, max_len=8, mode="train")
    one = dataloader.VideoDataset(*args, max_len=8, mode="train", captions_per_clip=1)
    three = dataloader.VideoDataset(*args, max_len=8, mode="train", captions_per_clip=3)
    # K = 1: today's item, today's RNG stream (the generator stands where it stood after the same items)
    np.random.seed(5)
    a = [today[i] for i in range(len(today))]
    after_a = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    b = [one[i] for i in range(len(one))]
    after_b = np.random.randint(0, 1 << 30)
    assert after_a == after_b
    for (fa, la, ia, ma), (fb, lb, ib, mb) in zip(a, b):
        assert ia == ib and torch.equal(fa, fb) and torch.equal(la, lb) and torch.equal(ma, mb)
        assert tuple(lb.shape) == (8,) and tuple(mb.shape) == (8,)
    # K = 3: [3, max_len], K successive draws of the same expression
    np.random.seed(5)
    items = [three[i] for i in range(len(three))]
    np.random.seed(5)
    for (feat, labels, vid, masks), path in zip(items, three.feat_paths):
        assert vid == path.stem and tuple(feat.shape) == (8, 16)
        assert labels.dtype == torch.int64 and tuple(labels.shape) == (3, 8)
        assert masks.dtype == torch.float32 and tuple(masks.shape) == (3, 8)
        refs = data["captions"][vid]
        for k in range(3):
            want = refs[int(np.random.randint(0, len(refs), size=1)[0])][:8]
            assert labels[k].tolist() == want + [0] * (8 - len(want))
            assert masks[k].tolist() == [1.0] * len(want) + [0.0] * (8 - len(want))
    loader = torch.utils.data.DataLoader(three, batch_size=2, shuffle=False)
    feats, targets, ids, masks = next(iter(dataloader.feed_batches(loader, dev=torch.device("cpu"))))
    assert tuple(feats.shape) == (2, 8, 16) and tuple(targets.shape) == (2, 3, 8) and tuple(masks.shape) == (2, 3, 8)
    with pytest.raises(ValueError):
        dataloader.VideoDataset(*args, max_len=8, mode="train", captions_per_clip=0)


def test_train_flags():
    sys.path.insert(0, ROOT)
    import train
    opt = train.parse([])
    assert opt.captions_per_clip == 1 and opt.sc_shared_encode is False
    assert train.parse(["--captions-per-clip", "4"]).captions_per_clip == 4
    opt = train.parse(["--self-critical", "--sc-samples", "5", "--sc-baseline", "mean", "--sc-shared-encode"])
    assert opt.sc_shared_encode is True and opt.sc_samples == 5
    for bad in (["--sc-shared-encode"], ["--captions-per-clip", "0"], ["--captions-per-clip", "-2"],
                ["--captions-per-clip", "3", "--model", "att_baseline"], ["--captions-per-clip", "3", "--scheduled-sampling-start", "0"],
                ["--captions-per-clip", "2", "--self-critical"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
    sig = inspect.signature(train.make_self_critical_step)
    assert sig.parameters["shared_encode"].default is False


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        json.dump(group_layout_table(capi.load()), out, separators=(",", ":"))
        out.write("\n")
    print("recorded", sys.argv[1], "from", capi.LIB_PATH)
