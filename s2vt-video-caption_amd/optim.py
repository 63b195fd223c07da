"""The reference's optimizer (train.py:89-93: torch.optim.Adam with default betas / eps) as ONE kernel launch per step.

`FlatAdam(model, lr)` moves the parameters of the HIP S2VT module into one flat fp32 buffer (every `param.data` becomes a
view into it: names, shapes, state_dict and pickles are unchanged), keeps the gradients in a second flat buffer that the backward
WRITES into directly (`functional.set_grad_sink`, the mechanism of `dp.FlatGradAllReducer.attach`; `param.grad` are views of it,
so hooks / inspection still see them) and the two moments in two more; `step()` is `s2vt_adam_step` - 28 bytes per parameter
in one launch instead of torch's multi-tensor launches.  Same arithmetic as `torch.optim.Adam` operation for operation
(`tests/test_gpu_kernels.py::test_flat_adam_step_is_torch_adam`, `::test_flat_adam_trains_the_model_as_torch_adam_does`); `lr` may be changed through `param_groups[0]["lr"]`, so
`ReduceLROnPlateau` works on it unchanged.

Around that step, on the device and off by default: global-norm gradient clipping (`max_grad_norm`), weight decay (`weight_decay`,
coupled as in `torch.optim.Adam(weight_decay=)` or `decoupled` as in `torch.optim.AdamW`, with `no_decay` parameters left out) and
a guard that skips a step whose gradient is not finite (`skip_nonfinite`).  With any of them set `step()` enqueues
`s2vt_grad_norm` (two launches: the norm in fp64, in a fixed order, and a record {grad_norm, scale, nonfinite, skipped_total} on
the device) and `s2vt_adam_step_clipped`, which reads the record on the device - three launches and no host read; the arithmetic is
stated at "clipped step" in include/s2vt_hip.h and restated in numpy by tests/optim_ref.py.  At the defaults `step()` makes the
single `s2vt_adam_step` call it always made.
"""
import ctypes
import math

import torch

from . import capi, functional

# the keys the clipped step added to param_groups[0] and their defaults: a state saved before they existed loads with these
CLIP_DEFAULTS = dict(max_grad_norm=None, weight_decay=0.0, decoupled=False, no_decay=(), skip_nonfinite=False)


def matches_no_decay(name, no_decay):
    """An entry of `no_decay` matches a parameter name that ENDS with it ("embedding.weight", "bias" for `feat_linear.bias`) or whose
    last dotted component STARTS with it ("bias" for `vid_rnn.bias_ih_l0`, whose names carry the gate set and layer behind)."""
    last = name.rsplit(".", 1)[-1]
    return any(name.endswith(e) or last.startswith(e) for e in no_decay)


def decay_segments(names, slices, no_decay):
    """(seg_end, seg_decay) of s2vt_adam_step_clipped for parameters `names` that occupy `slices` [(lo, hi), ...] of the flat buffers,
    in that order: one segment per run of neighbouring parameters with the same decay flag (0 where matches_no_decay).  The slices
    must tile [0, n) in ascending order; more than 16 segments after merging raise ValueError."""
    ends, flags, at = [], [], 0
    for name, (lo, hi) in zip(names, slices):
        if lo != at or hi <= lo:
            raise ValueError("decay_segments: the slices must tile the flat buffer in ascending order (%r at %d)" % (name, at))
        at = hi
        flag = 0 if matches_no_decay(name, no_decay) else 1
        if flags and flags[-1] == flag:
            ends[-1] = hi
        else:
            ends.append(hi)
            flags.append(flag)
    if len(ends) > capi.ADAM_MAX_SEGMENTS:
        raise ValueError("no_decay=%r cuts the parameters into %d segments; the step takes at most %d" % (tuple(no_decay), len(ends),
                                                                                                         capi.ADAM_MAX_SEGMENTS))
    return ends, flags


def check_clip_args(max_grad_norm, weight_decay):
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
        raise ValueError("max_grad_norm must be positive (None: no clipping), got %r" % (max_grad_norm,))
    if not (math.isfinite(float(weight_decay)) and float(weight_decay) >= 0.0):
        raise ValueError("weight_decay must be finite and >= 0, got %r" % (weight_decay,))


class FlatAdam(torch.optim.Optimizer):
    """FlatAdam(model, lr, betas, eps, reducer, *, max_grad_norm=None, weight_decay=0.0, decoupled=False, no_decay=(),
    skip_nonfinite=False).

    max_grad_norm   c > 0: every gradient is multiplied by min(c / (norm + 1e-6), 1), norm = the 2-norm of ALL gradients
                    (torch.nn.utils.clip_grad_norm_'s rule; the norm is summed in fp64).  THE CLIPPED GRADIENT IS NOT WRITTEN BACK:
                    `p.grad` keeps the unclipped gradient, the norm and the scale are `grad_norm` / `clip_scale`.
    weight_decay    wd >= 0; decoupled False: g += wd * p (torch.optim.Adam(weight_decay=)); True: p *= 1 - lr * wd before the update
                    (torch.optim.AdamW).  decoupled with wd == 0 is a no-op.
    no_decay        parameter-name entries (matches_no_decay: the name ends with the entry, or its last component starts with it; e.g.
                    ("bias", "embedding.weight")) whose parameters are not decayed.
    skip_nonfinite  a step whose gradient norm is inf or NaN leaves parameters and moments untouched and counts in `skipped_steps`.
                    It still advances `steps` (the bias corrections are formed on the host, which does not learn of a skip).
    These five live in param_groups[0] beside lr, so state_dict / load_state_dict carry them.
    Data parallel: dp.train_step calls reducer.all_reduce() before optimizer.step(), and with reducer= the gradient buffer IS the
    all-reduce buffer - the norm is that of the AVERAGED gradient, the same number on every rank, by construction."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, reducer=None, *, max_grad_norm=None, weight_decay=0.0,
                 decoupled=False, no_decay=(), skip_nonfinite=False):
        check_clip_args(max_grad_norm, weight_decay)
        hip = list(model._hip_params())
        if any(p.dtype != torch.float32 or not p.is_cuda for p in hip):
            raise capi.S2VTHipError("FlatAdam needs the fp32 HIP parameters of an S2VT module")
        if reducer is not None:                    # data-parallel: the all-reduce buffer IS the gradient buffer, in its parameter order
            if reducer.model is not model or not reducer.flat.is_cuda:
                raise capi.S2VTHipError("FlatAdam(reducer=...): attach the reducer to this model first (FlatGradAllReducer.attach)")
            params, slices = list(reducer.params), [tuple(s) for s in reducer.slices]
        else:
            params, slices, off = hip, [], 0
            for p in params:
                slices.append((off, off + p.numel()))
                off += p.numel()
        name_of = {id(p): n for n, p in model.named_parameters()}
        self._names, self._slices = [name_of[id(p)] for p in params], slices
        decay_segments(self._names, slices, tuple(no_decay))          # ValueError before anything is moved
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, weight_decay=weight_decay,
                                      decoupled=bool(decoupled), no_decay=tuple(no_decay), skip_nonfinite=bool(skip_nonfinite)))
        n = slices[-1][1]
        dev = params[0].device
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, (lo, hi) in zip(params, slices):
                self.flat_p[lo:hi].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[lo:hi].view_as(p)
        if reducer is not None:
            self.flat_g = reducer.flat
        else:
            self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
            for p, (lo, hi) in zip(params, slices):
                p.grad = self.flat_g[lo:hi].view_as(p)
            functional.set_grad_sink(model, [p.grad for p in hip])
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.n = n
        self.steps = 0
        self._lib = capi.load()
        # the clip record (s2vt_clip_record, 24 bytes, zeroed once) and the norm's fp64 partials
        self._record = torch.zeros(8, dtype=torch.int32, device=dev)
        self._norm_ws = torch.empty(max(1, self._lib.s2vt_grad_norm_workspace_bytes(n) // 8), dtype=torch.float64, device=dev)

    def zero_grad(self, set_to_none=False):
        pass                                       # the backward overwrites every gradient in the flat buffer

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        self.steps += 1
        dev = self.flat_p.device
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        clip, wd = g.get("max_grad_norm"), float(g.get("weight_decay", 0.0))
        skip = bool(g.get("skip_nonfinite", False))
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if clip is None and wd == 0.0 and not skip:
                capi.check(self._lib.s2vt_adam_step(ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_v), self.n, float(g["lr"]),
                                                    float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), self.steps, stream),
                           "s2vt_adam_step")
            else:
                check_clip_args(clip, wd)
                record = None
                if clip is not None or skip:       # weight decay alone needs no norm: the step then runs at scale 1, without a record
                    record = ptr(self._record)
                    capi.check(self._lib.s2vt_grad_norm(ptr(self.flat_g), self.n, 0.0 if clip is None else float(clip), int(skip),
                                                        ptr(self._norm_ws), self._norm_ws.numel() * 8, record, stream), "s2vt_grad_norm")
                ends, flags = decay_segments(self._names, self._slices, tuple(g.get("no_decay", ())))
                capi.check(self._lib.s2vt_adam_step_clipped(ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_v), self.n,
                                                            float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                                            self.steps, wd, int(bool(g.get("decoupled", False))),
                                                            (ctypes.c_int64 * len(ends))(*ends), (ctypes.c_int32 * len(flags))(*flags),
                                                            len(ends), int(skip), record, stream), "s2vt_adam_step_clipped")
        # the kernel wrote through raw pointers: bump the version counters, as an in-place torch op would have (autograd's saved-tensor
        # check and the decode-image cache of functional.py key on them)
        torch.autograd.graph.increment_version(g["params"])

    # what the last step's s2vt_grad_norm left on the device (zeros before the first one, and stale after steps that ran without a
    # norm: neither max_grad_norm nor skip_nonfinite set)
    @property
    def grad_norm(self):
        """fp32 2-norm of the whole (unclipped) gradient of the last step: a 0-dim view of the device record, no synchronisation"""
        return self._record.view(torch.float32)[0]

    @property
    def clip_scale(self):
        """what the last step multiplied every gradient with (1 where the norm was within max_grad_norm): 0-dim device view, no
        synchronisation"""
        return self._record.view(torch.float32)[1]

    @property
    def skipped_steps(self):
        """steps that skip_nonfinite left out so far, as a Python int: READS THE DEVICE RECORD, so it synchronises with the stream"""
        return int(self._record.view(torch.int64)[2].item())

    # (the reference checkpoints the module only, train.py:160-175; a resumable optimizer costs two methods)
    def state_dict(self):
        return {"steps": self.steps, "exp_avg": self.flat_m.detach().clone(), "exp_avg_sq": self.flat_v.detach().clone(),
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}

    @torch.no_grad()
    def load_state_dict(self, state):
        if state["exp_avg"].numel() != self.n or state["exp_avg_sq"].numel() != self.n:
            raise capi.S2VTHipError("FlatAdam.load_state_dict: the state belongs to a model of another size")
        loaded = dict(CLIP_DEFAULTS)               # a state saved before the clipped step existed: the plain step
        loaded.update(state["param_groups"][0])
        check_clip_args(loaded["max_grad_norm"], loaded["weight_decay"])
        decay_segments(self._names, self._slices, tuple(loaded["no_decay"]))
        self.steps = int(state["steps"])
        self.flat_m.copy_(state["exp_avg"])
        self.flat_v.copy_(state["exp_avg_sq"])
        for k, v in loaded.items():
            self.param_groups[0][k] = v
