"""torch.optim.Adam on this library: every parameter of a group in ONE launch (pmp_adam_step_device, include/pmp.h TRAINING STEP)
where torch's optimiser runs a train of launches per tensor list.

    opt = optim.Adam(engine, itertools.chain(net_q.parameters(), net_bd.parameters()), lr=args.lr)     # Train_QBD.py:339
    loss.backward(); opt.step()

Adam is a torch.optim.Optimizer: param_groups[i]["lr"] is read at every step (Metrics.adjust_learning_rate writes it), zero_grad()
is torch's, and state_dict() / load_state_dict() interchange with torch.optim.Adam's - per parameter `step` (a float32 scalar on the
host), `exp_avg` and `exp_avg_sq`, and param groups that carry torch's keys.  No weight decay, no amsgrad, no maximize: a state loaded
from a torch optimiser that uses one is refused at the next step.  Parameters without a .grad are skipped, as torch skips them.  One
library call per param group and step number (parameters of a group that have taken different numbers of steps go in one call per
number), through torch_call.run: ordered with torch's current stream, no host synchronisation.  Parameters must be dense contiguous
float32 tensors on the engine's GPU.  torch is imported on use (Adam is built on first access).

THE DIVERGENCE GUARD, opt-in: Adam(..., max_grad_norm=X, skip_nonfinite=True).  With both at their defaults step() is the code path and
the launches above.  Otherwise a step() first runs ONE pmp_grad_guard_device call over every parameter of every group that has a
gradient, in param_groups order - the global norm of the gradients and the count of their NaN and inf elements, in an order the shapes
fix - into a record in device memory that the optimiser owns, and the Adam calls (pmp_adam_step_guarded_device) read that record:
clipping by global norm as torch.nn.utils.clip_grad_norm_(params, X) would (the .grads themselves stay as they are), and, with
skip_nonfinite, NO write at all to any parameter or moment when a gradient element is not finite.  The host is not asked:
    opt.step_taken       a device bool tensor of the last step(), to mask a loop's own sums with torch.where
    opt.guard_record()   the last step's record as a dict (sumsq, norm, nonfinite, coef, action, skip, clip): one D2H read
    opt.guard_state()    the running counters as a dict (steps, skipped, clipped, run, max_run, max_norm): one D2H read
    opt.load_guard_state(d)   puts such a dict back (a resumed run)
A SKIPPED STEP STILL COUNTS AS A STEP: every parameter's `step` advances, so the bias corrections of the next step are those of its
number.  torch's GradScaler leaves the step number alone when it skips; counting keeps the host out of the loop and state_dict()
interchangeable with torch.optim.Adam's.  The counters are not part of state_dict()."""
import math

from .torch_call import P, lazy, run

GUARD_STATE_KEYS = ("steps", "skipped", "clipped", "run", "max_run", "max_norm")


@lazy
def _classes():
    import torch

    class Adam(torch.optim.Optimizer):
        def __init__(self, engine, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, skip_nonfinite=False):
            # torch.optim.Adam's own defaults (and its checks of lr, betas and eps), so that a state_dict of this optimiser loads there
            defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, foreach=False).defaults)
            super().__init__(params, defaults)
            self.engine = engine
            if not (math.isfinite(max_grad_norm) and max_grad_norm >= 0):
                raise ValueError("optim.Adam: max_grad_norm must be finite and >= 0 (0: no clipping)")
            self.max_grad_norm, self.skip_nonfinite = float(max_grad_norm), bool(skip_nonfinite)
            self.guarded = self.max_grad_norm > 0 or self.skip_nonfinite
            self.step_taken = None
            self._guard = None                            # the guard's device tensors: record, counters, scratch
            self._pending_state = None                    # counters loaded before those tensors exist

        def _guard_tensors(self, device, scratch_bytes):
            if self._guard is None:
                self._guard = {"record": torch.zeros(4, dtype=torch.float64, device=device),
                               "state": torch.zeros(6, dtype=torch.int64, device=device), "scratch": None}
                pending, self._pending_state = self._pending_state, None
                if pending is not None:
                    self.load_guard_state(pending)
            g = self._guard
            if g["scratch"] is None or g["scratch"].numel() * 8 < scratch_bytes:
                g["scratch"] = torch.empty(scratch_bytes // 8, dtype=torch.float64, device=device)
            return g

        def guard_record(self):
            """The last step's pmp_guard_record as a dict; None before the first guarded step.  One D2H read."""
            from . import _lib
            if self._guard is None:
                return None
            r = _lib.GuardRecord.from_buffer_copy(self._guard["record"].cpu().numpy().tobytes())
            return {"sumsq": r.sumsq, "norm": r.norm, "nonfinite": r.nonfinite, "coef": r.coef, "action": r.action,
                    "skip": bool(r.action & 1), "clip": bool(r.action & 2)}

        def guard_state(self):
            """The running counters (pmp_guard_state) as a dict; zeros before the first guarded step.  One D2H read."""
            from . import _lib
            if self._guard is None:
                return dict(self._pending_state) if self._pending_state else {**dict.fromkeys(GUARD_STATE_KEYS[:5], 0), "max_norm": 0.0}
            s = _lib.GuardState.from_buffer_copy(self._guard["state"].cpu().numpy().tobytes())
            return {k: getattr(s, k) for k in GUARD_STATE_KEYS}

        def load_guard_state(self, d):
            """Puts guard_state()'s dict back into the counters"""
            import numpy as np
            d = {k: d[k] for k in GUARD_STATE_KEYS}
            if self._guard is None:
                self._pending_state = d                   # the device tensors come with the first guarded step
                return
            words = np.array([int(d[k]) for k in GUARD_STATE_KEYS[:5]] + [0], np.int64)
            words[5:6].view(np.float64)[0] = float(d["max_norm"])
            self._guard["state"].copy_(torch.from_numpy(words))

        def _run_guard(self):
            """The one guard call of a step: every parameter of every group that has a gradient -> {parameter: the gradient tensor
            the guard read, which the Adam calls read too}, and the record's pointer"""
            grads = {}
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None and not p.grad.is_sparse and p.is_cuda:
                        grads[p] = p.grad.to(torch.float32).contiguous()
            if not grads:
                return grads, None
            gs = list(grads.values())
            counts = [t.numel() for t in gs]
            g = self._guard_tensors(gs[0].device, self.engine.grad_guard_scratch_bytes(counts))
            run(self.engine, gs[0].device, lambda: self.engine.grad_guard_device(
                [P(t) for t in gs], counts, P(g["scratch"]), P(g["record"]), P(g["state"]), max_norm=self.max_grad_norm,
                skip_nonfinite=self.skip_nonfinite))
            self.step_taken = (g["record"].view(torch.int32)[7] & 1) == 0
            return grads, P(g["record"])

        @torch.no_grad()
        def step(self, closure=None):
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
            grads, record = self._run_guard() if self.guarded else (None, None)
            for group in self.param_groups:
                if group.get("weight_decay", 0) or group.get("amsgrad") or group.get("maximize"):
                    raise ValueError("optim.Adam: weight_decay, amsgrad and maximize are not supported")
                by_step = {}
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                        raise ValueError("optim.Adam: parameters must be dense contiguous float32 tensors on the GPU")
                    st = self.state[p]
                    if not st:
                        st["step"] = torch.tensor(0.0, dtype=torch.float32)
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["step"] = st["step"].cpu() + 1
                    by_step.setdefault(int(st["step"]), []).append(p)
                for step, ps in by_step.items():
                    gs = [p.grad.to(torch.float32).contiguous() for p in ps] if grads is None else [grads[p] for p in ps]
                    ms, vs = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]
                    tensors = ([P(t) for t in ps], [P(t) for t in gs], [P(t) for t in ms], [P(t) for t in vs], [t.numel() for t in ps], step)
                    hyper = dict(lr=group["lr"], betas=group["betas"], eps=group["eps"])
                    if record is None:
                        run(self.engine, ps[0].device, lambda: self.engine.adam_step_device(*tensors, **hyper))
                    else:
                        run(self.engine, ps[0].device, lambda: self.engine.adam_step_guarded_device(*tensors, record, **hyper))
            return loss

    return {"Adam": Adam}


def __getattr__(name):
    if name == "Adam":
        return _classes()[name]
    raise AttributeError(name)
