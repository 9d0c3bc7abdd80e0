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
float32 tensors on the engine's GPU.  torch is imported on use (Adam is built on first access)."""
from .torch_call import P, lazy, run


@lazy
def _classes():
    import torch

    class Adam(torch.optim.Optimizer):
        def __init__(self, engine, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
            # torch.optim.Adam's own defaults (and its checks of lr, betas and eps), so that a state_dict of this optimiser loads there
            defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, foreach=False).defaults)
            super().__init__(params, defaults)
            self.engine = engine

        @torch.no_grad()
        def step(self, closure=None):
            loss = None
            if closure is not None:
                with torch.enable_grad():
                    loss = closure()
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
                    gs = [p.grad.to(torch.float32).contiguous() for p in ps]
                    ms, vs = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]
                    run(self.engine, ps[0].device, lambda: self.engine.adam_step_device(
                        [P(t) for t in ps], [P(t) for t in gs], [P(t) for t in ms], [P(t) for t in vs], [t.numel() for t in ps], step,
                        lr=group["lr"], betas=group["betas"], eps=group["eps"]))
            return loss

    return {"Adam": Adam}


def __getattr__(name):
    if name == "Adam":
        return _classes()[name]
    raise AttributeError(name)
