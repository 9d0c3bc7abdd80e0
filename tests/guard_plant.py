"""What test_gpu_train_qbd_guard.py shares with the rank processes it starts: Trainer.accumulate wrapped so that ONE NaN lands in one
parameter's .grad behind the backward pass of one step, on one rank (None: every rank), and so that the step's values are kept.

    python tests/guard_plant.py STEP RANK [train_qbd's arguments]          (RANK -1: every rank)

runs train_qbd.main under that wrap: as a one-rank job, as a rank under a launcher's environment, or, with --gpus N and no launcher,
as the parent that starts N copies of THIS command in train_qbd's own way (parallel.spawn_ranks).  Not a test module."""
import os
import sys


def plant(monkeypatch_setattr, step, rank=None, kept=None):
    """Wraps train_qbd.Trainer.accumulate through monkeypatch_setattr(object, name, value): the `step`-th call (from 1) of a process
    plants NaN in element 5 of the first parameter that has a gradient, if the process is `rank` of its group (None: whatever it is).
    kept: a list that receives every call's values (device tensors, before the guard masks them)."""
    from pmp_vvc_tip2023_amd import train_qbd
    inner = train_qbd.Trainer.accumulate
    calls = [0]

    def accumulate(self, batch, n=None):
        values = inner(self, batch, n)
        calls[0] += 1
        mine = rank is None or int(os.environ.get("RANK", "0")) == rank
        if calls[0] == step and mine:
            p = next(p for net in self.nets.values() for p in net.parameters() if p.grad is not None)
            p.grad.view(-1)[5] = float("nan")
        if kept is not None:
            kept.append(values.clone())
        return values
    monkeypatch_setattr(train_qbd.Trainer, "accumulate", accumulate)


def main(argv):
    from pmp_vvc_tip2023_amd import parallel, train_qbd
    step, rank, rest = int(argv[0]), int(argv[1]), argv[2:]
    plant(setattr, step, None if rank < 0 else rank)

    def launch_ranks(n, args):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        rc, _ = parallel.spawn_ranks([sys.executable, os.path.abspath(__file__), str(step), str(rank)] + list(args), n,
                                     env_extra={"PYTHONPATH": root + os.pathsep + os.environ.get("PYTHONPATH", "")})
        return rc
    train_qbd.launch_ranks = launch_ranks
    return train_qbd.main(rest)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
