"""The cases of pmp_adam_step_device (include/pmp.h, TRAINING STEP) and its restatements, for test_adam_cases_cpu.py and
test_gpu_adam.py: the tensor lists, gradients and states, the formula in float64 (adam64), the header's float32 order of operations
in numpy (adam32: what the kernel must compute), torch.optim.Adam(foreach=False) on the CPU in either precision (torch_adam), and the
bound: per tensor, each of param, m and v within four times the distance of torch's CPU float32 run from float64, and never tighter
than one float32 ulp of that tensor's largest magnitude.  The largest magnitude is taken over the values the tensor has from the
start of the run to its end (peaks), not over the final ones alone: every step rounds at the magnitude the tensor has THEN, and a
short tensor that shrinks carries those roundings along.  Seen on one of the 300 one-element tensors, a parameter that goes
-3.4e-3, -2.4e-3, -1.4e-3, -4.0e-4 in three steps: torch's float32 CPU Adam lies 1.54e-10 from float64 on one machine (0.66 ulp of 3.4e-3,
5.3 ulps of 4.0e-4) and 3.8e-11 on another - its bits depend on the CPU it runs on - so torch's run on the first machine would miss a
floor taken at the final value under the bound from the second.  A plain module."""
import math

import numpy as np
import torch

DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
SIZES = (1, 2, 3, 63, 64, 65, 255, 257, 1025, 204800)
SCALES = (1e-3, 1.0, 1e3)


def joint_step_shapes():
    """The 92 parameter shapes of the luma joint step (train_QBD): the QT net's 20 tensors and the MTT net's 72."""
    from pmp_vvc_tip2023_amd import synth, weights as W
    q = [tuple(np.shape(v)) for v in W.load_net_weights("Luma_Q", 22)[0].values()]
    bd = [tuple(np.shape(v)) for v in synth.synth_msbd_weights("Luma", 1).values()]
    assert len(q) == 20 and len(bd) == 72
    return q + bd


def lists():
    """name -> the element counts of one call's tensors"""
    return {"sizes": list(SIZES), "joint": [int(np.prod(s)) for s in joint_step_shapes()], "ones": [1] * 300}


def tensors(counts, seed, scale=1.0, zeros=False, state=False):
    """-> {"param", "grad", "m", "v"}: lists of float32 arrays.  grad = scale * randn (zeros: every third element exactly 0); state:
    m and v as a run in progress leaves them (m of the gradient's size, v of its square), otherwise zero."""
    rng = np.random.default_rng(seed)
    out = {"param": [], "grad": [], "m": [], "v": []}
    for n in counts:
        g = (scale * rng.standard_normal(n)).astype(np.float32)
        if zeros:
            g[::3] = 0.0
        out["param"].append(rng.standard_normal(n).astype(np.float32))
        out["grad"].append(g)
        out["m"].append((0.3 * scale * rng.standard_normal(n)).astype(np.float32) if state else np.zeros(n, np.float32))
        out["v"].append((scale * scale * rng.random(n)).astype(np.float32) if state else np.zeros(n, np.float32))
    return out


def adam64(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """The formula in float64 on float64 copies of the float32 inputs -> (param, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    with np.errstate(all="ignore"):
        p = p - (lr / (1 - b1 ** step)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v


def _fma(a, b, c):
    """a*b + c rounded once to float32: exact in float64 up to the final sum, whose double rounding can differ from a true fma in
    the last bit on rare elements - the CPU test that uses this counts, it does not demand equality."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def adam32(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """include/pmp.h's float32 order of operations -> (param, m, v) float32."""
    f = np.float32
    b1, b2 = betas
    d1, b2f, d2 = f(1.0 - b1), f(b2), f(1.0 - b2)
    neg_af, rf, ef = f(-f(lr / (1.0 - b1 ** step))), f(math.sqrt(1.0 - b2 ** step)), f(eps)
    with np.errstate(all="ignore"):
        m = _fma(d1, g - m, m)
        v = _fma(d2 * g, g, b2f * v)
        p = p + (neg_af * m) / (np.sqrt(v) / rf + ef)
    return p.astype(f), m, v.astype(f)


def torch_adam(t, steps, dtype, first_step=1, grads=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam(foreach=False) on the CPU in `dtype` from tensors() t: `steps` steps, the first being step number first_step
    (the state's step counter starts at first_step - 1), with the gradient t["grad"] at every step or grads[i] at step i.
    -> {"param", "m", "v"} lists of numpy arrays of that dtype, and the optimiser."""
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dtype)) for a in t["param"]]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, foreach=False)
    for p, m, v in zip(ps, t["m"], t["v"]):
        opt.state[p] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": torch.from_numpy(np.array(m)).to(dtype),
                        "exp_avg_sq": torch.from_numpy(np.array(v)).to(dtype)}
    for i in range(steps):
        for p, g in zip(ps, t["grad"] if grads is None else grads[i]):
            p.grad = torch.from_numpy(np.array(g)).to(dtype)
        opt.step()
    return {"param": [p.detach().numpy() for p in ps], "m": [opt.state[p]["exp_avg"].numpy() for p in ps],
            "v": [opt.state[p]["exp_avg_sq"].numpy() for p in ps]}, opt


def run(step_fn, t, steps, first_step=1, **hyper):
    """steps steps of step_fn(p, g, m, v, step, **hyper) (adam64, adam32) per tensor of t -> {"param", "m", "v"}"""
    out = {"param": [], "m": [], "v": []}
    for p, g, m, v in zip(t["param"], t["grad"], t["m"], t["v"]):
        for i in range(steps):
            p, m, v = step_fn(p, g, m, v, first_step + i, **hyper)
        out["param"].append(p); out["m"].append(m); out["v"].append(v)
    return out


def peaks(t, steps, first_step=1, **hyper):
    """-> {"param", "m", "v"}: per tensor, the largest magnitude it has in float64 from its initial values through every step"""
    out = {"param": [], "m": [], "v": []}
    for p, g, m, v in zip(t["param"], t["grad"], t["m"], t["v"]):
        top = [float(np.abs(a).max()) for a in (p, m, v)]
        for i in range(steps):
            p, m, v = adam64(p, g, m, v, first_step + i, **hyper)
            top = [max(a, float(np.abs(b).max())) for a, b in zip(top, (p, m, v))]
        for k, a in zip(("param", "m", "v"), top):
            out[k].append(a)
    return out


def ulp32(x):
    """one float32 ulp at magnitude x > 0 (the smallest normal's for anything below it)"""
    return float(np.spacing(np.float32(max(float(x), float(np.finfo(np.float32).tiny)))))


def check_bound(what, got, t32, r64, peak):
    """Per tensor and per key of param, m, v: max |got - r64| <= max(4 * max |t32 - r64|, one float32 ulp of peak), peak = peaks() of
    the run.  -> the worst ratio of a distance to its bound, for the record."""
    worst = 0.0
    for key in ("param", "m", "v"):
        for i, (a, b, c) in enumerate(zip(got[key], t32[key], r64[key])):
            a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
            assert np.isfinite(c).all() and a.shape == c.shape, (what, key, i)
            assert peak[key][i] >= np.abs(c).max()
            bound = max(4 * float(np.abs(b - c).max()), ulp32(peak[key][i]))
            d = float(np.abs(a - c).max())
            assert d <= bound, (what, key, i, a.size, d, bound)
            worst = max(worst, d / bound)
    return worst


def nonfinite_case():
    """One tensor of 9 whose gradient holds NaN, +inf and -inf between finite values, from a finite state."""
    t = tensors([9], 41, state=True)
    t["grad"][0][[1, 4, 7]] = [np.nan, np.inf, -np.inf]
    return t


def pattern(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, element by element"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))
