"""What the training calls' case tables share (resblock_cases, grad_cases, stem_cases import these names): a float64 result as the
float32 a kernel must produce, bit equality of float32 tensors, and the largest error of a tensor in units of its bound."""
import numpy as np


def as_f32(a):
    """A float64 result as the float32 a kernel must produce: rounded once, zeros positive (a kernel's sums start from +0)."""
    return None if a is None else (np.asarray(a, np.float64) + 0.0).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ratio(got, ref, bound):
    """max |got - ref| / bound over a tensor (0 / 0 = 0; a difference where the bound is 0 is inf)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / bound).max())
