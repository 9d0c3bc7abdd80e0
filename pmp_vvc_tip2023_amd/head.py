"""An MTT net's head - conv_B1..3 (a 3x3 bias convolution, 8 -> 2), the carry out_k[:, 0] += out_{k-1}[:, 0] and the next attention
trunk's input - and the gate product of an attention trunk, each as ONE torch autograd function over pmp_head_*_device /
pmp_gate_*_device (include/pmp.h; api_train.cpp, head_train.hip).

Drop-in for the joints of the reference's forward:

    reference (Model_QBD.py:139-140, :237-238)                      here
    out0 = self.conv_B1(x6)                                         out0, out0q = head.head_of(engine, self.conv_B1, x6, q=x1, up=(2, 1))
    out0q = torch.cat([F.interpolate(x1, scale_factor=2), out0], 1)

    reference (:143, :241)
    xb1 = x5 * x_att0                                               xb1 = head.gate(engine, x5, x_att0)

    reference (:145-147, :243-245)
    out1 = self.conv_B2(xb2)                                        out1, out1q = head.head_of(engine, self.conv_B2, xb2, prev=out0, q=x1,
    out1[:, 0:1] = out1[:, 0:1] + out0[:, 0:1]                                                  up=(4, 2))
    out1q = torch.cat([F.interpolate(x1, scale_factor=4), F.interpolate(out1, scale_factor=2)], 1)

    reference (:152-153, :250-251)
    out2 = self.conv_B3(xb4)                                        out2 = head.head_of(engine, self.conv_B3, xb4, prev=out1)
    out2[:, 0:1] = out2[:, 0:1] + out1[:, 0:1]

    head(engine, x, w, b, prev=None, q=None, up=(0, 0))             the same on bare tensors

x is f32[n, cin, h, w], w [cout, cin, 3, 3], b [cout], prev [n, cout, h, w] (only its channel 0 is read), q [n, 1, up_y h / up_q,
up_y w / up_q].  The result is y [n, cout, h, w], or with up = (up_q, up_y) != (0, 0) the pair (y, att) with att = cat[nearest(q, up_q),
nearest(y, up_y)] built from the CARRIED y, as the reference interpolates out1 after the carry.  Backward returns the gradients of x
(when it requires one), w and b, of prev (channel 0: the effective gradient of y's channel 0, the window sums of att's gradient
included; zero elsewhere) and of q only when q requires one.  Streams are handled by torch_call.run(); torch is imported on use.
"""
from . import torch_call
from .torch_call import P, f32, lazy


def shape_of(x, w, b, prev, q, up):
    """(n, h, w, cin, cout, up_q, up_y); ValueError on anything that is not a head."""
    up = tuple(int(v) for v in up)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[1], 3, 3) or b is None or tuple(b.shape) != (w.shape[0],):
        raise ValueError("a head is a 3x3 convolution with a bias on a 4-d input, not %s on %s" % (tuple(w.shape), tuple(x.shape)))
    n, cin, h, w_ = x.shape
    cout = w.shape[0]
    if up not in ((0, 0), (2, 1), (4, 2)):
        raise ValueError("up must be (0, 0), (2, 1) or (4, 2), not %s" % (up,))
    if prev is not None and tuple(prev.shape) != (n, cout, h, w_):
        raise ValueError("prev must have y's shape %s, not %s" % ((n, cout, h, w_), tuple(prev.shape)))
    if (q is not None) != (up[1] != 0):
        raise ValueError("q is given exactly when up != (0, 0)")
    if q is not None and tuple(q.shape) != (n, 1, up[1] * h // up[0], up[1] * w_ // up[0]):
        raise ValueError("q must be %s, not %s" % ((n, 1, up[1] * h // up[0], up[1] * w_ // up[0]), tuple(q.shape)))
    return (n, h, w_, cin, cout) + up


@lazy
def _head():
    """The head's autograd.Function, built on first use (torch is not imported before)."""
    import torch

    class HeadFn(torch.autograd.Function):
        """(engine, up, x, w, b, prev or None, q or None) -> y, or (y, att) with an attention input"""

        @staticmethod
        def forward(ctx, engine, up, x, w, b, prev, q):
            dev = x.device
            x_, w_, b_, prev_, q_ = (f32(t, dev) for t in (x, w, b, prev, q))
            shape = shape_of(x_, w_, b_, prev_, q_, up)
            n, h, wd, _, cout, _, up_y = shape
            y = torch.empty((n, cout, h, wd), dtype=torch.float32, device=dev)
            att = torch.empty((n, 1 + cout, up_y * h, up_y * wd), dtype=torch.float32, device=dev) if up_y else None
            torch_call.run(engine, dev, lambda: engine.head_forward_device(shape, P(x_), P(w_), P(b_), P(prev_), P(q_), P(y), P(att)))
            ctx.engine, ctx.shape = engine, shape
            ctx.save_for_backward(x_, w_)
            return (y, att) if up_y else y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g_y, g_att=None):
            x, w = ctx.saved_tensors
            n, h, wd, cin, cout, up_q, up_y = ctx.shape
            dev = x.device
            g, ga = f32(g_y, dev), f32(g_att, dev) if up_y else None
            need = ctx.needs_input_grad
            new = lambda *shp: torch.empty(shp, dtype=torch.float32, device=dev)
            g_x = new(n, cin, h, wd) if need[2] else None
            g_w, g_b = torch.empty_like(w), new(cout)
            g_prev = new(n, cout, h, wd) if need[5] else None
            g_q = new(n, 1, up_y * h // up_q, up_y * wd // up_q) if up_y and need[6] else None
            torch_call.run(ctx.engine, dev, lambda: ctx.engine.head_backward_device(
                ctx.shape, P(x), P(w), P(g), P(ga), P(g_x), P(g_w), P(g_b), P(g_q), P(g_prev)))
            # g_w and g_b are required outputs of the C call (one reduction makes both); a frozen head's are dropped here
            return None, None, g_x, g_w if need[3] else None, g_b if need[4] else None, g_prev, g_q

    return HeadFn


@lazy
def _gate():
    """The gate's autograd.Function."""
    import torch

    class GateFn(torch.autograd.Function):
        """(engine, x, a) -> x * a"""

        @staticmethod
        def forward(ctx, engine, x, a):
            if x.shape != a.shape:
                raise ValueError("the gate multiplies tensors of one shape, not %s and %s" % (tuple(x.shape), tuple(a.shape)))
            x_, a_ = f32(x, x.device), f32(a, x.device)
            y = torch.empty_like(x_)
            torch_call.run(engine, x.device, lambda: engine.gate_forward_device(x_.numel(), P(x_), P(a_), P(y)))
            ctx.engine = engine
            ctx.save_for_backward(x_, a_)
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, g_y):
            x, a = ctx.saved_tensors
            g = f32(g_y, x.device)
            g_x, g_a = torch.empty_like(x), torch.empty_like(x)
            torch_call.run(ctx.engine, x.device, lambda: ctx.engine.gate_backward_device(x.numel(), P(x), P(a), P(g), None, P(g_x), P(g_a)))
            # one pass over g_y makes both products (the C call's two required outputs)
            return None, g_x if ctx.needs_input_grad[1] else None, g_a if ctx.needs_input_grad[2] else None

    return GateFn


def head(engine, x, w, b, prev=None, q=None, up=(0, 0)):
    """conv3x3(x, w, padding 1) + b, channel 0 carried from prev; with up = (up_q, up_y) also cat[nearest(q, up_q), nearest(y, up_y)]."""
    shape_of(x, w, b, prev, q, up)
    return _head().apply(engine, tuple(int(v) for v in up), x, w, b, prev, q)


def head_of(engine, module, x, prev=None, q=None, up=(0, 0)):
    """The same with the parameters of net.conv_B1, conv_B2, conv_B3 (or a QT net's conv_q2)."""
    return head(engine, x, module.weight, module.bias, prev, q, up)


def gate(engine, x, a):
    """x * a, an attention trunk's gate (xb1 = x5 * x_att0)."""
    return _gate().apply(engine, x, a)
