"""A net's stem - its first layer: ZeroPad2d, a bias convolution (the MTT nets: three, concatenated) and a ReLU - as ONE torch autograd
function over pmp_stem_forward_device / pmp_stem_backward_device (include/pmp.h; api_train.cpp, stem_train.hip).

Drop-in for the first statements of the reference's forward:

    reference (Model_QBD.py:79-80, :177-178)        here
    x1 = self.padding_rb(x)                         x2 = stem.stem_of(engine, (self.conv_q1,), x)
    x2 = F.relu(self.conv_q1(x1))

    reference (Model_QBD.py:132-135, :230-233)      here
    x3_1 = F.relu(self.conv_b1_1(self.padding_rb(x2)))
    x3_2 = F.relu(self.conv_b1_2(self.padding_r(x2)))      x3 = stem.stem_of(engine, (self.conv_b1_1, self.conv_b1_2, self.conv_b1_3), x2)
    x3_3 = F.relu(self.conv_b1_3(self.padding_b(x2)))
    x3 = torch.cat([x3_1, x3_2, x3_3], 1)

    stem(engine, x, convs)                          the same on bare tensors: convs = [(w, b)] with w [32, cin, k, k], or three pairs
                                                    with w [16, cin, k, k], [8, cin, k//2 + 1, k] and [8, cin, k, k//2 + 1]

x is f32[n, cin, h + k//2, w + k//2] - the nets' own input, before their right and bottom padding, which the kernels fold into index
arithmetic - and the result f32[n, 32, h, w].  k (5 or 9) and the form are read from the weights' shapes; anything that is not a stem
raises ValueError.  Backward masks the upstream gradient where the output is zero (torch's rule for relu) and returns the gradients of
every weight and bias, and of x only when x requires one (the MTT net's qt channel in train_QBD).  The modules keep their parameters:
.grad arrives through autograd.  Streams are handled by torch_call.run(); torch is imported on use.
"""
from . import torch_call
from .torch_call import P, f32, lazy


def shape_of(x, convs):
    """(n, h, w, cin, k, split) of x and convs = [(w, b)] or three pairs; ValueError on anything that is not a stem."""
    convs = list(convs)
    if len(convs) not in (1, 3) or x.dim() != 4:
        raise ValueError("a stem has one convolution or three, and a 4-d input")
    n, cin, hx, wx = x.shape
    k = convs[0][0].shape[-1] if convs[0][0].dim() == 4 else 0
    p = k // 2
    want = [(32, cin, k, k)] if len(convs) == 1 else [(16, cin, k, k), (8, cin, p + 1, k), (8, cin, k, p + 1)]
    if k not in (5, 9) or not 1 <= cin <= 4:
        raise ValueError("a stem has 5x5 or 9x9 taps and 1..4 input channels, not %s" % (tuple(convs[0][0].shape),))
    for (w, b), shp in zip(convs, want):
        if tuple(w.shape) != shp or b is None or tuple(b.shape) != shp[:1]:
            raise ValueError("stem weights %s with bias %s where %s with bias %s belong" %
                             (tuple(w.shape), None if b is None else tuple(b.shape), shp, shp[:1]))
    h, w_ = hx - p, wx - p
    if h < 16 or w_ < 16 or h % 16 or w_ % 16:
        raise ValueError("x must be (h + %d, w + %d) with h and w multiples of 16, not %s" % (p, p, (hx, wx)))
    return (n, h, w_, cin, k, 1 if len(convs) == 3 else 0)


@lazy
def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    import torch

    class StemFn(torch.autograd.Function):
        """(engine, x, w, b [, w, b, w, b]) -> y f32[n, 32, h, w]"""

        @staticmethod
        def forward(ctx, engine, x, *wb):
            x_, ws, bs = f32(x, x.device), [f32(t, x.device) for t in wb[0::2]], [f32(t, x.device) for t in wb[1::2]]
            shape = shape_of(x_, list(zip(ws, bs)))
            n, h, w = shape[:3]
            y = torch.empty((n, 32, h, w), dtype=torch.float32, device=x.device)
            torch_call.run(engine, x.device, lambda: engine.stem_forward_device(shape, P(x_), [P(t) for t in ws], [P(t) for t in bs], P(y)))
            ctx.engine, ctx.shape, ctx.nconv = engine, shape, len(ws)
            ctx.save_for_backward(x_, y, *ws)
            return y

        @staticmethod
        def backward(ctx, g_y):
            x, y = ctx.saved_tensors[:2]
            ws = ctx.saved_tensors[2:]
            g = f32(g_y, g_y.device)
            g_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            g_ws = [torch.empty_like(t) for t in ws]
            g_bs = [torch.empty(t.shape[0], dtype=torch.float32, device=t.device) for t in ws]
            torch_call.run(ctx.engine, x.device, lambda: ctx.engine.stem_backward_device(
                ctx.shape, P(x), P(y), [P(t) for t in ws], P(g), P(g_x), [P(t) for t in g_ws], [P(t) for t in g_bs]))
            out = [None, g_x]
            for gw, gb in zip(g_ws, g_bs):
                out += [gw, gb]
            return tuple(out)

    return StemFn


def stem(engine, x, convs):
    """relu(cat[conv(pad(x), w) + b for (w, b) in convs]) with the nets' right / bottom zero padding: convs = [(w, b)] or three pairs."""
    convs = list(convs)
    shape_of(x, convs)
    flat = []
    for w, b in convs:
        flat += [w, b]
    return _function().apply(engine, x, *flat)


def stem_of(engine, modules, x):
    """The same with the parameters of (net.conv_q1,) or (net.conv_b1_1, net.conv_b1_2, net.conv_b1_3)."""
    return stem(engine, x, [(m.weight, m.bias) for m in modules])
