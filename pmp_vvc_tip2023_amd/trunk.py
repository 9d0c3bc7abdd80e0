"""A trunk of Model_QBD.ResidualBlocks - an nn.Sequential of them, optionally followed by F.max_pool2d(., 2) - as ONE torch autograd
function over pmp_trunk_forward_device / pmp_trunk_backward_device (include/pmp.h; api_train.cpp, trunk_glue.hip).

Drop-in for a trunk of the reference's forward:

    reference (Model_QBD.py:136-137)                here
    x4 = self.trunk_M1(x3)                          x4 = trunk.trunk_of(engine, self.trunk_M1, x3, pool=True)
    x4 = F.max_pool2d(x4, 2)

    trunk(engine, x, blocks, pool=False)            the same on bare tensors: blocks = [(w0, w2, wsc or None), ...], each as
                                                    resblock.residual_block takes them

Where a chain of resblock.residual_block calls converts between torch's dense layout and the kernels' blocked one around every block,
the trunk converts x once on the way in and y once on the way out (and g_y, g_x on the way back).  Everything between - x, every
block's intermediate t and output - stays blocked in one opaque uint8 tensor that lives on the autograd context from forward to
backward; the pool's backward is recomputed from it (first maximum of a window, torch's rule).  The results are those of the chain,
bit for bit.  Streams are handled by torch_call.run(); one Engine serves one stream at a time.  torch is imported on use.
"""
from . import torch_call
from .torch_call import P, f32, lazy


@lazy
def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    import torch

    class TrunkFn(torch.autograd.Function):
        """(engine, pool, x, w0, w2, wsc-or-None of block 0, of block 1, ...) -> y f32[n, cout_last, h(/2), w(/2)]"""

        @staticmethod
        def forward(ctx, engine, pool, x, *ws):
            x_, ws_ = f32(x, x.device), [f32(t, x.device) for t in ws]
            n, cin, h, w = x_.shape
            shape = (n, h, w, cin, [(w0.shape[0], w0.shape[2]) for w0 in ws_[0::3]], 1 if pool else 0)
            saved = torch.empty(engine.trunk_saved_bytes(shape), dtype=torch.uint8, device=x.device)
            y = torch.empty((n, shape[4][-1][0], h // 2 if pool else h, w // 2 if pool else w), dtype=torch.float32, device=x.device)
            torch_call.run(engine, x.device, lambda: engine.trunk_forward_device(shape, P(x_), [P(t) for t in ws_], P(saved), P(y)))
            ctx.engine, ctx.shape, ctx.saved, ctx.ws = engine, shape, saved, ws_
            return y

        @staticmethod
        def backward(ctx, g_y):
            g = f32(g_y, g_y.device)
            n, h, w, cin = ctx.shape[:4]
            g_x = torch.empty((n, cin, h, w), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
            g_ws = [None if t is None else torch.empty_like(t) for t in ctx.ws]
            torch_call.run(ctx.engine, g.device, lambda: ctx.engine.trunk_backward_device(
                ctx.shape, P(ctx.saved), [P(t) for t in ctx.ws], P(g), P(g_x), [P(t) for t in g_ws]))
            return (None, None, g_x) + tuple(g_ws)

    return TrunkFn


def trunk(engine, x, blocks, pool=False):
    """[max_pool2d(., 2)] of the chain of ResidualBlocks blocks = [(w0, w2, wsc or None), ...] applied to x f32[n, cin, h, w]."""
    flat = []
    for w0, w2, wsc in blocks:
        flat += [w0, w2, wsc]
    return _function().apply(engine, bool(pool), x, *flat)


def trunk_of(engine, sequential, x, pool=False):
    """The same with the weights of an nn.Sequential of Model_QBD.ResidualBlock modules (trunk_M1, trunk_B3, ...)."""
    sc = lambda m: m.shortcut[0].weight if len(m.shortcut) else None
    return trunk(engine, x, [(m.left[0].weight, m.left[2].weight, sc(m)) for m in sequential], pool)
