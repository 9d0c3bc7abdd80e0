"""Model_QBD.ResidualBlock as a torch autograd function over pmp_resblock_forward_device / pmp_resblock_backward_device
(include/pmp.h; conv_mfma.hip, conv_wgrad.hip).

Drop-in for the body of the reference's ResidualBlock.forward:

    reference (Model_QBD.py:40-44)                  here
    out = self.left(x); out += self.shortcut(x)     return residual_block_of(engine, self, x)
    return F.relu(out)

    residual_block(engine, x, w0, w2, wsc=None)     the same on bare tensors: w0 [cout,cin,k,k], w2 [cout,cout,k,k], wsc [cout,cin,1,1]
                                                    (or [cout,cin]) exactly when cin != cout

Forward saves x, the activation t between the two convolutions and the output; backward hands them to one library call that returns
the gradients of x and of the weights.  Everything runs on torch's current stream, float32 on the exact fp32 MFMA datapath; nothing
synchronises with the host.  One Engine serves ONE stream at a time: its context has a single activation workspace, so calls from
two torch streams that are not ordered with each other need an Engine each.  The gradient of x is skipped when x does not require one (the first block of a net).  torch is imported
on use, so the package stays importable without it.
"""

from . import torch_call
from .torch_call import P, block_weights, f32, lazy


@lazy
def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    import torch

    def shape_of(x, w0):
        n, cin, h, w = x.shape
        return (n, h, w, cin, w0.shape[0], w0.shape[2])

    class ResidualBlockFn(torch.autograd.Function):
        """(engine, x, w0, w2, wsc or None) -> out f32[n,cout,h,w]"""

        @staticmethod
        def forward(ctx, engine, x, w0, w2, wsc):
            x_, w0_, w2_, wsc_ = (f32(t, x.device) for t in (x, w0, w2, wsc))
            shape = shape_of(x_, w0_)
            t = torch.empty((shape[0], shape[4], shape[1], shape[2]), dtype=torch.float32, device=x.device)
            out = torch.empty_like(t)
            torch_call.run(engine, x.device, lambda: engine.resblock_forward_device(shape, P(x_), P(w0_), P(w2_), P(wsc_), P(t), P(out)))
            ctx.engine, ctx.has_sc = engine, wsc is not None
            ctx.save_for_backward(x_, t, out, w0_, w2_, *(() if wsc_ is None else (wsc_,)))
            return out

        @staticmethod
        def backward(ctx, g_out):
            x, t, out, w0, w2 = ctx.saved_tensors[:5]
            wsc = ctx.saved_tensors[5] if ctx.has_sc else None
            g = f32(g_out, g_out.device)
            g_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            g_w0, g_w2 = torch.empty_like(w0), torch.empty_like(w2)
            g_wsc = None if wsc is None else torch.empty_like(wsc)
            torch_call.run(ctx.engine, x.device, lambda: ctx.engine.resblock_backward_device(
                shape_of(x, w0), P(x), P(t), P(out), P(w0), P(w2), P(wsc), P(g), P(g_x), P(g_w0), P(g_w2), P(g_wsc)))
            return None, g_x, g_w0, g_w2, g_wsc

    return ResidualBlockFn


def residual_block(engine, x, w0, w2, wsc=None):
    """relu(conv(relu(conv(x, w0)), w2) + shortcut(x)): shortcut the identity (wsc None, cin == cout) or the 1x1 convolution wsc."""
    return _function().apply(engine, x, w0, w2, wsc)


def residual_block_of(engine, module, x):
    """The same with the weights of a Model_QBD.ResidualBlock: module.left[0], module.left[2] and, if it has one, module.shortcut[0]."""
    return residual_block(engine, x, *block_weights(module))
