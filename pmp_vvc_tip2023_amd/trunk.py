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
from .torch_call import block_weights, lazy, saved_chain_function


@lazy
def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    def _shape_of(x, ws, pool):
        n, cin, h, w = x.shape
        return (n, h, w, cin, [(w0.shape[0], w0.shape[2]) for w0 in ws[0::3]], 1 if pool else 0)

    def _y_shape(shape):
        n, h, w, _, blocks, pool = shape
        return (n, blocks[-1][0], h // 2 if pool else h, w // 2 if pool else w)

    return saved_chain_function("TrunkFn", "(engine, pool, x, w0, w2, wsc-or-None of block 0, of block 1, ...) -> y f32[n, cout_last, h(/2), w(/2)]",
                                "trunk", 1, _shape_of, _y_shape)


def trunk(engine, x, blocks, pool=False):
    """[max_pool2d(., 2)] of the chain of ResidualBlocks blocks = [(w0, w2, wsc or None), ...] applied to x f32[n, cin, h, w]."""
    flat = []
    for w0, w2, wsc in blocks:
        flat += [w0, w2, wsc]
    return _function().apply(engine, bool(pool), x, *flat)


def trunk_of(engine, sequential, x, pool=False):
    """The same with the weights of an nn.Sequential of Model_QBD.ResidualBlock modules (trunk_M1, trunk_B3, ...)."""
    return trunk(engine, x, [block_weights(m) for m in sequential], pool)
