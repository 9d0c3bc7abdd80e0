"""A QT net's tail - resblock_q3, the multi-scale pool, resblock_q4, resblock_q5 with its 2x2 pool and resblock_q6 - as ONE torch
autograd function over pmp_qtail_forward_device / pmp_qtail_backward_device (include/pmp.h; api_train.cpp, qtail_train.hip).

Drop-in for the reference's forward (Model_QBD.py:83-90, :181-188):

    reference                                                       here
    x5 = self.resblock_q3(x4)                                       x9 = qtail.qtail_of(engine, self, x4)
    x6 = torch.cat([x5, F.interpolate(F.max_pool2d(x5, 2), scale_factor=2), ... 4 ..., ... 8 ...], 1)
    x7 = self.resblock_q4(x6)
    x8 = F.max_pool2d(self.resblock_q5(x7), 2)
    x9 = self.resblock_q6(x8)

    qtail(engine, x4, blocks)                                       the same on bare tensors: blocks = [(w0, w2, wsc or None)] * 4 of
                                                                    q3, q4, q5, q6, each as resblock.residual_block takes them

x4 is f32[n, 64, h, w] with h and w multiples of 16 (the nets: 16 x 16), the result [n, 8, h/2, w/2].  Everything between stays in
the kernels' blocked layout in one opaque uint8 tensor that lives on the autograd context from forward to backward; x6 is rebuilt
from x5 on the way back.  Streams are handled by torch_call.run(); one Engine serves one stream at a time.  torch is imported on use.
"""
from .torch_call import block_weights, lazy, saved_chain_function

# (cout, cin) of q3, q4, q5, q6; every convolution 3x3, the shortcut 1x1 where cin != cout
CHANNELS = ((32, 64), (32, 128), (32, 32), (8, 32))


def shape_of(x4, blocks):
    """(n, h, w); ValueError on anything that is not a QT net's tail."""
    blocks = list(blocks)
    if x4.dim() != 4 or x4.shape[1] != 64:
        raise ValueError("a QT tail reads x4 [n, 64, h, w], not %s" % (tuple(x4.shape),))
    if len(blocks) != 4 or any(len(b) != 3 for b in blocks):
        raise ValueError("a QT tail has the four blocks resblock_q3 .. q6, each (w0, w2, wsc or None)")
    for i, ((cout, cin), (w0, w2, wsc)) in enumerate(zip(CHANNELS, blocks)):
        want = ((cout, cin, 3, 3), (cout, cout, 3, 3), (cout, cin, 1, 1) if cin != cout else None)
        have = tuple(None if t is None else tuple(t.shape) for t in (w0, w2, wsc))
        if have[2] is not None and len(have[2]) == 2:
            have = have[:2] + (have[2] + (1, 1),)
        if have != want:
            raise ValueError("resblock_q%d's weights must be %s, not %s" % (i + 3, want, have))
    return tuple(int(v) for v in (x4.shape[0], x4.shape[2], x4.shape[3]))


@lazy
def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    return saved_chain_function("QtailFn", "(engine, x4, w0, w2, wsc-or-None of q3, q4, q5, q6) -> x9 f32[n, 8, h/2, w/2]", "qtail", 0,
                                lambda x4, ws: shape_of(x4, zip(ws[0::3], ws[1::3], ws[2::3])), lambda s: (s[0], 8, s[1] // 2, s[2] // 2))


def qtail(engine, x4, blocks):
    """resblock_q6(max_pool2d(resblock_q5(resblock_q4(multi-scale pool(resblock_q3(x4)))), 2)) with blocks = the four blocks' weights."""
    blocks = [tuple(b) for b in blocks]
    shape_of(x4, blocks)
    return _function().apply(engine, x4, *[t for b in blocks for t in b])


def qtail_of(engine, net, x4):
    """The same with the weights of net.resblock_q3 .. resblock_q6 (Model_QBD.ResidualBlock modules, or q_net.QNet's)."""
    return qtail(engine, x4, [block_weights(m) for m in (net.resblock_q3, net.resblock_q4, net.resblock_q5, net.resblock_q6)])
