"""The torch glue shared by every training wrapper (resblock.py, trunk.py, qtail.py, stem.py, head.py, train_loss.py): the stream a library call runs
on, tensors as the library takes them, a ResidualBlock module's weights, the autograd.Function built on first use, and the one of a
chain of blocks whose activations stay in a saved tensor (trunk.py, qtail.py).  torch is imported on use, so the package stays
importable without it."""

_SIDE = {}          # device -> the side stream that stands in for the legacy default stream


def run(engine, dev, call):
    """call() with the engine on torch's current stream, and back on the stream it was on afterwards.  The legacy default stream
    has no handle the library could adopt (a null stream selects the context's OWN non-blocking stream, which torch's work is not
    ordered with): the call then runs on a side stream fenced against the current one on both ends, still without a host
    synchronisation.  Shared by every training wrapper.

    Two calls from two torch streams on one engine are safe: every set_stream here that changes the stream of a context with work in
    flight makes the new stream wait, on the device, for what the context enqueued on the old one (include/pmp.h, pmp_set_stream), so
    the context's workspace and scratch buffers are never used by two calls at once.  The tensors handed to call() are the caller's:
    torch's stream rules order them, as for any op on the current stream."""
    import torch
    cur = torch.cuda.current_stream(dev)
    before = engine.stream_ptr
    try:
        if cur.cuda_stream:
            engine.set_stream(cur.cuda_stream)
            call()
            return
        s = _SIDE.setdefault(dev, torch.cuda.Stream(dev))
        s.wait_stream(cur)
        engine.set_stream(s.cuda_stream)
        call()
        cur.wait_stream(s)
    finally:
        engine.set_stream(before)


def P(t):
    """The device pointer of a tensor; None stays None (an absent optional tensor)."""
    return None if t is None else t.data_ptr()


def f32(t, device):
    """t as the library reads it: detached, float32, contiguous, on device; None stays None."""
    import torch
    return None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()


def block_weights(m):
    """(w0, w2, wsc or None) of a Model_QBD.ResidualBlock module: left[0], left[2] and, if it has one, shortcut[0]."""
    return m.left[0].weight, m.left[2].weight, m.shortcut[0].weight if len(m.shortcut) else None


def saved_chain_function(name, doc, calls, extra, shape_of, y_shape):
    """-> the autograd.Function `name` of a chain of ResidualBlocks whose activations stay in one opaque uint8 tensor: (engine, `extra`
    arguments that are no tensors, x, w0, w2, wsc-or-None of every block) -> y, over the engine's <calls>_saved_bytes, _forward_device
    and _backward_device (calls: "trunk" or "qtail").  shape_of(x, ws, *the extra arguments) -> the calls' shape, y_shape(shape) -> y's.
    Backward skips x's gradient when x requires none, and is differentiable once: its results are fresh tensors the library wrote."""
    import torch

    def fwd(ctx, engine, *args):
        x, ws = args[extra], args[extra + 1:]
        x_, ws_ = f32(x, x.device), [f32(t, x.device) for t in ws]
        shape = shape_of(x_, ws_, *args[:extra])
        saved = torch.empty(getattr(engine, calls + "_saved_bytes")(shape), dtype=torch.uint8, device=x.device)
        y = torch.empty(y_shape(shape), dtype=torch.float32, device=x.device)
        run(engine, x.device, lambda: getattr(engine, calls + "_forward_device")(shape, P(x_), [P(t) for t in ws_], P(saved), P(y)))
        ctx.engine, ctx.shape, ctx.saved, ctx.ws, ctx.x_shape = engine, shape, saved, ws_, x_.shape
        return y

    def bwd(ctx, g_y):
        g = f32(g_y, g_y.device)
        g_x = torch.empty(ctx.x_shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1 + extra] else None
        g_ws = [None if t is None else torch.empty_like(t) for t in ctx.ws]
        run(ctx.engine, g.device, lambda: getattr(ctx.engine, calls + "_backward_device")(
            ctx.shape, P(ctx.saved), [P(t) for t in ctx.ws], P(g), P(g_x), [P(t) for t in g_ws]))
        return (None,) * (1 + extra) + (g_x,) + tuple(g_ws)

    return type(name, (torch.autograd.Function,), {"__doc__": doc, "forward": staticmethod(fwd),
                                                   "backward": staticmethod(torch.autograd.function.once_differentiable(bwd))})


def lazy(build):
    """-> a function that returns build()'s result, built on the first call: a module's autograd.Function, so that torch is not
    imported before it is used."""
    made = []

    def get():
        if not made:
            made.append(build())
        return made[0]
    return get
