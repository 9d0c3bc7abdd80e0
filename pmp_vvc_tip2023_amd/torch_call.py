"""The torch glue shared by every training wrapper (resblock.py, trunk.py, stem.py): the stream a library call runs on, tensors as
the library takes them, and the autograd.Function built on first use.  torch is imported on use, so the package stays importable
without it."""

_SIDE = {}          # device -> the side stream that stands in for the legacy default stream


def run(engine, dev, call):
    """call() with the engine on torch's current stream, and back on the stream it was on afterwards.  The legacy default stream
    has no handle the library could adopt (a null stream selects the context's OWN non-blocking stream, which torch's work is not
    ordered with): the call then runs on a side stream fenced against the current one on both ends, still without a host
    synchronisation.  Shared by every training wrapper."""
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


def lazy(build):
    """-> a function that returns build()'s result, built on the first call: a module's autograd.Function, so that torch is not
    imported before it is used."""
    made = []

    def get():
        if not made:
            made.append(build())
        return made[0]
    return get
