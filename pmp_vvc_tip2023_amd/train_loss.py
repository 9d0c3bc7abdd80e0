"""Train_QBD's losses as torch autograd functions over pmp_train_loss_device (include/pmp.h; logitstats.hip).

Drop-in for the loss calls of the reference's training loops:

    reference (Train_QBD.py)                                        here
    loss_func_QBD(qt_out, bd0, bd1, bd2, ql, bl, dl, isLuma)        loss_func_QBD(engine, qt_out, bd0, bd1, bd2, qt8, msbt, msdire, isLuma, qp)
    loss_func_MSBD(bd0, bd1, bd2, bl, dl, isLuma)                   loss_func_MSBD(engine, bd0, bd1, bd2, msbt, msdire, isLuma, qp)
    L1_Loss(qt_out, ql)                            (pre_train_Q)    l1_loss_Q(engine, qt_out, qt8)

The nets' own head tensors go in (qt_out [n,1,8,8]; bd_outK [n,2,16,16]: channel 0 the BT depth, channel 1 the direction) and the labels
in the dtypes of the label FILES (qt8 uint8 RAW qtDepth, msbt uint8, msdire int8): the kernel converts them as the reference's loader
does.  One launch gives the loss and the gradients of all heads; backward() hands them out, scaled by grad_output.  Regrouping heads
into the library's layouts and gradients back is done with torch ops.  The loss comes back as a 0-dim float32 tensor on the device;
nothing synchronises with the host.  torch is imported on use, so the package stays importable without it.
"""
from . import _lib
from .torch_call import P, run

_FUNCTION = None


def _function():
    """The autograd.Function, built on first use (torch is not imported before)."""
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch

    class TrainLoss(torch.autograd.Function):
        """(engine, comp, qp, params, qt, bt, dire, qt8, msbt, msdire) -> (loss f32[], terms f64[13]); qt f32[n,8,8], bt / dire
        f32[n,3,16,16] contiguous or None as the three forms of pmp_train_loss allow."""

        @staticmethod
        def forward(ctx, engine, comp, qp, params, qt, bt, dire, qt8, msbt, msdire):
            from .engine import loss_params
            ref = qt if qt is not None else bt
            n = ref.shape[0]
            dev = ref.device
            c = lambda t, dt: None if t is None else t.detach().to(device=dev, dtype=dt).contiguous()
            qt_, bt_, dire_ = c(qt, torch.float32), c(bt, torch.float32), c(dire, torch.float32)
            qt8_, msbt_, msdire_ = c(qt8, torch.uint8), c(msbt, torch.uint8), c(msdire, torch.int8)
            want = any(t is not None and t.requires_grad for t in (qt, bt, dire))
            out = torch.empty(_lib.PMP_LOSS_NTERMS + 1, dtype=torch.float64, device=dev)      # thirteen sums | loss
            g_qt = torch.empty_like(qt_) if want and qt_ is not None else None
            g_bt = torch.empty_like(bt_) if want and bt_ is not None else None
            g_dire = torch.empty_like(dire_) if want and dire_ is not None else None
            # ordered with torch's work on the legacy default stream too: a bare set_stream(0) would select the context's own stream
            run(engine, dev, lambda: engine.train_loss_device(
                comp, qp, P(qt_), P(bt_), P(dire_), P(qt8_), P(msbt_), P(msdire_), n, out.data_ptr(),
                out.data_ptr() + 8 * _lib.PMP_LOSS_NTERMS, P(g_qt), P(g_bt), P(g_dire), params=loss_params(params)))
            ctx.grads = (g_qt, g_bt, g_dire)
            terms = out[:_lib.PMP_LOSS_NTERMS]
            ctx.mark_non_differentiable(terms)
            return out[_lib.PMP_LOSS_NTERMS].to(torch.float32), terms

        @staticmethod
        def backward(ctx, grad_loss, _grad_terms):
            s = lambda g: None if g is None else g * grad_loss.to(g.dtype)
            g_qt, g_bt, g_dire = ctx.grads
            return (None, None, None, None, s(g_qt), s(g_bt), s(g_dire), None, None, None)

    _FUNCTION = TrainLoss
    return TrainLoss


def _comp(isLuma):
    return "Luma" if isLuma else "Chroma"


def _heads(bd_out0, bd_out1, bd_out2):
    """Three heads [n,2,16,16] -> bt, dire [n,3,16,16] (layer k = bd_outK[:, 0] / [:, 1]); autograd splits the gradients back."""
    import torch
    bd = torch.stack((bd_out0, bd_out1, bd_out2), dim=1)              # [n,3,2,16,16]
    return bd[:, :, 0].contiguous(), bd[:, :, 1].contiguous()


def loss_func_QBD(engine, qt_out, bd_out0, bd_out1, bd_out2, qt8, msbt, msdire, isLuma, qp, params=None, return_terms=False):
    """Train_QBD.loss_func_QBD (Train_QBD.py:68-90) with args.qp = qp and the ten args.lamb* = params (None: the defaults)."""
    bt, dire = _heads(bd_out0, bd_out1, bd_out2)
    loss, terms = _function().apply(engine, _comp(isLuma), int(qp), params, qt_out.reshape(-1, 8, 8), bt, dire, qt8, msbt, msdire)
    return (loss, terms) if return_terms else loss


def loss_func_MSBD(engine, bd_out0, bd_out1, bd_out2, msbt, msdire, isLuma, qp, params=None, return_terms=False):
    """Train_QBD.loss_func_MSBD (Train_QBD.py:44-66).  With return_terms also the thirteen sums f64[13] on the device: terms[1..6] /
    (256 n) are the six L1 losses pre_train_BD prints (:246-251)."""
    bt, dire = _heads(bd_out0, bd_out1, bd_out2)
    loss, terms = _function().apply(engine, _comp(isLuma), int(qp), params, None, bt, dire, None, msbt, msdire)
    return (loss, terms) if return_terms else loss


def l1_loss_Q(engine, qt_out, qt8, return_terms=False):
    """pre_train_Q's L1_Loss(qt_out_batch, qt_label_batch) (Train_QBD.py:161) against the RAW uint8 qtDepth labels."""
    loss, terms = _function().apply(engine, "Luma", 22, {"lambq": 1.0}, qt_out.reshape(-1, 8, 8), None, None, qt8, None, None)
    return (loss, terms) if return_terms else loss
