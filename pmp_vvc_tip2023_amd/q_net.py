"""A whole QT net for training: Model_QBD.Luma_Q_Net / Chroma_Q_Net as ONE torch module whose forward runs on this library's
training calls - stem.stem_of, trunk.trunk_of, qtail.qtail_of and head.head_of - and whose 20 parameters carry the reference's names
and shapes, so that a state_dict goes back and forth between the two (and takes what weights.load_net_weights("Luma_Q", qp) returns).

    qnet = QNet(engine, luma=True).cuda()
    qnet.load_state_dict(reference_net.state_dict())
    q = qnet(x)                                                 # Model_QBD.py:78-98 (luma), :176-196 (chroma): f32[n, 1, 8, 8]
    train_loss.l1_loss_Q(engine, q, qt_label).backward()        # pre_train_Q

    outs = msbd_net.MSBDNet(engine, luma=True).cuda()(x, q)     # train_QBD: the gradient reaches the QT net through x1 = q

x is the block f32[n, 1, 68, 68] (luma) or [n, 3, 34, 34] (chroma).  Luma pools behind resblock_q1, chroma does not; both pool behind
resblock_q2.  No eager torch is left in the forward.  INTEGRATION.md section 12 has the reference's statements next to these.  torch
is imported on use (QNet is built on first access).
"""
from . import head, qtail, stem, trunk
from .torch_call import lazy

# (cin, cout) of resblock_q1 .. q6, as the reference declares them; q1 and q2 are 5x5 in the luma net and 3x3 in the chroma net, the
# others 3x3 in both
BLOCKS = [(32, 64), (64, 64), (64, 32), (128, 32), (32, 32), (32, 8)]


@lazy
def _classes():
    from torch import nn

    from .msbd_net import Block

    class QNet(nn.Module):
        def __init__(self, engine, luma):
            super().__init__()
            self.engine, self.luma = engine, bool(luma)
            self.conv_q1 = nn.Conv2d(1, 32, 9) if luma else nn.Conv2d(3, 32, 5)
            for i, (cin, cout) in enumerate(BLOCKS):
                setattr(self, "resblock_q%d" % (i + 1), Block(cin, cout, 5 if luma and i < 2 else 3))
            self.conv_q2 = nn.Conv2d(8, 1, 3, padding=1)

        def forward(self, x):
            e = self.engine
            x2 = stem.stem_of(e, (self.conv_q1,), x)
            x3 = trunk.trunk_of(e, [self.resblock_q1], x2, pool=self.luma)
            x4 = trunk.trunk_of(e, [self.resblock_q2], x3, pool=True)
            return head.head_of(e, self.conv_q2, qtail.qtail_of(e, self, x4))

    return {"QNet": QNet}


def __getattr__(name):
    if name == "QNet":
        return _classes()[name]
    raise AttributeError(name)
