"""A whole MTT net for training: Model_QBD.Luma_MSBD_Net / Chroma_MSBD_Net as ONE torch module whose forward runs on this library's
training calls - stem.stem_of, trunk.trunk_of, head.head_of and head.gate - and whose parameters carry the reference's names and
shapes, so that a state_dict goes back and forth between the two (and through weights.py's .pkl reader).

    net = MSBDNet(engine, luma=True).cuda()
    net.load_state_dict(reference_net.state_dict())             # or {name: tensor} of a *_BD_*.pkl file
    out0, out1, out2 = net(x, x1)                               # Model_QBD.py:127-155 (luma), :225-253 (chroma)
    train_loss.loss_func_MSBD(engine, out0, out1, out2, msbt, msdire, isLuma, qp).backward()

x is the block f32[n, 1, 68, 68] (luma) or [n, 3, 34, 34] (chroma), x1 the QT depth map f32[n, 1, 8, 8].  The only eager torch
left is the building of the stem's input - interpolate x1, pad it on the left and top, concatenate: one channel of input data, no
weights.  Luma pools behind trunk_M1, chroma does not; both pool behind trunk_M2 and trunk_B3.  INTEGRATION.md section 11 has the
reference's statements next to these.  torch is imported on use (MSBDNet is built on first access).
"""
from . import head, stem, trunk
from .torch_call import lazy

# (cin, cout, k) of every block, as the reference declares its trunks
TRUNKS = {
    "trunk_M1": [(32, 64, 5)] + [(64, 64, 3)] * 5,
    "trunk_M2": [(64, 64, 3)] * 4,
    "trunk_B1": [(64, 32, 3), (32, 16, 3), (16, 8, 3)],
    "trunk_B2": [(64, 32, 3), (32, 16, 3), (16, 8, 3)],
    "trunk_B3": [(64, 32, 3), (32, 16, 3), (16, 8, 3)],
    "trunk_Att1": [(3, 32, 3), (32, 64, 3)],
    "trunk_Att2": [(3, 32, 3), (32, 64, 3)],
}


@lazy
def _classes():
    import torch
    import torch.nn.functional as F
    from torch import nn

    class Block(nn.Module):
        """The parameters of a ResidualBlock under the reference's names: left.0, left.2 and, where cin != cout, shortcut.0."""

        def __init__(self, cin, cout, k):
            super().__init__()
            self.left = nn.Sequential(nn.Conv2d(cin, cout, k, padding=k // 2, bias=False), nn.ReLU(inplace=True),
                                      nn.Conv2d(cout, cout, k, padding=k // 2, bias=False))
            self.shortcut = nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False)) if cin != cout else nn.Sequential()

    class MSBDNet(nn.Module):
        def __init__(self, engine, luma):
            super().__init__()
            self.engine, self.luma = engine, bool(luma)
            cin, k = (2, 9) if luma else (4, 5)
            p = k // 2
            self.conv_b1_1 = nn.Conv2d(cin, 16, (k, k))
            self.conv_b1_2 = nn.Conv2d(cin, 8, (p + 1, k))
            self.conv_b1_3 = nn.Conv2d(cin, 8, (k, p + 1))
            for name, blocks in TRUNKS.items():
                setattr(self, name, nn.Sequential(*[Block(*b) for b in blocks]))
            for name in ("conv_B1", "conv_B2", "conv_B3"):
                setattr(self, name, nn.Conv2d(8, 2, 3, padding=1))

        def forward(self, x, x1):
            e, p = self.engine, self.conv_b1_1.weight.shape[-1] // 2
            x1_1 = F.pad(F.interpolate(x1, scale_factor=2 * p), (p, 0, p, 0))
            x3 = stem.stem_of(e, (self.conv_b1_1, self.conv_b1_2, self.conv_b1_3), torch.cat([x, x1_1], 1))
            x4 = trunk.trunk_of(e, self.trunk_M1, x3, pool=self.luma)
            x5 = trunk.trunk_of(e, self.trunk_M2, x4, pool=True)
            x6 = trunk.trunk_of(e, self.trunk_B1, x5)
            out0, out0q = head.head_of(e, self.conv_B1, x6, q=x1, up=(2, 1))
            xb1 = head.gate(e, x5, trunk.trunk_of(e, self.trunk_Att1, out0q))
            xb2 = trunk.trunk_of(e, self.trunk_B2, xb1)
            out1, out1q = head.head_of(e, self.conv_B2, xb2, prev=out0, q=x1, up=(4, 2))
            xb3 = head.gate(e, x4, trunk.trunk_of(e, self.trunk_Att2, out1q))
            xb4 = trunk.trunk_of(e, self.trunk_B3, xb3, pool=True)
            out2 = head.head_of(e, self.conv_B3, xb4, prev=out1)
            return out0, out1, out2

    return {"MSBDNet": MSBDNet, "Block": Block}


def __getattr__(name):
    if name in ("MSBDNet", "Block"):
        return _classes()[name]
    raise AttributeError(name)
