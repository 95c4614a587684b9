"""``UNet`` of the reference's ``network/dtc.py`` (dual-task consistency, Luo et al. 2021) on gfx950 kernels: the stock U-Net with two
1x1 heads on the last decoder feature -- ``decoder.fc1 = conv1x1 + Tanh`` regresses a level-set function per class, ``decoder.fc2``
gives the segmentation logits.  Constructor signature, attribute names and ``state_dict`` keys / shapes are the reference's
(``decoder.fc1.0.weight``, ``decoder.fc2.weight``), so its checkpoints load unchanged.  ``forward(x) -> (tanh_out, logits)``, both NCHW
with channels_last memory.  The two heads are two launches of the 1x1 kernel on the same feature tensor.
"""
import torch.nn as nn

from .. import ops
from .blocks import BasicBlock, Encoder, UpSampleAndConcat, conv1x1, init_conv_kaiming


class Tanh(nn.Module):
    def forward(self, x):
        return ops.tanh(x)


class Decoder(nn.Module):
    def __init__(self, out_ch, block, width=32, norm="batch", act="lrelu", **kwargs):
        super().__init__()
        for lvl, m in zip((4, 3, 2, 1), (8, 4, 2, 1)):
            setattr(self, f"up{lvl}", UpSampleAndConcat(2 * m * width, m * width))
            setattr(self, f"layer{lvl}", block(2 * m * width, m * width, norm, act, **kwargs))
        self.fc1 = nn.Sequential(conv1x1(width, out_ch), Tanh())
        self.fc2 = conv1x1(width, out_ch)

    def forward(self, x, skips):
        for lvl in (4, 3, 2, 1):
            x = getattr(self, f"layer{lvl}")(getattr(self, f"up{lvl}")(x, skips[lvl - 1]))
        return self.fc1(x), self.fc2(x)


class UNet(nn.Module):
    def __init__(self, in_ch, out_ch, base_width=64, norm_type="batch", act_type="relu"):
        super().__init__()
        self.encoder = Encoder(in_ch, BasicBlock, base_width, norm=norm_type, act=act_type)
        self.decoder = Decoder(out_ch, BasicBlock, base_width, norm=norm_type, act=act_type)
        init_conv_kaiming(self, "relu" if act_type == "relu" else "leaky_relu")

    def forward(self, x):
        x, skips = self.encoder(x)
        return self.decoder(x, skips)
