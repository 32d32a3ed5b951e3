"""The U-Net blocks the CSS network is assembled from (networks/unet_parts.py of the reference): plain torch layers with the reference's
attribute names, so that a reference state_dict loads by name."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv_bn_relu(cin, cout):
    return [nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]


class double_conv(nn.Module):
    """two 3x3 conv + BatchNorm + ReLU stages; parameters live under `conv.{0,1,3,4}`"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = nn.Sequential(*(_conv_bn_relu(in_ch, out_ch) + _conv_bn_relu(out_ch, out_ch)))

    def forward(self, x):
        return self.conv(x)


class inconv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = double_conv(in_ch, out_ch)

    def forward(self, x):
        return self.conv(x)


class down(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.mpconv = nn.Sequential(nn.MaxPool2d(2), double_conv(in_ch, out_ch))

    def forward(self, x):
        return self.mpconv(x)


class up(nn.Module):
    """x2 upsampling of `low` (bilinear with aligned corners, or a transposed convolution), `skip` padded to its size and concatenated in
    front of it (add_shortcut) or ignored, then a double_conv"""

    def __init__(self, in_ch, out_ch, bilinear=True, add_shortcut=True):
        super().__init__()
        self.add_shortcut = add_shortcut
        if bilinear:
            self.up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)
        else:
            self.up = nn.ConvTranspose2d(in_ch // 2, in_ch // 2, 2, stride=2)
        self.conv = double_conv(in_ch, out_ch)

    def forward(self, low, skip):
        low = self.up(low)
        if self.add_shortcut:
            # the reference pads the LAST dimension by the height difference and the one before by the width difference; both are zero
            # for the network's power-of-two crops, and the order is kept for other sizes
            dh, dw = low.size(2) - skip.size(2), low.size(3) - skip.size(3)
            skip = F.pad(skip, (dh // 2, int(dh / 2), dw // 2, int(dw / 2)))
            low = torch.cat([skip, low], dim=1)
        return self.conv(low)


class outconv(nn.Module):
    """1x1 convolution, optionally followed by a sigmoid; the parameters live under `conv` (or `conv.0` with the sigmoid)"""

    def __init__(self, in_ch, out_ch, sigmoid=False):
        super().__init__()
        conv = nn.Conv2d(in_ch, out_ch, 1)
        self.conv = nn.Sequential(conv, nn.Sigmoid()) if sigmoid else conv

    def forward(self, x):
        return self.conv(x)
