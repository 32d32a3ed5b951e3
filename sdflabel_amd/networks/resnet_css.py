"""The CSS network (networks/resnet_css.py of the reference): a ResNet-18 encoder, four U-Net decoders (u, v, w, mask) and a latent head.

The convolutional body is plain torch layers (MIOpen on the GPU) under exactly the reference's state_dict names and shapes -- 354 entries,
14 921 413 parameters, the unused layer4 included -- so `torch.load` of a reference css.pt loads with strict=True.  The tail is not torch:
forward() hands the five head inputs to sdflabel_amd.css.css_head / css_latent (csrc/css_head.hip), which produce the reference's output
dict without writing anything 256 channels wide.  The out_u / out_v / out_w / out_mask / out_lat modules only hold the parameters.

forward() is the inference path and returns detached tensors.  loss() is the training path: features() with gradients, then
sdflabel_amd.css.css_head_loss / css_latent_loss (csrc/css_train.hip), which return the losses of the reference's pipelines/train_css.py and
hand torch's autograd the gradients of the five head inputs and the ten head parameters from one fused call each; the convolutional body
trains through torch's own autograd.  sdflabel_amd.pipelines.train_css runs the loop and saves css.pt under the reference's names.
features() is torch only and runs wherever torch runs; forward() and loss() need the GPU (no CPU fallback)."""
import torch
import torch.nn as nn

from .unet_parts import outconv, up

__all__ = ['ResNet', 'resnet18']

HEADS = ('u', 'v', 'w', 'mask')


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


def project_vecs_onto_sphere(vectors, radius, surface_only=True):
    """every row scaled to length `radius` (surface_only) or clipped to it, with the reference's 1e-8 guard; in place, like the reference"""
    for i in range(len(vectors)):
        length = torch.norm(vectors[i]).detach()
        if surface_only or float(length) > radius:
            vectors[i] = vectors[i].mul(radius / (length + 1e-8))
    return vectors


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        y += x if self.downsample is None else self.downsample(x)
        return self.relu(y)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        y += x if self.downsample is None else self.downsample(x)
        return self.relu(y)


class ResNet(nn.Module):
    """logprobs=True adds the reference's 'u', 'v', 'w' (log_softmax of the class logits, [B][256][H][W] each) to forward()'s dict; the
    refinement reads none of them, so they are off by default and nothing 256 channels wide is written."""

    def __init__(self, block, layers, num_classes=2, logprobs=False):
        super().__init__()
        self.logprobs = bool(logprobs)
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)          # never run; kept for the reference's state_dict
        # four decoders of the same shape, created head by head in the reference's order (the order fixes the random initialisation)
        for head in HEADS:
            setattr(self, 'up1_' + head, up(384, 128))
            setattr(self, 'up2_' + head, up(192, 64))
            setattr(self, 'up3_' + head, up(128, 64))
            setattr(self, 'up4_' + head, up(64, 64, add_shortcut=False))
        self.out_u = outconv(64, 256)
        self.out_v = outconv(64, 256)
        self.out_w = outconv(64, 256)
        self.out_lat = outconv(256, 3)
        self.out_mask = outconv(64, 2)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        for frozen in (self.conv1, self.bn1, self.layer1):                       # the stem stays as loaded
            for prm in frozen.parameters():
                prm.requires_grad = False

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        stages = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        stages += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stages)

    def features(self, x):
        """The five inputs of the output head for images x [B][3][H][W] (H, W multiples of 16): {'x4' [B][256][H/16][W/16], 'x_u', 'x_v',
        'x_w', 'x_mask' [B][64][H][W]}.  Torch layers only: runs on any device, with gradients if the caller wants them."""
        x1 = self.relu(self.bn1(self.conv1(x)))           # 1/2,  64
        x2 = self.maxpool(x1)                             # 1/4,  64
        x3 = self.layer2(self.layer1(x2))                 # 1/8,  128
        x4 = self.layer3(x3)                              # 1/16, 256
        out = {'x4': x4}
        for head in HEADS:
            y = getattr(self, 'up1_' + head)(x4, x3)
            y = getattr(self, 'up2_' + head)(y, x2)
            y = getattr(self, 'up3_' + head)(y, x1)
            out['x_' + head] = getattr(self, 'up4_' + head)(y, x)
        return out

    def head_weights(self):
        """the `weights` argument of sdflabel_amd.css.css_head"""
        return {h: (getattr(self, 'out_' + h).conv.weight, getattr(self, 'out_' + h).conv.bias) for h in HEADS}

    def forward(self, x):
        """The reference's output dict -- 'uvw_sm', 'uvw_sm_masked', 'mask', 'mask_sm', 'latent', and 'u', 'v', 'w' with logprobs=True -- as
        detached tensors: features() in torch, then one css_head and one css_latent launch."""
        from .. import css
        f = self.features(x)
        c = lambda t: t.detach().float().contiguous()     # noqa: E731
        out = css.css_head(c(f['x_u']), c(f['x_v']), c(f['x_w']), c(f['x_mask']), self.head_weights(), logprobs=self.logprobs)
        out['latent'] = css.css_latent(c(f['x4']), self.out_lat.conv.weight, self.out_lat.conv.bias)
        return out


    def loss(self, rgb, uvw_gt, mask_gt, latent_gt):
        """The training losses of the reference (pipelines/train_css.py:65-80) for images rgb [B][3][H][W], uvw_gt [B][3][H][W] and mask_gt
        [B][H][W] (uint8 or int64) and latent_gt [B][3]: {'loss': uvw + latent + mask, 'uvw': loss_u + loss_v + loss_w, 'mask': 2 CE,
        'latent': MSE}, scalar tensors with gradients towards every trainable parameter.  Nothing [B][256][H][W] is formed."""
        from .. import css
        f = self.features(rgb)
        c = lambda t: t.float().contiguous()              # noqa: E731
        lh = css.css_head_loss(c(f['x_u']), c(f['x_v']), c(f['x_w']), c(f['x_mask']), self.head_weights(), uvw_gt, mask_gt)
        latent = css.css_latent_loss(c(f['x4']), self.out_lat.conv.weight, self.out_lat.conv.bias, latent_gt.float().contiguous())
        uvw = lh['u'] + lh['v'] + lh['w']
        return {'loss': uvw + latent + lh['mask'], 'uvw': uvw, 'mask': lh['mask'], 'latent': latent}


def resnet18(pretrained=False, **kwargs):
    """ResNet-18 encoder.  pretrained=True would fetch ImageNet weights in the reference; this module never downloads (see setup_css)."""
    if pretrained:
        raise RuntimeError("resnet18(pretrained=True): this module never downloads weights; pass a model_path to setup_css")
    return ResNet(BasicBlock, [2, 2, 2, 2], **kwargs)


def setup_css(pretrained=False, model_path=None, mode='train', logprobs=False):
    """The CSS network, optionally restored from `model_path` (a reference css.pt; strict load) and put into `mode`.

    mode keeps the reference's default 'train', which is how pipelines/refine_css.py:40 runs the network: BatchNorm then normalises with the
    statistics of the batch it is given, so the prediction for a crop depends on the other crops of the call.  In that mode only batches of
    one crop (css_batch=1 in refine_sample) reproduce the reference's per-crop statistics; mode='eval' uses the stored running statistics.
    pretrained=True never downloads: with a model_path the strict load overrides every ImageNet weight anyway, so it is accepted and
    ignored; without one it raises."""
    if pretrained and not model_path:
        raise RuntimeError("setup_css(pretrained=True) without a model_path would download ImageNet weights; this module never downloads")
    model = resnet18(pretrained=False, logprobs=logprobs)
    if model_path:
        model.load_state_dict(torch.load(model_path, map_location='cpu'), strict=True)
        print("CSS net restored.")
    if mode == 'train':
        model.train()
    elif mode == 'eval':
        model.eval()
    return model
