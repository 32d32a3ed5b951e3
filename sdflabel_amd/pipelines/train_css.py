"""pipelines/train_css.py of the reference: training of the CSS network, with the output head's losses and their backward fused on the device
(sdflabel_amd.css.css_head_loss / css_latent_loss through networks.resnet_css.ResNet.loss).  The convolutional body trains through torch's
autograd as before; no [B][256][H][W] tensor exists at any point of a step.

train_step(net, optimizer, batch)    one optimisation step on a batch of the reference's Crops dataset
train_css(cfgp, trainloader=None, augment=None)
                                     the reference's loop: Adam, `lr` and `epochs` from the config, its print line, css.pt (the reference's
                                     state_dict names) under <log dir>/net every `analyse_epoch` epochs; augment='device' reads the crops with
                                     sdflabel_amd.datasets.crops and augments them on the device (no torchvision)

The image dumps of the reference (torchvision.utils.save_image) are not written."""
import os

import torch

from ..networks.resnet_css import setup_css


def _cfg(cfgp, section, key, default, conv):
    return conv(cfgp.get(section, key)) if cfgp.has_option(section, key) else default


def train_step(net, optimizer, batch, device=None):
    """One step: batch is a dict with 'rgb' [B][3][H][W] float, 'mask' [B][H][W], 'uvw' [B][3][H][W] (integer classes 0 ... 255) and 'latent'
    [B][3] (or [1][B][3], which the reference squeezes).  Returns the four loss values as detached tensors {'loss', 'uvw', 'mask', 'latent'}.
    Reproducible: the same weights and batch give the same bits in every call."""
    device = device if device is not None else next(net.parameters()).device
    rgb = batch['rgb'].to(device).float()
    mask_gt = batch['mask'].to(device)
    uvw_gt = batch['uvw'].to(device)
    latent_gt = batch['latent'].to(device).float().reshape(-1, 3)
    if mask_gt.dtype != torch.uint8:
        mask_gt = mask_gt.long()
    if uvw_gt.dtype != torch.uint8:
        uvw_gt = uvw_gt.long()
    optimizer.zero_grad()
    # The body's convolutions run with the library's deterministic solvers: with the default choice layer2's output, and with it every loss
    # and gradient, changed in the last bits from call to call for the same weights and images (the fused head losses have no atomics and
    # never did).  A step then has the same bits whenever it is repeated.  The caller's setting is restored on the way out.
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        losses = net.loss(rgb, uvw_gt, mask_gt, latent_gt)
        losses['loss'].backward()
    finally:
        torch.backends.cudnn.deterministic = was
    optimizer.step()
    return {k: v.detach() for k, v in losses.items()}


def train_css(cfgp, trainloader=None, augment=None):
    """Training of the CSS network (the reference's train_css).  cfgp: a ConfigParser with the reference's keys ([input] css_path, data_path;
    [train] lr, batch_size, epochs; [log] dir, analyse_epoch; [optimization] cpu_threads).

    trainloader: any iterable of the reference's batches with a .dataset.  With trainloader=None the loader is built as the reference builds
    it, from the CALLER's datasets.crops.Crops: that module is the reference's own and is not ported here (its augmentations need
    torchvision, which this package does not depend on), so it has to be importable from the caller's path.

    augment: None keeps that behaviour.  'device' (with trainloader=None) builds sdflabel_amd.datasets.crops.DeviceCropLoader over
    sdflabel_amd.datasets.crops.Crops from the config's data_path and batch_size: the reference's augmentation, byte for byte Pillow's for
    the same random parameters, batched on the device (sdflabel_amd.augment)."""
    if augment not in (None, 'device'):
        raise ValueError("train_css: augment must be None or 'device', got %r" % (augment,))
    if augment is not None and trainloader is not None:
        raise ValueError("train_css: augment=%r builds the loader itself; pass either it or trainloader" % (augment,))
    if not torch.cuda.is_available():
        from .._lib import SdfrError
        raise SdfrError("train_css: sdflabel_amd runs on the GPU only; there is no CPU fallback")
    device = torch.device("cuda")
    css_path = _cfg(cfgp, 'input', 'css_path', '', str)
    css_net = setup_css(pretrained=bool(css_path), model_path=css_path).to(device)
    lr = _cfg(cfgp, 'train', 'lr', 1e-4, float)
    optimizer = torch.optim.Adam(css_net.parameters(), lr=lr)
    log_dir = _cfg(cfgp, 'log', 'dir', 'log', str)
    os.makedirs(log_dir, exist_ok=True)
    if augment == 'device':
        from ..datasets.crops import Crops, DeviceCropLoader
        trainloader = DeviceCropLoader(Crops(_cfg(cfgp, 'input', 'data_path', None, str)), _cfg(cfgp, 'train', 'batch_size', 32, int),
                                       shuffle=True, device=device)
    elif trainloader is None:
        from datasets.crops import Crops                   # the caller's (the reference's) dataset
        batch_size = _cfg(cfgp, 'train', 'batch_size', 32, int)
        cpu_threads = _cfg(cfgp, 'optimization', 'cpu_threads', 3, int)
        data_path = _cfg(cfgp, 'input', 'data_path', None, str)
        if Crops.__module__ == 'sdflabel_amd.datasets.crops':  # the compat path resolved it to this package's dataset (raw uint8 images):
            from ..datasets.crops import DeviceCropLoader      # that one is batched by the device loader, not by DataLoader's collate
            trainloader = DeviceCropLoader(Crops(data_path), batch_size, shuffle=True, device=device)
        else:
            trainloader = torch.utils.data.DataLoader(Crops(data_path), batch_size=batch_size, shuffle=True, num_workers=cpu_threads)
    epochs = _cfg(cfgp, 'train', 'epochs', 1000, int)
    analyse_epoch = _cfg(cfgp, 'log', 'analyse_epoch', 10, int)
    for epoch in range(epochs):
        for batch_idx, batch in enumerate(trainloader):
            n = len(batch['rgb'])
            losses = train_step(css_net, optimizer, batch, device)
            print(
                'Train Epoch: {} [{}/{} ({:.0f}%)]\tLosses: global - {:.6f}, uvw - {:.6f}, mask - {:.6f}, latent - {:.6f}'
                .format(
                    epoch, batch_idx * n, len(trainloader.dataset), 100. * batch_idx / len(trainloader),
                    losses['loss'].item(), losses['uvw'].item(), losses['mask'].item(), losses['latent'].item()
                )
            )
        if (epoch + 1) % analyse_epoch == 0:
            net_dir = os.path.join(log_dir, 'net')
            os.makedirs(net_dir, exist_ok=True)
            torch.save(css_net.state_dict(), os.path.join(net_dir, 'css.pt'))
    return css_net
