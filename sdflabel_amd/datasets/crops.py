"""datasets/crops.py of the reference without torchvision: the dataset reads the crops, the loader augments a whole batch on the device.

  Crops(path)                                                   crops.json and the %05d_rgb.png / %05d_uvw.png files under `path`
  DeviceCropLoader(dataset, batch_size, shuffle, generator)     an iterable of the reference's batch dicts, augmented on the device

The reference's Crops.__getitem__ runs its torchvision transforms per sample on the host; here __getitem__ returns the decoded uint8 images
and DeviceCropLoader hands a batch of them to sdflabel_amd.augment.augment_many.  Pillow is imported lazily and used for decoding only.
The reference's `quat` and `z` (computed with scipy's removed Rotation.from_dcm and never returned) are dropped."""
import json
import os

import numpy as np
import torch

from ..augment import augment_many, draw_params


class Crops(torch.utils.data.Dataset):
    def __init__(self, path):
        self.path = path
        with open(os.path.join(path, 'crops.json'), 'r') as f:
            self.gt = json.load(f)

    def __len__(self):
        return len(self.gt)

    def _read(self, idx, kind):
        from PIL import Image                                  # decoding only
        with Image.open(os.path.join(self.path, '{:05d}_{}.png'.format(idx, kind))) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8)

    def __getitem__(self, idx):
        """The sample before augmentation: 'rgb' and 'uvw' uint8 [h][w][3] arrays, and 'latent' float32 [3], 'crop_size' int64 (w, h),
        'intrinsics' float32 [3][3], 'pose' float32 [4][4] as the reference returns them."""
        gt_sample = self.gt[str(idx)][0]
        rgb, uvw = self._read(idx, 'rgb'), self._read(idx, 'uvw')
        if rgb.shape != uvw.shape:
            raise ValueError("Crops: sample %d has an RGB image of %s and a UVW image of %s" % (idx, rgb.shape, uvw.shape))
        return {
            'rgb': rgb,
            'uvw': uvw,
            'latent': torch.from_numpy(np.array(gt_sample['latent'])).float(),
            'crop_size': torch.Tensor((rgb.shape[1], rgb.shape[0])).long(),
            'intrinsics': torch.Tensor(np.array(gt_sample['intrinsics']).reshape((3, 3))).float(),
            'pose': torch.Tensor(np.array(gt_sample['extrinsics']).reshape((4, 4))).float(),
        }


class DeviceCropLoader:
    """Batches of a Crops dataset with the reference's augmentation done on the device: per batch one draw of the random parameters on the
    host (sdflabel_amd.augment.draw_params, from `generator`) and one augment_many call.  Yields the reference's batch dict: 'rgb' float32
    [B][3][128][128], 'uvw' uint8 [B][3][128][128] and 'mask' uint8 [B][128][128] on the device (train_step takes uint8 labels), 'latent',
    'crop_size', 'intrinsics', 'pose' stacked on the host.  The last batch may be smaller, as with DataLoader's drop_last=False."""

    def __init__(self, dataset, batch_size=32, shuffle=True, generator=None, device=None):
        if batch_size < 1:
            raise ValueError("DeviceCropLoader: batch_size must be positive")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.generator = generator
        self.device = device

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for first in range(0, n, self.batch_size):
            samples = [self.dataset[i] for i in order[first:first + self.batch_size]]
            params = draw_params([(s['rgb'].shape[1], s['rgb'].shape[0]) for s in samples], self.generator)
            rgb, uvw, mask = augment_many([s['rgb'] for s in samples], [s['uvw'] for s in samples], params, device=self.device)
            batch = {'rgb': rgb, 'uvw': uvw, 'mask': mask}
            for key in ('latent', 'crop_size', 'intrinsics', 'pose'):
                batch[key] = torch.stack([s[key] for s in samples])
            yield batch
