"""pipelines/train_css.py of the reference on sdflabel_amd.pipelines.train_css: `from pipelines.train_css import train_css` trains the CSS
network with the output head's losses and backward fused on the device.  train_css(cfgp, augment='device') reads and augments the crops
without torchvision (compat/datasets/crops.py); without it datasets.crops.Crops is whatever the caller's path resolves it to.
"""
from sdflabel_amd.pipelines.train_css import train_css, train_step  # noqa: F401
