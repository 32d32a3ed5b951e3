"""pipelines/train_css.py of the reference on sdflabel_amd.pipelines.train_css: `from pipelines.train_css import train_css` trains the CSS
network with the output head's losses and backward fused on the device.  datasets.crops.Crops stays the caller's (the reference's) module.
"""
from sdflabel_amd.pipelines.train_css import train_css, train_step  # noqa: F401
