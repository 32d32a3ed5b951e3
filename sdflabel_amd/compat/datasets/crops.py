"""datasets/crops.py of the reference on sdflabel_amd.datasets.crops: `from datasets.crops import Crops` reads the same files without
torchvision; the augmentation runs on the device in DeviceCropLoader, not in __getitem__.
"""
from sdflabel_amd.datasets.crops import Crops, DeviceCropLoader  # noqa: F401
