from sdflabel_amd.networks.unet_parts import double_conv, down, inconv, outconv, up  # noqa: F401
