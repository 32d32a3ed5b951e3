"""`networks` of the reference: both of its modules (resnet_css, unet_parts) resolve to the sdflabel_amd drop-ins.  A regular package, so it wins
over the reference's own networks/ directory (a namespace portion without __init__.py) wherever that comes on sys.path."""
