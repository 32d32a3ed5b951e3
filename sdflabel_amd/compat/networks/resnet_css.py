from sdflabel_amd.networks.resnet_css import BasicBlock, Bottleneck, ResNet, project_vecs_onto_sphere, resnet18, setup_css  # noqa: F401
