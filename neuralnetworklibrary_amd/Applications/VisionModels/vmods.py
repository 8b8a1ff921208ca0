"""Model registry of the drop-in API (mirror of Applications/VisionModels/vmods.py).  Of the Cadene zoo the reference vendors, the
SENet family (senet.py), NASNet-A-Large (nasnet.py), InceptionV4 (inceptionv4.py), InceptionResNetV2 (inceptionresnetv2.py) and the two
legacy-converted ResNeXt-101 networks (resnext.py) are all built here on the HIP kernels."""
from . import retinanet, resnet, senet, nasnet, resnext  # noqa: F401
from .resnet import ResNet, resnet18, resnet34, resnet50, resnet101, resnet152  # noqa: F401
from .senet import SENet, senet154, se_resnet50, se_resnet101, se_resnet152, se_resnext50_32x4d, se_resnext101_32x4d  # noqa: F401
from .nasnet import NASNetALarge, nasnetalarge  # noqa: F401
from .inceptionv4 import InceptionV4, inceptionv4  # noqa: F401
from .inceptionresnetv2 import InceptionResNetV2, inceptionresnetv2  # noqa: F401
from .resnext import ResNeXt101_32x4d, ResNeXt101_64x4d, resnext101_32x4d, resnext101_64x4d  # noqa: F401
