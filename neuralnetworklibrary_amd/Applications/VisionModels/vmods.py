"""Model registry of the drop-in API (mirror of Applications/VisionModels/vmods.py).  Of the Cadene zoo the reference vendors, the
SENet family (senet.py) and NASNet-A-Large (nasnet.py) are built here on the HIP kernels; inception / the legacy-converted resnext are
out of scope (not on any BASELINE config): their class names exist as placeholders so that `default_cut` /
`default_split` isinstance checks keep working."""
from . import retinanet, resnet, senet, nasnet  # noqa: F401
from .resnet import ResNet, resnet18, resnet34, resnet50, resnet101, resnet152  # noqa: F401
from .senet import SENet, senet154, se_resnet50, se_resnet101, se_resnet152, se_resnext50_32x4d, se_resnext101_32x4d  # noqa: F401
from .nasnet import NASNetALarge, nasnetalarge  # noqa: F401


class _NotVendored:
    "placeholder type for a vendored-zoo architecture that this build does not ship"


ResNeXt101_32x4d = type('ResNeXt101_32x4d', (_NotVendored,), {})
ResNeXt101_64x4d = type('ResNeXt101_64x4d', (_NotVendored,), {})
InceptionV4 = type('InceptionV4', (_NotVendored,), {})
