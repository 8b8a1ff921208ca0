"""InceptionResNetV2 of the drop-in API (mirror of the reference's Applications/VisionModels/inceptionresnetv2.py; the Cadene
pretrained-models lineage, BSD 3-Clause, is credited there) built on the HIP-backed modules.

Same classes, constructor arguments, sub-module names and registration order (=> state_dict keys and named_parameters order).
Differences:
  * BasicConv2d is inceptionv4.py's: HipConv2d through ops.conv_bn_act for the square kernels, HipLineConv2d (csrc/lineconv.hip) for the
    (1, 7) / (7, 1) of Block17 and the (1, 3) / (3, 1) of Block8: 60 of the network's 204 BasicConv2d;
  * the tail of the 10 Block35, relu(x + scale * conv2d(cat(branches))), is ONE ops.cat_conv1x1_residual (csrc/catproj.hip, K20): the
    concatenation is never written, and scale, residual and ReLU are the kernel's epilogue; `self.conv2d` is a HipConv2d that only
    holds the parameters.  Block17 and Block8 compose the tail of torch.cat, their HipConv2d and ATen's elementwise passes: there the
    fused kernels measured slower (README "InceptionResNetV2"), and `fused = True` on the class switches them over;
  * the pools are HipMaxPool2d / HipAvgPool2d (csrc/pool.hip); `logits` pools at the map's width with ops.avgpool2d (widths up to 15);
  * the torch.cat of the Mixed_* blocks stays ATen;
  * `features` is a method, as in the reference, and forward(input, use_logits=False) returns the features by default: the model is
    its own body (Vision.default_cut applies no cut and default_split no split to it), so it carries `num_features`;
  * `pretrained` defaults to None and nothing is ever downloaded: `pretrained='imagenet'` raises.
"""
import torch
import torch.nn as nn

from ... import ops
from .retinanet import HipAvgPool2d, HipConv2d, HipMaxPool2d
from .inceptionv4 import BasicConv2d, _Branches, _maxpool, _pool_conv, _seq

__all__ = ['BasicConv2d', 'Mixed_5b', 'Block35', 'Mixed_6a', 'Block17', 'Mixed_7a', 'Block8', 'InceptionResNetV2', 'inceptionresnetv2']


def _holder(in_planes, out_planes):
    "the closing 1x1 convolution of a residual block: it holds the parameters and never runs, so the prepared-filter window skips it"
    conv = HipConv2d(in_planes, out_planes, kernel_size=1, stride=1)
    conv.nnl_hip_conv = False
    return conv


class _Residual(nn.Module):
    """relu(x + scale * conv2d(cat(branch0(x), branch1(x), ...))) behind the branches: in one kernel where `fused`, else composed of
    torch.cat, ops.conv2d and ATen's elementwise passes.  Which block class takes which is measured: README "InceptionResNetV2"."""
    noReLU = False
    fused = True

    def forward(self, x):
        branches = [getattr(self, 'branch%d' % i)(x) for i in range(self.n_branches)]
        if self.fused:
            return ops.cat_conv1x1_residual(branches, self.conv2d.weight, self.conv2d.bias, x, self.scale, relu=not self.noReLU)
        out = self.conv2d(torch.cat(branches, 1)) * self.scale + x
        return out if self.noReLU else torch.relu(out)


class Mixed_5b(_Branches):
    n_branches = 4

    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(192, 96, kernel_size=1, stride=1)
        self.branch1 = _seq(192, [(48, 1, 0), (64, 5, 2)])
        self.branch2 = _seq(192, [(64, 1, 0), (96, 3, 1), (96, 3, 1)])
        self.branch3 = _pool_conv(192, 64)


class Block35(_Residual):
    n_branches = 3

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.branch0 = BasicConv2d(320, 32, kernel_size=1, stride=1)
        self.branch1 = _seq(320, [(32, 1, 0), (32, 3, 1)])
        self.branch2 = _seq(320, [(32, 1, 0), (48, 3, 1), (64, 3, 1)])
        self.conv2d = _holder(128, 320)
        self.relu = nn.ReLU(inplace=False)


class Mixed_6a(_Branches):
    n_branches = 3

    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(320, 384, kernel_size=3, stride=2)
        self.branch1 = _seq(320, [(256, 1, 0), (256, 3, 1), (384, 3, 0, 2)])
        self.branch2 = _maxpool()


class Block17(_Residual):
    n_branches = 2
    fused = False                                        # measured slower than the composed route at 17 x 17

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.branch0 = BasicConv2d(1088, 192, kernel_size=1, stride=1)
        self.branch1 = _seq(1088, [(128, 1, 0), (160, (1, 7), (0, 3)), (192, (7, 1), (3, 0))])
        self.conv2d = HipConv2d(384, 1088, kernel_size=1, stride=1)
        self.relu = nn.ReLU(inplace=False)


class Mixed_7a(_Branches):
    n_branches = 4

    def __init__(self):
        super().__init__()
        self.branch0 = _seq(1088, [(256, 1, 0), (384, 3, 0, 2)])
        self.branch1 = _seq(1088, [(256, 1, 0), (288, 3, 0, 2)])
        self.branch2 = _seq(1088, [(256, 1, 0), (288, 3, 1), (320, 3, 0, 2)])
        self.branch3 = _maxpool()


class Block8(_Residual):
    n_branches = 2
    fused = False                                        # measured slower than the composed route at 8 x 8

    def __init__(self, scale=1.0, noReLU=False):
        super().__init__()
        self.scale = scale
        self.noReLU = noReLU
        self.branch0 = BasicConv2d(2080, 192, kernel_size=1, stride=1)
        self.branch1 = _seq(2080, [(192, 1, 0), (224, (1, 3), (0, 1)), (256, (3, 1), (1, 0))])
        self.conv2d = HipConv2d(448, 2080, kernel_size=1, stride=1)
        if not self.noReLU:
            self.relu = nn.ReLU(inplace=False)


class InceptionResNetV2(nn.Module):
    num_features = 1536                                  # conv2d_7b's channels: what `forward` returns by default

    def __init__(self, num_classes=1001):
        super().__init__()
        self.input_space = None
        self.input_size = (299, 299, 3)
        self.mean = None
        self.std = None
        self.conv2d_1a = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.conv2d_2a = BasicConv2d(32, 32, kernel_size=3, stride=1)
        self.conv2d_2b = BasicConv2d(32, 64, kernel_size=3, stride=1, padding=1)
        self.maxpool_3a = HipMaxPool2d(3, stride=2)
        self.conv2d_3b = BasicConv2d(64, 80, kernel_size=1, stride=1)
        self.conv2d_4a = BasicConv2d(80, 192, kernel_size=3, stride=1)
        self.maxpool_5a = HipMaxPool2d(3, stride=2)
        self.mixed_5b = Mixed_5b()
        self.repeat = nn.Sequential(*[Block35(scale=0.17) for _ in range(10)])
        self.mixed_6a = Mixed_6a()
        self.repeat_1 = nn.Sequential(*[Block17(scale=0.10) for _ in range(20)])
        self.mixed_7a = Mixed_7a()
        self.repeat_2 = nn.Sequential(*[Block8(scale=0.20) for _ in range(9)])
        self.block8 = Block8(noReLU=True)
        self.conv2d_7b = BasicConv2d(2080, 1536, kernel_size=1, stride=1)
        self.avgpool_1a = HipAvgPool2d(8, count_include_pad=False)           # kept for its name: `logits` pools at the map's own width
        self.last_linear = nn.Linear(1536, num_classes)

    def features(self, input):
        x = self.conv2d_1a(input)
        x = self.conv2d_2a(x)
        x = self.conv2d_2b(x)
        x = self.maxpool_3a(x)
        x = self.conv2d_3b(x)
        x = self.conv2d_4a(x)
        x = self.maxpool_5a(x)
        x = self.mixed_5b(x)
        x = self.repeat(x)
        x = self.mixed_6a(x)
        x = self.repeat_1(x)
        x = self.mixed_7a(x)
        x = self.repeat_2(x)
        x = self.block8(x)
        return self.conv2d_7b(x)

    def logits(self, features):
        x = ops.avgpool2d(features, features.shape[2], 1, 0)                 # the reference's AvgPool2d(8) at 299; any last map up to 15 wide
        return ops.linear(x.reshape(x.size(0), -1), self.last_linear.weight, self.last_linear.bias)

    def forward(self, input, use_logits=False):
        x = self.features(input)
        if use_logits:
            x = self.logits(x)
        return x


def inceptionresnetv2(num_classes=1000, pretrained=None):
    if pretrained is not None:
        raise RuntimeError("pretrained=%r: this package never downloads weights.  Build the model with pretrained=None and load a "
                           "locally held checkpoint with load_state_dict: the state_dict keys and shapes are the reference's." % (pretrained,))
    return InceptionResNetV2(num_classes=num_classes)
