"""InceptionV4 of the drop-in API (mirror of the reference's Applications/VisionModels/inceptionv4.py; the Cadene pretrained-models
lineage, BSD 3-Clause, is credited there) built on the HIP-backed modules.

Same classes, constructor arguments, sub-module names and registration order (=> state_dict keys and named_parameters order).
Differences:
  * a BasicConv2d's convolution is a `HipConv2d` when its kernel is square and a `HipLineConv2d` (csrc/lineconv.hip, K19) when it is
    (1, T) or (T, 1): 64 of the network's 149 convolutions.  A square one runs ops.conv_bn_act (BatchNorm statistics from the
    convolution's epilogue); a line convolution runs conv -> ops.bn_act, because conv_bn_act's fused route reads `conv.padding[0]` for
    both axes and would mis-pad it;
  * the pools are HipMaxPool2d / HipAvgPool2d (csrc/pool.hip); `logits` pools at the map's width with ops.avgpool2d (widths up to 15);
  * torch.cat stays ATen;
  * `pretrained` defaults to None and nothing is ever downloaded: `pretrained='imagenet'` raises.
A block's branches are written as rows of (out_planes, kernel_size, padding[, stride]) and chained by _chain.
"""
import torch
import torch.nn as nn

from ... import ops
from .retinanet import HipConv2d, HipLineConv2d, HipMaxPool2d, HipAvgPool2d

__all__ = ['BasicConv2d', 'Mixed_3a', 'Mixed_4a', 'Mixed_5a', 'Inception_A', 'Reduction_A', 'Inception_B', 'Reduction_B', 'Inception_C',
           'InceptionV4', 'inceptionv4']


class BasicConv2d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride, padding=0):
        super().__init__()
        square = isinstance(kernel_size, int) or kernel_size[0] == kernel_size[1]
        self.conv = (HipConv2d if square else HipLineConv2d)(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding,
                                                             bias=False)
        self.bn = nn.BatchNorm2d(out_planes, eps=0.001, momentum=0.1, affine=True)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        if isinstance(self.conv, HipLineConv2d):                             # never through conv_bn_act: see the module docstring
            return ops.bn_act(self.bn, self.conv(x), relu=True)
        return ops.conv_bn_act(self.conv, self.bn, x, relu=True)


def _chain(in_planes, rows):
    "BasicConv2d modules for rows of (out_planes, kernel_size, padding[, stride]), each fed by the one before it"
    mods = []
    for out_planes, kernel_size, padding, *stride in rows:
        mods.append(BasicConv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride[0] if stride else 1, padding=padding))
        in_planes = out_planes
    return mods


def _seq(in_planes, rows):
    return nn.Sequential(*_chain(in_planes, rows))


def _pool_conv(in_planes, out_planes):
    return nn.Sequential(HipAvgPool2d(3, stride=1, padding=1, count_include_pad=False), *_chain(in_planes, [(out_planes, 1, 0)]))


def _maxpool():
    return HipMaxPool2d(3, stride=2)


class _Branches(nn.Module):
    "concatenation of branch0, branch1, ... on the same input"

    def forward(self, x):
        return torch.cat([getattr(self, 'branch%d' % i)(x) for i in range(self.n_branches)], 1)


class Mixed_3a(nn.Module):
    def __init__(self):
        super().__init__()
        self.maxpool = _maxpool()
        self.conv = BasicConv2d(64, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat((self.maxpool(x), self.conv(x)), 1)


class Mixed_4a(_Branches):
    n_branches = 2

    def __init__(self):
        super().__init__()
        self.branch0 = _seq(160, [(64, 1, 0), (96, 3, 0)])
        self.branch1 = _seq(160, [(64, 1, 0), (64, (1, 7), (0, 3)), (64, (7, 1), (3, 0)), (96, (3, 3), 0)])


class Mixed_5a(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = BasicConv2d(192, 192, kernel_size=3, stride=2)
        self.maxpool = _maxpool()

    def forward(self, x):
        return torch.cat((self.conv(x), self.maxpool(x)), 1)


class Inception_A(_Branches):
    n_branches = 4

    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(384, 96, kernel_size=1, stride=1)
        self.branch1 = _seq(384, [(64, 1, 0), (96, 3, 1)])
        self.branch2 = _seq(384, [(64, 1, 0), (96, 3, 1), (96, 3, 1)])
        self.branch3 = _pool_conv(384, 96)


class Reduction_A(_Branches):
    n_branches = 3

    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(384, 384, kernel_size=3, stride=2)
        self.branch1 = _seq(384, [(192, 1, 0), (224, 3, 1), (256, 3, 0, 2)])
        self.branch2 = _maxpool()


class Inception_B(_Branches):
    n_branches = 4

    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(1024, 384, kernel_size=1, stride=1)
        self.branch1 = _seq(1024, [(192, 1, 0), (224, (1, 7), (0, 3)), (256, (7, 1), (3, 0))])
        self.branch2 = _seq(1024, [(192, 1, 0), (192, (7, 1), (3, 0)), (224, (1, 7), (0, 3)), (224, (7, 1), (3, 0)), (256, (1, 7), (0, 3))])
        self.branch3 = _pool_conv(1024, 128)


class Reduction_B(_Branches):
    n_branches = 3

    def __init__(self):
        super().__init__()
        self.branch0 = _seq(1024, [(192, 1, 0), (192, 3, 0, 2)])
        self.branch1 = _seq(1024, [(256, 1, 0), (256, (1, 7), (0, 3)), (320, (7, 1), (3, 0)), (320, 3, 0, 2)])
        self.branch2 = _maxpool()


class Inception_C(nn.Module):
    def __init__(self):
        super().__init__()
        along_w, along_h = ((1, 3), (0, 1)), ((3, 1), (1, 0))
        self.branch0 = BasicConv2d(1536, 256, kernel_size=1, stride=1)
        self.branch1_0 = BasicConv2d(1536, 384, kernel_size=1, stride=1)
        self.branch1_1a, = _chain(384, [(256,) + along_w])
        self.branch1_1b, = _chain(384, [(256,) + along_h])
        self.branch2_0 = BasicConv2d(1536, 384, kernel_size=1, stride=1)
        self.branch2_1, self.branch2_2 = _chain(384, [(448,) + along_h, (512,) + along_w])
        self.branch2_3a, = _chain(512, [(256,) + along_w])
        self.branch2_3b, = _chain(512, [(256,) + along_h])
        self.branch3 = _pool_conv(1536, 256)

    def forward(self, x):
        x1 = self.branch1_0(x)
        x2 = self.branch2_2(self.branch2_1(self.branch2_0(x)))
        return torch.cat((self.branch0(x), self.branch1_1a(x1), self.branch1_1b(x1), self.branch2_3a(x2), self.branch2_3b(x2),
                          self.branch3(x)), 1)


class InceptionV4(nn.Module):
    def __init__(self, num_classes=1001):
        super().__init__()
        self.input_space = None
        self.input_size = (299, 299, 3)
        self.mean = None
        self.std = None
        stem = _chain(3, [(32, 3, 0, 2), (32, 3, 0), (64, 3, 1)])
        self.features = nn.Sequential(*stem, Mixed_3a(), Mixed_4a(), Mixed_5a(), *[Inception_A() for _ in range(4)], Reduction_A(),
                                      *[Inception_B() for _ in range(7)], Reduction_B(), *[Inception_C() for _ in range(3)])
        self.features.num_features = 1536               # Inception_C concatenates 6 x 256 (its last BatchNorm has 256 channels)
        self.last_linear = nn.Linear(1536, num_classes)

    def logits(self, features):
        x = ops.avgpool2d(features, features.shape[2], 1, 0)                 # any image size whose last map is at most 15 wide
        return ops.linear(x.reshape(x.size(0), -1), self.last_linear.weight, self.last_linear.bias)

    def forward(self, input):
        return self.logits(self.features(input))


def inceptionv4(num_classes=1000, pretrained=None):
    if pretrained is not None:
        raise RuntimeError("pretrained=%r: this package never downloads weights.  Build the model with pretrained=None and load a "
                           "locally held checkpoint with load_state_dict: the state_dict keys and shapes are the reference's." % (pretrained,))
    return InceptionV4(num_classes=num_classes)
