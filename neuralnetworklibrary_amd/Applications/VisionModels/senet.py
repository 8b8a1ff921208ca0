"""SENet-154, SE-ResNet and SE-ResNeXt (mirror of the reference's Applications/VisionModels/senet.py:118-475, the Cadene
pretrained-models lineage credited there) built on the HIP-backed modules.

Same classes, constructor arguments, sub-module names (=> state_dict keys and shapes) and outputs.  Differences:
  * dense convolutions are `HipConv2d` (the 3x3 / stride 2 projection shortcuts and the three-convolution stem of SENet-154
    included), the grouped 3x3 is `HipGroupedConv2d` (csrc/gconv.hip); conv -> BN (-> ReLU) runs through ops.conv_bn_act, and
    ops.bn_act after the grouped convolution;
  * the tail of a block — SEModule, `+ residual`, ReLU (senet.py:161-162) — is one call of ops.se_excite (csrc/se.hip);
  * the stem pool is the ceil-mode `HipMaxPool2d`;
  * `pretrained` defaults to None and nothing is ever downloaded: `pretrained='imagenet'` raises.  A locally held Cadene checkpoint
    loads with `load_state_dict`, the keys are identical.
"""
import math
from collections import OrderedDict

import torch.nn as nn

from ... import ops
from .retinanet import HipConv2d, HipGroupedConv2d, HipMaxPool2d, _Downsample

__all__ = ['SENet', 'SEModule', 'SEBottleneck', 'SEResNetBottleneck', 'SEResNeXtBottleneck', 'senet154', 'se_resnet50', 'se_resnet101',
           'se_resnet152', 'se_resnext50_32x4d', 'se_resnext101_32x4d']


class _SEFc(nn.Conv2d):
    "the 1x1 convolution with bias of an SEModule on its [N, C, 1, 1] input (senet.py:123-127): a GEMM on the [N, C] matrix"

    def forward(self, x):
        y = ops.linear(x.flatten(1), self.weight.reshape(self.out_channels, self.in_channels), self.bias)
        return y[:, :, None, None]


class SEModule(nn.Module):
    "x * sigmoid(fc2(relu(fc1(avg_pool(x)))))   (senet.py:118-137)"

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = _SEFc(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = _SEFc(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        # (the blocks below do not come through here: they fuse the module with their closing add and ReLU)
        return x * self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))


def _conv(inplanes, planes, kernel_size, stride=1, padding=0, groups=1):
    "HipConv2d, or HipGroupedConv2d for groups > 1; no bias"
    if groups == 1:
        return HipConv2d(inplanes, planes, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
    return HipGroupedConv2d(inplanes, planes, kernel_size=kernel_size, stride=stride, padding=padding, groups=groups, bias=False)


class Bottleneck(nn.Module):
    "conv1-BN-ReLU-conv2-BN-ReLU-conv3-BN -> SE scaling (+ downsample(x)) -> ReLU   (senet.py:140-164)"

    def forward(self, x):
        out = ops.conv_bn_act(self.conv1, self.bn1, x, relu=True)
        if isinstance(self.conv2, HipGroupedConv2d):
            out = ops.bn_act(self.bn2, self.conv2(out), relu=True)
        else:
            out = ops.conv_bn_act(self.conv2, self.bn2, out, relu=True)
        out = ops.conv_bn_act(self.conv3, self.bn3, out, relu=False)
        residual = x if self.downsample is None else self.downsample(x)
        return ops.se_excite(out, self.se_module.fc1, self.se_module.fc2, residual)


class SEBottleneck(Bottleneck):
    "Bottleneck for SENet154   (senet.py:167-188)"
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes * 2, 1)
        self.bn1 = nn.BatchNorm2d(planes * 2)
        self.conv2 = _conv(planes * 2, planes * 4, 3, stride=stride, padding=1, groups=groups)
        self.bn2 = nn.BatchNorm2d(planes * 4)
        self.conv3 = _conv(planes * 4, planes * 4, 1)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride


class SEResNetBottleneck(Bottleneck):
    "ResNet bottleneck with an SE module; Caffe style: the stride sits in conv1   (senet.py:191-213)"
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 1, stride=stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _conv(planes, planes, 3, padding=1, groups=groups)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = _conv(planes, planes * 4, 1)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride


class SEResNeXtBottleneck(Bottleneck):
    "ResNeXt bottleneck type C with an SE module   (senet.py:216-237)"
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None, base_width=4):
        super().__init__()
        width = math.floor(planes * (base_width / 64)) * groups
        self.conv1 = _conv(inplanes, width, 1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3, stride=stride, padding=1, groups=groups)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv(width, planes * 4, 1)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride


class _Stem(nn.Sequential):
    "layer0 (senet.py:290-316): (conv, BN, ReLU) once or three times, then the ceil-mode pool; conv -> BN -> ReLU through ops.conv_bn_act"

    def forward(self, x):
        mods = list(self.children())
        while len(mods) >= 3 and isinstance(mods[0], HipConv2d) and isinstance(mods[1], nn.BatchNorm2d) and isinstance(mods[2], nn.ReLU):
            x = ops.conv_bn_act(mods[0], mods[1], x, relu=True)
            mods = mods[3:]
        for m in mods:
            x = m(x)
        return x


class SENet(nn.Module):
    """senet.py:240-399; the arguments are the reference's:
    block SEBottleneck (SENet154) / SEResNetBottleneck / SEResNeXtBottleneck, layers = blocks per stage, groups 64 / 1 / 32,
    reduction 16, dropout_p 0.2 / None / None, inplanes 128 / 64 / 64, input_3x3 True / False / False (three 3x3 convolutions
    instead of one 7x7 in layer0), downsample_kernel_size 3 / 1 / 1 and downsample_padding 1 / 0 / 0 (projection shortcuts of
    layer2 .. layer4), num_classes."""

    def __init__(self, block, layers, groups, reduction, dropout_p=0.2, inplanes=128, input_3x3=True, downsample_kernel_size=3,
                 downsample_padding=1, num_classes=1000):
        super().__init__()
        self.inplanes = inplanes
        if input_3x3:
            layer0_modules = [
                ('conv1', _conv(3, 64, 3, stride=2, padding=1)), ('bn1', nn.BatchNorm2d(64)), ('relu1', nn.ReLU(inplace=True)),
                ('conv2', _conv(64, 64, 3, stride=1, padding=1)), ('bn2', nn.BatchNorm2d(64)), ('relu2', nn.ReLU(inplace=True)),
                ('conv3', _conv(64, inplanes, 3, stride=1, padding=1)), ('bn3', nn.BatchNorm2d(inplanes)), ('relu3', nn.ReLU(inplace=True)),
            ]
        else:
            layer0_modules = [('conv1', _conv(3, inplanes, 7, stride=2, padding=3)), ('bn1', nn.BatchNorm2d(inplanes)),
                              ('relu1', nn.ReLU(inplace=True))]
        # ceil_mode instead of padding=1: compatibility with the Caffe weights (senet.py:312-315)
        layer0_modules.append(('pool', HipMaxPool2d(3, stride=2, ceil_mode=True)))
        self.layer0 = _Stem(OrderedDict(layer0_modules))
        self.layer1 = self._make_layer(block, planes=64, blocks=layers[0], groups=groups, reduction=reduction, downsample_kernel_size=1,
                                       downsample_padding=0)
        ds = dict(groups=groups, reduction=reduction, stride=2, downsample_kernel_size=downsample_kernel_size,
                  downsample_padding=downsample_padding)
        self.layer2 = self._make_layer(block, planes=128, blocks=layers[1], **ds)
        self.layer3 = self._make_layer(block, planes=256, blocks=layers[2], **ds)
        self.layer4 = self._make_layer(block, planes=512, blocks=layers[3], **ds)
        self.avg_pool = nn.AvgPool2d(7, stride=1)
        self.dropout = nn.Dropout(dropout_p) if dropout_p is not None else None
        self.last_linear = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, blocks, groups, reduction, stride=1, downsample_kernel_size=1, downsample_padding=0):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = _Downsample(
                _conv(self.inplanes, planes * block.expansion, downsample_kernel_size, stride=stride, padding=downsample_padding),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, groups, reduction, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups, reduction))
        return nn.Sequential(*layers)

    def features(self, x):
        return self.layer4(self.layer3(self.layer2(self.layer1(self.layer0(x)))))

    def logits(self, x):
        x = self.avg_pool(x)
        if self.dropout is not None:
            x = self.dropout(x)
        x = x.reshape(x.size(0), -1)
        return ops.linear(x, self.last_linear.weight, self.last_linear.bias)

    def forward(self, x):
        return self.logits(self.features(x))


def _build(pretrained, num_classes, *args, **kw):
    if pretrained is not None:
        raise RuntimeError("pretrained=%r: this package never downloads weights.  Build the model with pretrained=None and load a "
                           "locally held Cadene checkpoint with model.load_state_dict(torch.load(path)): the state_dict keys are "
                           "identical." % (pretrained,))
    return SENet(*args, num_classes=num_classes, **kw)


_PLAIN = dict(dropout_p=None, inplanes=64, input_3x3=False, downsample_kernel_size=1, downsample_padding=0)


def senet154(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEBottleneck, [3, 8, 36, 3], groups=64, reduction=16, dropout_p=0.2)


def se_resnet50(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEResNetBottleneck, [3, 4, 6, 3], groups=1, reduction=16, **_PLAIN)


def se_resnet101(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEResNetBottleneck, [3, 4, 23, 3], groups=1, reduction=16, **_PLAIN)


def se_resnet152(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEResNetBottleneck, [3, 8, 36, 3], groups=1, reduction=16, **_PLAIN)


def se_resnext50_32x4d(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEResNeXtBottleneck, [3, 4, 6, 3], groups=32, reduction=16, **_PLAIN)


def se_resnext101_32x4d(num_classes=1000, pretrained=None):
    return _build(pretrained, num_classes, SEResNeXtBottleneck, [3, 4, 23, 3], groups=32, reduction=16, **_PLAIN)
