"""ResNeXt-101 32x4d and 64x4d (mirror of the reference's Applications/VisionModels/resnext.py:70-138 and of the module trees under
resnext_features/, the Cadene pretrained-models lineage credited there: networks converted from Torch7, hence the ConcatTable /
CAddTable containers) built on the HIP-backed modules.

The reference writes each `features` tree out as a literal listing; here one loop over a width table builds the same nesting, so the
state_dict keys, their shapes and the named_parameters order are the reference's (`features.4.0.0.0.0.0.weight`, ...):
  features = Sequential(conv 7x7/2, BN, ReLU, MaxPool 3/2/1, stage, stage, stage, stage)          stages of 3 / 4 / 23 / 3 blocks
  block    = Sequential(LambdaMap(main, shortcut), LambdaReduce(), ReLU())
  main     = Sequential(Sequential(conv 1x1, BN, ReLU, grouped conv 3x3 (stride), BN, ReLU), conv 1x1, BN)
  shortcut = Sequential(conv 1x1 (stride), BN) in the first block of a stage, Lambda() (the identity) elsewhere
Differences:
  * dense convolutions are `HipConv2d`, the grouped 3x3 is `HipGroupedConv2d` (csrc/gconv.hip; 26 of the 33 have 16 or 32 channels per
    group and run on the MFMA kernels of csrc/gconv_mfma.h), the stem pool is `HipMaxPool2d`, `avg_pool` is `HipAvgPool2d`;
  * a block evaluates conv -> BN (-> ReLU) through ops.conv_bn_act / ops.bn_act and folds the closing add + ReLU into the last of them;
    the stem runs through ops.conv_bn_relu_maxpool.  The containers still work as plain modules when called on their own;
  * every instance builds its own `features` (the reference shares ONE module-level object between all instances of a class);
  * `pretrained` defaults to None and nothing is ever downloaded: `pretrained='imagenet'` raises.  A locally held Cadene checkpoint
    loads with `load_state_dict`, the keys are identical.
"""
from functools import reduce

import torch.nn as nn

from ... import ops
from .resnet import ResNetBody
from .retinanet import HipAvgPool2d, HipConv2d, HipGroupedConv2d, HipMaxPool2d

__all__ = ['ResNeXt101_32x4d', 'resnext101_32x4d', 'ResNeXt101_64x4d', 'resnext101_64x4d']

STAGES = (3, 4, 23, 3)
OUT = (256, 512, 1024, 2048)               # channels a stage hands on; its grouped width is width0 << stage


class LambdaBase(nn.Sequential):
    def forward_prepare(self, input):
        output = [module(input) for module in self._modules.values()]
        return output if output else input


class Lambda(LambdaBase):
    "the identity (Torch7's Identity)"

    def forward(self, input):
        return self.forward_prepare(input)


class LambdaMap(LambdaBase):
    "every child on the same input, as a list (Torch7's ConcatTable)"

    def forward(self, input):
        return list(self.forward_prepare(input))


class LambdaReduce(LambdaBase):
    "the sum of a list (Torch7's CAddTable)"

    def forward(self, input):
        return reduce(lambda a, b: a + b, self.forward_prepare(input))


class _Block(nn.Sequential):
    "Sequential(LambdaMap(main, shortcut), LambdaReduce(), ReLU()) evaluated with the fused BN epilogues"

    def forward(self, x):
        main, shortcut = self[0][0], self[0][1]
        inner = main[0]
        out = ops.conv_bn_act(inner[0], inner[1], x, relu=True)
        out = ops.bn_act(inner[4], inner[3](out), relu=True)
        residual = x if isinstance(shortcut, Lambda) else ops.conv_bn_act(shortcut[0], shortcut[1], x, relu=False)
        return ops.conv_bn_act(main[1], main[2], out, residual=residual, relu=True)


def _conv1x1(cin, cout, stride=1):
    return HipConv2d(cin, cout, kernel_size=1, stride=stride, bias=False)


def _block(cin, width, cout, groups, stride, project):
    inner = nn.Sequential(_conv1x1(cin, width), nn.BatchNorm2d(width), nn.ReLU(),
                          HipGroupedConv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=groups, bias=False),
                          nn.BatchNorm2d(width), nn.ReLU())
    main = nn.Sequential(inner, _conv1x1(width, cout), nn.BatchNorm2d(cout))
    shortcut = nn.Sequential(_conv1x1(cin, cout, stride), nn.BatchNorm2d(cout)) if project else Lambda()
    return _Block(LambdaMap(main, shortcut), LambdaReduce(), nn.ReLU())


def _features(groups, width0, stages=STAGES):
    mods = [HipConv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(), HipMaxPool2d(3, 2, 1)]
    cin = 64
    for i, blocks in enumerate(stages):
        stage = []
        for b in range(blocks):
            stage.append(_block(cin, width0 << i, OUT[i], groups, stride=2 if (b == 0 and i > 0) else 1, project=b == 0))
            cin = OUT[i]
        mods.append(nn.Sequential(*stage))
    return ResNetBody(*mods)               # the stem through ops.conv_bn_relu_maxpool, then the stages


class _ResNeXt(nn.Module):
    groups, width0 = None, None

    def __init__(self, num_classes=1000, stages=STAGES):
        super().__init__()
        self.num_classes = num_classes
        self.features = _features(self.groups, self.width0, stages)
        self.avg_pool = HipAvgPool2d((7, 7), (1, 1))
        self.last_linear = nn.Linear(2048, num_classes)

    def logits(self, input):
        x = self.avg_pool(input)
        x = x.reshape(x.size(0), -1)
        return ops.linear(x, self.last_linear.weight, self.last_linear.bias)

    def forward(self, input):
        return self.logits(self.features(input))


class ResNeXt101_32x4d(_ResNeXt):
    "resnext.py:70-88; grouped widths 128 / 256 / 512 / 1024 at 32 groups"
    groups, width0 = 32, 128


class ResNeXt101_64x4d(_ResNeXt):
    "resnext.py:91-109; grouped widths 256 / 512 / 1024 / 2048 at 64 groups"
    groups, width0 = 64, 256


def _build(cls, num_classes, pretrained):
    if pretrained is not None:
        raise RuntimeError("pretrained=%r: this package never downloads weights.  Build the model with pretrained=None and load a "
                           "locally held Cadene checkpoint with model.load_state_dict(torch.load(path)): the state_dict keys are "
                           "identical." % (pretrained,))
    return cls(num_classes=num_classes)


def resnext101_32x4d(num_classes=1000, pretrained=None):
    return _build(ResNeXt101_32x4d, num_classes, pretrained)


def resnext101_64x4d(num_classes=1000, pretrained=None):
    return _build(ResNeXt101_64x4d, num_classes, pretrained)
