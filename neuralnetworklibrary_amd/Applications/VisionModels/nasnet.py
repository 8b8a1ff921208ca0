"""NASNet-A-Large of the drop-in API (mirror of the reference's Applications/VisionModels/nasnet.py; the Cadene pretrained-models
lineage, BSD 3-Clause, is credited there) built on the HIP-backed modules.

Same classes, constructor arguments, sub-module names and registration order (=> state_dict keys and named_parameters order).
Differences:
  * a SeparableConv2d is a `HipDepthwiseConv2d` (csrc/dwconv.hip, K18) followed by a 1x1 `HipConv2d`; a BranchSeparables runs
    dwconv(relu fused into the load) -> conv_bn_act(relu) -> dwconv -> conv_bn_act, so the branch's input ReLU never makes a pass of its own;
  * the pools are HipMaxPool2d / HipAvgPool2d (csrc/pool.hip);
  * "pad top/left by one, convolve or pool at stride 2, drop the first row and column" (MaxPoolPad, AvgPoolPad, BranchSeparablesReduction)
    is ONE asymmetric window op (ops.fold_zero_pad): no padded copy and no sliced, non-contiguous view reaches a kernel.  MaxPoolPad is
    exactly the 3x3 / stride 2 / pad 0 ceil-mode max-pool;
  * the two shifted stride-2 paths of CellStem1 / FirstCell are ops.subsample2d with offsets 0 and 1;
  * torch.cat and the branch additions stay ATen;
  * `pretrained` defaults to None and nothing is ever downloaded: `pretrained='imagenet'` raises.
The five-way wiring of a cell is written once per cell family (_reduce_wiring, _normal_wiring) instead of once per class.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .retinanet import HipConv2d, HipDepthwiseConv2d, HipMaxPool2d, HipAvgPool2d

__all__ = ['MaxPoolPad', 'AvgPoolPad', 'SeparableConv2d', 'BranchSeparables', 'BranchSeparablesStem', 'BranchSeparablesReduction',
           'CellStem0', 'CellStem1', 'FirstCell', 'NormalCell', 'ReductionCell0', 'ReductionCell1', 'NASNetALarge', 'nasnetalarge']


def _bn(channels):
    return nn.BatchNorm2d(channels, eps=0.001, momentum=0.1, affine=True)


def _maxpool():
    return HipMaxPool2d(3, stride=2, padding=1)


def _avgpool(stride):
    return HipAvgPool2d(3, stride=stride, padding=1, count_include_pad=False)


class MaxPoolPad(nn.Module):
    def __init__(self):
        super().__init__()
        self.pad = nn.ZeroPad2d((1, 0, 1, 0))
        self.pool = HipMaxPool2d(3, stride=2, padding=1)

    def forward(self, x):
        # window i of the padded, sliced chain covers rows 2i .. 2i + 2 of x, H // 2 of them: the pad-0 ceil-mode pool
        return ops.maxpool2d(x, 3, 2, 0, ceil_mode=True)


class AvgPoolPad(nn.Module):
    def __init__(self, stride=2, padding=1):
        super().__init__()
        self.pad = nn.ZeroPad2d((1, 0, 1, 0))
        self.pool = HipAvgPool2d(3, stride=stride, padding=padding, count_include_pad=False)

    def forward(self, x):
        return self.pool(x, zero_pad=1)


class SeparableConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, dw_kernel, dw_stride, dw_padding, bias=False):
        super().__init__()
        self.depthwise_conv2d = HipDepthwiseConv2d(in_channels, in_channels, dw_kernel, stride=dw_stride, padding=dw_padding, bias=bias,
                                                   groups=in_channels)
        self.pointwise_conv2d = HipConv2d(in_channels, out_channels, 1, stride=1, bias=bias)

    def forward(self, x):
        return self.pointwise_conv2d(self.depthwise_conv2d(x))


def _separable_bn(sep, bn, x, relu_in, relu_out, zero_pad=None):
    "bn(sep(relu?(x))) with the ReLUs fused: into the depthwise load, and into the BatchNorm that follows the pointwise convolution"
    y = sep.depthwise_conv2d(x, relu_in=relu_in, zero_pad=zero_pad)
    return ops.conv_bn_act(sep.pointwise_conv2d, bn, y, relu=relu_out)


class _Branch(nn.Module):
    "relu -> separable_1 -> bn_sep_1 -> relu1 -> separable_2 -> bn_sep_2, the middle width being `mid`"
    zero_pad = None

    def __init__(self, in_channels, mid, out_channels, kernel_size, stride, padding, bias):
        super().__init__()
        self.relu = nn.ReLU()
        self.separable_1 = SeparableConv2d(in_channels, mid, kernel_size, stride, padding, bias=bias)
        self.bn_sep_1 = _bn(mid)
        self.relu1 = nn.ReLU()
        self.separable_2 = SeparableConv2d(mid, out_channels, kernel_size, 1, padding, bias=bias)
        self.bn_sep_2 = _bn(out_channels)

    def forward(self, x):
        y = _separable_bn(self.separable_1, self.bn_sep_1, x, True, True, zero_pad=self.zero_pad)
        return _separable_bn(self.separable_2, self.bn_sep_2, y, False, False)


class BranchSeparables(_Branch):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, bias=False):
        super().__init__(in_channels, in_channels, out_channels, kernel_size, stride, padding, bias)


class BranchSeparablesStem(_Branch):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, bias=False):
        super().__init__(in_channels, out_channels, out_channels, kernel_size, stride, padding, bias)


class BranchSeparablesReduction(BranchSeparables):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, z_padding=1, bias=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias)
        self.padding = nn.ZeroPad2d((z_padding, 0, z_padding, 0))
        self.zero_pad = z_padding


class _ReluConvBN(nn.Sequential):
    "relu -> 1x1 conv -> bn under the reference's child names"

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.add_module('relu', nn.ReLU())
        self.add_module('conv', HipConv2d(in_channels, out_channels, 1, stride=1, bias=False))
        self.add_module('bn', _bn(out_channels))

    def forward(self, x):
        return ops.conv_bn_act(self.conv, self.bn, F.relu(x), relu=False)


class _ConvBN(nn.Sequential):
    "the network's first layer: 3x3 / stride 2 / no padding convolution -> bn, no ReLU (the cells rectify their own inputs)"

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.add_module('conv', HipConv2d(in_channels, out_channels, kernel_size=3, padding=0, stride=2, bias=False))
        self.add_module('bn', _bn(out_channels))

    def forward(self, x):
        return ops.conv_bn_act(self.conv, self.bn, x, relu=False)


def _two_path_children(cell, in_channels, out_channels):
    "the factorized reduction of CellStem1 / FirstCell: relu, path_1, path_2, final_path_bn, registered in the reference's order"
    cell.relu = nn.ReLU()
    cell.path_1 = nn.Sequential()
    cell.path_1.add_module('avgpool', HipAvgPool2d(1, stride=2, count_include_pad=False))
    cell.path_1.add_module('conv', HipConv2d(in_channels, out_channels, 1, stride=1, bias=False))
    cell.path_2 = nn.ModuleList()
    cell.path_2.add_module('pad', nn.ZeroPad2d((0, 1, 0, 1)))
    cell.path_2.add_module('avgpool', HipAvgPool2d(1, stride=2, count_include_pad=False))
    cell.path_2.add_module('conv', HipConv2d(in_channels, out_channels, 1, stride=1, bias=False))
    cell.final_path_bn = _bn(2 * out_channels)


def _two_path(cell, x):
    "every second pixel from (0, 0) and from (1, 1), each through its own 1x1 convolution, concatenated and normalised"
    r = F.relu(x)
    a = cell.path_1.conv(ops.subsample2d(r, 2, 0))
    b = cell.path_2.conv(ops.subsample2d(r, 2, 1))
    return ops.bn_act(cell.final_path_bn, torch.cat([a, b], 1), relu=False)


def _reduce_children(cell, Branch, left, right, stem=None, pad_pools=False):
    """comb_iter_* of the four stride-2 cells.  `left` / `right` are the widths of the two cell inputs after their 1x1; with `stem` the
    right-hand branches widen from `stem` channels (CellStem0)."""
    def rb(k, s, p):
        return BranchSeparablesStem(stem, left, k, s, p, bias=False) if stem is not None else Branch(right, right, k, s, p, bias=False)
    cell.comb_iter_0_left = Branch(left, left, 5, 2, 2)
    cell.comb_iter_0_right = rb(7, 2, 3)
    cell.comb_iter_1_left = MaxPoolPad() if pad_pools else _maxpool()
    cell.comb_iter_1_right = rb(7, 2, 3)
    cell.comb_iter_2_left = AvgPoolPad() if pad_pools else _avgpool(2)
    cell.comb_iter_2_right = rb(5, 2, 2)
    cell.comb_iter_3_right = _avgpool(1)
    cell.comb_iter_4_left = Branch(left, left, 3, 1, 1, bias=False)
    cell.comb_iter_4_right = MaxPoolPad() if pad_pools else _maxpool()


def _reduce_wiring(cell, a, b):
    c0 = cell.comb_iter_0_left(a) + cell.comb_iter_0_right(b)
    c1 = cell.comb_iter_1_left(a) + cell.comb_iter_1_right(b)
    c2 = cell.comb_iter_2_left(a) + cell.comb_iter_2_right(b)
    c3 = cell.comb_iter_3_right(c0) + c1
    c4 = cell.comb_iter_4_left(c0) + cell.comb_iter_4_right(a)
    return torch.cat([c1, c2, c3, c4], 1)


def _normal_children(cell, left, right):
    cell.comb_iter_0_left = BranchSeparables(right, right, 5, 1, 2, bias=False)
    cell.comb_iter_0_right = BranchSeparables(left, left, 3, 1, 1, bias=False)
    cell.comb_iter_1_left = BranchSeparables(left, left, 5, 1, 2, bias=False)
    cell.comb_iter_1_right = BranchSeparables(left, left, 3, 1, 1, bias=False)
    cell.comb_iter_2_left = _avgpool(1)
    cell.comb_iter_3_left = _avgpool(1)
    cell.comb_iter_3_right = _avgpool(1)
    cell.comb_iter_4_left = BranchSeparables(right, right, 3, 1, 1, bias=False)


def _normal_wiring(cell, left, right):
    c0 = cell.comb_iter_0_left(right) + cell.comb_iter_0_right(left)
    c1 = cell.comb_iter_1_left(left) + cell.comb_iter_1_right(left)
    c2 = cell.comb_iter_2_left(right) + left
    c3 = cell.comb_iter_3_left(left) + cell.comb_iter_3_right(left)
    c4 = cell.comb_iter_4_left(right) + right
    return torch.cat([left, c0, c1, c2, c3, c4], 1)


class CellStem0(nn.Module):
    def __init__(self, stem_filters, num_filters=42):
        super().__init__()
        self.num_filters = num_filters
        self.stem_filters = stem_filters
        self.conv_1x1 = _ReluConvBN(stem_filters, num_filters)
        _reduce_children(self, BranchSeparables, num_filters, None, stem=stem_filters)

    def forward(self, x):
        return _reduce_wiring(self, self.conv_1x1(x), x)


class CellStem1(nn.Module):
    def __init__(self, stem_filters, num_filters):
        super().__init__()
        self.num_filters = num_filters
        self.stem_filters = stem_filters
        self.conv_1x1 = _ReluConvBN(2 * num_filters, num_filters)
        _two_path_children(self, stem_filters, num_filters // 2)
        _reduce_children(self, BranchSeparables, num_filters, num_filters)

    def forward(self, x_conv0, x_stem_0):
        return _reduce_wiring(self, self.conv_1x1(x_stem_0), _two_path(self, x_conv0))


class FirstCell(nn.Module):
    def __init__(self, in_channels_left, out_channels_left, in_channels_right, out_channels_right):
        super().__init__()
        self.conv_1x1 = _ReluConvBN(in_channels_right, out_channels_right)
        _two_path_children(self, in_channels_left, out_channels_left)
        # (the reference sizes every branch of this cell by out_channels_right, which equals 2 * out_channels_left wherever it is built)
        _normal_children(self, out_channels_right, out_channels_right)

    def forward(self, x, x_prev):
        left = _two_path(self, x_prev)
        return _normal_wiring(self, left, self.conv_1x1(x))


class NormalCell(nn.Module):
    def __init__(self, in_channels_left, out_channels_left, in_channels_right, out_channels_right):
        super().__init__()
        self.conv_prev_1x1 = _ReluConvBN(in_channels_left, out_channels_left)
        self.conv_1x1 = _ReluConvBN(in_channels_right, out_channels_right)
        _normal_children(self, out_channels_left, out_channels_right)

    def forward(self, x, x_prev):
        return _normal_wiring(self, self.conv_prev_1x1(x_prev), self.conv_1x1(x))


class _ReductionCell(nn.Module):
    pad_pools = False
    Branch = BranchSeparables

    def __init__(self, in_channels_left, out_channels_left, in_channels_right, out_channels_right):
        super().__init__()
        self.conv_prev_1x1 = _ReluConvBN(in_channels_left, out_channels_left)
        self.conv_1x1 = _ReluConvBN(in_channels_right, out_channels_right)
        # (every branch is sized by out_channels_right, as in the reference; the two widths are equal wherever the cell is built)
        _reduce_children(self, self.Branch, out_channels_right, out_channels_right, pad_pools=self.pad_pools)

    def forward(self, x, x_prev):
        return _reduce_wiring(self, self.conv_1x1(x), self.conv_prev_1x1(x_prev))


class ReductionCell0(_ReductionCell):
    "the reduction whose stride-2 ops pad top/left and drop the first row and column: it needs an even map (as the reference does)"
    pad_pools = True
    Branch = BranchSeparablesReduction


class ReductionCell1(_ReductionCell):
    pass


class NASNetALarge(nn.Module):
    """NASNetALarge (6 @ 4032)"""

    def __init__(self, num_classes=1001, stem_filters=96, penultimate_filters=4032, filters_multiplier=2):
        super().__init__()
        self.num_classes = num_classes
        self.stem_filters = stem_filters
        self.penultimate_filters = penultimate_filters
        self.filters_multiplier = filters_multiplier
        f = penultimate_filters // 24
        self.num_features = 24 * f                      # channels of features(): six concatenated 4f-wide outputs of the last cell

        self.conv0 = _ConvBN(3, stem_filters)
        self.cell_stem_0 = CellStem0(stem_filters, num_filters=f // (filters_multiplier ** 2))
        self.cell_stem_1 = CellStem1(stem_filters, num_filters=f // filters_multiplier)

        index = 0
        for stage, m in enumerate((1, 2, 4)):           # three stages of a FirstCell and five NormalCells at widths f, 2f, 4f
            if stage:
                Reduction = ReductionCell0 if stage == 1 else ReductionCell1
                setattr(self, 'reduction_cell_%d' % (stage - 1), Reduction(3 * m * f, m * f, 3 * m * f, m * f))
            prev = 3 * m * f if stage else f            # width of x_prev for the FirstCell: the cell before the reduction (or stem 0)
            cur = 4 * m * f if stage else 2 * f         # width of its x: the reduction's (or stem 1's) four concatenated branches
            setattr(self, 'cell_%d' % index, FirstCell(prev, m * f // 2, cur, m * f))
            setattr(self, 'cell_%d' % (index + 1), NormalCell(cur, m * f, 6 * m * f, m * f))
            for j in range(2, 6):
                setattr(self, 'cell_%d' % (index + j), NormalCell(6 * m * f, m * f, 6 * m * f, m * f))
            index += 6

        self.relu = nn.ReLU()
        self.avg_pool = HipAvgPool2d(11, stride=1, padding=0)
        self.dropout = nn.Dropout()
        self.last_linear = nn.Linear(24 * f, num_classes)

    def features(self, input):
        conv0 = self.conv0(input)
        stem0 = self.cell_stem_0(conv0)
        prev, x = stem0, self.cell_stem_1(conv0, stem0)
        for i in range(18):
            if i in (6, 12):
                # the reduction reads (x, prev); the FirstCell after it keeps that same prev (the cell before the reduction's input)
                x = getattr(self, 'reduction_cell_%d' % (i // 6 - 1))(x, prev)
            x, prev = getattr(self, 'cell_%d' % i)(x, prev), x
        return x

    def logits(self, features):
        x = self.avg_pool(F.relu(features))
        x = self.dropout(x.reshape(x.size(0), -1))
        return ops.linear(x, self.last_linear.weight, self.last_linear.bias)

    def forward(self, input, use_logits=False):
        x = self.features(input)
        return self.logits(x) if use_logits else x


def nasnetalarge(num_classes=1000, pretrained=None):
    if pretrained is not None:
        raise RuntimeError("pretrained=%r: this package never downloads weights.  Build the model with pretrained=None and load a "
                           "locally held checkpoint with load_state_dict: the state_dict keys and shapes are the reference's." % (pretrained,))
    return NASNetALarge(num_classes=num_classes)
