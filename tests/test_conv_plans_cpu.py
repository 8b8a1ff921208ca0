"""The conv planners' numbers at the workloads' own shapes, pinned without a device.

tests/test_conv_routes_cpu.py pins the dispatcher over the small geometries of tests/conv_cases.py; this file pins the split-schedule
planners (csrc/split_plan.h and its three users) where they matter: the 3x3 / stride-1 layers of ResNet-34 at 224 x 224 for 5 ... 64
images, every stride-1 3x3 and 1x1 layer of the RetinaNet configuration of bench.py (enumerated from the model), the language model's
decoder Linear and one KTAIL Linear, under the default switches and, on a subset, under each switch that reaches a planner.  One line
per (shape, switches): the predicted times of nnl_debug_conv_plan_times (direct, 1-D, 2-D Winograd, printed with %.17g: near ties are
decided by the last bits) and its return value, the forward / dgrad workspace sizes, nnl_conv2d_wino_preferred for both directions and
the first route note of nnl_conv2d_fwd / _dgrad given the queried workspace and tile counters; for a 3x3 shape also that of
nnl_conv2d_fwd_pre with a prepared filter, which skips the Winograd filter pass, so that the note is the kernel's own and carries the
plan (main_ks, tail_slices, pos_cs).  The table is compared with
tests/golden/conv_plans.txt, recorded from the commit before the planners were merged into one:

    python tests/test_conv_plans_cpu.py tests/golden/conv_plans.txt        # regenerate (on a machine without a GPU)

Every buffer is a fake non-null pointer, so nothing here may run where a launch could succeed (see test_conv_routes_cpu.py).
"""
import ctypes
import difflib
import os
import sys

import pytest
import torch

from test_conv_routes_cpu import SWITCHES, _call

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='fake pointers: only where no launch can happen')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plans.txt')
SWITCH_ROWS = ({'NNL_WINO_BALANCE': '0'}, {'NNL_IGEMM_BALANCE': '0'}, {'NNL_IGEMM_BALANCE': '2'},
               {'NNL_WINO_PLAN_KS': '2', 'NNL_WINO_PLAN_S': '4'}, {'NNL_WINO2_POS': '0'}, {'NNL_WINO2_POS': '2'}, {'NNL_CONV_WINO': '2'},
               {'NNL_CONV_WINO': '3'})


def _out(conv, h):
    return (h + 2 * conv.padding[0] - conv.kernel_size[0]) // conv.stride[0] + 1


def retinanet_shapes(bs=16, sz=512):
    """(N, H, W, C, K, R) of every stride-1 3x3 / pad 1 and 1x1 / pad 0 convolution of bench.py's RetinaNet, in model order, each once"""
    from neuralnetworklibrary_amd.Applications.Vision import ObjectDetectionNet
    with torch.device('meta'):
        net = ObjectDetectionNet(20)
    seen = []

    def visit(conv, h):
        k, p = conv.kernel_size[0], conv.padding[0]
        if conv.stride == (1, 1) and (k, p) in ((3, 1), (1, 0)):
            s = (bs, h, h, conv.in_channels, conv.out_channels, k)
            if s not in seen:
                seen.append(s)
        return _out(conv, h)

    pool = net.layer0[3]
    h = (visit(net.layer0[0], sz) + 2 * pool.padding - pool.kernel_size) // pool.stride + 1                # stem convolution, max pool
    feats = []
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for block in layer:
            if block.downsample is not None:
                visit(block.downsample[0], h)
            for conv in (block.conv1, block.conv2, block.conv3):
                h = visit(conv, h)
        feats.append(h)
    c3, c4, c5 = feats[1:]
    f = net.fpn
    for lateral, smooth, hh in ((f.P5_1, f.P5_2, c5), (f.P4_1, f.P4_2, c4), (f.P3_1, f.P3_2, c3)):
        visit(smooth, visit(lateral, hh))
    p6 = visit(f.P6, c5)
    p7 = visit(f.P7_2, p6)
    for hh in (c3, c4, c5, p6, p7):
        for head in (net.regressor, net.classifier):
            for name in ('conv1', 'conv2', 'conv3', 'conv4', 'output'):
                visit(getattr(head, name), hh)
    return seen


def shape_rows():
    """[(name, (N, H, W, C, K, R), switches)]"""
    resnet = [('rn34-c%d-%dx%d-n%d' % (c, h, h, n), (n, h, h, c, c, 3)) for c, h in ((64, 56), (128, 28), (256, 14), (512, 7))
              for n in (5, 8, 16, 24, 32, 40, 64)]
    retina = [('retina-c%d-%dx%d-k%d-%dx%d' % (s[3], s[1], s[2], s[4], s[5], s[5]), s) for s in retinanet_shapes()]
    linear = [('lm-decoder', (4480, 1, 1, 400, 47343, 1)), ('ktail-linear', (1024, 1, 1, 500, 1000, 1))]
    rows = [(name, s, {}) for name, s in resnet + retina + linear]
    subset = [(name, s) for name, s in resnet if s[0] in (8, 32)]
    subset += [(name, s) for name, s in retina if s[5] == 3 and s[3] == 256 and s[4] == 256 and s[1] in (16, 32, 64)] + linear[1:]
    rows += [(name, s, env) for env in SWITCH_ROWS for name, s in subset]
    return rows


def plan_table():
    from neuralnetworklibrary_amd import _lib
    lib = _lib.lib
    fake = ctypes.c_void_p(0x1000)
    saved = {k: os.environ.get(k) for k in SWITCHES}
    lines = []
    try:
        for name, (N, H, W, Cc, K, R), env in shape_rows():
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(env)
            lib.nnl_reload_env()
            geom = _lib.ConvGeom(N, H, W, Cc, K, R, R, 1, R // 2, H, W)
            g = ctypes.byref(geom)
            times = '-'
            if R == 3:
                t = (ctypes.c_double * 4)()
                mode = lib.nnl_debug_conv_plan_times(N, H, W, Cc, K, t)
                times = '%s mode=%d' % (','.join('%.17g' % v for v in t), mode)
            wf, wd = lib.nnl_conv2d_fwd_workspace_bytes(g), lib.nnl_conv2d_dgrad_workspace_bytes(g)
            fwd = _call(lib, lambda: lib.nnl_conv2d_fwd(fake, fake, fake, fake, g, 0, fake, wf, fake, None, None, None, None))
            pre = dgrad = '-'
            if R == 3:
                pre = _call(lib, lambda: lib.nnl_conv2d_fwd_pre(fake, fake, fake, fake, g, 0, fake, wf, fake, None, None, None, fake, None))
            if K % 4 == 0:
                dgrad = _call(lib, lambda: lib.nnl_conv2d_dgrad(fake, fake, fake, g, None, fake, wd, fake, None))
            lines.append('%s %s t=%s ws fwd=%d dgrad=%d wino fwd=%d dgrad=%d | fwd %s | pre %s | dgrad %s' % (
                name, ','.join('%s=%s' % kv for kv in sorted(env.items())) or 'default', times, wf, wd, lib.nnl_conv2d_wino_preferred(g, 0),
                lib.nnl_conv2d_wino_preferred(g, 1), fwd.split(';')[0], pre.split(';')[0], dgrad.split(';')[0]))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.nnl_reload_env()
    return lines


def test_the_planners_predict_as_the_golden_table_says():
    got = plan_table()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [d for d in difflib.unified_diff(want, got, 'tests/golden/conv_plans.txt', 'this build', n=0, lineterm='')]
    assert not diff, 'the conv planners no longer predict as tests/golden/conv_plans.txt records (%d lines differ):\n%s' % (
        sum(1 for d in diff[2:] if d[0] in '+-'), '\n'.join(diff))
    # the table is worth something only if the split schedules are in it and launches were attempted (each refused with NNL_ERR_HIP, -2)
    assert sum(1 for ln in got if '| fwd -2 ' in ln) == len(got)
    for note in ('balanced<', 'wino1d<', 'wino2d<', ':ksliced', 'pos_cs=', ':ktail'):
        assert any(note in ln for ln in got), note


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    assert not torch.cuda.is_available(), 'generate the table on a machine without a GPU'
    with open(sys.argv[1], 'w') as out:
        out.write('\n'.join(plan_table()) + '\n')
