"""The conv dispatcher's decisions, pinned without a device.

libnnl_hip.so loads on a machine without a GPU, and a launch site records its route note (the kernel, its template arguments and the plan
after `@`: main_ks, tail_slices, splits) before the launch fails.  So for every case of tests/conv_cases.py, under the case's own
switches, this file records the three workspace-size queries and the first route note of nnl_conv2d_fwd / _dgrad in the three calling
modes of the GPU sweep (workspace of the queried size plus tile counters, workspace only, neither) and of nnl_conv2d_wgrad with a
workspace, and compares the whole table with tests/golden/conv_routes.txt.  A planner change shows up as a reviewed diff of that file:

    python tests/test_conv_routes_cpu.py tests/golden/conv_routes.txt        # regenerate (on a machine without a GPU)

Every buffer is a fake non-null pointer, so nothing here may run where a launch could succeed: the module is skipped when a device is
present, and the helper that makes the calls asserts it again.
"""
import ctypes
import difflib
import os
import sys

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='fake pointers: only where no launch can happen')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_routes.txt')
SWITCHES = ('NNL_CONV_WINO', 'NNL_CONV_WINO2', 'NNL_WINO2_POS', 'NNL_WINO_PLAN_KS', 'NNL_WINO_PLAN_S', 'NNL_IGEMM_BALANCE', 'NNL_WGRAD_WINO',
            'NNL_WGRAD_WINO2D', 'NNL_WINO_BALANCE', 'NNL_WINO2_CHUNK')
CALL_MODES = ('ws+cnt', 'ws', 'none')


def _call(lib, call):
    """'<status> <route notes>' of one library call that cannot launch"""
    assert not torch.cuda.is_available(), 'a fake pointer must never reach a device'
    buf = ctypes.create_string_buffer(4096)
    lib.nnl_debug_route_record(1)
    try:
        st = call()
        n = lib.nnl_debug_route_collect(buf, len(buf))
    finally:
        lib.nnl_debug_route_record(0)
    assert n >= 0
    return '%d %s' % (st, buf.value.decode() or '-')


def _by_mode(results):
    """the three calling modes on one line; modes that answer alike are printed once"""
    if len(set(results)) == 1:
        return 'all: ' + results[0]
    return ' | '.join('%s: %s' % mr for mr in zip(CALL_MODES, results))


def route_table():
    from neuralnetworklibrary_amd import _lib
    lib = _lib.lib
    fake = ctypes.c_void_p(0x1000)
    saved = {k: os.environ.get(k) for k in SWITCHES}
    lines = []
    try:
        for c in cc.CASES:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(c.env)
            lib.nnl_reload_env()
            P, Q = cc.PQ(c)
            geom = _lib.ConvGeom(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, P, Q)
            g = ctypes.byref(geom)
            wf, wd, ww = lib.nnl_conv2d_fwd_workspace_bytes(g), lib.nnl_conv2d_dgrad_workspace_bytes(g), lib.nnl_conv2d_wgrad_workspace_bytes(g)
            lines.append('%s %s ws fwd=%d dgrad=%d wgrad=%d' % (cc.case_id(c), ','.join('%s=%s' % kv for kv in sorted(c.env.items())) or 'default',
                                                                  wf, wd, ww))

            def modes(nbytes):
                return [(fake, nbytes, fake), (fake, nbytes, None), (None, 0, None)]
            lines.append('  fwd   ' + _by_mode([_call(lib, lambda: lib.nnl_conv2d_fwd(fake, fake, fake, fake, g, 0, ws, wsb, cnt, None, None, None, None))
                                                for ws, wsb, cnt in modes(wf)]))
            if c.K % 4 != 0:
                continue
            lines.append('  dgrad ' + _by_mode([_call(lib, lambda: lib.nnl_conv2d_dgrad(fake, fake, fake, g, None, ws, wsb, cnt, None))
                                                for ws, wsb, cnt in modes(wd)]))
            lines.append('  wgrad ' + _call(lib, lambda: lib.nnl_conv2d_wgrad(fake, fake, fake, g, fake, ww, None)))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.nnl_reload_env()
    return lines


def test_the_dispatcher_decides_as_the_golden_table_says():
    got = route_table()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [d for d in difflib.unified_diff(want, got, 'tests/golden/conv_routes.txt', 'this build', n=1, lineterm='')]
    assert not diff, 'the conv dispatcher no longer decides as tests/golden/conv_routes.txt records (%d lines differ):\n%s' % (
        sum(1 for d in diff[2:] if d[0] in '+-'), '\n'.join(diff))
    # the table is worth something only if launches were attempted: each is refused with NNL_ERR_HIP (-2) after its note
    assert sum(1 for ln in got if ' -2 ' in ln) >= 3 * len(cc.CASES) - 10


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    assert not torch.cuda.is_available(), 'generate the table on a machine without a GPU'
    with open(sys.argv[1], 'w') as out:
        out.write('\n'.join(route_table()) + '\n')
