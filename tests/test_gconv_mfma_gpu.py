"""Grouped convolution at Cg, Kg in {16, 32} (csrc/gconv_mfma.h through ops.grouped_conv2d) against fp64 with the modes, helpers and tolerance of
tests/test_gconv_gpu.py; every case asserts that the three MFMA routes ran; other shapes, and NNL_GCONV_MFMA=0, keep the direct kernels."""
import ctypes
import os

import pytest
import torch

from test_gconv_gpu import GCase, check_case, gid, make, run_hip

CASES = [
    GCase(2, 3, 16, 16, 5, 9, 3),         # 90 pixels: a full and a partial M tile; odd G: the last two-group block is half empty
    GCase(2, 2, 32, 32, 7, 7, 3),         # two column tiles per group, one group per block
    GCase(2, 2, 16, 32, 6, 11, 3),        # rows and reduction differ: the forward and the dgrad see different tilings
    GCase(2, 2, 32, 16, 6, 11, 3),
    GCase(2, 2, 16, 16, 8, 8, 1),         # R = 1, pad 0
    GCase(3, 2, 16, 16, 33, 31, 3),       # the weight gradient runs in more than one slice
]
SLICED, MFMA_NOTES, DIRECT_NOTES = CASES[5], ('gconv_mfma_fwd<', 'gconv_mfma_dgrad<', 'gconv_mfma_wgrad<'), ('gconv_fwd<', 'gconv_dgrad<', 'gconv_wgrad@')


def routes(call):
    from neuralnetworklibrary_amd._lib import lib
    buf = ctypes.create_string_buffer(16384)
    lib.nnl_debug_route_record(1)                         # (notes are per thread: keep the backward on this one)
    try:
        with torch.autograd.set_multithreading_enabled(False):
            out = call()
        assert lib.nnl_debug_route_collect(buf, len(buf)) >= 0
    finally:
        lib.nnl_debug_route_record(0)
    return out, [n for n in buf.value.decode().split(';') if n]


def assert_routes(notes, want, what):
    assert all(any(n.startswith(w) for n in notes) for w in want), '%s: not all of %s among %s' % (what, want, notes)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['int', 'randn'])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c', CASES, ids=gid)
def test_mfma_grouped_conv_matches_fp64(c, stride, mode):
    if c is SLICED:
        from neuralnetworklibrary_amd._lib import lib
        assert lib.nnl_gconv2d_workspace_bytes(c.N, c.H, c.W, c.G * c.Cg, c.G * c.Kg, c.G, c.R, stride, c.R // 2) > 0, 'one slice only'
    _, notes = routes(lambda: check_case(c, stride, mode))      # y, dx, dw, db against fp64 with bias and the fused ReLU on and off
    assert_routes(notes, MFMA_NOTES, '%s stride %d' % (gid(c), stride))
    assert not any(n.startswith(DIRECT_NOTES) for n in notes), notes


@pytest.mark.gpu
def test_selection_by_shape_and_switch():
    from neuralnetworklibrary_amd._lib import lib
    for c in (GCase(2, 2, 16, 8, 8, 8, 3), GCase(2, 2, 8, 16, 8, 8, 3)):
        _, notes = routes(lambda: run_hip(c, 1, make(c, 1, 'int'), False, False))
        assert_routes(notes, DIRECT_NOTES, gid(c))
        assert not any('mfma' in n for n in notes), notes
    old = os.environ.get('NNL_GCONV_MFMA')
    try:
        os.environ['NNL_GCONV_MFMA'] = '0'
        lib.nnl_reload_env()
        _, notes = routes(lambda: run_hip(CASES[0], 1, make(CASES[0], 1, 'int'), False, False))
        assert_routes(notes, DIRECT_NOTES, 'NNL_GCONV_MFMA=0')
        assert not any('mfma' in n for n in notes), notes
    finally:
        if old is None:
            del os.environ['NNL_GCONV_MFMA']
        else:
            os.environ['NNL_GCONV_MFMA'] = old
        lib.nnl_reload_env()


@pytest.mark.gpu
def test_mfma_repeat_calls_give_the_same_bits():
    for c, stride in ((SLICED, 1), (CASES[2], 2)):
        d = make(c, stride, 'randn')
        a, b = run_hip(c, stride, d, True, True), run_hip(c, stride, d, True, True)
        for k in ('y', 'dx', 'dw', 'db'):
            assert torch.equal(a[k], b[k]), '%s stride %d: %s differs between two calls' % (gid(c), stride, k)
