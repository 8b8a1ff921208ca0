"""Host-side logic of the 3x3 / stride 1 convolution dispatcher (csrc/conv2d.hip: wino_mode; wino.hip / wino2.hip planners): no GPU
needed — the planners are plain C++ behind the C ABI.  Checks that the three predictions are finite and positive over a grid of
shapes, that the kernel choice follows the documented switches, and that the workspace the size query returns covers the kernel
the launch will take (the launch falls back to the direct kernel when it does not: a silent slow path)."""
import ctypes as C
import os

import pytest


@pytest.fixture()
def lib():
    from neuralnetworklibrary_amd import _lib
    saved = {k: os.environ.get(k) for k in ('NNL_CONV_WINO', 'NNL_CONV_WINO2')}
    yield _lib.lib
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    _lib.lib.nnl_reload_env()


def _geom(N, H, C_, K):
    from neuralnetworklibrary_amd import ops
    return ops._geom(N, H, H, C_, K, 3, 3, 1, 1)


SHAPES = [(N, H, C_, K) for N in (1, 8, 16, 64, 128) for H in (2, 7, 14, 28, 56, 64) for C_, K in ((16, 8), (64, 64), (128, 128), (256, 256), (512, 512), (256, 36))
          if N * H * H * max(C_, K) * 4 < 2 ** 31]


def test_predictions_finite_and_modes_consistent(lib):
    out = (C.c_double * 4)()
    seen = set()
    for N, H, C_, K in SHAPES:
        os.environ.pop('NNL_CONV_WINO', None); os.environ.pop('NNL_CONV_WINO2', None); lib.nnl_reload_env()
        mode = lib.nnl_debug_conv_plan_times(N, H, H, C_, K, out)
        assert mode in (0, 1, 2)
        assert out[3] == -1.0                           # (the slot of round 4's spatially staged kernel: removed in round 5)
        assert all(0.0 < out[i] < 1e7 for i in range(3)), (N, H, C_, K, list(out))
        g = _geom(N, H, C_, K)
        assert lib.nnl_conv2d_wino_preferred(g, 0) == mode
        seen.add(mode)
        t_d, t_w = out[0] + 6.0, out[1] + 9.0 + 21.0 * C_ * K * 4.0 / 4.0e6
        if mode == 2:
            assert lib.nnl_conv2d_fwd_workspace_bytes(g) >= lib.nnl_debug_conv_wino2_workspace_bytes(N, H, H, C_, K)
            # the documented 10 % margin: over the 1-D prediction where that beats the direct kernel, else (the position-split plan of
            # the small grids, round 5) over the direct kernel's
            assert out[2] < 0.9 * (t_w if t_w < 0.97 * t_d else t_d) + 1e-9
            os.environ['NNL_CONV_WINO2'] = '0'; lib.nnl_reload_env()
            assert lib.nnl_conv2d_wino_preferred(g, 0) == (1 if t_w < 0.97 * t_d else 0)
            os.environ.pop('NNL_CONV_WINO2'); lib.nnl_reload_env()
        elif mode == 1:
            assert lib.nnl_conv2d_fwd_workspace_bytes(g) >= lib.nnl_debug_conv_wino_workspace_bytes(N, H, H, C_, K)
        os.environ['NNL_CONV_WINO'] = '0'; lib.nnl_reload_env()
        assert lib.nnl_conv2d_wino_preferred(g, 0) == 0
        os.environ['NNL_CONV_WINO'] = '2'; lib.nnl_reload_env()
        assert lib.nnl_conv2d_wino_preferred(g, 0) == 1
        os.environ['NNL_CONV_WINO'] = '3'; lib.nnl_reload_env()
        assert lib.nnl_conv2d_wino_preferred(g, 0) == (2 if H >= 2 else 1)
        assert lib.nnl_conv2d_fwd_workspace_bytes(g) >= lib.nnl_debug_conv_wino2_workspace_bytes(N, H, H, C_, K)
    os.environ.pop('NNL_CONV_WINO', None); lib.nnl_reload_env()
    assert seen >= {0, 1, 2}, 'the shape grid no longer reaches the direct, 1-D and 2-D kernels: %r' % (seen,)


def test_headline_and_small_batch_choices(lib):
    """ResNet-34 at 64 images: every 3x3 stride-1 stage on the 2-D kernel; at 8 images every stage is either on the direct kernel or on the 2-D
    kernel's position-split plan (round 5: profiles/r5_wino2_pos_*.log) — never on a k-sliced 2-D plan or the 1-D kernel, which measured slower
    there (profiles/README.md: r3_wino2d_ab_bs64.log, r3_wino_bs8.log)."""
    os.environ.pop('NNL_CONV_WINO', None); os.environ.pop('NNL_CONV_WINO2', None); lib.nnl_reload_env()
    out = (C.c_double * 4)()
    assert [lib.nnl_debug_conv_plan_times(64, H, H, C_, C_, out) for C_, H in ((64, 56), (128, 28), (256, 14), (512, 7))] == [2, 2, 2, 2]
    small = [lib.nnl_debug_conv_plan_times(8, H, H, C_, C_, out) for C_, H in ((128, 28), (256, 14), (512, 7))]
    assert all(m in (0, 2) for m in small), small
    os.environ['NNL_WINO2_POS'] = '0'; lib.nnl_reload_env()
    assert [lib.nnl_debug_conv_plan_times(8, H, H, C_, C_, out) for C_, H in ((128, 28), (256, 14), (512, 7))] == [0, 0, 0]
    os.environ.pop('NNL_WINO2_POS'); lib.nnl_reload_env()
    # dgrad direction: geometry with K != C goes through the same rule with the roles swapped
    from neuralnetworklibrary_amd import ops
    g = ops._geom(64, 56, 56, 64, 128, 3, 3, 1, 1)
    assert lib.nnl_conv2d_wino_preferred(g, 1) == lib.nnl_debug_conv_plan_times(64, 56, 56, 128, 64, out)


def test_modes_the_graph_rebuild_test_relies_on(lib):
    """tests/test_graph_gpu.py::test_replay_across_batch_sizes_keeps_captured_filter_buffers needs a 3x3 128 -> 128 convolution at 28 x 28
    to take a DIFFERENT kernel at each of its three batch sizes: the 2-D Winograd kernel at 32 images (the first captured graph), the
    1-D kernel at 24 (the ragged step whose eager warm-up rebuilds the prepared-filter batch) and the direct kernel at 5 (the evaluation
    pass) — in the forward and in the dgrad direction."""
    from neuralnetworklibrary_amd import ops
    os.environ.pop('NNL_CONV_WINO', None); os.environ.pop('NNL_CONV_WINO2', None); lib.nnl_reload_env()
    for which in (0, 1):
        got = {N: int(lib.nnl_conv2d_wino_preferred(ops._geom(N, 28, 28, 128, 128, 3, 3, 1, 1), which)) for N in (32, 24, 5)}
        assert got == {32: 2, 24: 1, 5: 0}, (
            'the planner changed its choice for 3x3 128 -> 128 at 28 x 28 (which=%d): %r; test_graph_gpu.py::'
            'test_replay_across_batch_sizes_keeps_captured_filter_buffers needs new batch sizes that still reach the 2-D, 1-D and direct '
            'kernels (or it no longer exercises the rebuild of the prepared-filter batch)' % (which, got))
