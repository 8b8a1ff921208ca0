"""Host-side bookkeeping of the prepared conv filters (ops._Filters, ops.filter_window): which Winograd modes a weight's calls record
and when, and that the window is closed however its body ends.  No GPU: the planner behind nnl_conv2d_wino_preferred is host code,
the weights are fake addresses and nothing is launched.  The geometry is the one test_conv_planner_cpu.py::
test_modes_the_graph_rebuild_test_relies_on pins: 3x3, 128 -> 128 at 28 x 28 takes mode 2 / 1 / 0 at 32 / 24 / 5 images, both directions."""
import os

import pytest
import torch
import torch.nn as nn


@pytest.fixture()
def ops():
    from neuralnetworklibrary_amd import _lib, ops
    saved = {k: os.environ.pop(k, None) for k in ('NNL_CONV_WINO', 'NNL_CONV_WINO2')}
    _lib.lib.nnl_reload_env()
    yield ops
    ops.finish_backward()
    os.environ.update({k: v for k, v in saved.items() if v is not None})
    _lib.lib.nnl_reload_env()


def _g(ops, N):
    return ops._geom(N, 28, 28, 128, 128, 3, 3, 1, 1)


@pytest.mark.parametrize('which', [0, 1], ids=['forward', 'dgrad'])
def test_modes_are_those_of_the_last_step_inside_the_window(ops, which):
    model, A, B = nn.Sequential(), 0x1000, 0x2000              # no conv modules: the prepare calls launch nothing
    f = ops._filters(model)
    ops.prepare_forward(model)
    assert f.wino(A, which, _g(ops, 32)) is None
    assert f.recorded(A, which) == {2}
    ops.finish_backward()
    assert f.wino(A, which, _g(ops, 24)) is None               # evaluation, no_grad, a bare backward: outside the window
    assert f.recorded(A, which) == {2}, 'a call outside the window was recorded'
    ops.prepare_forward(model)
    f.wino(A, which, _g(ops, 24))
    assert f.recorded(A, which) == {1}, "the first call of a new step did not forget the old step's mode"
    assert not f.recorded(A, 1 - which), 'the other direction was recorded'
    ops.finish_backward()
    ops.prepare_forward(model)
    f.wino(A, which, _g(ops, 32))
    f.wino(A, which, _g(ops, 24))
    assert f.recorded(A, which) == {1, 2}                      # a weight shared between geometries needs both layouts
    assert f.wino(0, which, _g(ops, 32)) is None               # key 0: a channel-padded dgrad
    assert 0 not in f.modes
    assert f.wino(B, which, _g(ops, 5)) is None
    assert B not in f.modes, 'a weight that never took a Winograd kernel got an entry'
    ops.finish_backward()
    ops.prepare_forward(model)
    f.wino(A, which, _g(ops, 5))                               # a known weight whose call now takes the direct kernel
    assert f.recorded(A, which) == set()


def test_prepared_filter_is_handed_out_only_inside_the_window_and_in_the_calls_layout(ops):
    model, A = nn.Sequential(), 0x1000
    f = ops._filters(model)
    u2, u1 = torch.empty(128 * 16 * 128), torch.empty(128 * 12 * 128)
    for which in (0, 1):
        ops.prepare_backward(model)                            # opens the window itself
        assert ops._OPEN is f
        f.u[which][(A, 2)], f.u[which][(A, 1)] = u2, u1
        assert ops.prepared_filter_counts()[which] == 2
        assert f.wino(A, which, _g(ops, 32)) is u2 and f.wino(A, which, _g(ops, 24)) is u1
        assert (ops._OPEN or ops._CLOSED).wino(A, which, _g(ops, 32)) is u2      # as the convolutions ask
        assert f.wino(A, which, _g(ops, 5)) is None
        assert f.wino(0, which, _g(ops, 32)) is None
        f.u[which][(A, 2)] = u1                                # a buffer of another layout's size is not handed over
        assert f.wino(A, which, _g(ops, 32)) is None
        ops.finish_backward()
        assert ops._OPEN is None and ops.prepared_filter_counts() == (0, 0, 0) and not f.u[which]
        f.u[which][(A, 2)] = u2                                # views from before, however they got there: not through a closed window
        assert f.wino(A, which, _g(ops, 32)) is None
        assert (ops._OPEN or ops._CLOSED).wino(A, which, _g(ops, 32)) is None
        f.u[which].clear()


def test_opening_one_models_window_closes_anothers(ops):
    a, b = nn.Sequential(), nn.Sequential()
    ops.prepare_forward(a)
    ops._filters(a).wt[0x1000] = torch.empty(1)
    ops.prepare_forward(b)
    assert ops._OPEN is ops._filters(b) and not ops._filters(a).wt


def _cpu_net():
    from neuralnetworklibrary_amd.Applications.VisionModels.retinanet import HipConv2d
    return nn.Sequential(HipConv2d(8, 8, 3, padding=1), nn.ReLU(), HipConv2d(8, 8, 3, padding=1))


def _closed(ops):
    return ops._OPEN is None and ops.prepared_filter_counts() == (0, 0, 0)


def test_filter_window_closes_when_the_body_raises(ops):
    net = _cpu_net()
    with pytest.raises(KeyError, match='forward'):
        with ops.filter_window(net):
            assert ops._OPEN is ops._filters(net)
            raise KeyError('forward')
    assert _closed(ops), 'an exception before the backward left the window open'

    class Loss:
        @staticmethod
        def backward():
            assert ops._OPEN is ops._filters(net)
            raise KeyError('backward')
    with pytest.raises(KeyError, match='backward'):
        with ops.filter_window(net) as backward:
            backward(Loss)
    assert _closed(ops), 'an exception inside the backward left the window open'
    with pytest.raises(KeyError, match='after'):
        with ops.filter_window(net) as backward:
            backward(torch.zeros((), requires_grad=True) * 2)
            raise KeyError('after')
    assert _closed(ops), 'an exception after the backward left the window open'
    with ops.filter_window(net):
        assert ops._OPEN is ops._filters(net)
    assert _closed(ops)
    assert ops._filters(net).modes == {} and ops.prepared_batches(net) == ()      # nothing was launched or recorded
    assert ops._CLOSED.modes == {} and ops._CLOSED.step == 0 and not ops._CLOSED.wt_padded      # the stand-in of "no window" is never written


def test_batch_tables_and_views(ops):
    """the one builder behind both *_multi launches, on CPU tensors (nothing is launched): views tile the flat buffer in item order,
    every descriptor row names its source, its view and its first block, the block table maps each block to its item, and a model that
    carries such a batch can still be deep-copied (Learner's SWA copy, Core.combine_models)."""
    import copy
    import numpy as np
    ws = [torch.empty(40, 36, 3, 3), torch.empty(8, 64, 1, 1)]
    b = ops._wt_batch('key', ws)
    assert b.key == 'key' and b.flat.numel() == sum(w.numel() for w in ws) and b.extra == (float(b.flat.numel()),)
    tiles = [9 * 2 * 2, 1 * 1 * 2]
    assert b.n_blocks == sum(tiles) and b.block_desc.tolist() == [0] * tiles[0] + [1] * tiles[1]
    assert [tuple(b.views[w.data_ptr()].shape) for w in ws] == [(36, 3, 3, 40), (64, 1, 1, 8)]
    assert b.views[ws[1].data_ptr()].data_ptr() == b.flat.data_ptr() + 4 * ws[0].numel()
    rows = b.desc.numpy().view(np.dtype([('w', '<u8'), ('wt', '<u8'), ('K', '<i4'), ('RS', '<i4'), ('C', '<i4'), ('first', '<i4')]))
    assert rows.tolist() == [(ws[0].data_ptr(), b.views[ws[0].data_ptr()].data_ptr(), 40, 9, 36, 0),
                             (ws[1].data_ptr(), b.views[ws[1].data_ptr()].data_ptr(), 8, 1, 64, tiles[0])]
    t = torch.empty(40, 3, 3, 36)
    u = ops._wino_batch('k2', [(7, t, 0, 1), (7, t, 0, 2), (9, t, 1, 2)])
    n1, n2 = 40 * 12 * 36, 40 * 16 * 36
    blocks = [(40 * 3 * 36 + 255) // 256, (40 * 36 + 255) // 256, (40 * 36 + 255) // 256]
    assert [u.views[k].numel() for k in ((7, 1), (7, 2), (9, 2))] == [n1, n2, n2] and u.flat.numel() == n1 + 2 * n2
    assert u.n_blocks == sum(blocks) and u.block_desc.tolist() == [0] * blocks[0] + [1] * blocks[1] + [2] * blocks[2]
    rows = u.desc.numpy().view(np.dtype([('src', '<u8'), ('dst', '<u8'), ('rows', '<i4'), ('ch', '<i4'), ('flip', '<i4'), ('first', '<i4'),
                                         ('two_d', '<i4'), ('reserved', '<i4')]))
    base = u.flat.data_ptr()
    assert rows.tolist() == [(t.data_ptr(), base, 40, 36, 0, 0, 0, 0), (t.data_ptr(), base + 4 * n1, 40, 36, 0, blocks[0], 1, 0),
                             (t.data_ptr(), base + 4 * (n1 + n2), 40, 36, 1, blocks[0] + blocks[1], 1, 0)]
    net = _cpu_net()
    ops._filters(net).batches.update(wt=b, fwd=u)
    twin = copy.deepcopy(net)
    assert twin._nnl_filters is not net._nnl_filters and twin._nnl_filters.mods == [twin[0], twin[2]]
