"""Detection test-time augmentation: DetectionBatches.with_transform, the undo rows, the merge kernel (ops.tta_bbox_merge,
csrc/detect.hip), BBoxPredictor.survivors_on_device, ImageLearner.TTA_bbox and golden G19 (tools/gen_golden_tta_bbox.py: the real
reference's nms on hand-made, undone and concatenated per-pass survivor lists).

The module carries a numpy RESTATEMENT of Vision.py:2092-2112 on fp32 tables (`r_merge`): per (image, pass) the four array
statements of the undo, one fp32 operation at a time, and the concatenation in pass order.  A CPU test pins it to the generator's own
four lines (Python ints and floats against float32 arrays, as the reference has them) on G19's inputs; the GPU tests compare the kernel
with it bit for bit."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import reference_detect, synth
from tools.gen_golden_tta_bbox import SETTINGS, concatenate

from neuralnetworklibrary_amd import device_data, ops
from neuralnetworklibrary_amd.Applications import Vision as V
from neuralnetworklibrary_amd.Applications.VisionModels import retinanet as RN

DEV = 'cuda:0'
P = 5


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def r_undo(b, u):
    "Vision.py:2092-2096 on a float32 [n, 4] array with the row's fp32 values: every operation is one fp32 array operation"
    b = np.array([b[:, 0] - u['col_jit'], b[:, 1] - u['row_jit'], b[:, 2] - u['col_jit'], b[:, 3] - u['row_jit']]).T
    b = u['inv'] * b
    if u['flip']:
        b = np.array([u['cols'] - b[:, 2], b[:, 1], u['cols'] - b[:, 0], b[:, 3]]).T
    return b.reshape(-1, 4)


def r_merge(boxes, classes, scores, counts, undo):
    """what ops.tta_bbox_merge returns, as numpy: candidates compacted per image in pass order, then slot order; order = position; the
    slots past the count hold box 0, class -1, score 0"""
    L, passes, M = classes.shape
    cap = passes * M
    cb, cc = np.zeros((L, cap, 4), np.float32), np.full((L, cap), -1, np.int32)
    cs, co, cn = np.zeros((L, cap), np.float32), np.tile(np.arange(cap, dtype=np.int32), (L, 1)), np.zeros(L, np.int32)
    for l in range(L):
        d = 0
        for p in range(passes):
            n = int(counts[l, p])
            got = r_undo(boxes[l, p, :n], undo[l, p])
            assert got.dtype == np.float32
            cb[l, d:d + n], cc[l, d:d + n], cs[l, d:d + n] = got, classes[l, p, :n], scores[l, p, :n]
            d += n
        cn[l] = d
    return cb, cc, cs, co, cn


def g19_undo(g):
    "the TTA_UNDO rows [L, P] of G19's inputs through ops.tta_undo_rows, pass by pass as TTA_bbox builds them"
    L = len(g['in.cols'])
    rows = [ops.tta_undo_rows([dict(row_jit=int(g['in.row_jit'][l, p]), col_jit=int(g['in.col_jit'][l, p]), rand_scale=float(g['in.rand_scale'][l, p]),
                                    flip=int(g['in.flip'][l, p])) for l in range(L)], g['in.scale'], g['in.cols']) for p in range(P)]
    return np.stack(rows, axis=1)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

SHAPES = [(13, 17), (17, 13), (16, 16), (9, 31)]
SCALES = [0.61, 1.3, 1.0, 1.7]


def _images(seed=3, shapes=SHAPES, scales=SCALES):
    rs = np.random.RandomState(seed)
    return [{'img': rs.randint(0, 256, (H, W, 3)).astype(np.uint8), 'target': [(np.array([1., 2., W - 2., H - 1.]), i % 3)],
             'scale': scales[i % len(scales)], 'aspect_ratio': W / H} for i, (H, W) in enumerate(shapes)]


@pytest.fixture
def stub_kernel(monkeypatch):
    "ops.detect_aug replaced by a recorder: [(parameter rows, dict of the batch values)] per call, zeros out"
    calls = []

    def fake(arena, desc, image_mean, box_arena, cat_arena, params, Hp, Wp, N, row_jit, col_jit, rand_scale, stats=None):
        rows = params.numpy().view(ops.DETECT_AUG_PARAM).reshape(-1).copy()
        calls.append((rows, dict(Hp=Hp, Wp=Wp, N=N, row_jit=row_jit, col_jit=col_jit, rand_scale=rand_scale)))
        return torch.zeros(len(rows), Hp, Wp, 3), -torch.ones(len(rows), N, 4), -torch.ones(len(rows), N, dtype=torch.int64)
    monkeypatch.setattr(ops, 'detect_aug', fake)
    return calls


def _val_loader(tfm=None, seed=5, bs=1):
    tfm = tfm or V.get_transforms_bbox('SideOn')[0]
    return device_data.DetectionBatches(V.ImageDataset('', _images(), tfm, 'bbox', 'val'), bs, grouped=False, seed=seed, device='cpu')


def test_with_transform_shares_the_arenas_and_remembers_its_draws(stub_kernel):
    val = _val_loader()
    assert val.last_draws is None
    tfm = V.TransformBBox('SideOn', jitter=7, scale_range=[0.7, 1.3])
    view = val.with_transform(tfm, bs=1, seed=9)
    assert view is not val and view.transform is tfm and val.transform is val.ds.transform
    for name in ('arena', 'desc', 'image_mean', 'box_arena', 'cat_arena'):
        assert getattr(view, name).data_ptr() == getattr(val, name).data_ptr(), name
    assert (view.bs, view.seed, view.grouped, view.rank, view.world, view.epoch, view.explicit_params) == (1, 9, False, 0, 1, 0, None)
    assert len(view) == 4 and view.last_draws == [None] * 4
    batches = list(view)
    assert [rows['image'].tolist() for rows, _ in stub_kernel] == [[0], [1], [2], [3]]           # dataset order, batch size 1
    assert all(x.shape[0] == 1 for x, _ in batches)
    rs = np.random.RandomState(9)
    want = [tfm.sample(rs) for _ in range(4)]
    assert [d['sample'] for d in view.last_draws] == want
    for (rows, v), d, w in zip(stub_kernel, view.last_draws, want):                              # every image is its minibatch's first
        assert (d['row_jit'], d['col_jit'], d['rand_scale'], d['flip']) == (w['row_jit'], w['col_jit'], w['rand_scale'], w['flip'])
        assert (v['row_jit'], v['col_jit'], v['rand_scale']) == (w['row_jit'], w['col_jit'], w['rand_scale'])
        assert int(bool(rows['flags'][0] & ops.IMAGE_AUG_FLIP)) == d['flip']
    assert {d['flip'] for d in view.last_draws} == {0, 1}
    assert view.epoch == 1 and val.epoch == 0 and val.last_draws is None
    # defaults: the loader's own batch size and seed; a wider batch: its first sample's values for every image of it
    del stub_kernel[:]
    wide = _val_loader(bs=3).with_transform(tfm)
    assert (wide.bs, wide.seed) == (3, 5) and [g.tolist() for g in wide.groups] == [[0, 1, 2], [3]]
    list(wide)
    first = wide.last_draws[0]['sample']
    assert all((wide.last_draws[i]['row_jit'], wide.last_draws[i]['rand_scale']) == (first['row_jit'], first['rand_scale']) for i in range(3))
    # a view of a sharded, grouped training loader is rank-local and covers the full set in dataset order
    train = device_data.DetectionBatches(V.ImageDataset('', _images(), tfm, 'bbox', 'train'), 2, grouped=True, seed=1, rank=1, world=2, device='cpu')
    tv = train.with_transform(V.get_transforms_bbox('SideOn')[0], bs=1)
    assert (tv.rank, tv.world, tv.grouped) == (0, 1, False) and [g.tolist() for g in tv.groups] == [[0], [1], [2], [3]]
    assert [g.tolist() for g in train.groups] != [g.tolist() for g in tv.groups] and train.last_draws is None


def test_undo_rows_equal_the_numpy_restatement(stub_kernel):
    val = _val_loader()
    cols = [W for _, W in val.shapes]
    assert ops.TTA_UNDO.itemsize == 20 and 'tta_bbox_merge' in ops.__all__
    for tfm_type in ('SideOn', 'Basic'):
        tfm = V.TransformBBox(tfm_type, None, None, jitter=7, scale_range=[0.7, 1.3])
        view = val.with_transform(tfm, bs=1, seed=11)
        list(view)
        rows = ops.tta_undo_rows(view.last_draws, val.scales, cols)
        rs = np.random.RandomState(11)
        draws = [tfm.sample(rs) for _ in range(4)]
        assert {d['flip'] for d in draws} == {0, 1} and rows.dtype == ops.TTA_UNDO and rows.shape == (4,)
        for i, d in enumerate(draws):
            quotient = 1.0 / (d['rand_scale'] * SCALES[i])                                        # float64
            assert isinstance(quotient, float) and rows['inv'][i] == np.float32(quotient) and rows['inv'].dtype == np.float32
            assert float(rows['inv'][i]) != quotient or quotient == 1.0                          # it WAS rounded
            assert (rows['col_jit'][i], rows['row_jit'][i], rows['cols'][i]) == (d['col_jit'], d['row_jit'], SHAPES[i][1])
            assert rows['flip'][i] == (d['flip'] if tfm_type == 'SideOn' else 0)                  # 'Basic' never mirrors: nothing to undo
    # chosen draws: inv against a float32 array is what numpy makes of the Python float
    rows = ops.tta_undo_rows([dict(row_jit=7, col_jit=0, rand_scale=0.83, flip=1), dict(row_jit=0, col_jit=7, rand_scale=1.17, flip=0)], [0.61, 1.3], [96, 64])
    b = np.array([[10.25, 20.5, 30.75, 41.125]], np.float32)
    assert np.array_equal(rows['inv'][0] * b, (1 / (0.83 * 0.61)) * b) and np.array_equal(rows['inv'][1] * b, (1 / (1.17 * 1.3)) * b)
    assert rows.tolist() == [(0.0, 7.0, float(np.float32(1 / (0.83 * 0.61))), 96.0, 1), (7.0, 0.0, float(np.float32(1 / (1.17 * 1.3))), 64.0, 0)]


def test_restatement_is_the_generators_numpy_on_g19():
    g = load_golden('g19_tta_bbox')
    cb, cc, cs, co, cn = r_merge(g['in.boxes'], g['in.classes'], g['in.scores'], g['in.counts'], g19_undo(g))
    assert cn.tolist() == [14, 5, 0] and (g['in.counts'][2] == 0).all() and g['in.counts'].max() == 4 and g['in.flip'].any()
    for l in range(3):
        b, c, s = concatenate(g, l)
        n = cn[l]
        assert np.array_equal(cb[l, :n], b) and np.array_equal(cc[l, :n], c) and np.array_equal(cs[l, :n], s)
        assert np.array_equal(b, g['cat%d.boxes' % l]) and np.array_equal(s, g['cat%d.scores' % l])


def test_oracle_nms_matches_g19():
    "the verified oracle (oracle.reference_detect.nms) over G19's concatenations gives the real reference's survivors, both settings"
    g = load_golden('g19_tta_bbox')
    for l in range(3):
        b, c, s = g['cat%d.boxes' % l], g['cat%d.classes' % l], g['cat%d.scores' % l]
        assert len(np.unique(s)) == len(s)
        for name, kw in SETTINGS.items():
            B, C, S = reference_detect.nms(b, c, s, **kw)
            assert np.array_equal(np.array(B, np.float32).reshape(-1, 4), g['%s.img%d.boxes' % (name, l)]), (name, l)
            assert [int(v) for v in C] == g['%s.img%d.classes' % (name, l)].tolist() and np.array_equal(np.array(S, np.float32), g['%s.img%d.scores' % (name, l)])
    assert sum(len(g['rel_dup.img%d.scores' % l]) for l in range(3)) < sum(len(g['default.img%d.scores' % l]) for l in range(3))
    assert {0, 1} <= set(g['default.img0.classes'].tolist()) and len(g['default.img2.scores']) == 0


def test_tta_bbox_merge_c_entry_reports_bad_arguments_and_op_refuses_cpu_tensors():
    from neuralnetworklibrary_amd._lib import NnlError, lib
    assert lib.nnl_tta_bbox_merge(None, None, None, None, None, 3, 5, 4, None, None, None, None, None, None, None) == -1
    assert b'tta_bbox_merge' in lib.nnl_last_error() and b'null' in lib.nnl_last_error()
    one = torch.zeros(64, dtype=torch.float64)                                               # any non-null host address: validation reads nothing
    p = one.data_ptr()
    for L, passes, M in [(0, 5, 4), (-1, 5, 4), (3, 0, 4), (3, 65, 4), (3, 5, 0), (3, 5, -2), (3, 64, 1 << 15), (1 << 31, 5, 4)]:
        assert lib.nnl_tta_bbox_merge(p, p, p, p, p, L, passes, M, p, p, p, p, p, None, None) == -1, (L, passes, M)
        assert b'tta_bbox_merge' in lib.nnl_last_error() and b'sizes' in lib.nnl_last_error()
    for window in [(-1., 0., 96., 64.), (0., -1., 96., 64.), (96., 0., 96., 64.), (0., 64., 96., 10.)]:
        assert lib.nnl_bbox_decode_window(p, p, p, 1, 9, 3, p, p, 0.5, *window, p, p, p, p, p, None) == -1 and b'window' in lib.nnl_last_error()
    assert lib.nnl_bbox_decode_window(None, p, p, 1, 9, 3, p, p, 0.5, 0., 0., 96., 64., p, p, p, p, p, None) == -1 and b'null' in lib.nnl_last_error()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    with pytest.raises(NnlError):
        ops.tta_bbox_merge(z(3, 5, 4, 4), z(3, 5, 4, dt=torch.int32), z(3, 5, 4), z(3, 5, dt=torch.int32), z(3, 5, 20, dt=torch.uint8))


def test_tta_bbox_rejections(stub_kernel):
    tfms = V.get_transforms_bbox('SideOn')
    learner = object.__new__(V.ImageLearner)
    learner.data = types.SimpleNamespace(val_dl=_val_loader(), test_dl=None)
    learner.target_type = 'single_label'
    with pytest.raises(ValueError, match='bbox'):
        learner.TTA_bbox('val', tfms)
    learner.target_type = 'bbox'
    with pytest.raises(ValueError, match='ds_type'):
        learner.TTA_bbox('train', tfms)
    with pytest.raises(ValueError, match='test set'):
        learner.TTA_bbox('test', tfms)
    for bad in (tfms[0], [tfms[0]], tfms + [tfms[1]], [tfms[0], V.get_transforms('SideOn', 8)[1]], [tfms[0], None]):
        with pytest.raises(ValueError, match='TransformBBox'):
            learner.TTA_bbox('val', bad)
    assert stub_kernel == []                                                                 # refused before any pass ran


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------------------------

def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _undo_bytes(undo):
    return torch.from_numpy(np.ascontiguousarray(undo).view(np.uint8).reshape(undo.shape + (ops.TTA_UNDO.itemsize,))).to(DEV)


def _kernel_case(M):
    """L = 3, P = 5: counts 0, 1, M - 1 and M, image 2 empty in every pass; jitter 0 and 7; inv from 0.83 * 0.61 and 1.17 * 1.3;
    mirror on and off within one image; coordinates that use the whole fp32 mantissa"""
    rs = np.random.RandomState(190 + M)
    counts = np.array([[M, M - 1, 1, M, M], [1, M, 0, 0, M], [0, 0, 0, 0, 0]], np.int32)
    boxes = rs.uniform(0, 200, (3, P, M, 4)).astype(np.float32)
    boxes[..., 2:] += boxes[..., :2]
    classes, scores = rs.randint(0, 3, (3, P, M)).astype(np.int32), np.sort(rs.uniform(0.05, 1, (3, P, M)).astype(np.float32), axis=2)[:, :, ::-1].copy()
    draws = [[dict(row_jit=(0, 7)[(l + p) % 2], col_jit=(7, 0, 3)[p % 3], rand_scale=(0.83, 1.17)[p % 2], flip=(p + l) % 2) for l in range(3)] for p in range(P)]
    undo = np.stack([ops.tta_undo_rows(draws[p], [0.61, 1.3, 0.61], [96, 64, 80]) for p in range(P)], axis=1)
    assert undo.shape == (3, P) and {0, 1} == set(undo['flip'][0].tolist()) and {0.0, 7.0} <= set(undo['row_jit'].reshape(-1).tolist())
    assert np.float32(1 / (0.83 * 0.61)) in undo['inv'] and np.float32(1 / (1.17 * 1.3)) in undo['inv']
    return boxes, classes, scores, counts, undo


@pytest.mark.gpu
@pytest.mark.parametrize('M', [4, 20])
def test_gpu_merge_kernel_is_the_restatement_bit_for_bit(M):
    "M = 20, the default max_boxes: P M = 100 positions, the prefix and the moves cross a wave's 64 lanes"
    boxes, classes, scores, counts, undo = _kernel_case(M)
    want = r_merge(boxes, classes, scores, counts, undo)
    assert want[4].tolist() == [counts[0].sum(), counts[1].sum(), 0] and want[4].max() > 64 * (M == 20)
    args = _dev(boxes, classes, scores, counts) + [_undo_bytes(undo)]
    got = [t.cpu().numpy() for t in ops.tta_bbox_merge(*args)]
    again = [t.cpu().numpy() for t in ops.tta_bbox_merge(*args)]
    for name, a, b, w in zip(('boxes', 'classes', 'scores', 'order', 'count'), got, again, want):
        assert a.dtype == w.dtype and a.shape == w.shape, name
        assert np.array_equal(a.view(np.int32), w.view(np.int32)), name                          # bit for bit, filler included
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name + ': two runs differ'
    ops.raise_if_index_error()                                                                   # no count was out of range


@pytest.mark.gpu
def test_gpu_merge_kernel_flags_a_count_above_m_and_does_not_follow_it():
    boxes, classes, scores, counts, undo = _kernel_case(4)
    counts[0, 1], counts[1, 2] = 5, -1
    args = _dev(boxes, classes, scores, counts) + [_undo_bytes(undo)]
    got = [t.cpu().numpy() for t in ops.tta_bbox_merge(*args)]
    counts[0, 1], counts[1, 2] = 0, 0                                                            # those passes contribute nothing
    want = r_merge(boxes, classes, scores, counts, undo)
    assert all(np.array_equal(a.view(np.int32), w.view(np.int32)) for a, w in zip(got, want))
    with pytest.raises(IndexError):
        ops.raise_if_index_error()
    ops.raise_if_index_error()                                                                   # the flag was cleared


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SETTINGS))
def test_gpu_merge_and_batched_nms_match_g19(name):
    g, kw = load_golden('g19_tta_bbox'), SETTINGS[name]
    args = _dev(g['in.boxes'], g['in.classes'], g['in.scores'], g['in.counts']) + [_undo_bytes(g19_undo(g))]
    cand = ops.tta_bbox_merge(*args)
    for l in range(3):
        n = int(cand[4][l])
        assert n == len(g['cat%d.scores' % l]) and np.array_equal(cand[0][l, :n].cpu().numpy(), g['cat%d.boxes' % l])
        assert cand[3][l, :n].tolist() == list(range(n))                                         # the reference's concatenation order
    kept = RN._device_nms_kept(cand, 3, P * 4, kw['top_k'], kw['max_overlap'], torch.device(DEV))
    for l, (b, c, s) in enumerate(RN._kept_to_host(kept, 3)):
        B, C, S = RN._prune(list(b), list(c), list(s), kw['rel_thresh'], kw['max_boxes'], kw['dup'], kw['inc']) if len(b) else ([], [], [])
        assert np.array_equal(np.array(B, np.float32).reshape(-1, 4), g['%s.img%d.boxes' % (name, l)]), (name, l)
        assert [int(v) for v in C] == g['%s.img%d.classes' % (name, l)].tolist(), (name, l)
        assert np.array_equal(np.array(S, np.float32), g['%s.img%d.scores' % (name, l)]), (name, l)


# ---- GPU: TTA_bbox from the public API --------------------------------------------------------------------------------------------------

NET_SHAPES = [(64, 96), (96, 64), (80, 80)]
NET_SCALES = [1.0, 1.5, 1.3]                        # the eval minibatches pad: 96 x 144 -> 96 x 160, 104 x 104 -> 128 x 128
FLUSH_SCALES = [1.0, 1.0, 0.8]                      # they do not: 64 x 96, 96 x 64, 64 x 64
THRESH = 0.05                                       # the default; the filled net scores around 0.1: every image has candidates


@pytest.fixture(scope='module')
def net():
    """ObjectDetectionNet(3) with the seeded closed-form fill of the detection parity tests (oracle.synth.fill_detection_net_: every
    activation O(1) in eval mode, sigmoid outputs around 0.1 and unsaturated, non-zero box regressions)"""
    from neuralnetworklibrary_amd.General.Core import set_default_device
    set_default_device(DEV)
    return synth.fill_detection_net_(V.ObjectDetectionNet(3), seed=19)


def _learner(net, tmp_path, n=3, test=False, seed=3, scales=NET_SCALES):
    shapes = [NET_SHAPES[i % 3] for i in range(n)]
    images = lambda s: _images(s, shapes, scales)
    tfms = V.get_transforms_bbox('SideOn', jitter=5, scale_range=[0.9, 1.1])
    data = V.ImageDataObj(str(tmp_path), 'bbox', {0: 'a', 1: 'b', 2: 'c'}, 2, tfms, images(1), images(2), images(4) if test else None,
                          test_name='test' if test else None, seed=seed)
    return V.ImageLearner(str(tmp_path), data, net, optimizer='SGD_Mom', loss_func=V.SSD_loss(0.5, 0.25, 2.0)), tfms


def _same(a, b):
    assert len(a) == len(b)
    for (ba, ca, sa), (bb, cb, sb) in zip(a, b):
        assert len(ba) == len(bb) and [int(v) for v in ca] == [int(v) for v in cb]
        assert np.array_equal(np.array(ba, np.float32), np.array(bb, np.float32)) and np.array_equal(np.array(sa, np.float32), np.array(sb, np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize('rel_thresh', [None, [0.5, 0.9]], ids=['device_path', 'host_filter_path'])
def test_gpu_identity_passes_return_predict(net, tmp_path, rel_thresh):
    """four 'Basic' passes without jitter, scaling or lighting see pass 0's images: their survivors have IoU 1 with pass 0's and are
    suppressed, so TTA_bbox equals predict exactly.  The images' scales make every eval minibatch a multiple of 32 on both sides:
    TTA_bbox clips to the image and predict to the padded minibatch, which is the same window when nothing is padded"""
    learner, tfms = _learner(net, tmp_path, scales=FLUSH_SCALES)
    assert all(x.shape[2:] == (int(H * s), int(W * s)) for (x, _), (H, W), s in zip(learner.data.val_dl, NET_SHAPES, FLUSH_SCALES))
    aug = V.TransformBBox('Basic', None, None, jitter=0, scale_range=[1, 1])
    want = learner.predict('val', thresh=THRESH, rel_thresh=rel_thresh)
    assert len(want) == 3 and all(len(b) > 0 for b, _, _ in want), [len(b) for b, _, _ in want]      # pass 0 is not empty
    assert any(len(b) > 1 for b, _, _ in want) and all(isinstance(b[0], np.ndarray) and b[0].dtype == np.float32 for b, _, _ in want)
    got = learner.TTA_bbox('val', [tfms[0], aug], thresh=THRESH, rel_thresh=rel_thresh)
    print([len(b) for b, _, _ in want], [len(b) for b, _, _ in got])
    _same(got, want)
    assert all(type(c[0]) == type(w[0]) and type(s[0]) == type(ws[0]) for (_, c, s), (_, w, ws) in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize('rel_thresh', [None, [0.5, 0.9]], ids=['device_path', 'host_filter_path'])
def test_gpu_identity_passes_on_padded_images_return_the_windowed_predict(net, tmp_path, rel_thresh):
    """the general case: the eval minibatches of NET_SCALES pad (96 x 144 -> 96 x 160, 104 x 104 -> 128 x 128).  Under four identity
    passes TTA_bbox equals, exactly, what predict computes when BBoxPredictor clips to the image [0, rw] x [0, rh] in place of the
    padded minibatch; it differs from predict('val') itself, whose boxes reach into the padding.  (That a box which does not touch
    the window is the same box with and without it is checked at the decode, where it is exactly true:
    test_gpu_decode_window_...; after the suppression a clipped neighbour can decide differently.)"""
    learner, tfms = _learner(net, tmp_path)
    aug = V.TransformBBox('Basic', None, None, jitter=0, scale_range=[1, 1])
    want = []
    learner.model.eval()
    with torch.no_grad():
        for j, (x, _) in enumerate(learner.data.val_dl):
            (H, W), s = NET_SHAPES[j], NET_SCALES[j]
            assert x.shape[2] > int(H * s) or x.shape[3] > int(W * s) or j == 0                  # padded (image 0 is flush)
            anchors, reg, clas = learner.model(x)
            B, C, S = learner.model.BBoxPredictor(x, reg, clas, anchors, THRESH, 0.5, rel_thresh, 1000, 20, None, None, (0, 0, int(W * s), int(H * s)))
            want.append([[b * (1 / s) for b in B[0]], C[0], S[0]])
    assert all(len(b) > 0 for b, _, _ in want)
    got = learner.TTA_bbox('val', [tfms[0], aug], thresh=THRESH, rel_thresh=rel_thresh)
    _same(got, want)
    plain = learner.predict('val', thresh=THRESH, rel_thresh=rel_thresh)
    _same(got[:1], plain[:1])                                                                    # the flush image: the same window
    with pytest.raises(AssertionError):
        _same(got[1:], plain[1:])


@pytest.fixture(scope='module')
def flipped(net, tmp_path_factory):
    "TTA_bbox('val') twice under a 'SideOn' tfm_aug with jitter 5 and scale_range [0.9, 1.1], computed once for the tests below"
    learner, tfms = _learner(net, tmp_path_factory.mktemp('flipped'), test=True)
    aug = V.TransformBBox('SideOn', None, None, jitter=5, scale_range=[0.9, 1.1])
    run = lambda ds_type: learner.TTA_bbox(ds_type, [tfms[0], aug], thresh=THRESH)
    return learner, run('val'), run('val'), run('test')


@pytest.mark.gpu
def test_gpu_flip_and_scale_passes(flipped):
    "bitwise repeatable under one loader seed; sorted, non-empty boxes; compute_mAP takes the result"
    learner, a, b, test = flipped
    _same(a, b)
    assert len(a) == 3 and all(0 < len(bx) <= 20 for bx, _, _ in a) and len(test) == 3
    for boxes, _, scores in a:
        bx = np.array(boxes)
        assert list(scores) == sorted(scores, reverse=True) and (bx[:, 2] > bx[:, 0]).all() and (bx[:, 3] > bx[:, 1]).all()
    m = learner.compute_mAP(predictions=a, mAP_thresholds=[0.5])
    assert np.isfinite(m) and 0.0 <= m <= 1.0


@pytest.mark.gpu
def test_gpu_flip_and_scale_boxes_lie_within_one_pixel_of_the_original_image(flipped):
    """every returned box within [0, cols] x [0, rows] of its original image, up to one pixel.  The eval minibatches of these images
    pad (NET_SCALES), and the augmented ones pad and carry a jitter border: every pass clips to the window of the minibatch that is
    the image (nnl_bbox_decode_window), [col_jit, col_jit + rw] x [row_jit, row_jit + rh], which the undo maps onto
    [0, rw inv] x [0, rh inv] with rw inv <= W up to fp32 rounding.  (Clipped to the padded minibatch, as predict clips, the largest
    excess measured here was 18.462 = 128 / 1.3 - 80.)  predict('val') on the same images does leave the image: the test asserts that
    too, so that it cannot pass because the net happens to stay inside."""
    learner, a, _, test = flipped
    for name, res in (('val', a), ('test', test)):
        lo, hi = np.inf, -np.inf
        for (boxes, _, _), (H, W) in zip(res, NET_SHAPES):
            bx = np.array(boxes)
            lo, hi = min(lo, bx.min()), max(hi, (bx[:, [0, 2]] - W).max(), (bx[:, [1, 3]] - H).max())
        print('%s: smallest coordinate %.3f, largest excess over the original image %.3f' % (name, lo, hi))
        assert lo >= -1.0 and hi <= 1.0
    beyond = max(max((np.array(b)[:, [0, 2]] - W).max(), (np.array(b)[:, [1, 3]] - H).max()) for (b, _, _), (H, W) in zip(learner.predict('val', thresh=THRESH), NET_SHAPES))
    print('predict: largest excess over the original image %.3f' % beyond)
    assert beyond > 1.0


@pytest.mark.gpu
def test_gpu_decode_window_clips_to_the_window_and_the_full_window_is_the_plain_decode():
    g = torch.Generator().manual_seed(7)
    x = torch.zeros(2, 3, 64, 96, device=DEV)
    anchors = RN.AnchorGenerator()(x)
    A = anchors.shape[0]
    reg, clas = (torch.randn(2, A, 4, generator=g) * 2).to(DEV), torch.rand(2, A, 3, generator=g).to(DEV)
    pred = RN.BBoxPredictor()
    plain = pred.survivors_on_device(x, reg, clas, anchors, 0.5, 0.5, 1000)
    full = pred.survivors_on_device(x, reg, clas, anchors, 0.5, 0.5, 1000, window=(0, 0, 96, 64))
    assert torch.equal(plain[3], full[3]) and int(plain[3].min()) > 20                           # the slots past the count are not written
    assert all(torch.equal(p[i, :int(plain[3][i])], f[i, :int(plain[3][i])]) for p, f in zip(plain[:3], full[:3]) for i in range(2))
    win = (5, 7, 70.5, 50)
    kb, kc, ks, kn = pred.survivors_on_device(x, reg, clas, anchors, 0.5, 0.5, 1000, window=win)
    for i in range(2):
        b = kb[i, :int(kn[i])].cpu().numpy()
        assert len(b) > 20 and b[:, 0].min() >= 5 and b[:, 1].min() >= 7 and b[:, 2].max() <= 70.5 and b[:, 3].max() <= 50
        assert (b[:, 0] == 5).any() and (b[:, 2] == 70.5).any() and (b[:, 2] > b[:, 0]).all() and (b[:, 3] > b[:, 1]).all()
    B, C, S = pred(x, reg, clas, anchors, 0.5, 0.5, None, 1000, 1000, None, None, win)        # __call__ takes the window too
    assert [len(v) for v in B] == kn.tolist() and np.array_equal(np.array(B[0]), kb[0, :int(kn[0])].cpu().numpy())
    # without suppression (no IoU exceeds 1) every candidate survives, sorted: a box that does not touch the window's border is the same
    # box, class and score with and without the window, and the two lists differ in nothing else
    rows = lambda kept, i: {tuple(b.tolist()) + (int(c), float(sc)) for b, c, sc in zip(*[t[i, :int(kept[3][i])].cpu() for t in kept[:3]])}
    inside = lambda r: r[0] > win[0] and r[1] > win[1] and r[2] < win[2] and r[3] < win[3]
    every = pred.survivors_on_device(x, reg, clas, anchors, 0.5, 1.0, A)
    clipped = pred.survivors_on_device(x, reg, clas, anchors, 0.5, 1.0, A, window=win)
    for i in range(2):
        a, b = {r for r in rows(every, i) if inside(r)}, {r for r in rows(clipped, i) if inside(r)}
        print("image %d: %d of %d candidates do not touch the window" % (i, len(b), len(rows(clipped, i))))
        assert a == b and len(a) >= 3 and len(rows(clipped, i)) > len(b) and int(every[3][i]) >= int(clipped[3][i])


@pytest.mark.gpu
def test_gpu_device_path_makes_no_per_image_copy(net, tmp_path, monkeypatch):
    "device->host copies (Tensor.cpu) during TTA_bbox at the defaults: the same number for 2 images as for 4"
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    counts = []
    for n in (2, 4):
        learner, tfms = _learner(net, tmp_path / str(n), n=n)
        del calls[:]
        out = learner.TTA_bbox('val', tfms, thresh=THRESH)
        counts.append(len(calls))
        assert len(out) == n
    print('Tensor.cpu calls for 2 and 4 images:', counts)
    assert counts[0] == counts[1] and 0 < counts[0] <= 8
