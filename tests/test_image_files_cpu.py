"""Image datasets from files, the host side: ImageDataObj.from_csv / from_folders / from_json_bbox, Vision.open_image_u8 and
device_data.ImageStore.from_files on the CPU device, against golden G25 (tools/gen_golden_image_files.py: the reference's own
categories, file lists, targets, aspect ratios, scales and splits on the same tree, which is rebuilt here from G25's arrays).
No GPU: the stores and loaders are built on the CPU device and no kernel runs."""
import os

import numpy as np
import pytest
import torch

import image_files_cases as cases
from neuralnetworklibrary_amd import device_data
from neuralnetworklibrary_amd.Applications import Vision as V

ARRAYS, REF_STATS, SPEC = cases.load_golden()
REF = SPEC['cases']


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return cases.write_tree(str(tmp_path_factory.mktemp('g25')), ARRAYS, SPEC)


@pytest.fixture(autouse=True)
def _cpu_default_device(monkeypatch):
    from neuralnetworklibrary_amd.General import Core
    monkeypatch.setattr(Core, '_DEVICE', torch.device('cpu'))


def tfms():
    return V.get_transforms('Basic', sz=8)


def check_sets(data, ref, folder_of, multi=False):
    assert data.categories == {i: n for i, n in enumerate(ref['categories'])}
    for k in ('train', 'val', 'test'):
        ds = getattr(data, k + '_ds')
        if k not in ref:
            assert ds is None
            continue
        assert [im['file'] for im in ds.images] == [f for f, _ in ref[k]], k
        for im, (f, t) in zip(ds.images, ref[k]):
            if multi:
                assert im['target'].dtype == np.float32 and np.array_equal(im['target'], np.array(t, dtype=np.float32)), (k, f)
            else:
                assert isinstance(im['target'], int) and im['target'] == t, (k, f)
            # the handle is the decoded file
            assert isinstance(im['img'], device_data.ResidentImage)
            assert np.array_equal(im['img'].numpy(), cases.rgb_of(ARRAYS, SPEC, folder_of[k] + '/' + f)), (k, f)
        assert ds.y == [im['target'] for im in ds.images] or multi


def test_from_csv_header_val_csv_and_listed_test_folder(tree):
    data = V.ImageDataObj.from_csv(tree, tfms(), 4, train_csv='train.csv', val_csv='val.csv', val_name='val', test_name='test')
    check_sets(data, REF['csv_val_test'], {'train': 'train', 'val': 'val', 'test': 'test'})
    assert data.target_type == 'single_label' and data.bs == 4 and tuple(data.sz) == (8, 8)
    assert data.train_ds.IMG_PATH == tree + '/train/' and data.test_ds.IMG_PATH == tree + '/test/'
    assert data.train_dl.store is not data.val_dl.store                     # two folders, two stores


def test_from_csv_no_header_suffix_and_val_frac_split(tree):
    np.random.seed(SPEC['seeds']['csv_nohdr_suffix_split'])
    data = V.ImageDataObj.from_csv(tree, tfms(), 4, train_csv='train_nohdr.csv', val_frac=0.25, skip_first=False, suffix='.png')
    check_sets(data, REF['csv_nohdr_suffix_split'], {'train': 'train', 'val': 'train'})
    assert data.train_dl.store is data.val_dl.store                         # one folder: one resident copy
    assert data.train_dl.arena.data_ptr() == data.val_dl.arena.data_ptr()
    assert data.val_ds.IMG_PATH == tree + '/train/'


def test_from_csv_multi_label(tree):
    np.random.seed(SPEC['seeds']['csv_multi_split'])
    data = V.ImageDataObj.from_csv(tree, tfms(), 4, train_csv='multi.csv', target_type='multi_label', val_frac=0.25)
    check_sets(data, REF['csv_multi_split'], {'train': 'train', 'val': 'train'}, multi=True)
    assert data.train_dl.y.dtype == torch.float32 and tuple(data.train_dl.y.shape) == (9, 4)


def test_from_csv_unknown_category_in_val_csv_raises(tree, tmp_path):
    bad = tmp_path / 'bad_val.csv'
    bad.write_text('img_name,category\nv0.png,horse\n')
    with pytest.raises(ValueError, match='horse'):
        V.ImageDataObj.from_csv(tree, tfms(), 4, train_csv='train.csv', val_csv=os.path.relpath(str(bad), tree), val_name='val')


def test_from_folders(tree):
    np.random.seed(SPEC['seeds']['folders_split'])
    data = V.ImageDataObj.from_folders(tree, tfms(), 4, train_name='folders', val_frac=0.3)
    check_sets(data, REF['folders_split'], {'train': 'folders', 'val': 'folders'})
    assert data.train_dl.arena.data_ptr() == data.val_dl.arena.data_ptr()
    data = V.ImageDataObj.from_folders(tree, tfms(), 4, train_name='folders', val_name='foldersval', test_name='test')
    check_sets(data, REF['folders_val_test'], {'train': 'folders', 'val': 'foldersval', 'test': 'test'})


def test_from_folders_skips_resource_forks(tree, tmp_path):
    root = cases.write_tree(str(tmp_path), ARRAYS, {'png': {'train/a/x.png': 'img_00', 'train/a/y.png': 'img_02', 'train/b/z.png': 'img_03',
                                                             'train/b/w.png': 'img_05', 'train/b/v.png': 'img_06'},
                                                     'text': {'train/a/._x.png': 'not an image', 'train/._b': 'junk'}})
    np.random.seed(0)
    data = V.ImageDataObj.from_folders(root, tfms(), 2, val_frac=0.2)
    assert data.categories == {0: 'a', 1: 'b'}
    assert sorted(im['file'] for ds in (data.train_ds, data.val_ds) for im in ds.images) == ['a/x.png', 'a/y.png', 'b/v.png', 'b/w.png', 'b/z.png']


def test_from_json_bbox(tree):
    ref = REF['json_split']
    np.random.seed(SPEC['seeds']['json_split'])
    data = V.ImageDataObj.from_json_bbox(tree, V.get_transforms_bbox('Basic'), 2, train_json='train.json', val_frac=0.25, test_name='test',
                                         get_ARS=SPEC['get_ARS'])
    assert data.target_type == 'bbox' and data.sz is None
    assert data.categories == {i: n for i, n in enumerate(ref['categories'])}
    assert data.cat2dscat == {i: c for i, c in enumerate(ref['cat2dscat'])}
    import json
    coco = json.loads(SPEC['text']['train.json'])
    skipped = [hw for a in coco['annotations'] if a.get('ignore') == 1 or a.get('iscrowd') == 1 for hw in [V.hw_to_mm(a['bbox']).tolist()]]
    assert len(skipped) == 2
    n_boxes = 0
    for k in ('train', 'val', 'test'):
        ds = getattr(data, k + '_ds')
        assert [im['file'] for im in ds.images] == [f for f, _ in ref[k]], k
        for im, (f, t), (ar, sc), ID in zip(ds.images, ref[k], ref[k + '_ars'], ref[k + '_id']):
            assert im['aspect_ratio'] == ar and im['scale'] == sc, (k, f)          # float64, bit-equal
            if k == 'test':
                assert im['target'] == 0 == t
                continue
            assert im['id'] == ID
            assert len(im['target']) == len(t)
            for (box, cat), (rbox, rcat) in zip(im['target'], t):
                assert np.array_equal(np.asarray(box, dtype=np.float64), np.array(rbox, dtype=np.float64)) and cat == rcat
                n_boxes += 1
    assert n_boxes == len(coco['annotations']) - 2                                # the ignore and the iscrowd annotation are absent
    assert data.train_dl.arena.data_ptr() == data.val_dl.arena.data_ptr()
    assert data.val_dl.bs == 1 and data.test_dl.bs == 1


def test_from_json_bbox_refuses_presize(tree):
    with pytest.raises(ValueError, match='presize'):
        V.ImageDataObj.from_json_bbox(tree, V.get_transforms_bbox('Basic'), 2, train_json='train.json', presize=8)


def test_presize_needs_a_gpu_device(tree):
    with pytest.raises(ValueError, match='presize'):
        device_data.ImageStore.from_files([tree + '/train/img00.png'], device='cpu', presize=4)


def test_presize_shape_rule():
    ps = device_data.presize_shape
    assert ps(23, 17, 8) == (int(23 * 8 / 17), 8) and ps(9, 16, 8) == (8, int(16 * 8 / 9))
    assert ps(5, 7, 8) == (5, 7) and ps(8, 30, 8) == (8, 30)                      # never enlarged; a shorter side of s stays
    assert ps(5, 7, 8, enlarge=True) == (8, int(7 * 8 / 5))                       # save_resized enlarges
    assert ps(5, 7, (3, 4)) == (3, 4) and ps(5, 7, None) == (5, 7)


def test_image_dataset_still_refuses_a_file_name():
    with pytest.raises(NotImplementedError, match='file name'):
        V.ImageDataset('x/', [{'img': 'a.png', 'target': 0}], tfms()[0], 'single_label', 'train')


# ---- decode ------------------------------------------------------------------------------------------------------

def test_open_image_u8_gray_and_rgba(tree):
    g = V.open_image_u8(tree + '/extra/gray.png')
    assert g.dtype == np.uint8 and np.array_equal(g, np.repeat(ARRAYS['gray'][:, :, None], 3, axis=2))
    a = V.open_image_u8(tree + '/extra/rgba.png')
    assert np.array_equal(a, ARRAYS['rgba'][:, :, :3])                            # Pillow's RGBA -> RGB drops alpha
    f = V.open_image(tree + '/train/img03.png')
    assert f.dtype == np.float32 and np.array_equal(f, ARRAYS['img_03'].astype(np.float32) / 255)


def test_open_image_u8_ignores_exif_orientation(tmp_path):
    from PIL import Image
    a = ARRAYS['img_04']                                                          # 16 x 9: a transpose would change the shape
    exif = Image.Exif()
    exif[0x0112] = 6                                                              # Orientation: rotate 90 degrees
    p = str(tmp_path / 'o.png')
    Image.fromarray(a).save(p, exif=exif)
    assert Image.open(p).getexif().get(0x0112) == 6
    assert np.array_equal(V.open_image_u8(p), a)


def test_open_image_u8_bad_files_name_the_file(tree, tmp_path):
    from PIL import Image
    whole = open(tree + '/train/img01.png', 'rb').read()
    cut = tmp_path / 'cut.png'
    cut.write_bytes(whole[:len(whole) // 2])
    with pytest.raises(ValueError, match='cut.png'):
        V.open_image_u8(str(cut))
    deep = tmp_path / 'deep.png'
    Image.fromarray((np.arange(35, dtype=np.uint16) * 1000).reshape(5, 7)).save(str(deep))
    with pytest.raises(ValueError, match='deep.png'):
        V.open_image_u8(str(deep))
    # a store refuses the set before it returns anything
    with pytest.raises(ValueError, match='cut.png'):
        device_data.ImageStore.from_files([tree + '/train/img00.png', str(cut)], device='cpu')


# ---- ImageStore.from_files on the CPU device -------------------------------------------------------------------------

def store_files(tree):
    names = ['img%02d.png' % i for i in range(12)]
    return [tree + '/train/' + n for n in names], [ARRAYS['img_%02d' % i] for i in range(12)]


def expect_concat(imgs):
    desc = np.zeros((len(imgs), 3), dtype=np.int64)
    desc[:, 1:] = [a.shape[:2] for a in imgs]
    desc[1:, 0] = np.cumsum([a.size for a in imgs])[:-1]
    return np.concatenate([a.reshape(-1) for a in imgs]), desc


@pytest.mark.parametrize('threads, chunk_bytes', [(1, 256 << 20), (4, 256 << 20), (4, 50), (3, 5 * 7 * 3 + 23 * 17 * 3), (2, 1000)])
def test_image_store_from_files_is_the_concatenation(tree, threads, chunk_bytes):
    "chunk_bytes = 50: smaller than every image; 105 + 1173: the first chunk ends exactly on an image boundary"
    paths, imgs = store_files(tree)
    store = device_data.ImageStore.from_files(paths, device='cpu', threads=threads, chunk_bytes=chunk_bytes)
    arena, desc = expect_concat(imgs)
    assert store.arena.dtype == torch.uint8 and np.array_equal(store.arena.numpy(), arena)
    assert np.array_equal(store.desc.numpy(), desc) and np.array_equal(store.desc_host, desc)
    assert store.shapes == store.orig_shapes == [a.shape[:2] for a in imgs] and len(store) == 12
    assert store[3].shape == imgs[3].shape and np.array_equal(store[-1].numpy(), imgs[-1])
    # the same table as a store of the arrays
    same = device_data.ImageStore.from_arrays(imgs, device='cpu')
    assert torch.equal(same.arena, store.arena) and torch.equal(same.desc, store.desc)


def test_decode_threads_default_and_cap(tree, monkeypatch):
    from concurrent import futures
    seen = []
    real = futures.ThreadPoolExecutor

    class Spy(real):
        def __init__(self, max_workers=None, *a, **k):
            seen.append(max_workers)
            super().__init__(max_workers, *a, **k)
    monkeypatch.setattr(futures, 'ThreadPoolExecutor', Spy)
    paths, _ = store_files(tree)
    monkeypatch.delenv('NNL_DECODE_THREADS', raising=False)
    device_data.ImageStore.from_files(paths[:2], device='cpu')
    monkeypatch.setenv('NNL_DECODE_THREADS', '64')
    device_data.ImageStore.from_files(paths[:2], device='cpu')
    device_data.ImageStore.from_files(paths[:2], device='cpu', threads=40)
    assert seen == [8, 16, 16]


def test_mixed_or_foreign_handles_are_refused(tree):
    paths, imgs = store_files(tree)
    s1 = device_data.ImageStore.from_files(paths[:2], device='cpu')
    s2 = device_data.ImageStore.from_files(paths[2:4], device='cpu')
    t = tfms()[0]
    with pytest.raises(ValueError, match='one ImageStore'):
        device_data.ImageBatches(V.ImageDataset('x/', [{'img': s1[0], 'target': 0}, {'img': s2[0], 'target': 1}], t, 'single_label', 'val'), 2, False, device='cpu')
    with pytest.raises(ValueError, match='all'):
        device_data.ImageBatches(V.ImageDataset('x/', [{'img': s1[0], 'target': 0}, {'img': imgs[5], 'target': 1}], t, 'single_label', 'val'), 2, False, device='cpu')


def test_cpu_store_stats_are_the_integer_sums(tree):
    paths, imgs = store_files(tree)
    store = device_data.ImageStore.from_files(paths, device='cpu')
    want = np.stack([np.concatenate([a.reshape(-1, 3).astype(np.int64).sum(0), (a.reshape(-1, 3).astype(np.int64) ** 2).sum(0)]) for a in imgs])
    assert store.stats().dtype == np.uint64 and np.array_equal(store.stats().astype(np.int64), want)
    assert np.array_equal(store.stats([4, 1]).astype(np.int64), want[[4, 1]])


def test_get_cat_counts_and_size_histograms(tree):
    counts = V.get_cat_counts(tree + '/train.csv', plot_hist=False)
    assert dict(zip(counts['category'], counts['count'])) == {'cat': 5, 'dog': 4, 'bird': 3}
    assert V.get_cat_counts(tree + '/train_nohdr.csv', skip_first=False, plot_hist=False)['count'].sum() == 12
    import matplotlib
    matplotlib.use('Agg')
    rows, cols, ratios = V.plot_imgsize_histograms(tree + '/train', num_bins=4)
    assert rows == [ARRAYS['img_%02d' % i].shape[0] for i in range(12)] and cols == [ARRAYS['img_%02d' % i].shape[1] for i in range(12)]
    assert ratios == [c / r for r, c in zip(rows, cols)]
