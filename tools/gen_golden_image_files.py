"""Golden G25 for the image-file constructors (reference Applications/Vision.py:54-189 get_stats, :901-1200 ImageDataObj.from_csv /
from_folders / from_json_bbox; General/Core.py:220-247 SplitTrainVal).

Runs the REAL reference on CPU through oracle/_ref_import.py (read-only) on a tiny tree of PNG files written into a temporary
directory, and writes data only:
  tests/golden/g25_image_files.npz   the seeded uint8 arrays the PNG files are written from (PNG is lossless: the decoded pixels are
                                     these arrays; no claim is made about JPEG bits against OpenCV) and the reference's get_stats
                                     result `ref_stats` [2, 3];
  tests/golden/g25_image_files.json  the tree ('png': path -> array key, 'text': path -> csv / json content) and, per case, the
                                     reference's categories, (file name, target) lists of the train / val / test sets, for 'bbox'
                                     also id, aspect_ratio, scale and cat2dscat.  Python's json round-trips float64 exactly.
After the import the tool gives the shim's empty `cv2` stub an imread / cvtColor / flags backed by Pillow (BGR out, as OpenCV), so that
the reference's open_image, get_stats and from_json_bbox run, and makes os.listdir return sorted names while the reference runs: the
reference takes the directory order as it comes, which differs from machine to machine, and the split a seed gives depends on it.
One reference function is replaced, convert_labels_multi, by the same statements written with `.iat` (see convert_labels_multi_iat:
the original loses its writes under pandas 2 and raises).  The gray and the RGBA file of the tree are for this project's decoder only: no reference call reads them.
Usage: python tools/gen_golden_image_files.py   (needs the reference checkout the oracle shim points at)"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import image_files_cases as cases  # noqa: E402

SIZES = [(5, 7), (23, 17), (8, 8), (7, 5), (16, 9), (9, 16), (11, 13), (6, 21), (20, 6), (12, 12), (17, 23), (10, 15)]
CATS = ['cat', 'dog', 'bird']
LABEL = [0, 1, 2, 0, 1, 2, 0, 1, 0, 2, 1, 0]                      # category of train image i
MULTI = [['sky'], ['sky', 'road'], ['tree'], ['road', 'tree', 'sky'], ['water'], ['sky'], ['tree', 'water'], ['road'], ['sky', 'tree'],
         ['water', 'road'], ['tree'], ['sky', 'water']]
GET_ARS = [16, 24]


def arrays():
    out = {}
    for i, (h, w) in enumerate(SIZES):
        out['img_%02d' % i] = np.random.RandomState(2500 + i).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    out['gray'] = np.random.RandomState(2590).randint(0, 256, size=(9, 14)).astype(np.uint8)
    out['rgba'] = np.random.RandomState(2591).randint(0, 256, size=(13, 6, 4)).astype(np.uint8)
    return out


def tree():
    png, text = {}, {}
    names = ['img%02d.png' % i for i in range(12)]
    for i, n in enumerate(names):
        png['train/' + n] = 'img_%02d' % i
    for k, i in enumerate([1, 4, 8]):                              # a validation folder and a test folder of their own
        png['val/v%d.png' % k] = 'img_%02d' % i
    for k, i in enumerate([2, 9]):
        png['test/t%d.png' % k] = 'img_%02d' % i
    png['extra/gray.png'], png['extra/rgba.png'] = 'gray', 'rgba'
    for i, n in enumerate(names):                                  # labelled folders
        png['folders/%s/%s' % (CATS[LABEL[i]], n)] = 'img_%02d' % i
    for k, i in enumerate([0, 1, 2, 5]):
        png['foldersval/%s/w%d.png' % (CATS[LABEL[i]], k)] = 'img_%02d' % i
    text['train.csv'] = 'img_name,category\n' + ''.join('%s,%s\n' % (n, CATS[LABEL[i]]) for i, n in enumerate(names))
    text['train_nohdr.csv'] = ''.join('%s,%s\n' % (n[:-4], CATS[LABEL[i]]) for i, n in enumerate(names))       # names without suffix
    text['val.csv'] = 'img_name,category\n' + ''.join('v%d.png,%s\n' % (k, CATS[LABEL[i]]) for k, i in enumerate([1, 4, 8]))
    text['multi.csv'] = 'img_name,tags\n' + ''.join('%s,%s\n' % (n, ' '.join(MULTI[i])) for i, n in enumerate(names))
    rng = np.random.RandomState(2599)
    anns, aid = [], 1
    for i, (h, w) in enumerate(SIZES):
        for _ in range(int(rng.randint(0, 4))):                    # some images have no box
            bw, bh = int(rng.randint(2, w)), int(rng.randint(2, h))
            x, y = int(rng.randint(0, w - bw + 1)), int(rng.randint(0, h - bh + 1))
            anns.append({'id': aid, 'image_id': 100 + 7 * i, 'bbox': [x + 0.5 * (aid % 2), y, bw, bh], 'category_id': [3, 8, 21][aid % 3]})
            aid += 1
    anns[2]['ignore'] = 1
    anns[5]['iscrowd'] = 1
    anns[6]['iscrowd'] = 0
    coco = {'categories': [{'id': 8, 'name': 'dog'}, {'id': 3, 'name': 'cat'}, {'id': 21, 'name': 'bird'}],
            'images': [{'id': 100 + 7 * i, 'file_name': n} for i, n in enumerate(names)], 'annotations': anns}
    text['train.json'] = json.dumps(coco)
    return {'png': png, 'text': text}


def install_cv2():
    "Pillow-backed imread / cvtColor on the shim's cv2 stub: BGR uint8 out, as OpenCV"
    from PIL import Image
    cv2 = sys.modules['cv2']
    cv2.IMREAD_UNCHANGED, cv2.IMREAD_ANYCOLOR, cv2.COLOR_BGR2RGB = -1, 4, 4
    cv2.imread = lambda name, flags=None: np.ascontiguousarray(np.asarray(Image.open(name).convert('RGB'))[:, :, ::-1])
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1])


def convert_labels_multi_iat(dataframe, categories_rev):
    """The reference's convert_labels_multi (Vision.py:892-898) with its writes through `dataframe.iloc[i][1] = ...` spelled
    `dataframe.iat[i, 1] = ...`: under pandas 2 `iloc[i]` is a copy, the reference's write is lost and its next line raises."""
    num_cats = len(categories_rev)
    for i in range(len(dataframe)):
        idx = [categories_rev[c] for c in dataframe.iat[i, 1]]
        presence_absence = np.zeros(num_cats)
        presence_absence[idx] = 1
        dataframe.iat[i, 1] = presence_absence.astype('float32')


def plain(v):
    "reference values -> json (numpy scalars and arrays become Python numbers and lists)"
    if isinstance(v, np.ndarray):
        return [plain(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def record(data, bbox=False):
    out = {'categories': [data.categories[i] for i in range(len(data.categories))]}
    for k in ('train', 'val', 'test'):
        ds = getattr(data, k + '_ds')
        if ds is None:
            continue
        out[k] = [[im['img'], plain(im['target'])] for im in ds.images]
        if bbox:
            out[k + '_ars'] = [[float(im['aspect_ratio']), float(im['scale'])] for im in ds.images]
            out[k + '_id'] = [plain(im.get('id', -1)) for im in ds.images]
    if bbox:
        out['cat2dscat'] = [data.cat2dscat[i] for i in range(len(data.cat2dscat))]
    return out


def main():
    from oracle import _ref_import
    V = _ref_import.load()['Applications.Vision']
    install_cv2()
    V.ImageDataObj.convert_labels_multi = staticmethod(convert_labels_multi_iat)
    import warnings
    warnings.simplefilter('ignore', FutureWarning)
    listdir = os.listdir
    os.listdir = lambda p='.': sorted(listdir(p))
    A, spec = arrays(), tree()
    tfms, tfms_bbox = V.get_transforms('Basic', sz=8), V.get_transforms_bbox('Basic')
    res = {}
    with tempfile.TemporaryDirectory() as root:
        cases.write_tree(root, A, spec)
        res['csv_val_test'] = record(V.ImageDataObj.from_csv(root, tfms, 4, train_csv='train.csv', val_csv='val.csv', val_name='val',
                                                             test_name='test'))
        np.random.seed(3)
        res['csv_nohdr_suffix_split'] = record(V.ImageDataObj.from_csv(root, tfms, 4, train_csv='train_nohdr.csv', val_frac=0.25,
                                                                       skip_first=False, suffix='.png'))
        np.random.seed(5)
        res['csv_multi_split'] = record(V.ImageDataObj.from_csv(root, tfms, 4, train_csv='multi.csv', target_type='multi_label',
                                                                val_frac=0.25))
        np.random.seed(7)
        res['folders_split'] = record(V.ImageDataObj.from_folders(root, tfms, 4, train_name='folders', val_frac=0.3))
        res['folders_val_test'] = record(V.ImageDataObj.from_folders(root, tfms, 4, train_name='folders', val_name='foldersval',
                                                                     test_name='test'))
        np.random.seed(11)
        res['json_split'] = record(V.ImageDataObj.from_json_bbox(root, tfms_bbox, 2, train_json='train.json', val_frac=0.25,
                                                                 test_name='test', get_ARS=GET_ARS), bbox=True)
        stats_names = ['img%02d.png' % i for i in range(12)]
        ref_stats = np.stack(V.get_stats(os.path.join(root, 'train'), stats_names)).astype(np.float64)
    os.listdir = listdir
    spec.update(cases=res, seeds={'csv_nohdr_suffix_split': 3, 'csv_multi_split': 5, 'folders_split': 7, 'json_split': 11},
                get_ARS=GET_ARS, stats_names=stats_names)
    np.savez_compressed(cases.NPZ, ref_stats=ref_stats, **A)
    with open(cases.JSON, 'w') as f:
        json.dump(spec, f, indent=1, sort_keys=True)
    print('wrote', cases.NPZ, os.path.getsize(cases.NPZ), 'bytes;', cases.JSON, os.path.getsize(cases.JSON), 'bytes')
    for k, v in res.items():
        print(k, v['categories'], {s: len(v[s]) for s in ('train', 'val', 'test') if s in v})
    print('ref_stats', ref_stats)


if __name__ == '__main__':
    main()
