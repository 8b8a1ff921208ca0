"""Golden vectors G19 for detection test-time augmentation (reference Applications/Vision.py:2036-2121, TTA_bbox; the final step is
Applications/VisionModels/retinanet.py:523-711, nms).

Hand-made per-pass survivor lists for 3 images x 5 passes x 4 slots, as BBoxPredictor would leave them in the TRANSFORMED images
(descending score per pass): image 0 (96 wide) has two objects of class 0 and 1 and a cross-class near-duplicate of the first, seen by
most passes with a small perturbation each (near-duplicates across passes); image 1 (64 wide) has two overlapping objects of one class
and passes that see nothing; image 2 is empty in every pass.  Pass 0 is the eval transform (no jitter, rand_scale 1, no mirror), passes
1-4 have jitter, rand_scale and mirrors of their own.  The tool undoes them with four lines of numpy of its own (`undo_numpy`, the
statements of Vision.py:2092-2096), concatenates the passes per image and runs the REAL reference's nms on the union, on CPU tensors
through oracle/_ref_import.py, for the default arguments and for one rel_thresh + dup setting.  It asserts that no two candidates of an
image have the same score, so the reference's unstable sort decides nothing.  Writes data only: tests/golden/g19_tta_bbox.npz.
Usage: python tools/gen_golden_tta_bbox.py   (needs the reference checkout the oracle shim points at)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g19_tta_bbox.npz')
L, P, M = 3, 5, 4
COLS, ROWS, SCALES = [96, 64, 80], [64, 96, 80], [1.3, 0.61, 1.0]
SETTINGS = {'default': dict(max_overlap=0.5, rel_thresh=None, top_k=1000, max_boxes=20, dup=None, inc=None),
            'rel_dup': dict(max_overlap=0.5, rel_thresh=[0.3, 0.8], top_k=1000, max_boxes=20, dup=[0.5, [(0, 1), (1, 0)]], inc=None)}
# per pass: (row_jit, col_jit, rand_scale, mirrored)
PASSES = [(0, 0, 1.0, 0), (7, 3, 0.83, 1), (0, 5, 1.17, 0), (2, 0, 0.9, 1), (4, 7, 1.1, 0)]
# objects in ORIGINAL coordinates: (box, class, base score, passes that see it)
OBJECTS = [
    [([10., 8., 50., 40.], 0, 0.90, (0, 1, 2, 3, 4)), ([55., 20., 90., 60.], 1, 0.70, (0, 1, 3, 4)),
     ([12., 10., 48., 42.], 1, 0.55, (0, 2, 4)), ([60., 2., 80., 18.], 0, 0.20, (0, 1))],
    [([5., 10., 40., 70.], 0, 0.80, (0, 2)), ([8., 30., 44., 90.], 0, 0.60, (0, 2, 4))],
    [],
]


def undo_numpy(boxes, col_jit, row_jit, rand_scale, scale, flip, cols):
    "Vision.py:2092-2096 for one (pass, image): boxes float32 [n, 4] in the transformed image -> in the original image"
    boxes = np.array([boxes[:, 0] - col_jit, boxes[:, 1] - row_jit, boxes[:, 2] - col_jit, boxes[:, 3] - row_jit]).T
    boxes = (1 / (rand_scale * scale)) * boxes
    if flip == 1:
        boxes = np.array([cols - boxes[:, 2], boxes[:, 1], cols - boxes[:, 0], boxes[:, 3]]).T
    return boxes


def concatenate(g, l):
    "image l's candidates of the golden's input tables, undone and concatenated in pass order: (boxes [n, 4] f32, classes i64, scores f32)"
    B, C, S = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for p in range(g['in.boxes'].shape[1]):
        n = int(g['in.counts'][l, p])
        if n:
            B.append(undo_numpy(g['in.boxes'][l, p, :n], int(g['in.col_jit'][l, p]), int(g['in.row_jit'][l, p]), float(g['in.rand_scale'][l, p]),
                                float(g['in.scale'][l]), int(g['in.flip'][l, p]), int(g['in.cols'][l])))
            C.append(g['in.classes'][l, p, :n].astype(np.int64))
            S.append(g['in.scores'][l, p, :n])
    return np.concatenate(B).astype(np.float32), np.concatenate(C), np.concatenate(S)


def inputs():
    rs = np.random.RandomState(1900)
    boxes, classes = np.zeros((L, P, M, 4), np.float32), np.zeros((L, P, M), np.int32)
    scores, counts = np.zeros((L, P, M), np.float32), np.zeros((L, P), np.int32)
    for l in range(L):
        for p, (row_jit, col_jit, rand_scale, mirrored) in enumerate(PASSES):
            seen = []
            for box, cls, score, passes in OBJECTS[l]:
                if p not in passes:
                    continue
                b = np.array(box) + (rs.uniform(-1.5, 1.5, 4) if p else 0.0)                  # what this pass makes of the object
                if mirrored:
                    b = np.array([COLS[l] - b[2], b[1], COLS[l] - b[0], b[3]])
                b = b * SCALES[l] * rand_scale + np.array([col_jit, row_jit, col_jit, row_jit])
                seen.append((np.float32(score - 0.013 * p + rs.uniform(-0.004, 0.004)), cls, b.astype(np.float32)))
            seen.sort(key=lambda t: -t[0])
            counts[l, p] = len(seen)
            for r, (s, c, b) in enumerate(seen):
                boxes[l, p, r], classes[l, p, r], scores[l, p, r] = b, c, s
    tab = lambda k: np.array([[PASSES[p][k] for p in range(P)]] * L)
    return {'in.boxes': boxes, 'in.classes': classes, 'in.scores': scores, 'in.counts': counts, 'in.row_jit': tab(0).astype(np.int32),
            'in.col_jit': tab(1).astype(np.int32), 'in.rand_scale': tab(2).astype(np.float64), 'in.flip': tab(3).astype(np.int32),
            'in.scale': np.array(SCALES, np.float64), 'in.cols': np.array(COLS, np.int32), 'in.rows': np.array(ROWS, np.int32)}


def main():
    import torch
    from oracle import _ref_import
    RN = _ref_import.load()['Applications.VisionModels.retinanet']
    out = inputs()
    assert sorted(out['in.counts'].reshape(-1).tolist())[0] == 0 and out['in.counts'].max() == M and (out['in.counts'][2] == 0).all()
    for l in range(L):
        b, c, s = concatenate(out, l)
        assert len(np.unique(s)) == len(s), 'image %d: two candidates share a score' % l
        out.update({'cat%d.boxes' % l: b, 'cat%d.classes' % l: c, 'cat%d.scores' % l: s})
        for name, kw in SETTINGS.items():
            B, C, S = RN.nms(torch.from_numpy(b), torch.from_numpy(c), torch.from_numpy(s), **kw)
            out['%s.img%d.boxes' % (name, l)] = np.array(B, dtype=np.float32).reshape(-1, 4)
            out['%s.img%d.classes' % (name, l)] = np.array(C, dtype=np.int64).reshape(-1)
            out['%s.img%d.scores' % (name, l)] = np.array(S, dtype=np.float32).reshape(-1)
            print('image %d %-8s %d candidates -> %d boxes, classes %s' % (l, name, len(b), len(B), [int(v) for v in C]))
    a, r = (sum(len(out['%s.img%d.scores' % (n, l)]) for l in range(L)) for n in SETTINGS)
    assert 0 < r < a, 'the rel_thresh + dup setting must prune something the default keeps (%d vs %d)' % (r, a)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.1f KB' % (os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
