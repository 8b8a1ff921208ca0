"""Bit identity of every kernel that reduces or scans through csrc/block_ops.h.

Each entry below builds a small seeded input, calls the Python binding of one kernel family and hashes the bytes of every output; the
hashes are compared with tests/golden/block_ops_bits.json, which was recorded from the library as it stood BEFORE the kernels' private
reduction helpers were replaced by block_ops.h: the order of every sum, maximum and scan is part of the contract, down to the last
bit.  The shapes sit just past the constants of the kernels (a partly filled last wave, more than one wave, the multi-block path).

    python tests/test_block_ops_bits_gpu.py --record

runs every entry twice, writes the JSON from the entries whose two runs agree and names the others.  NNL_LIB_PATH selects the library.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'block_ops_bits.json')
DEV = 'cuda'
ENTRIES = {}

pytestmark = pytest.mark.gpu


def entry(fn):
    ENTRIES[fn.__name__] = fn
    return fn


def _rs(seed):
    return np.random.RandomState(seed)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sha(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(name):
    torch.cuda.synchronize()
    out = ENTRIES[name]()
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in out.items()}


# ---- loss.hip: 1024-thread halving tree; kLossOneBlock = 65536 elements in one block, two launches above -------------------------------
LOSS_N = [1, 1000, 65536, 65537]


def _loss(fn, seed, target_of):
    out = {}
    for n in LOSS_N:
        rs = _rs(seed + n)
        x = rs.standard_normal(n).astype(np.float32) * 3
        out['n%d' % n] = fn(_dev(x), _dev(target_of(rs, n)))
    return out


@entry
def mse_loss():
    from neuralnetworklibrary_amd import ops
    return _loss(ops.mse_loss, 11, lambda rs, n: rs.standard_normal(n).astype(np.float32))


@entry
def bce_with_logits():
    from neuralnetworklibrary_amd import ops
    return _loss(ops.bce_with_logits, 12, lambda rs, n: rs.uniform(0, 1, n).astype(np.float32))


# ---- text.hip: kBlock = 256 threads per vocabulary row (4 loads in flight: 4 * 256 per trip), mean_kernel over the rows -------------------
def _softmax_ce(rows, V, seed):
    from neuralnetworklibrary_amd import ops_text
    rs = _rs(seed)
    logits = _dev((rs.standard_normal((rows, V)) * 4).astype(np.float32)).requires_grad_(True)
    target = _dev(rs.randint(0, V, rows).astype(np.int64))
    loss = ops_text.softmax_cross_entropy(logits, target)
    loss.backward()
    return {'loss': loss.detach(), 'dlogits': logits.grad}


@entry
def softmax_ce():
    out = {}
    for V in (1, 255, 257, 4 * 256 + 3):
        out.update({'V%d.%s' % (V, k): v for k, v in _softmax_ce(3, V, 20 + V).items()})
    for rows in (1, 300):                                # mean_kernel: one thread busy; more rows than its 256 threads
        out.update({'rows%d.%s' % (rows, k): v for k, v in _softmax_ce(rows, 257, 30 + rows).items()})
    return out


@entry
def seq_reg():
    """kRegBlock = 256 columns per block: one partly filled block; 258 blocks (more partials than seq_reg_final_kernel has threads)"""
    from neuralnetworklibrary_amd import ops_text
    out = {}
    for T, R in ((5, 100), (3, 257 * 256 + 5)):
        h = _dev(_rs(40 + T).standard_normal((T, 1, R)).astype(np.float32))
        out['T%d.R%d' % (T, R)] = ops_text.seq_activation_reg(h, 2.0, 1.0)
    return out


# ---- retina_loss.hip: 256 anchors per block, pairwise fold of the 4 waves ---------------------------------------------------------------
@entry
def retina_loss():
    from neuralnetworklibrary_amd import ops
    out = {}
    for A in (1, 255, 257):
        rs = _rs(50 + A)
        side = 16.0
        ax, ay = (np.arange(A) % 16) * 8.0, (np.arange(A) // 16) * 8.0
        anchors = np.stack([ax, ay, ax + side, ay + side], 1).astype(np.float32)
        K, M = 3, 3
        boxes = np.full((2, M, 4), -1.0, dtype=np.float32)                # image 0: no object
        cats = np.full((2, M), -1, dtype=np.int64)
        pick = rs.choice(A, size=min(2, A), replace=False)
        for j, a in enumerate(pick):                                      # image 1: objects on (and next to) anchors
            boxes[1, j] = anchors[a] + np.float32([0, 0, 1, 2])
            cats[1, j] = rs.randint(0, K)
        reg = _dev(rs.standard_normal((2, A, 4)).astype(np.float32) * 0.5).requires_grad_(True)
        clas = _dev(rs.uniform(0.01, 0.99, (2, A, K)).astype(np.float32)).requires_grad_(True)
        loss = ops.retina_loss(_dev(anchors), reg, clas, _dev(boxes), _dev(cats))
        loss[0].backward()
        out.update({'A%d.loss' % A: loss.detach(), 'A%d.dreg' % A: reg.grad, 'A%d.dclas' % A: clas.grad})
    return out


# ---- optim.hip: 4096-element chunks, pairwise fold per chunk, 256-thread fp64 tree over the chunks -----------------------------------------
def _clip_step(sizes, seed):
    from neuralnetworklibrary_amd.fused_optim import FusedStep
    rs = _rs(seed)
    params = [_dev(rs.standard_normal(n).astype(np.float32)).requires_grad_(True) for n in sizes]
    for p in params:
        p.grad = _dev(rs.standard_normal(p.numel()).astype(np.float32))
    fs = FusedStep(torch.optim.SGD(params, lr=0.1, momentum=0.9))
    fs.step([0.1], [1.0], 0.5)
    out = {'coef_norm_partials': fs.clip_ws}
    out.update({'p%d' % i: p.detach() for i, p in enumerate(params)})
    return out


@entry
def grad_norm_clip():
    out = {'three.' + k: v for k, v in _clip_step([1, 4097, 8192 + 5], 60).items()}
    many = _clip_step([257 * 4096 + 1], 61)              # 258 chunks: more than clip_coef_kernel's block has threads
    out['chunks258.coef_norm_partials'] = many['coef_norm_partials']
    return out


# ---- attn_pool.hip: kBlock = 256 threads, chunks of at least 8 rows merged by the column's last workgroup ----------------------------------
@entry
def attn_pool():
    from neuralnetworklibrary_amd import ops_text
    rs = _rs(70)
    T, B, E, A = 257, 2, 4 * 257, 20                     # 257 timesteps and 257 float4 units per row: one past kBlock
    x = np.full((B, T), 1, dtype=np.int64)               # 1 = the pad token
    x[0, 0] = 5                                          # a sequence of length 1
    x[1, :] = rs.randint(2, 50, T)                       # and one of length T
    h = _dev(rs.standard_normal((T, B, A)).astype(np.float32)).requires_grad_(True)
    enc = _dev(rs.standard_normal((T, B, E)).astype(np.float32)).requires_grad_(True)
    w2 = _dev(rs.standard_normal((1, A)).astype(np.float32)).requires_grad_(True)
    b2 = _dev(rs.standard_normal(1).astype(np.float32)).requires_grad_(True)
    attn, pooled = ops_text.attention_pool(h, w2, b2, enc, _dev(x))
    ga, gp = _dev(rs.standard_normal((T, B)).astype(np.float32)), _dev(rs.standard_normal((B, E)).astype(np.float32))
    ((attn * ga).sum() + (pooled * gp).sum()).backward()
    return {'attn': attn.detach(), 'pooled': pooled.detach(), 'dh': h.grad, 'denc': enc.grad, 'dw2': w2.grad, 'db2': b2.grad}


# ---- image_aug.hip: block partials of the channel means (lighting) ---------------------------------------------------------------------------
@entry
def image_aug():
    from neuralnetworklibrary_amd import ops
    rs = _rs(80)
    shapes = [(13, 17), (20, 11)]
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in shapes]
    offs = np.cumsum([0] + [im.size for im in imgs])
    arena = np.concatenate([im.reshape(-1) for im in imgs])
    desc = np.array([[offs[i], H, W] for i, (H, W) in enumerate(shapes)], dtype=np.int64)
    params = np.zeros(2, dtype=ops.IMAGE_AUG_PARAM)
    for i, (H, W) in enumerate(shapes):
        c, s = np.cos(0.1 * (i + 1)), np.sin(0.1 * (i + 1))
        params[i] = (i, 1, 2, H - 2, W - 3, (c, -s, 0.5, s, c, -0.25), ops.IMAGE_AUG_FLIP if i else 0, 0, 0.05 * (i + 1), 1.0 + 0.1 * i)
    stats = [[0.485, 0.456, 0.406], [0.229, 0.224, 0.225]]
    out = ops.image_aug(_dev(arena), _dev(desc), _dev(params.view(np.uint8).reshape(2, -1)), (9, 7), stats=stats, lighting=True)
    return {'out': out}


# ---- tab_assoc.hip: 300 rows (one tile, a partly filled last wave), fp64 -------------------------------------------------------------------------
@entry
def tab_assoc():
    from neuralnetworklibrary_amd import ops
    rs = _rs(90)
    n, card = 300, [3, 4]
    codes = np.stack([rs.randint(-1, c, n) for c in card]).astype(np.int32)           # -1: missing
    vals = np.round(rs.standard_normal((2, n)) * 16) / 8                              # multiples of 1/8: the atomic fp64 sums are exact
    vals[1] += np.round(vals[0] * 4) / 8
    vals[0, rs.rand(n) < 0.05] = np.nan
    shift = np.array([0.5, -0.25])
    tables, offsets = ops.assoc_contingency(_dev(codes), card, [0], [1])
    return {'contingency': tables,
            'table_stats': ops.assoc_table_stats(tables, card, [0], [1], offsets),
            'cat_cont': ops.assoc_cat_cont(_dev(codes), card, _dev(vals), _dev(shift), [0, 1], [0, 1]),
            'cont_cont': ops.assoc_cont_cont(_dev(vals), _dev(shift), [0], [1], with_abs=True)}


# ---- det_eval.hip: 256-thread scans over a category's detections in score order ------------------------------------------------------------------
def _det_set():
    "2 images, 2 categories, 75 detections: 70 in category 0 (more than a wave), and a group of detections without a ground truth"
    rs = _rs(100)
    ids, cat_ids = [1, 2], [10, 11]
    coco = {'images': [{'id': i} for i in ids], 'categories': [{'id': c} for c in cat_ids], 'annotations': []}
    n_gt, n_dt = {(0, 0): 3, (0, 1): 0, (1, 0): 2, (1, 1): 1}, {(0, 0): 40, (0, 1): 5, (1, 0): 30, (1, 1): 0}
    preds, targets = [], []
    for i in range(2):
        B, Cl, Sc, tg = [], [], [], []
        for c in range(2):
            gts = []
            for g in range(n_gt[i, c]):
                x, y, w, h = (float(np.round(rs.uniform(lo, hi) * 4) / 4) for lo, hi in ((0, 200), (0, 150), (20, 90), (20, 90)))
                gts.append((x, y, w, h))
                coco['annotations'].append({'id': len(coco['annotations']) + 1, 'image_id': ids[i], 'category_id': cat_ids[c],
                                            'bbox': [x, y, w, h], 'area': w * h, 'iscrowd': int(i == 1 and c == 0 and g == 1)})
                tg.append((np.array([x, y, x + w, y + h]), c))
            for d in range(n_dt[i, c]):
                if gts and d % 3:
                    x, y, w, h = gts[d % len(gts)]
                    j = np.round(rs.uniform(-0.2, 0.2, 4) * np.array([w, h, w, h]) * 4) / 4
                    b = np.array([x + j[0], y + j[1], x + w + j[2], y + h + j[3]])
                else:
                    x, y = rs.uniform(0, 200), rs.uniform(0, 150)
                    b = np.round(np.array([x, y, x + rs.uniform(10, 90), y + rs.uniform(10, 90)]) * 4) / 4
                B.append(b.astype(np.float32)); Cl.append(c); Sc.append(np.float32(rs.randint(1, 8) / 8))
        preds.append([B, Cl, Sc])
        targets.append(tg)
    return coco, ids, preds, {0: 10, 1: 11}, targets


@entry
def det_eval():
    from neuralnetworklibrary_amd import ops
    coco, ids, preds, cat2dscat, targets = _det_set()
    p = ops.det_eval_pack(preds, coco=coco, image_ids=ids, cat2dscat=cat2dscat, max_det=100)
    assert np.diff(p['cat_dt_off']).max() > 64 and (np.diff(p['gt_off'])[np.diff(p['dt_off']) > 0] == 0).any()
    thr, rng = np.array([0.5, 0.75]), np.array([[0, 1e10], [0, 48.0 ** 2]])
    precision, recall, scores = ops.det_eval_coco(p, thr, np.linspace(0, 1, 11), [1, 10, 100], rng)
    m = ops.det_eval_pack(preds, targets=targets, n_categories=2)
    return {'precision': precision, 'recall': recall, 'scores': scores, 'map': ops.det_map(m, [0.5, 0.75])}


# ---- tab_features.hip: kTile = 1024 rows per scan tile --------------------------------------------------------------------------------------------
@entry
def seg_event_gaps():
    from neuralnetworklibrary_amd import ops
    out = {}
    for n in (1, ops.SEG_SCAN_TILE - 1, ops.SEG_SCAN_TILE + 1):
        rs = _rs(110 + n)
        head = (rs.rand(n) < 0.02).astype(np.uint8)
        head[0] = 1
        t = np.cumsum(rs.randint(1, 5, n)).astype(np.int64)
        event = (rs.rand(n) < 0.1).astype(np.uint8)
        res = ops.seg_event_gaps(_dev(t), _dev(head), _dev(event), 2.0)
        out.update({'n%d.%s' % (n, k): v for k, v in zip(('before', 'after', 'seg_start', 'seg_end'), res)})
    return out


# ---- detect.hip: the first wave's inclusive sum of the passes' counts ---------------------------------------------------------------------------------
@entry
def tta_bbox_merge():
    from neuralnetworklibrary_amd import ops
    rs = _rs(120)
    L, P, M = 2, 3, 4
    boxes = np.round(rs.uniform(0, 200, (L, P, M, 4)) * 4).astype(np.float32) / 4
    classes = rs.randint(0, 5, (L, P, M)).astype(np.int32)
    scores = rs.uniform(0, 1, (L, P, M)).astype(np.float32)
    counts = np.array([[0, M, 1], [M, 1, 0]], dtype=np.int32)
    undo = np.zeros((L, P), dtype=ops.TTA_UNDO)
    for i in range(L):
        for p in range(P):
            undo[i, p] = (rs.randint(0, 8), rs.randint(0, 8), np.float32(1.0 / rs.uniform(0.8, 1.3)), 320.0, p % 2)
    res = ops.tta_bbox_merge(_dev(boxes), _dev(classes), _dev(scores), _dev(counts), _dev(undo.view(np.uint8).reshape(L, P, -1)))
    return dict(zip(('boxes', 'classes', 'scores', 'order', 'count'), res))


# ---- lm_generate.hip: 64 vocabulary rows per slice, lm_pick_kernel's 256 threads over the slices ---------------------------------------------------------
@entry
def lm_next_token():
    from neuralnetworklibrary_amd import ops_text
    V, E = 64 * 300 + 7, 36                              # 301 slices (the last one partly filled): some threads own two
    g = torch.Generator().manual_seed(130)
    emb = (torch.rand(V, E, generator=g) * 2 - 1).to(DEV)
    h = ((torch.rand(E, generator=g) * 2 - 1) * (3.0 / E ** 0.5)).to(DEV)
    out = {}
    for k in (1, 4):
        tokens = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        top_p, top_i = torch.zeros(1, k, device=DEV), torch.full((1, k), -1, dtype=torch.int64, device=DEV)
        logits = torch.zeros(V, device=DEV)
        u = torch.tensor([0.37], device=DEV)
        ops_text.lm_next_token(emb, h, k, u, 0, tokens, 0, top_p, top_i, 4, logits_out=logits)
        out.update({'k%d.tokens' % k: tokens, 'k%d.top_probs' % k: top_p, 'k%d.top_indices' % k: top_i, 'k%d.logits' % k: logits})
    return out


# ---- the test -------------------------------------------------------------------------------------------------------------------------------------------
def _golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


def test_every_entry_is_recorded():
    assert sorted(_golden()) == sorted(ENTRIES)


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_bits_equal_the_recorded_ones(name):
    want, got = _golden()[name], digests(name)
    differ = sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))
    assert not differ, '%s: the bytes of %s differ from the recorded ones' % (name, ', '.join(differ))


def record():
    from neuralnetworklibrary_amd import _lib
    print('recording from %s (source stamp %s; this tree is %s)' % (_lib.LIB_PATH, _lib.source_stamp(), _lib.source_stamp_of_tree()))
    golden, unstable = {}, []
    for name in sorted(ENTRIES):
        a, b = digests(name), digests(name)
        if a == b:
            golden[name] = a
        else:
            unstable.append((name, sorted(k for k in a if a[k] != b[k])))
        print('%-18s %s' % (name, 'recorded (%d outputs)' % len(a) if a == b else 'NOT DETERMINISTIC: %s' % unstable[-1][1]), flush=True)
    with open(GOLDEN_JSON, 'w') as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d entries, %d left out' % (GOLDEN_JSON, len(golden), len(unstable)))


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if '--record' in sys.argv[1:]:
        record()
    else:
        sys.exit('usage: python tests/test_block_ops_bits_gpu.py --record')
