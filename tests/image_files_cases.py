"""The tiny image-file tree of golden G25 (tests/golden/g25_image_files.npz + .json), shared by tools/gen_golden_image_files.py, which
runs the reference on it, and by the tests, which rebuild it in a temporary directory: PNG files (lossless: the decoded pixels ARE
the stored arrays), csv and json files.  No reference code and no GPU here."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NPZ = os.path.join(GOLDEN, 'g25_image_files.npz')
JSON = os.path.join(GOLDEN, 'g25_image_files.json')


def load_golden():
    "(arrays: {key: uint8 array}, ref_stats float64 [2, 3], spec: the json)"
    z = np.load(NPZ)
    with open(JSON) as f:
        spec = json.load(f)
    return {k: z[k] for k in z.files if k != 'ref_stats'}, z['ref_stats'], spec


def write_tree(root, arrays, spec):
    """spec['png'] = {relative path: array key}, spec['text'] = {relative path: file content}.  An array of shape H x W is written as
    mode L, H x W x 3 as RGB, H x W x 4 as RGBA."""
    from PIL import Image
    for rel, key in spec['png'].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(arrays[key])).save(path)
    for rel, text in spec['text'].items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text)
    return root


def rgb_of(arrays, spec, rel):
    "the H x W x 3 RGB pixels that file `rel` of the tree decodes to (the 3-channel arrays only)"
    a = arrays[spec['png'][rel]]
    assert a.ndim == 3 and a.shape[2] == 3
    return a
