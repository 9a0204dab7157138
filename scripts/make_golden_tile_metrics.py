"""Writes tests/golden/f10_crop_center.json from the reference's own validation_utils/val_utils.py:crop_center (numpy only).

    python scripts/make_golden_tile_metrics.py --reference <checkout of the reference project>

Per case: the input shape, the target side, the output shape and the four corner values (per channel) of the crop of an
``arange`` image -- together they pin the crop's offsets.  Only these numbers are stored; nothing of the reference's text is.
"""
import argparse
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((3, 256, 256), 240), ((1, 256, 256), 240), ((3, 67, 93), 41), ((1, 67, 93), 40), ((12, 12), 12), ((64, 64), 48),
         ((2, 9, 8), 3), ((31, 50), 7), ((1, 276, 276), 256), ((4, 5, 5), 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "f10_crop_center.json"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_val_utils", os.path.join(a.reference, "validation_utils", "val_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cases = []
    for shape, target in CASES:
        im = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
        out = mod.crop_center(im, target)
        corners = np.stack([out[..., 0, 0], out[..., 0, -1], out[..., -1, 0], out[..., -1, -1]], axis=-1)
        cases.append({"shape": list(shape), "target": target, "out_shape": list(out.shape), "corners": corners.tolist()})
    with open(a.out, "w") as f:
        json.dump({"source": "validation_utils/val_utils.py:crop_center", "cases": cases}, f, indent=1)
    print("wrote", a.out, len(cases), "cases")


if __name__ == "__main__":
    main()
