#!/usr/bin/env python
"""Writes tests/golden/metrics.npz: the reference's own ConfMatrix(7) (downstream/semantic_segmentation/utils/metrics.py:7-86, on
sklearn's confusion_matrix) run over six seeded 64 x 64 label pairs.  The reference module is loaded by file path from the
reference checkout (oracle/ref_loader.py's REF_ROOT, MMAE_REFERENCE_ROOT); needs sklearn.  Run by hand; no test imports this file.

The maps: ground truth over {0 .. 6} with class 0 the reference's ignored label (metrics.py:32-33) on ~15 % of the pixels, class 5
never present (an absent class: zero row), and a prediction that agrees with the ground truth on ~70 % of the pixels and is
uniform over {0 .. 6} elsewhere (so class 5 is predicted although it never occurs).  The fixture holds numeric arrays only."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_loader import REF_ROOT  # noqa: E402
K, N, SIDE = 7, 6, 64


def load_reference_metrics():
    path = os.path.join(REF_ROOT, "downstream", "semantic_segmentation", "utils", "metrics.py")
    spec = importlib.util.spec_from_file_location("_ref_seg_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference_metrics()
    rng = np.random.default_rng(20231)
    present = np.array([1, 2, 3, 4, 6])
    gt = present[rng.integers(0, len(present), size=(N, SIDE, SIDE))]
    gt[rng.random((N, SIDE, SIDE)) < 0.15] = 0
    gt[3, :8] = 0                                                       # a block of ignored pixels
    noise = rng.integers(0, K, size=(N, SIDE, SIDE))
    pred = np.where(rng.random((N, SIDE, SIDE)) < 0.7, gt, noise)
    gt, pred = gt.astype(np.uint8), pred.astype(np.uint8)
    assert not (gt == 5).any() and (pred == 5).any() and (gt == 0).any()

    cm = ref.ConfMatrix(K)
    cm.add_batch(gt[:3], pred[:3])                                     # two calls: the state accumulates
    cm.add_batch(gt[3:], pred[3:])
    out = {
        "gt": gt, "pred": pred,
        "state": cm.state.astype(np.int64),
        "aa": np.float64(cm.get_aa()), "sa": np.asarray(cm.get_sa(), dtype=np.float64),
        "iou": np.asarray(cm.get_IoU(), dtype=np.float64), "miou": np.float64(cm.get_mIoU()),
        "cf": np.asarray(cm.get_cf(), dtype=np.float64), "existing": np.float64(cm.get_existing_classes()),
        "calc0": np.asarray(cm.calc(gt[0], pred[0]), dtype=np.int64),
    }
    assert np.array_equal(out["state"], cm.state)                      # the float64 counts are integers
    path = os.path.join(ROOT, "tests", "golden", "metrics.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; existing %d, mIoU %.6f, AA %.6f" % (path, os.path.getsize(path), out["existing"], out["miou"], out["aa"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
