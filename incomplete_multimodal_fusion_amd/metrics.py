"""Segmentation metrics with the state on the device: the surface of the reference's
downstream/semantic_segmentation/utils/metrics.py:7-124 (ConfMatrix, AA, IoU, mIoU; driven from maskformer_train_seg.py:243-281)
on the kernels of csrc/segmetrics.hip.

The reference copies every prediction to the host and calls sklearn's confusion_matrix per 64 x 64 image.  Here add / add_batch /
add_logits launch one kernel each and never synchronise with the host; only the get_* methods (numpy float64 results, as the
reference returns them) and the module functions AA / IoU / mIoU read the matrix back.

Beyond the reference:
  add_logits(pred, gt, mask=None, ...): the fused path -- argmax over the logits and the counting in one kernel, on the fp32 logit
    image or on the decoder's token-major output (multimae_crossattn.PredTokens), optionally over the masked patches only;
  scores(): the device tensor of ops.confusion_scores (mIoU, AA, overall accuracy, existing classes, per-class IoU and recall).

Deliberate deviations:
  * `state` is a (K, K) int64 tensor on the device; the reference keeps float64 numpy.  Counts are exact either way;
  * the leftover `assert gt.shape == (64, 64)` of metrics.py:26 is not mirrored: any shape counts;
  * calc() returns the int64 matrix as a device tensor, not numpy, so that it does not synchronise;
  * there is no CPU path: a ConfMatrix whose state is on the host raises _lib.MmaeLibraryError at the first count.
"""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops


def _on(x, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device, non_blocking=True)


class ConfMatrix:
    def __init__(self, num_classes: int, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.MmaeLibraryError("ConfMatrix keeps its state on the device and no GPU is available; there is no CPU path")
            device = torch.device("cuda", torch.cuda.current_device())
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        self.state = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=self.device)

    # -- counting: no host synchronisation ----------------------------------------------------------------------------
    def calc(self, gt, pred):
        """The confusion matrix of one pair, no ignore label, the state untouched (metrics.py:13-17): (K, K) int64 on the device."""
        return ops.label_confusion(_on(gt, self.device), _on(pred, self.device), self.num_classes, ignore_label=-1)

    def add(self, gt, pred):
        """Adds one label mask; pixels with gt == 0 are dropped (metrics.py:22-39)."""
        assert tuple(gt.shape) == tuple(pred.shape)
        ops.label_confusion(_on(gt, self.device), _on(pred, self.device), self.num_classes, conf=self.state, ignore_label=0)
        return None

    def add_batch(self, gt, pred):
        """Adds a (B, H, W) batch of label masks in one launch (metrics.py:41-55)."""
        assert len(gt.shape) == 3
        return self.add(gt, pred)

    def add_logits(self, pred, gt, mask=None, pred_offset: int = 0, ignore_label: int = 0, patch: Optional[int] = None):
        """The fused path: state[gt, argmax_c(pred) + pred_offset] += 1 over the pixels of the patches with mask == 1 (all
        patches without a mask), gt == ignore_label dropped (negative: none).  pred: (B, C, H, W) fp32 logits or PredTokens;
        gt (B, H, W).  patch: taken from the PredTokens, from the mask's (B, P) shape, or given."""
        gt = _on(gt, self.device)
        if mask is not None:
            mask = _on(mask, self.device)
        if hasattr(pred, "tokens") and hasattr(pred, "meta"):
            patch = pred.meta[4] if patch is None else patch
        else:
            pred = _on(pred, self.device)
            if patch is None:
                patch = _infer_patch(tuple(pred.shape), mask)
        ops.argmax_confusion(pred, gt, mask, self.num_classes, patch, conf=self.state, pred_offset=pred_offset,
                             ignore_label=ignore_label)
        return None

    def scores(self) -> torch.Tensor:
        """(4 + 2K,) float64 on the device, see ops.confusion_scores.  No host synchronisation."""
        return ops.confusion_scores(self.state)

    # -- results: numpy float64 like the reference; these synchronise --------------------------------------------------
    def _host_scores(self):
        return self.scores().cpu().numpy()

    def get_existing_classes(self):
        return int(self._host_scores()[3])

    def norm_on_lines(self):
        a = self.state.cpu().numpy().astype(np.float64)
        b = np.sum(a, axis=1)[:, None]
        return np.divide(a, b, out=np.zeros_like(a), where=b != 0)

    def get_aa(self):
        return self._host_scores()[1]

    def get_sa(self):
        K = self.num_classes
        return self._host_scores()[4 + K:4 + 2 * K].copy()

    def get_cf(self):
        return self.norm_on_lines()

    def get_IoU(self):
        K = self.num_classes
        return self._host_scores()[4:4 + K].copy()

    def get_mIoU(self):
        return self._host_scores()[0]


def _infer_patch(shape, mask):
    """A patch size for a logit image: the one the (B, P) mask implies, else any size the kernel takes (16 fills a wave)."""
    if len(shape) != 4:
        raise ValueError("add_logits: a (B, C, H, W) logit image expected (got shape %s)" % (shape,))
    _, _, H, W = shape
    if mask is not None:
        P = mask.numel() // max(shape[0], 1)
        for p in range(4, min(H, W) + 1, 4):
            if H % p == 0 and W % p == 0 and (H // p) * (W // p) == P:
                return p
        raise ValueError("add_logits: no patch size fits a mask of %d patches on a %d x %d image; pass patch=" % (P, H, W))
    for p in (16, 32, 8, 4):
        if H % p == 0 and W % p == 0:
            return p
    raise ValueError("add_logits: H and W must be multiples of 4 (got %d x %d)" % (H, W))


def AA(gt, pred, num_classes, device=None):
    """Mean over ALL classes of the row-normalised diagonal, gt == 0 dropped (metrics.py:89-97)."""
    cm = ConfMatrix(num_classes, device)
    cm.add(gt, pred)
    return np.mean(np.diagonal(cm.norm_on_lines()))


def IoU(gt, pred, num_classes, device=None):
    """Per-class intersection over union of one pair, nothing ignored; 0 / 0 is NaN as in the reference (metrics.py:100-120)."""
    cm = ConfMatrix(num_classes, device).calc(gt, pred).cpu().numpy().astype(np.float64)
    d = np.diagonal(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        return d / (cm.sum(axis=1) + cm.sum(axis=0) - d)


def mIoU(gt, pred, num_classes, device=None):
    return np.mean(IoU(gt, pred, num_classes, device))
