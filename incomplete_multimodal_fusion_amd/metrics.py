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

The Mask2Former tail of the same evaluation loop (maskformer_train_seg.py:258-308), on the kernel of csrc/query_semseg.hip:
  semantic_inference(mask_cls, mask_pred, size=None): the reference's method, with the bilinear resize folded in;
  ConfMatrix.add_queries(pred_logits, pred_masks, gt): the body of evaluate(mode='eval') in one launch;
  dice(pred_logits, pred_masks, target): the other mode's _get_dice, for every sample of the batch.

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

    def add_queries(self, pred_logits, pred_masks, gt, void_index: int = 0, pred_offset: int = 1, ignore_label: int = 0):
        """evaluate(mode='eval') of maskformer_train_seg.py:258-270 in one launch: the masks (B, Q, h, w) resized bilinearly to
        gt's (H, W), sigmoid, mixed by softmax(pred_logits (B, Q, K1)) without column void_index, and
        state[gt, argmax + pred_offset] += 1.  The defaults are the reference's: class 0 dropped, + 1, gt == 0 ignored."""
        ops.query_confusion(_on(pred_logits, self.device), _on(pred_masks, self.device), _on(gt, self.device), self.num_classes,
                            conf=self.state, void_index=void_index, pred_offset=pred_offset, ignore_label=ignore_label)
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


def semantic_inference(mask_cls, mask_pred, size=None):
    """semantic_inference of maskformer_train_seg.py:304-308: softmax(mask_cls, -1)[..., 1:] mixed with mask_pred.sigmoid() by
    einsum("bqc,bqhw->bchw") (batched: (B, Q, K1) and (B, Q, h, w)) or "qc,qhw->chw" (per image: (Q, K1) and (Q, h, w), the form of
    mask2former_infer_seg.py).  The reference resizes the masks before the call; here `size` = (H, W) folds that
    F.interpolate(..., mode="bilinear", align_corners=False) in, None keeps the masks' size.  fp32 scores on the device."""
    if mask_cls.dim() == 2:
        return ops.query_semseg(mask_cls[None], mask_pred[None], size=size, void_index=0)[0]
    return ops.query_semseg(mask_cls, mask_pred, size=size, void_index=0)


def dice(pred_logits, pred_masks, target, smooth: float = 1e-5):
    """_get_dice of maskformer_train_seg.py:287-295 on semantic_inference's scores and the one-hot target without class 0
    (:297-302), masks resized to target's (H, W): element b is sum_c(2 * num_c + smooth) / sum_c(den_c + smooth) of sample b, with
    num_c = sum(p_c * t_c) and den_c = sum(p_c) + sum(t_c) over the pixels.  Returns a (B,) float64 device tensor without a host
    synchronisation.  The reference only ever evaluates sample 0 of a batch (`pred_masks[0]`, `target[0]`, :272-274): that is
    dice(...)[0]."""
    s = ops.query_dice_sums(pred_logits, pred_masks, target, void_index=0, label_offset=1)
    num, den = s[..., 0], s[..., 1] + s[..., 2]
    return (2 * num + smooth).sum(-1) / (den + smooth).sum(-1)


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
