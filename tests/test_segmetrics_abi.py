"""Segmentation metrics (csrc/segmetrics.hip; utils/metrics.py:7-86 of the reference's downstream/semantic_segmentation) without
a GPU: the three C entry points are declared and exported, refuse every documented bad argument on the host before any HIP call,
the Python ops and ConfMatrix refuse host tensors, and pretrain.evaluate_batch exists beside an unchanged PretrainStep."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib

I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p


def test_header_declares_and_library_exports_the_three_entry_points():
    protos = _lib.parse_header()
    want = {
        "mmae_argmax_confusion": [I] * 7 + [P] * 3 + [I, I, L, P, P],
        "mmae_label_confusion": [L, P, P, I, L, P, P],
        "mmae_confusion_scores": [I, P, P, P],
    }
    for name, argt in want.items():
        assert name in protos, name
        ret, got = protos[name]
        assert ret is ctypes.c_int and got == argt, name
        assert callable(getattr(_lib.lib(), name))
    assert _lib.lib().mmae_abi_version() == 7          # additive entry points: the version stays


def test_invalid_arguments_return_err_arg_without_launch():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16       # a HOST address: were anything launched, it would fault instead of returning -1
    p, null = P(a16), P(None)

    # every call below breaks exactly one rule; all other arguments are valid (a call with none broken would launch)
    def am(dtype=1, tokens=1, B=2, C=9, H=64, W=48, patch=16, pred=p, target=p, mask=None, K=9, off=0, ign=-1, conf=p):
        return l.mmae_argmax_confusion(dtype, tokens, B, C, H, W, patch, pred, target, mask, K, off, ign, conf, None)
    assert am(K=0) == -1 and am(K=129) == -1 and am(K=-1) == -1
    assert am(C=0) == -1
    assert am(patch=6, H=48, W=48) == -1 and am(patch=0) == -1         # patch a positive multiple of 4
    assert am(H=72) == -1 and am(W=40) == -1                           # H, W multiples of patch
    assert am(dtype=1, tokens=0) == -1                                 # the image form is fp32 only
    assert am(dtype=2) == -1
    assert am(off=-1) == -1
    assert am(B=0) == -1
    assert am(B=32768, H=256, W=256) == -1                             # B*H*W = 2^31
    assert am(B=1, H=65536, W=65536) == -1                             # H*W alone past 2^31
    assert am(pred=null) == -1 and am(target=null) == -1 and am(conf=null) == -1
    assert am(pred=P(a16 + 8)) == -1 and am(target=P(a16 + 8)) == -1   # 16 bytes per lane: aligned operands

    def lc(n=100, gt=p, pred=p, K=7, ign=0, conf=p):
        return l.mmae_label_confusion(n, gt, pred, K, ign, conf, None)
    assert lc(n=0) == -1 and lc(n=-5) == -1 and lc(n=1 << 31) == -1
    assert lc(K=0) == -1 and lc(K=129) == -1
    assert lc(gt=null) == -1 and lc(pred=null) == -1 and lc(conf=null) == -1

    def sc(K=7, conf=p, out=p):
        return l.mmae_confusion_scores(K, conf, out, None)
    assert sc(K=0) == -1 and sc(K=129) == -1
    assert sc(conf=null) == -1 and sc(out=null) == -1
    for _ in range(3):                                                 # nothing launched: no error left behind
        assert l.mmae_last_hip_error() == 0


def test_ops_and_confmatrix_refuse_host_tensors():
    from incomplete_multimodal_fusion_amd import metrics, ops
    E = _lib.MmaeLibraryError
    tgt = torch.zeros(2, 32, 32, dtype=torch.int64)
    with pytest.raises(E):
        ops.argmax_confusion(torch.randn(2, 5, 32, 32), tgt, None, 5, 16)
    with pytest.raises(E):
        ops.argmax_confusion((torch.randn(8, 5 * 256).bfloat16(), 5), tgt, torch.ones(2, 4, dtype=torch.int64), 5, 16)
    with pytest.raises(E):
        ops.label_confusion(tgt, tgt, 5)
    with pytest.raises(E):
        ops.confusion_scores(torch.zeros(5, 5, dtype=torch.int64))
    cm = metrics.ConfMatrix(7, device="cpu")                           # a host-only state: nothing can be counted into it
    assert cm.state.shape == (7, 7) and cm.state.dtype == torch.int64
    with pytest.raises(E):
        cm.add_batch(np.ones((2, 64, 64), dtype=np.uint8), np.ones((2, 64, 64), dtype=np.uint8))
    with pytest.raises(E):
        cm.add_logits(torch.randn(2, 7, 32, 32), tgt)
    with pytest.raises(E):
        cm.scores()
    with pytest.raises(E):
        cm.get_mIoU()
    for name in ("add", "add_batch", "calc", "get_existing_classes", "norm_on_lines", "get_aa", "get_sa", "get_cf", "get_IoU",
                 "get_mIoU", "add_logits", "scores"):
        assert callable(getattr(metrics.ConfMatrix, name)), name
    for name in ("AA", "IoU", "mIoU"):
        assert callable(getattr(metrics, name)), name


def test_evaluate_batch_signature_and_unchanged_pretrain_step():
    from incomplete_multimodal_fusion_amd import pretrain
    sig = inspect.signature(pretrain.evaluate_batch).parameters
    assert list(sig) == ["model", "tasks_dict", "loss_fns", "conf", "num_encoded_tokens", "task_masks", "patch_size", "alphas",
                         "loss_on_unmasked"]
    defaults = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"loss_fns": None, "conf": None, "num_encoded_tokens": None, "task_masks": None, "patch_size": 16,
                        "alphas": 1.0, "loss_on_unmasked": False}
    step = inspect.signature(pretrain.PretrainStep.__init__).parameters
    assert [(k, v.default) for k, v in step.items()][1:] == [
        ("model", inspect.Parameter.empty), ("optimizer", inspect.Parameter.empty), ("num_encoded_tokens", inspect.Parameter.empty),
        ("in_domains", None), ("alphas", 1.0), ("sample_tasks_uniformly", False), ("autocast", True), ("patch_size", 16),
        ("grad_reducer", None), ("side_stream_wgrad", False), ("clip_grad", None), ("skip_grad", None), ("contra", "dino"),
        ("contra_weight", None), ("loss_balancer", None), ("check_finite", True), ("balancer_lr_scale", 1.0),
        ("standardize_depth", False), ("loss_on_unmasked", False)]
