"""Truncated depth standardisation (pretrain_mmae.py:452-458, --standardize_depth) without a GPU: the C entry point is declared and
exported, refuses bad arguments on the host before any HIP call, the Python op refuses host tensors, and PretrainStep carries the
driver's two switches, off by default."""
import ctypes
import inspect

import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib


def test_header_declares_and_library_exports_trunc_standardize():
    protos = _lib.parse_header()
    assert "mmae_trunc_standardize" in protos
    ret, argt = protos["mmae_trunc_standardize"]
    assert ret is ctypes.c_int
    assert argt == [ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_float] + [ctypes.c_void_p] * 5
    assert callable(getattr(_lib.lib(), "mmae_trunc_standardize"))


def test_invalid_arguments_return_err_arg_without_launch():
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))    # a HOST address: were anything launched, it would fault instead of returning -1
    P = ctypes.c_void_p

    def call(B=1, n=10, k_lo=1, k_hi=9, x=p, y=p):
        return l.mmae_trunc_standardize(B, n, k_lo, k_hi, 1e-6, x, y, None, None, None)
    assert call(x=P(None)) == -1
    assert call(y=P(None)) == -1
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(k_lo=-1) == -1
    assert call(k_hi=11) == -1                    # k_hi > n
    assert call(k_lo=4, k_hi=5) == -1             # fewer than 2 values in the slice
    assert call(k_lo=5, k_hi=5) == -1 and call(k_lo=6, k_hi=5) == -1
    assert call(n=1 << 31, k_lo=1, k_hi=9) == -1  # more than 2^31 - 1 values per sample
    for _ in range(3):                            # nothing launched: no error left behind
        assert l.mmae_last_hip_error() == 0


def test_op_refuses_host_tensors():
    from incomplete_multimodal_fusion_amd import ops
    with pytest.raises(_lib.MmaeLibraryError):
        ops.trunc_standardize(torch.randn(2, 1, 16, 16))
    with pytest.raises(_lib.MmaeLibraryError):
        ops.trunc_standardize(torch.randn(2, 256), return_stats=True)


def test_pretrain_step_has_both_switches_off_by_default():
    from incomplete_multimodal_fusion_amd.pretrain import PretrainStep, standardize_depth, step_losses
    sig = inspect.signature(PretrainStep.__init__).parameters
    for name in ("standardize_depth", "loss_on_unmasked"):
        assert name in sig and sig[name].default is False, name
    assert inspect.signature(step_losses).parameters["loss_on_unmasked"].default is False
    assert callable(standardize_depth)
