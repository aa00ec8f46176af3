"""Error behaviour of the C ABI (include/mmae_hip.h): every entry point validates its arguments on the host BEFORE any HIP
call and returns MMAE_ERR_ARG (-1) -- so these run without a GPU.  The Python binding turns a non-zero code into
MmaeLibraryError; host tensors are refused (there is no CPU path)."""
import ctypes

import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib

QUERIES = {"mmae_abi_version", "mmae_last_hip_error", "mmae_modattn_bwd_nsplit",
           "mmae_add_ln_bwd_ws_floats", "mmae_hardneg_ws_floats", "mmae_mha_bwd_ws_floats",
           "mmae_gemm_nt_supported", "mmae_gemm_geglu_supported", "mmae_gemm_tn_supported", "mmae_gemm_tn_ws_floats",
           "mmae_mha_bwd_fused_supported", "mmae_mha_bwd_fused_ws_floats"}           # setters / size / shape queries: no pointers to validate


def test_every_entry_point_rejects_null_pointers():
    l = _lib.lib()
    for name, (_, argt) in _lib.parse_header().items():
        if name in QUERIES:
            continue
        args = [None if a is ctypes.c_void_p else a(0) for a in argt]
        assert getattr(l, name)(*args) == -1, name


def test_attention_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    a16 = (a + 15) // 16 * 16
    P = ctypes.c_void_p

    def fwd(dtype=1, dh=64, B=1, H=8, nseg=4, q=a16, stride=1536, seg=a16, rows=64):
        return l.mmae_mha_fwd(dtype, dh, B, H, nseg, P(q), P(a16), P(a16), P(a16), P(a16), stride, stride, stride, 512, rows,
                              P(seg), P(a16), P(a16), P(a16), 64, 64, 0.125, 0, None)
    assert fwd(dh=48) == -1                 # head_dim 32 / 64 only
    assert fwd(dtype=7) == -1               # fp32 / bf16 only
    assert fwd(q=a16 + 2) == -1             # operands must be 16-byte aligned
    assert fwd(stride=1531) == -1           # row strides in multiples of 8 elements
    assert fwd(B=0) == -1 and fwd(H=0) == -1 and fwd(nseg=0) == -1
    assert fwd(seg=0) == -1                 # missing segment table
    assert fwd(rows=0) == -1


def test_modattn_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p

    # every call below breaks exactly one rule; all other arguments are valid (a call with none broken would launch)
    def fwd(dtype=1, dh=64, B=2, Pn=4, ns=4, I=512, q=a16, kv=a16, out=a16, qs=512, kvs=1024, os_=512):
        return l.mmae_modattn_fwd(dtype, dh, B, Pn, ns, I, P(q), qs, P(kv), kvs, P(a16), P(out), os_, 0.125, None)

    def bwd(dtype=1, dh=64, B=2, Pn=4, ns=4, I=512, q=a16, kv=a16, dout=a16, dq=a16, dkv=a16, qs=512, kvs=1024, dos=512,
            dqs=512, dkvs=1024, shared_base=0):
        return l.mmae_modattn_bwd(dtype, dh, B, Pn, ns, I, P(q), qs, P(kv), kvs, P(a16), P(dout), dos, P(dq), dqs, P(dkv),
                                  dkvs, shared_base, 0.125, P(a16), None)
    for f in (fwd, bwd):
        assert f(ns=0) == -1 and f(ns=9) == -1              # 1 <= M+1 <= 8 slots
        assert f(I=1040) == -1 and f(I=1056, dh=32) == -1 and f(I=1088, dh=64) == -1   # at most two 512-column chunks
        assert f(I=520) == -1 and f(I=528, dh=64) == -1     # inner a multiple of head_dim
        assert f(dh=48, I=480) == -1                        # head_dim 32 / 64 only
        assert f(dtype=7) == -1                             # fp32 / bf16 only
        assert f(B=0) == -1 and f(Pn=0) == -1 and f(I=0) == -1
        assert f(qs=516) == -1 and f(kvs=1028) == -1        # row strides in multiples of 8 elements
        assert f(q=a16 + 2) == -1 and f(kv=a16 + 8) == -1   # operands 16-byte aligned
    assert fwd(os_=1020) == -1 and fwd(out=a16 + 4) == -1
    assert bwd(dos=508) == -1 and bwd(dqs=4) == -1 and bwd(dkvs=1030) == -1
    assert bwd(dout=a16 + 4) == -1 and bwd(dq=a16 + 2) == -1 and bwd(dkv=a16 + 8) == -1
    assert bwd(shared_base=-1) == -1
    assert l.mmae_modattn_bwd_nsplit(1) == 1 and l.mmae_modattn_bwd_nsplit(64) == 2
    assert l.mmae_modattn_bwd_nsplit(256) == 8 and l.mmae_modattn_bwd_nsplit(600) == 16


def test_row_kernel_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p
    assert l.mmae_geglu_fwd(9, 16, 2048, P(a16), P(a16), None) == -1          # dtype
    assert l.mmae_adamw_step(6, P(a16), P(a16), P(a16), P(a16), None, 1e-3, 0.9, 0.95, 1e-8, 0.05, 1, 1.0, None) == -1  # n % 4
    assert l.mmae_adamw_step(8, P(a16), P(a16), P(a16), P(a16), None, 1e-3, 0.9, 0.95, 1e-8, 0.05, 0, 1.0, None) == -1  # step >= 1
    assert l.mmae_splitk_sum(0, 64, P(a16), P(a16), None) == -1               # S >= 1
    assert l.mmae_splitk_sum(2, 60, P(a16), P(a16), None) == -1               # n % 8
    off = (ctypes.c_long * 15)()
    assert l.mmae_descriptor_layout(2, 3, 16, 24, off) == off[14] > 0
    assert l.mmae_descriptor_layout(-1, 3, 16, 24, off) == -1


def test_gemm_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p
    ok = lambda *a: l.mmae_gemm_nt_supported(*a)
    assert ok(163840, 4096, 768, 768, 768, 4096) == 1 and ok(1000, 256, 384, 384, 384, 256) == 1
    assert ok(1024, 300, 768, 768, 768, 300) == 0 and ok(1024, 256, 320, 320, 320, 256) == 0 and ok(1024, 256, 768, 760, 768, 256) == 0
    assert l.mmae_gemm_nt(1024, 256, 768, P(a16), 768, P(a16), 768, P(a16 + 4), 256, None) == -1      # C must be 8-byte aligned
    assert l.mmae_gemm_nt(1024, 256, 768, P(a16 + 8), 768, P(a16), 768, P(a16), 256, None) == -1      # A must be 16-byte aligned
    assert l.mmae_gemm_nt(1024, 250, 768, P(a16), 768, P(a16), 768, P(a16), 250, None) == -1
    assert l.mmae_gemm_geglu_supported(4096, 2048, 768, 768, 768, 4096, 2048) == 1
    assert l.mmae_gemm_geglu_supported(4096, 2000, 768, 768, 768, 4000, 2000) == 0                    # F % 128
    assert l.mmae_gemm_geglu(4096, 2048, 768, P(a16), 768, P(a16), 768, P(a16), 4096, None, 2048, None) == -1
    assert l.mmae_mha_bwd_ws_floats(8, 1000) == 24000 and l.mmae_mha_bwd_ws_floats(0, 5) == -1


def test_binding_raises_and_refuses_host_tensors():
    with pytest.raises(_lib.MmaeLibraryError, match="invalid argument"):
        _lib.call("mmae_shadow_bf16", 6, None, None, None)
    with pytest.raises(_lib.MmaeLibraryError, match="no CPU path"):
        _lib.ptr(torch.zeros(4))
    with pytest.raises(_lib.MmaeLibraryError, match="unsupported dtype"):
        _lib.dt(torch.float16)


def test_image_and_loss_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p
    nan = float("nan")

    # every call below breaks exactly one rule; all other arguments are valid (a call with none broken would launch)
    def patchify(dtype=1, nmod=3, chans=(1, 3, 1), cols=(0, 256, 1024), onehot=1280, Kcat=1288, H=64, W=64, patch=16,
                 tok_mod=a16, tok_patch=a16):
        n = max(nmod, 1)
        imgs = (ctypes.c_void_p * n)(*([a16] * n))
        ch = (ctypes.c_int * n)(*(list(chans) + [1] * n)[:n])
        co = (ctypes.c_int * n)(*(list(cols) + [0] * n)[:n])
        return l.mmae_patchify_gather(dtype, nmod, P(ctypes.addressof(imgs)), P(ctypes.addressof(ch)), P(ctypes.addressof(co)),
                                      onehot, Kcat, 2, H, W, patch, P(tok_mod), P(tok_patch), 24, P(a16), None)
    assert patchify(nmod=0) == -1 and patchify(nmod=9, chans=(1,) * 9, cols=tuple(16 * i for i in range(9))) == -1
    assert patchify(dtype=2) == -1                                          # fp32 / bf16 output only
    assert patchify(patch=6, H=60, W=60) == -1                              # patch a multiple of 4
    assert patchify(H=72) == -1 and patchify(W=40) == -1                    # H, W multiples of patch
    assert patchify(cols=(0, 258, 1024)) == -1                              # column offsets multiples of 4
    assert patchify(cols=(0, 256, 1036)) == -1                              # slot [1036, 1292) past Kcat 1288
    assert patchify(onehot=1286) == -1                                      # one-hot offset a multiple of 4
    assert patchify(onehot=1288) == -1                                      # one-hot block [1288, 1291) past Kcat 1288
    assert patchify(Kcat=1290) == -1                                        # Kcat % 4
    assert patchify(tok_mod=0) == -1 and patchify(tok_patch=0) == -1        # both descriptor tables or neither
    assert patchify(chans=(1, 0, 1)) == -1

    def unpatchify(dtype=1, C=3, H=64, W=64, patch=16):
        return l.mmae_unpatchify(dtype, 2, C, H, W, patch, P(a16), P(a16), None)
    assert unpatchify(patch=6, H=60, W=60) == -1 and unpatchify(H=72) == -1 and unpatchify(W=40) == -1
    assert unpatchify(dtype=2) == -1 and unpatchify(C=0) == -1

    def loss(which, dtype=1, tokens=1, kind=0, B=2, C=3, H=64, W=48, patch=16):
        if which == "fwd":
            return l.mmae_masked_loss_fwd(dtype, tokens, kind, B, C, H, W, patch, P(a16), P(a16), None, P(a16), P(a16), P(a16),
                                          None)
        return l.mmae_masked_loss_bwd(dtype, tokens, kind, B, C, H, W, patch, P(a16), P(a16), None, P(a16), P(a16), P(a16),
                                      P(a16), None)

    def ce(which, dtype=1, tokens=1, smooth=0.1, B=2, C=9, H=64, W=48, patch=16):
        if which == "fwd":
            return l.mmae_masked_ce_loss_fwd(dtype, tokens, B, C, H, W, patch, P(a16), P(a16), None, smooth, P(a16), P(a16),
                                             P(a16), None)
        return l.mmae_masked_ce_loss_bwd(dtype, tokens, B, C, H, W, patch, P(a16), P(a16), None, smooth, P(a16), P(a16), P(a16),
                                         P(a16), None)
    for w in ("fwd", "bwd"):
        for f in (lambda **k: loss(w, **k), lambda **k: ce(w, **k)):
            assert f(patch=6, H=48, W=48) == -1 and f(patch=0) == -1        # patch a positive multiple of 4
            assert f(H=72) == -1 and f(W=40) == -1                          # H, W multiples of patch
            assert f(tokens=0) == -1                                        # the image form is fp32 only (bf16 pred)
            assert f(dtype=2) == -1 and f(B=0) == -1 and f(C=0) == -1
        assert loss(w, kind=2) == -1 and loss(w, kind=-1) == -1             # 0 MSE, 1 L1
        assert ce(w, smooth=-0.01) == -1 and ce(w, smooth=1.01) == -1 and ce(w, smooth=nan) == -1

    def dino(which, B=4, D=256):
        if which == "fwd":
            return l.mmae_dino_loss_fwd(B, D, P(a16), P(a16), 0.1, 0.04, P(a16), P(a16), None)
        return l.mmae_dino_loss_bwd(B, D, P(a16), P(a16), 0.1, 0.04, P(a16), P(a16), None)

    def hardneg(which, B=4, D=64):
        if which == "fwd":
            return l.mmae_hardneg_loss_fwd(B, D, P(a16), P(a16), 0.1, 1.0, 0.5, P(a16), P(a16), None)
        return l.mmae_hardneg_loss_bwd(B, D, P(a16), P(a16), 0.1, 1.0, 0.5, P(a16), P(a16), P(a16), P(a16), None)
    for w in ("fwd", "bwd"):
        assert dino(w, D=258) == -1 and dino(w, D=1028) == -1               # D % 4 == 0, D <= 1024 (4 chunks of 64 x 4)
        assert dino(w, B=0) == -1 and dino(w, D=0) == -1
        assert hardneg(w, B=1) == -1 and hardneg(w, B=0) == -1              # at least one negative pair: B >= 2
        assert hardneg(w, D=0) == -1
