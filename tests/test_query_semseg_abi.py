"""Mask2Former semantic inference (csrc/query_semseg.hip; maskformer_train_seg.py:258-308 of the reference's
downstream/semantic_segmentation) without a GPU: the four C entry points are declared and exported, refuse every documented bad
argument on the host before any HIP call, and the Python wrappers refuse host tensors."""
import ctypes

import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib

I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p


def test_header_declares_and_library_exports_the_four_entry_points():
    protos = _lib.parse_header()
    want = {
        "mmae_query_semseg": (I, [I] * 9 + [P, P, I, P, P, I, P]),
        "mmae_query_confusion": (I, [I] * 9 + [P, P, I, P, I, I, L, P, P]),
        "mmae_query_dice_ws_floats": (L, [I] * 4),
        "mmae_query_dice": (I, [I] * 9 + [P, P, I, P, I, P, P, P]),
    }
    for name, (ret, argt) in want.items():
        assert name in protos, name
        assert protos[name] == (ret, argt), name
        assert callable(getattr(_lib.lib(), name))
    assert _lib.lib().mmae_abi_version() == 7          # additive entry points: the version stays


def test_invalid_arguments_return_err_arg_without_launch():
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)                          # a HOST address: were anything launched, it would fault instead of returning -1
    p, null = P(a), P(None)

    # every call below breaks exactly one rule; all other arguments are valid (a call with none broken would launch)
    def common(f):
        assert f(ldt=2) == -1 and f(mdt=2) == -1                           # fp32 / bf16 only, each input on its own
        assert f(Q=0) == -1 and f(Q=257) == -1
        assert f(K1=66, void=0) == -1 and f(K1=65, void=-1) == -1          # 65 kept classes
        assert f(K1=1, void=0) == -1                                       # no kept class
        assert f(void=10) == -1 and f(void=-2) == -1                       # void_index in [-1, K1)
        assert f(h=0) == -1 and f(w=0) == -1 and f(H=0) == -1 and f(W=0) == -1 and f(B=0) == -1
        assert f(B=32768, H=256, W=256) == -1                              # B*H*W = 2^31
        assert f(logits=null) == -1 and f(masks=null) == -1

    def sem(ldt=0, mdt=1, B=2, Q=10, K1=10, h=16, w=16, H=64, W=64, logits=p, masks=p, void=0, scores=p, labels=p, off=1):
        return l.mmae_query_semseg(ldt, mdt, B, Q, K1, h, w, H, W, logits, masks, void, scores, labels, off, None)
    common(sem)
    assert sem(scores=null, labels=null) == -1                             # at least one output

    def con(ldt=0, mdt=1, B=2, Q=10, K1=10, h=16, w=16, H=64, W=64, logits=p, masks=p, void=0, target=p, Kc=10, off=1, ign=0,
            conf=p):
        return l.mmae_query_confusion(ldt, mdt, B, Q, K1, h, w, H, W, logits, masks, void, target, Kc, off, ign, conf, None)
    common(con)
    assert con(Kc=0) == -1 and con(Kc=129) == -1
    assert con(target=null) == -1 and con(conf=null) == -1

    def dice(ldt=0, mdt=1, B=2, Q=10, K1=10, h=16, w=16, H=64, W=64, logits=p, masks=p, void=0, target=p, off=1, ws=p, sums=p):
        return l.mmae_query_dice(ldt, mdt, B, Q, K1, h, w, H, W, logits, masks, void, target, off, ws, sums, None)
    common(dice)
    assert dice(target=null) == -1 and dice(ws=null) == -1 and dice(sums=null) == -1

    ws = l.mmae_query_dice_ws_floats
    assert ws(2, 10, 64, 64) >= 2 * 16 * 9 * 3                             # at least one (K, 3) block per 16 x 16 tile
    assert ws(3, 3, 23, 17) > 0
    assert ws(0, 10, 64, 64) == -1 and ws(2, 0, 64, 64) == -1 and ws(2, 10, 0, 64) == -1 and ws(2, 10, 64, 0) == -1
    assert ws(32768, 10, 256, 256) == -1
    for _ in range(3):                                                     # nothing launched: no error left behind
        assert l.mmae_last_hip_error() == 0


def test_wrappers_refuse_host_tensors():
    from incomplete_multimodal_fusion_amd import metrics, ops
    E = _lib.MmaeLibraryError
    lg, mk = torch.randn(2, 5, 4), torch.randn(2, 5, 8, 8)
    tgt = torch.zeros(2, 16, 16, dtype=torch.int64)
    with pytest.raises(E):
        ops.query_semseg(lg, mk, size=(16, 16))
    with pytest.raises(E):
        ops.query_labels(lg.bfloat16(), mk.bfloat16())
    with pytest.raises(E):
        ops.query_confusion(lg, mk, tgt, 4)
    with pytest.raises(E):
        ops.query_dice_sums(lg, mk, tgt)
    with pytest.raises(E):
        metrics.semantic_inference(lg, mk)
    with pytest.raises(E):
        metrics.semantic_inference(lg[0], mk[0], size=(16, 16))
    with pytest.raises(E):
        metrics.dice(lg, mk, tgt)
    with pytest.raises(E):
        metrics.ConfMatrix(4, device="cpu").add_queries(lg, mk, tgt)
