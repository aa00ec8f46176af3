"""Mask2Former semantic inference on the device (csrc/query_semseg.hip; ops.query_semseg / query_labels / query_confusion /
query_dice_sums; metrics.semantic_inference / ConfMatrix.add_queries / dice).

The truth is the reference's composition (downstream/semantic_segmentation/maskformer_train_seg.py:258-274, 287-308), restated here
with torch on the CPU in fp64; for bf16 inputs on the bf16-rounded values, because the kernel widens exactly:
    mask_pred = F.interpolate(pred_masks, size=(H, W), mode="bilinear", align_corners=False)
    semseg    = einsum("bqc,bqhw->bchw", softmax(pred_logits, -1) without column void_index, mask_pred.sigmoid())
Inputs are seeded: pred_logits = 2 * randn, pred_masks = 3 * randn.

Score tolerance: 4 x the largest relative error of torch's own fp32 CPU composition against the fp64 one on the same inputs (the
kernel may sum up to 256 queries in another order and uses another expf), and never more than 1e-5 -- the near-tie gap of 1e-4 in
the label test is only valid while two scores together err by less than it.  That fp32-against-fp64 error, measured on the CPU
with these generators (fp32 inputs, void_index 0):
    (2, 100,  8, 16x16 -> 64x64)    6.8e-7        (2, 20,  8, 24x24 -> 16x16)   3.8e-7
    (2,  37,  5, 12x20 -> 40x52)    1.1e-6        (2, 16,  8, 16x16 -> 16x16)   3.4e-7
    (3,   7,  3,  9x7  -> 23x17)    7.7e-7        (1,  1,  2,  4x4  ->  8x8)    3.6e-7
    (1, 128, 33,  8x8  -> 32x32)    7.9e-7        (1, 256, 65, 4x4  ->  8x8)    1.0e-6
and on the four shapes added here for the kernel's other paths (a footprint far too large to stage; several tiles per workgroup
across sample boundaries; two staged query chunks per tile, at an integer and at a non-integer ratio):
    (2,   5,  4, 80x72 ->  8x8)     1.9e-7        (5,  6,  3,  8x8  -> 240x240) 2.9e-6
    (1, 200,  4, 16x16 -> 64x64)    8.2e-7        (1, 150, 3, 12x20 -> 40x52)   6.8e-7
These figures depend on how torch blocks its sums on the CPU at hand -- (3, 7, 3) measured 7.7e-7 to 8.1e-7, (1, 256, 65) 4.7e-7 to
1.0e-6 and (2, 5, 4) 1.9e-7 to 2.0e-7 -- which is why the bound is measured in the run and not written down.  The kernel itself
measured 0.7 to 1.1 x the run's torch figure on MI355X, and 1.0e-6 against 4.7e-7 (2.2 x) on (1, 256, 65), where it adds 256
queries one after the other.
The dtype combinations on the second shape measure 1.0e-6 to 1.1e-6, the void_index values on the third 7.3e-7 to 7.7e-7, the
saturated inputs 9.5e-8.  The share of near-tie pixels excluded from the label test is 0 to 0.39 % (one pixel in 256 of the
downsampling shape).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu

# (B, Q, K1, h, w, H, W): the smallest shapes at which each part of the kernel can go wrong
SHAPES = [
    (2, 100, 8, 16, 16, 64, 64),       # integer ratio; 6 x 6 footprints: all 100 queries in one staged chunk of at most 113
    (2, 37, 5, 12, 20, 40, 52),        # non-integer ratio, non-square
    (3, 7, 3, 9, 7, 23, 17),           # odd rows, partial tiles on both edges, unaligned loads
    (1, 128, 33, 8, 8, 32, 32),        # the 32-class instantiation boundary
    (2, 20, 8, 24, 24, 16, 16),        # downsampling: the footprint is not staged, taps come from global memory
    (2, 16, 8, 16, 16, 16, 16),        # identity: the same path
    (1, 1, 2, 4, 4, 8, 8),             # one query, one class
    (1, 256, 65, 4, 4, 8, 8),          # both limits at once
    (2, 5, 4, 80, 72, 8, 8),           # downsampling by 10 x 9: a footprint far beyond the staging buffer
    (5, 6, 3, 8, 8, 240, 240),         # 1125 tiles: two per workgroup, workgroups that cross a sample boundary
    (1, 200, 4, 16, 16, 64, 64),       # 6 x 6 footprints, 113 queries per chunk: two staged chunks (113 + 87) on every tile
    (1, 150, 3, 12, 20, 40, 52),       # 6 x 8 footprints at a non-integer ratio, 85 queries per chunk: 85 + 65, partial tiles
]
IDS = ["%dx%dx%d_%dx%d_to_%dx%d" % s for s in SHAPES]
CAP = 1e-5                             # a condition of the label test, not a measurement
GAP = 1e-4


def compose(lg, mk, size, void, dtype):
    """The reference composition in `dtype` on the CPU -> (B, K, H, W)."""
    lg, mk = lg.to(dtype), mk.to(dtype)
    up = F.interpolate(mk, size=size, mode="bilinear", align_corners=False)
    cls = F.softmax(lg, dim=-1)
    keep = [c for c in range(lg.shape[-1]) if c != void]
    return torch.einsum("bqc,bqhw->bchw", cls[..., keep], up.sigmoid())


def rel_err(a, ref, floor=0.0):
    return float(((a.double() - ref).abs() / (ref.abs() + floor)).max())


@functools.lru_cache(maxsize=None)
def case(i, lbf=False, mbf=False, void=0):
    """Seeded inputs of shape i (CPU, in the dtype the kernel gets), the fp64 truth and the score tolerance.  Computed once."""
    B, Q, K1, h, w, H, W = SHAPES[i]
    gen = torch.Generator().manual_seed(1000 + i)
    lg = 2 * torch.randn(B, Q, K1, generator=gen)
    mk = 3 * torch.randn(B, Q, h, w, generator=gen)
    lg = lg.bfloat16() if lbf else lg
    mk = mk.bfloat16() if mbf else mk
    truth = compose(lg, mk, (H, W), void, torch.float64)
    ratio = rel_err(compose(lg, mk, (H, W), void, torch.float32), truth)
    return {"lg": lg, "mk": mk, "size": (H, W), "void": void, "truth": truth, "ratio": ratio, "tol": min(4 * ratio, CAP)}


def target_for(i, K, seed=0):
    """A (B, H, W) target with labels 0 .. K (0 is the reference's ignored label), seeded."""
    B, _, _, _, _, H, W = SHAPES[i]
    return torch.randint(0, K + 1, (B, H, W), generator=torch.Generator().manual_seed(2000 + i + seed))


def dev(c):
    return c["lg"].to(DEV), c["mk"].to(DEV)


# ---- 1. scores against fp64 -----------------------------------------------------------------------------------------------------
def check_scores(c):
    from incomplete_multimodal_fusion_amd import ops
    lg, mk = dev(c)
    got = ops.query_semseg(lg, mk, size=c["size"], void_index=c["void"]).cpu()
    assert got.shape == c["truth"].shape and got.dtype == torch.float32
    err = rel_err(got, c["truth"])
    print("torch fp32 vs fp64 %.2e   kernel vs fp64 %.2e   allowed %.2e" % (c["ratio"], err, c["tol"]))
    assert err <= c["tol"], (err, c["tol"])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_scores_against_fp64(i):
    check_scores(case(i))


@pytest.mark.parametrize("lbf,mbf", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["f32_f32", "f32_bf16", "bf16_f32", "bf16_bf16"])
def test_scores_dtype_combinations(lbf, mbf):
    check_scores(case(1, lbf, mbf))


@pytest.mark.parametrize("void", [0, 2, -1, 1])                # K1 - 1 = 2
def test_scores_void_index(void):
    check_scores(case(2, False, False, void))


# ---- 2. labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_labels(i):
    from incomplete_multimodal_fusion_amd import ops
    c = case(i)
    truth = c["truth"]
    K = truth.shape[1]
    if K > 1:
        top2 = truth.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > GAP * top2[:, 0]
    else:
        clear = torch.ones_like(truth[:, 0], dtype=torch.bool)
    assert float((~clear).float().mean()) <= 0.01          # on the reference alone: the excluded near-ties are few
    lg, mk = dev(c)
    for off in (1, 0):
        labels = ops.query_labels(lg, mk, size=c["size"], void_index=c["void"], label_offset=off)
        assert labels.dtype == torch.int64 and tuple(labels.shape) == (truth.shape[0],) + tuple(truth.shape[2:])
        scores = ops.query_semseg(lg, mk, size=c["size"], void_index=c["void"])
        assert torch.equal(labels, torch.argmax(scores, 1) + off)          # the same routine: exactly
        want = truth.argmax(1) + off
        assert torch.equal(labels.cpu()[clear], want[clear])


# ---- 3. tie rule ----------------------------------------------------------------------------------------------------------------
def test_tie_rule_lowest_index_wins():
    from incomplete_multimodal_fusion_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, Q, K1, h, w, H, W = 2, 12, 6, 8, 8, 24, 40
    lg = 2 * torch.randn(B, Q, K1, generator=gen)
    mk = 3 * torch.randn(B, Q, h, w, generator=gen)
    lg[..., 2] += 1.0                                       # kept classes 1 and 3 (columns 2 and 4): identical and often the largest
    lg[..., 4] = lg[..., 2]
    scores = ops.query_semseg(lg.to(DEV), mk.to(DEV), size=(H, W)).cpu()
    labels = ops.query_labels(lg.to(DEV), mk.to(DEV), size=(H, W), label_offset=1).cpu()
    assert torch.equal(scores[:, 1].view(torch.int32), scores[:, 3].view(torch.int32))       # bitwise
    assert int((labels == 3 + 1).sum()) == 0
    assert int((labels == 1 + 1).sum()) > 0                 # the tie is the maximum somewhere, and the lower index took it
    lg[..., 2] += 1e-3                                      # class 1 slightly up: it wins those pixels outright
    labels2 = ops.query_labels(lg.to(DEV), mk.to(DEV), size=(H, W), label_offset=1).cpu()
    assert int((labels2 == 1 + 1).sum()) > 0 and int((labels2 == 3 + 1).sum()) == 0


# ---- 4. confusion ---------------------------------------------------------------------------------------------------------------
def ref_pairs(g, p, K, ign):
    g, p = g.reshape(-1).numpy().astype(np.int64), p.reshape(-1).numpy().astype(np.int64)
    ok = (g >= 0) & (g < K) & (p >= 0) & (p < K)
    if ign >= 0:
        ok &= g != ign
    return torch.from_numpy(np.bincount(g[ok] * K + p[ok], minlength=K * K).reshape(K, K).astype(np.int64))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 7, 8, 9, 10, 11], ids=[IDS[j] for j in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11)])
def test_confusion_equals_bincount_of_own_labels(i, off):
    from incomplete_multimodal_fusion_amd import ops
    c = case(i)
    K = c["truth"].shape[1]
    Kc = K + 1 if i != 7 else 60                            # shape 7 (64 classes): labels >= Kc are predicted as well
    tgt = target_for(i, K)
    flat = tgt.view(-1)
    flat[0], flat[1], flat[2] = 0, -3, Kc + 2               # the ignored label, a negative one, one past the matrix
    lg, mk = dev(c)
    labels = ops.query_labels(lg, mk, size=c["size"], label_offset=off).cpu()
    pre = torch.randint(0, 1000, (Kc, Kc), generator=torch.Generator().manual_seed(i))
    conf = pre.to(DEV)
    out = ops.query_confusion(lg, mk, tgt.to(DEV), Kc, conf=conf, pred_offset=off, ignore_label=0)
    assert out is conf
    assert torch.equal(conf.cpu() - pre, ref_pairs(tgt, labels, Kc, 0))
    none = ops.query_confusion(lg, mk, tgt.to(DEV), Kc, pred_offset=off, ignore_label=-1).cpu()
    assert torch.equal(none, ref_pairs(tgt, labels, Kc, -1))


def test_confusion_with_large_lds():
    """Q * KB and Kc at their limits: the workgroup needs more than 64 KB of LDS."""
    from incomplete_multimodal_fusion_amd import ops
    c = case(7)
    lg, mk = dev(c)
    tgt = torch.randint(0, 128, (1, 8, 8), generator=torch.Generator().manual_seed(5))
    labels = ops.query_labels(lg, mk, size=c["size"], label_offset=60).cpu()
    got = ops.query_confusion(lg, mk, tgt.to(DEV), 128, pred_offset=60, ignore_label=-1).cpu()
    assert torch.equal(got, ref_pairs(tgt, labels, 128, -1)) and int(got.sum()) == 64


def test_confmatrix_add_queries_accumulates_and_scores_agree():
    from incomplete_multimodal_fusion_amd import metrics, ops
    c = case(1)
    K = c["truth"].shape[1]
    tgt = target_for(1, K)
    lg, mk = dev(c)
    cm = metrics.ConfMatrix(K + 1)
    assert cm.add_queries(lg, mk, tgt.to(DEV)) is None
    once = cm.state.clone()
    cm.add_queries(lg, mk, tgt)                              # a host target is moved, as add_batch does
    assert int(once.sum()) == int((tgt != 0).sum()) and torch.equal(cm.state, 2 * once)
    other = metrics.ConfMatrix(K + 1)
    labels = ops.query_labels(lg, mk, size=c["size"])
    other.add_batch(tgt, labels)
    other.add_batch(tgt, labels)
    assert torch.equal(cm.state, other.state)
    assert cm.get_mIoU() == other.get_mIoU() and cm.get_aa() == other.get_aa()


# ---- 5. dice --------------------------------------------------------------------------------------------------------------------
def dice_truth(truth, tgt, off=1):
    """(B, K, 3) fp64 sums of p*t, p, t and the reference's _get_dice per sample."""
    K = truth.shape[1]
    onehot = torch.stack([(tgt - off) == k for k in range(K)], 1).double()
    sums = torch.stack([(truth * onehot).flatten(2).sum(-1), truth.flatten(2).sum(-1), onehot.flatten(2).sum(-1)], -1)
    smooth = 1e-5
    score = (2 * sums[..., 0] + smooth).sum(-1) / (sums[..., 1] + sums[..., 2] + smooth).sum(-1)
    return sums, score


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11], ids=[IDS[j] for j in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11)])
def test_dice_sums_and_score(i):
    from incomplete_multimodal_fusion_amd import metrics, ops
    c = case(i)
    K = c["truth"].shape[1]
    tgt = target_for(i, K, seed=7)
    if tgt.shape[0] > 1:
        tgt[-1] = 0                                          # the last sample is all-ignored: sum t = 0
    want, score = dice_truth(c["truth"], tgt)
    lg, mk = dev(c)
    got = ops.query_dice_sums(lg, mk, tgt.to(DEV))
    assert got.dtype == torch.float64 and tuple(got.shape) == (tgt.shape[0], K, 3)
    again = ops.query_dice_sums(lg, mk, tgt.to(DEV))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                     # bitwise reproducible
    got = got.cpu()
    assert torch.equal(got[..., 2], want[..., 2])                                          # counts are exact
    if tgt.shape[0] > 1:
        assert float(got[-1, :, 2].sum()) == 0.0 and float(got[-1, :, 0].abs().sum()) == 0.0
    g, w_ = got[..., :2], want[..., :2]                      # sums of non-negative terms: each within the scores' relative bound
    assert bool((g[w_ == 0] == 0).all())
    err = float(((g - w_).abs()[w_ > 0] / w_[w_ > 0]).max())
    print("dice sums vs fp64 %.2e   allowed %.2e" % (err, c["tol"]))
    assert err <= c["tol"]
    d = metrics.dice(lg, mk, tgt.to(DEV))
    assert d.dtype == torch.float64 and tuple(d.shape) == (tgt.shape[0],) and d.is_cuda
    # a quotient of two sums that are each within tol of the truth: within 2 * tol to first order
    assert abs(float(d[0]) - float(score[0])) <= 2 * c["tol"] * float(score[0])
    assert torch.allclose(d.cpu(), score, rtol=2 * c["tol"], atol=0)


# ---- 6. saturation --------------------------------------------------------------------------------------------------------------
def test_saturated_logits_stay_finite():
    from incomplete_multimodal_fusion_amd import ops
    gen = torch.Generator().manual_seed(6)
    B, Q, K1, h, w, H, W = 2, 9, 5, 10, 18, 20, 36           # ratio 2: the taps' weights are exact, so a mask logit between
    lg = 80.0 * (2 * torch.randint(0, 2, (B, Q, K1), generator=gen) - 1).float()
    mk = 200.0 * (2 * torch.randint(0, 2, (B, Q, h, w), generator=gen) - 1).float()   # -200 and 200 is not a rounding amplifier
    truth = compose(lg, mk, (H, W), 0, torch.float64)
    ratio = rel_err(compose(lg, mk, (H, W), 0, torch.float32), truth, floor=1e-30)
    tol = min(4 * ratio, CAP)
    got = ops.query_semseg(lg.to(DEV), mk.to(DEV), size=(H, W)).cpu()
    labels = ops.query_labels(lg.to(DEV), mk.to(DEV), size=(H, W)).cpu()
    assert bool(torch.isfinite(got).all()) and int(labels.min()) >= 1 and int(labels.max()) <= K1 - 1
    err = (got.double() - truth).abs()
    print("saturated: torch fp32 vs fp64 %.2e   kernel worst excess %.2e" % (ratio, float((err - tol * truth.abs()).max())))
    assert bool((err <= tol * truth.abs() + 1e-30).all())


# ---- 7. the reference's per-image form -------------------------------------------------------------------------------------------
def test_semantic_inference_per_image_form():
    from incomplete_multimodal_fusion_amd import metrics, ops
    c = case(2)
    lg, mk = dev(c)
    batched = metrics.semantic_inference(lg, mk, size=c["size"])
    assert torch.equal(batched, ops.query_semseg(lg, mk, size=c["size"], void_index=0))
    single = metrics.semantic_inference(lg[0], mk[0], size=c["size"])
    assert single.dim() == 3 and torch.equal(single, batched[0])
    same_size = metrics.semantic_inference(lg, mk)          # the reference's call: masks already at the output size
    assert tuple(same_size.shape[2:]) == tuple(mk.shape[2:])
    assert rel_err(same_size.cpu(), compose(c["lg"], c["mk"], tuple(mk.shape[2:]), 0, torch.float64)) <= CAP
