"""Segmentation metrics on the device (csrc/segmetrics.hip, ops.argmax_confusion / label_confusion / confusion_scores,
metrics.ConfMatrix, pretrain.evaluate_batch).  Counts are integers: every kernel comparison is exact (torch.equal on int64) against
a reference computed on the CPU inside the test -- torch.argmax over the fp32 view of the logits, the patch mask upsampled by
repeat_interleave, np.bincount(g*K + p) over the kept pixels.  The reference's own ConfMatrix (sklearn) is pinned through
tests/golden/metrics.npz (tools/make_metrics_golden.py)."""
import numpy as np
import pytest
import torch

from tests.conftest import Golden
from tests.test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu
QUAD = ("s1", "s2", "dem", "dnw")


def tokens_of(img, ps):
    """(B,C,H,W) -> the decoder's token-major (B*P, C*ps*ps) in (c ph pw) order (the permutation of tests/test_gpu_quad.py:79)."""
    B, C, H, W = img.shape
    return img.view(B, C, H // ps, ps, W // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // ps) * (W // ps), C * ps * ps)


def ref_pairs(g, p, K, ign, keep=None):
    """np.bincount over the kept (g, p) pairs: g == ign (ign >= 0) and labels outside [0, K) dropped."""
    g, p = g.reshape(-1).numpy().astype(np.int64), p.reshape(-1).numpy().astype(np.int64)
    ok = (g >= 0) & (g < K) & (p >= 0) & (p < K)
    if ign >= 0:
        ok &= g != ign
    if keep is not None:
        ok &= keep.reshape(-1).numpy()
    return torch.from_numpy(np.bincount(g[ok] * K + p[ok], minlength=K * K).reshape(K, K).astype(np.int64))


def ref_conf(img, tgt, mask, K, ps, off=0, ign=-1):
    """img: CPU (B,C,H,W) logits (any float dtype), tgt CPU (B,H,W) int64, mask CPU (B,P) or None."""
    B, C, H, W = img.shape
    p = torch.argmax(img.float().cpu(), 1) + off
    keep = None
    if mask is not None:
        keep = mask.view(B, H // ps, W // ps).repeat_interleave(ps, 1).repeat_interleave(ps, 2) == 1
    return ref_pairs(tgt, p, K, ign, keep)


def layout(img, which, ps):
    """-> (the `pred` argument of ops.argmax_confusion on the device, the CPU image whose argmax is the truth)."""
    C = img.shape[1]
    if which == "image":
        return img.to(DEV), img
    if which == "tok32":
        return (tokens_of(img, ps).contiguous().to(DEV), C), img
    q = img.bfloat16()
    return (tokens_of(q, ps).contiguous().to(DEV), C), q


def run(img, tgt, mask, K, ps, which, off=0, ign=-1, seed=0):
    """One fused call into a pre-filled matrix; returns (got - prefill, reference)."""
    from incomplete_multimodal_fusion_amd import ops
    pred, truth = layout(img, which, ps)
    pre = torch.randint(0, 1000, (K, K), generator=torch.Generator().manual_seed(seed))
    conf = pre.to(DEV)
    out = ops.argmax_confusion(pred, tgt.to(DEV), None if mask is None else mask.to(DEV), K, ps, conf=conf, pred_offset=off,
                               ignore_label=ign)
    assert out is conf
    return conf.cpu() - pre, ref_conf(truth, tgt, mask, K, ps, off, ign)


LAYOUTS = ["image", "tok32", "tokbf16"]


# ---- 1. layouts and lane coverage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maskkind", ["none", "random", "zero"])
@pytest.mark.parametrize("which", LAYOUTS)
@pytest.mark.parametrize("ps", [8, 16, 32])     # 64 pixels: 16 of 64 lanes; 256: one f32x4 per lane; 1024: four loop trips
def test_layouts_and_lane_coverage(ps, which, maskkind):
    gen = torch.Generator().manual_seed(100 + ps)
    B, C = 3, 5
    H, W = (64, 96) if ps == 32 else (32, 48)
    img = torch.randn(B, C, H, W, generator=gen)
    tgt = torch.randint(0, C, (B, H, W), generator=gen)
    P = (H // ps) * (W // ps)
    mask = {"none": None, "random": torch.randint(0, 2, (B, P), generator=gen), "zero": torch.zeros(B, P, dtype=torch.int64)}[maskkind]
    got, ref = run(img, tgt, mask, C, ps, which)
    assert torch.equal(got, ref)
    if maskkind == "zero":
        assert int(got.abs().sum()) == 0            # nothing counted: the matrix came back bit-identical
    else:
        assert int(ref.sum()) == (B * H * W if mask is None else int(mask.sum()) * ps * ps)


# ---- 2. row tail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", LAYOUTS)
def test_row_tail_partial_last_workgroup(which):
    gen = torch.Generator().manual_seed(2)
    img = torch.randn(1, 4, 8, 24, generator=gen)                      # 3 rows: the only workgroup is partial, 13 of its 16 waves idle
    tgt = torch.randint(0, 4, (1, 8, 24), generator=gen)
    got, ref = run(img, tgt, None, 4, 8, which)
    assert torch.equal(got, ref) and int(ref.sum()) == 8 * 24


# ---- 3. argmax rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", LAYOUTS)
def test_argmax_rule_ties_nan_and_all_minus_inf(which):
    gen = torch.Generator().manual_seed(3)
    B, C, H, W, ps = 2, 6, 16, 16, 8
    img = torch.randint(-1, 2, (B, C, H, W), generator=gen).float()    # {-1, 0, 1}: ties in most pixels
    nan, inf = float("nan"), float("inf")
    img[0, 2, 0, 0] = nan; img[0, 4, 0, 0] = nan                        # two NaNs: the first one wins
    img[0, C - 1, 3, 5] = nan                                           # a NaN in the last class beats every number
    img[1, 0, 9, 9] = nan; img[1, 3, 9, 9] = inf                        # a NaN in class 0 beats +inf
    img[1, :, 15, 15] = -inf                                            # all -inf: class 0
    img[0, 1, 7, 7] = inf; img[0, 5, 7, 7] = inf                        # tie of +inf: lowest index
    tgt = torch.randint(0, C, (B, H, W), generator=gen)
    truth = torch.argmax((img.bfloat16() if which == "tokbf16" else img).float(), 1)
    assert [int(truth[i]) for i in ((0, 0, 0), (0, 3, 5), (1, 9, 9), (1, 15, 15), (0, 7, 7))] == [2, C - 1, 0, 0, 1]
    got, ref = run(img, tgt, None, C, ps, which)
    assert torch.equal(got, ref) and int(ref.sum()) == B * H * W


# ---- 4. label rules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off,dK", [(0, 0), (1, 1), (1, 0)])           # plain; sem_seg.max(1)[1] + 1 with K = C + 1; top class drops out
@pytest.mark.parametrize("ign", [0, 2, -1])
@pytest.mark.parametrize("which", ["image", "tokbf16"])
def test_label_rules(which, ign, off, dK):
    gen = torch.Generator().manual_seed(4)
    B, C, H, W, ps = 2, 5, 16, 32, 8
    K = C + dK
    img = torch.randn(B, C, H, W, generator=gen)
    tgt = torch.randint(0, K, (B, H, W), generator=gen)
    tgt[0, :2, :7] = -100
    tgt[1, 5, 3:9] = K
    tgt[1, 11, 20:] = K + 3
    mask = torch.randint(0, 2, (B, (H // ps) * (W // ps)), generator=gen)
    mask[0, 0] = 1; mask[1, 0] = 1; mask[1, 7] = 1                     # the planted labels are among the counted pixels
    got, ref = run(img, tgt, mask, K, ps, which, off=off, ign=ign)
    assert torch.equal(got, ref)
    if off == 1 and dK == 0:
        assert int(ref[:, 0].sum()) == 0                               # no prediction below the offset


# ---- 5. range of K and C ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", LAYOUTS)
@pytest.mark.parametrize("C,B,H,W,ps", [(1, 2, 16, 16, 8), (128, 1, 16, 16, 8), (9, 2, 64, 64, 16)])
def test_range_of_k_and_c(C, B, H, W, ps, which):
    gen = torch.Generator().manual_seed(5 + C)
    img = torch.randn(B, C, H, W, generator=gen)
    tgt = torch.randint(0, C, (B, H, W), generator=gen)
    got, ref = run(img, tgt, None, C, ps, which)
    assert torch.equal(got, ref) and int(ref.sum()) == B * H * W


# ---- 6. accumulation and the grid-stride loop -----------------------------------------------------------------------------------
def test_two_calls_accumulate():
    from incomplete_multimodal_fusion_amd import ops
    gen = torch.Generator().manual_seed(6)
    C, ps = 7, 16
    conf, want = None, torch.zeros(C, C, dtype=torch.int64)
    for B in (2, 3):
        img = torch.randn(B, C, 32, 32, generator=gen)
        tgt = torch.randint(0, C, (B, 32, 32), generator=gen)
        mask = torch.randint(0, 2, (B, 4), generator=gen)
        conf = ops.argmax_confusion(img.to(DEV), tgt.to(DEV), mask.to(DEV), C, ps, conf=conf)
        want += ref_conf(img, tgt, mask, C, ps)
    assert conf.dtype == torch.int64 and torch.equal(conf.cpu(), want)


@pytest.mark.parametrize("which", ["image", "tokbf16"])
def test_grid_stride_loop_is_exact_and_repeatable(which):
    """B = 16, 128 x 128, patch 4: 16 384 rows = 1024 workgroups of 16 waves, twice the launch's cap of 512 workgroups."""
    gen = torch.Generator().manual_seed(66)
    B, C, H, W, ps = 16, 3, 128, 128, 4
    img = torch.randn(B, C, H, W, generator=gen)
    tgt = torch.randint(0, C, (B, H, W), generator=gen)
    mask = torch.randint(0, 2, (B, (H // ps) * (W // ps)), generator=gen)
    got1, ref = run(img, tgt, mask, C, ps, which)
    got2, _ = run(img, tgt, mask, C, ps, which)
    assert torch.equal(got1, ref) and torch.equal(got2, got1)


# ---- 7. label_confusion ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g_metrics():
    return Golden("metrics.npz")


@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("ign", [0, 2, -1])
def test_label_confusion_sizes_and_rules(n, ign):
    from incomplete_multimodal_fusion_amd import ops
    gen = torch.Generator().manual_seed(7 + n)
    K = 6
    g = torch.randint(0, K, (n,), generator=gen)
    p = torch.randint(0, K, (n,), generator=gen)
    if n > 1:
        g[5] = -100; g[17] = K; g[40] = K + 3; p[100] = K; p[200] = -1; p[300] = K + 3
    pre = torch.randint(0, 1000, (K, K), generator=gen)
    conf = pre.to(DEV)
    out = ops.label_confusion(g.to(DEV), p.to(DEV), K, conf=conf, ignore_label=ign)
    assert out is conf and torch.equal(conf.cpu() - pre, ref_pairs(g, p, K, ign))
    fresh = ops.label_confusion(g.to(DEV), p.to(DEV), K, ignore_label=ign)
    assert torch.equal(fresh.cpu(), ref_pairs(g, p, K, ign))


def test_label_confusion_fixture_maps(g_metrics):
    from incomplete_multimodal_fusion_amd import ops
    g, p = g_metrics.t("gt"), g_metrics.t("pred")
    assert g.numel() == 64 * 64 * 6
    for ign in (0, -1):
        got = ops.label_confusion(g.to(DEV), p.to(DEV), 7, ignore_label=ign)
        assert torch.equal(got.cpu(), ref_pairs(g, p, 7, ign))
    assert torch.equal(ops.label_confusion(g.to(DEV), p.to(DEV), 7, ignore_label=0).cpu(), g_metrics.t("state"))


# ---- 8. scores ------------------------------------------------------------------------------------------------------------------
def np_scores(cm):
    cm = cm.numpy().astype(np.int64)
    K = cm.shape[0]
    row, col, d = cm.sum(1), cm.sum(0), np.diagonal(cm)
    uni = row + col - d
    iou = np.divide(d.astype(np.float64), uni.astype(np.float64), out=np.zeros(K), where=uni != 0)
    rec = np.divide(d.astype(np.float64), row.astype(np.float64), out=np.zeros(K), where=row != 0)
    ex = int((row > 0).sum())
    nan = float("nan")
    return iou.mean(), (rec.sum() / ex if ex else nan), (d.sum() / cm.sum() if cm.sum() else nan), ex, iou, rec


def score_matrices():
    gen = torch.Generator().manual_seed(8)
    rnd = torch.randint(0, 100000, (128, 128), generator=gen)
    absent = torch.randint(1, 500, (7, 7), generator=gen)
    absent[5, :] = 0; absent[:, 5] = 0
    big = (1 << 40) + torch.randint(-1000, 1000, (16, 16), generator=gen)
    return {"random": rnd, "absent": absent, "big": big}


@pytest.mark.parametrize("name", ["random", "absent", "big"])
def test_confusion_scores(name):
    from incomplete_multimodal_fusion_amd import ops
    cm = score_matrices()[name]
    K = cm.shape[0]
    out = ops.confusion_scores(cm.to(DEV))
    assert out.dtype == torch.float64 and out.shape == (4 + 2 * K,) and out.is_cuda
    out = out.cpu().numpy()
    miou, aa, oa, ex, iou, rec = np_scores(cm)
    assert np.array_equal(out[4:4 + K], iou) and np.array_equal(out[4 + K:], rec)       # one IEEE division each: bit-equal
    for got, want in ((out[0], miou), (out[1], aa), (out[2], oa)):
        assert abs(got - want) <= 1e-11                                 # <= K additions of terms <= 1, any order: K^2 2^-53 = 1.8e-12
    assert out[3] == ex
    if name == "absent":
        assert ex == 6 and iou[5] == 0.0 and rec[5] == 0.0


def test_confusion_scores_of_the_empty_matrix():
    from incomplete_multimodal_fusion_amd import ops
    out = ops.confusion_scores(torch.zeros(9, 9, dtype=torch.int64, device=DEV)).cpu().numpy()
    assert out[0] == 0.0 and np.isnan(out[1]) and np.isnan(out[2]) and out[3] == 0.0
    assert not out[4:].any()


# ---- 9. the reference's ConfMatrix, through its fixture -------------------------------------------------------------------------
def test_confmatrix_matches_the_reference_fixture(g_metrics):
    from incomplete_multimodal_fusion_amd.metrics import ConfMatrix
    z = g_metrics.z
    cm = ConfMatrix(7)
    assert cm.state.is_cuda and cm.state.dtype == torch.int64
    cm.add_batch(z["gt"][:3], z["pred"][:3])                            # numpy in, as the reference's loop passes it
    cm.add_batch(torch.from_numpy(z["gt"][3:]).to(DEV), torch.from_numpy(z["pred"][3:]).to(DEV))
    assert np.array_equal(cm.state.cpu().numpy(), z["state"])
    for got, key in ((cm.get_IoU(), "iou"), (cm.get_sa(), "sa"), (cm.get_cf(), "cf")):
        assert got.dtype == np.float64 and got.shape == z[key].shape
        np.testing.assert_allclose(got, z[key], rtol=0, atol=1e-15)
    assert abs(cm.get_aa() - float(z["aa"])) <= 1e-12 and abs(cm.get_mIoU() - float(z["miou"])) <= 1e-12
    assert cm.get_existing_classes() == int(z["existing"]) == 5
    np.testing.assert_allclose(cm.norm_on_lines(), z["cf"], rtol=0, atol=1e-15)
    before = cm.state.clone()
    g0, p0 = torch.from_numpy(z["gt"][0]), torch.from_numpy(z["pred"][0])
    c0 = cm.calc(g0, p0)
    assert torch.equal(c0.cpu(), ref_pairs(g0, p0, 7, -1)) and np.array_equal(c0.cpu().numpy(), z["calc0"])
    assert torch.equal(cm.state, before)                                # calc leaves the state alone
    one = ConfMatrix(7)
    one.add(g0, p0)
    assert torch.equal(one.state.cpu(), ref_pairs(g0, p0, 7, 0))


def test_module_functions(g_metrics):
    from incomplete_multimodal_fusion_amd import metrics
    g0, p0 = g_metrics.z["gt"][1], g_metrics.z["pred"][1]
    full = ref_pairs(torch.from_numpy(g0), torch.from_numpy(p0), 7, -1).numpy().astype(np.float64)
    d = np.diagonal(full)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = d / (full.sum(1) + full.sum(0) - d)
    got = metrics.IoU(g0, p0, 7)
    assert np.array_equal(got, want, equal_nan=True)
    assert metrics.mIoU(g0, p0, 7) == np.mean(want) or (np.isnan(np.mean(want)) and np.isnan(metrics.mIoU(g0, p0, 7)))
    ign = ref_pairs(torch.from_numpy(g0), torch.from_numpy(p0), 7, 0).numpy().astype(np.float64)
    row = ign.sum(1)[:, None]
    norm = np.divide(ign, row, out=np.zeros_like(ign), where=row != 0)
    assert metrics.AA(g0, p0, 7) == np.mean(np.diagonal(norm))


# ---- 10. end to end: pretrain.evaluate_batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["image", "tokens_bf16"])
def test_evaluate_batch_end_to_end(fused):
    from incomplete_multimodal_fusion_amd.metrics import ConfMatrix
    from incomplete_multimodal_fusion_amd.multimae.multimae_crossattn import PredTokens
    from incomplete_multimodal_fusion_amd.pretrain import evaluate_batch, get_model, make_loss_fns, step_losses
    torch.manual_seed(10)
    model = get_model("tiny", in_domains=QUAD, input_size=64, decoder_dim=64, decoder_depth=1, decoder_num_heads=2)
    model.to(DEV).train()
    model.fuse_unpatchify_loss = fused
    gen = torch.Generator().manual_seed(11)
    B = 2
    x = {"s1": torch.randn(B, 2, 64, 64, generator=gen), "s2": torch.randn(B, 4, 64, 64, generator=gen),
         "dem": torch.randn(B, 1, 64, 64, generator=gen), "dnw": torch.randint(0, 9, (B, 64, 64), generator=gen)}
    x = {k: v.to(DEV) for k, v in x.items()}
    rec = {}
    inner = model.forward

    def recording_forward(*a, **k):
        rec["out"] = inner(*a, **k)
        return rec["out"]
    model.forward = recording_forward
    conf = {"dnw": ConfMatrix(9)}
    loss_fns = make_loss_fns(QUAD, 16)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=fused):
        losses, masks = evaluate_batch(model, x, loss_fns=loss_fns, conf=conf, num_encoded_tokens=12)        # 12 kept of 4 x 16: dnw keeps at most 12 of its 16
        with torch.no_grad():
            want_losses = step_losses(rec["out"], x, rec["out"][1], 16, loss_fns, contra="none")[0]
    pred = rec["out"][0]["dnw"]
    assert isinstance(pred, PredTokens) == fused
    img = pred.image() if fused else pred
    assert set(masks) == set(QUAD) and masks["dnw"].shape == (B, 16) and masks["dnw"] is rec["out"][1]["dnw"]
    ref = ref_conf(img.detach().cpu(), x["dnw"].cpu(), masks["dnw"].cpu(), 9, 16)
    assert torch.equal(conf["dnw"].state.cpu(), ref)
    assert int(ref.sum()) == int(masks["dnw"].sum()) * 256 > 0
    assert set(losses) == set(QUAD)
    for k in QUAD:
        assert torch.equal(losses[k], want_losses[k]) and bool(torch.isfinite(losses[k])), k
    assert all(p.grad is None for p in model.parameters())
    assert not any(l.requires_grad for l in losses.values())


# ---- 11. no host synchronisation in the accumulating calls ----------------------------------------------------------------------
def test_accumulating_calls_do_not_synchronise():
    from incomplete_multimodal_fusion_amd.metrics import ConfMatrix
    from incomplete_multimodal_fusion_amd.multimae.multimae_crossattn import PredTokens
    gen = torch.Generator().manual_seed(12)
    B, C, H, W, ps = 2, 9, 32, 32, 16
    img = torch.randn(B, C, H, W, generator=gen)
    tgt = torch.randint(0, C, (B, H, W), generator=gen)
    mask = torch.randint(0, 2, (B, 4), generator=gen)
    lab = torch.argmax(img, 1)
    d_img, d_tgt, d_mask, d_lab = img.to(DEV), tgt.to(DEV), mask.to(DEV), lab.to(DEV)
    toks = PredTokens(tokens_of(img.bfloat16(), ps).contiguous().to(DEV), B, C, H, W, ps)
    cm = ConfMatrix(C)
    for warm in (True, False):                    # the first pass loads the library and the kernels outside the guarded region
        if not warm:
            cm.state.zero_()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            cm.add_logits(d_img, d_tgt, mask=d_mask, ignore_label=-1)
            cm.add_logits(toks, d_tgt, mask=d_mask, ignore_label=-1)
            cm.add_batch(d_tgt, d_lab)
            s = cm.scores()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    want = ref_conf(img, tgt, mask, C, ps) + ref_conf(img.bfloat16(), tgt, mask, C, ps) + ref_pairs(tgt, lab, C, 0)
    assert torch.equal(cm.state.cpu(), want)
    assert s.is_cuda and abs(float(s[0]) - cm.get_mIoU()) == 0.0
