"""Patch gather / unpatchify (csrc/imageops.hip) and the loss heads (csrc/imageops.hip, csrc/losses.hip) against plain fp64.

Every kernel is called through the C ABI on NaN-prefilled outputs (so an element the kernel fails to write shows up), and
every call runs twice and must give the same bits (fixed reduction orders, no atomics):
  patchify_gather <float|bf16>, dense and descriptor mode       vs a torch reshape / permute / index restatement: bitwise
  unpatchify <float|bf16> and its backward (dense patchify)     bitwise
  masked_loss_partial / _bwd, masked_ce_partial / _bwd, each <float,false> (fp32 image), <float,true> (fp32 decoder tokens)
    and <bf16,true> (the bench step's bf16 decoder tokens), masked_loss_finish
                                                                vs oracle.masked_loss / masked_ce_loss in fp64 + autograd
  dino_fwd, mean_rows, dino_bwd                                  vs oracle.dino_loss
  hn_normalize / gram / rows / loss / du / finish                vs oracle.hardneg_loss (the cases test_gpu_kernels misses)
The fp64 references run with torch on the device (independent of these kernels); the gathers they start from are data
movement and so exact.

Tolerances (tests/test_gpu_kernels.py): fp32 losses to TIGHT of |ref|, gradients to GRAD x TIGHT of max|ref|.  bf16 tokens:
the inputs are exact in fp64 and the kernels accumulate in fp32, so the loss stays at TIGHT and every gradient ELEMENT (rounded
once to bf16) is held to 2^-8 |ref| + 2^-12 max|ref|."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from incomplete_multimodal_fusion_amd import _lib, ops
from incomplete_multimodal_fusion_amd._lib import call, ptr, stream
from incomplete_multimodal_fusion_amd.multimae import MaskedL1Loss, MaskedMSELoss
from oracle import mmae_oracle as O
from tests.test_gpu_kernels import GRAD, TIGHT, close
from tests.test_gpu_modattn import assert_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GLOSSES = (1.0, 0.3, -2.5)
FORMS = ("image", "tok_fp32", "tok_bf16")


def nanbuf(shape, T=F32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=T, device=DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def assert_bitwise(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert not bool(torch.isnan(got).any()), what + ": NaN left from the prefill"
    assert torch.equal(bits(got), bits(ref)), what + ": not bitwise equal to the restatement"


def twice(fn, what):
    """Run fn() twice; every returned tensor must be bitwise identical.  -> the first result."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y)), what + ": second run differs (not bitwise reproducible)"
    return a


def check_grad(T, got, ref, what):
    if T == F32:
        close(got, ref, GRAD * TIGHT[F32], what)
    else:
        assert_bf16(got, ref, what)


# ------------------------------------------------------------------------------------------------ restatements
def ref_patches(img, ps):
    """(B, C, H, W) -> (B, P, C*ps*ps), patches in row-major (nh, nw) order, columns in (c ph pw) order."""
    B, C, H, W = img.shape
    return img.reshape(B, C, H // ps, ps, W // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // ps) * (W // ps), C * ps * ps)


def ref_unpatchify(tok, B, C, H, W, ps):
    """(B*P, C*ps*ps) -> (B, C, H, W): the inverse of ref_patches."""
    return tok.reshape(B, H // ps, W // ps, C, ps, ps).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def ref_gather(images, col_offsets, onehot, Kcat, ps, tok_mod, tok_patch, tps):
    """Row r of sample r // tps, modality m = tok_mod[r], patch tok_patch[r] (dense: m 0, patch r % tps): zeros, a 1 in
    column onehot + m (onehot >= 0), then the patch's pixels in columns [col_offsets[m], col_offsets[m] + C_m ps^2)."""
    B = images[0].shape[0]
    rows = B * tps
    r = torch.arange(rows, device=DEV)
    b = r // tps
    mod = torch.zeros(rows, dtype=torch.long, device=DEV) if tok_mod is None else tok_mod.long()
    patch = r % tps if tok_patch is None else tok_patch.long()
    out = torch.zeros(rows, Kcat, dtype=F32, device=DEV)
    for m, im in enumerate(images):
        sel = (mod == m).nonzero(as_tuple=True)[0]
        if onehot >= 0:
            out[sel, onehot + m] = 1.0
        K = im.shape[1] * ps * ps
        out[sel, col_offsets[m]:col_offsets[m] + K] = ref_patches(im, ps)[b[sel], patch[sel]]
    return out


# ------------------------------------------------------------------------------------------------ 1. patchify / unpatchify
def run_patchify(T, images, col_offsets, onehot, Kcat, ps, tok_mod=None, tok_patch=None, tps=None):
    B, _, H, W = images[0].shape
    nmod = len(images)
    tps = tps or (H // ps) * (W // ps)
    arr = (ctypes.c_void_p * nmod)(*[im.data_ptr() for im in images])
    ch = (ctypes.c_int * nmod)(*[im.shape[1] for im in images])
    co = (ctypes.c_int * nmod)(*col_offsets)
    out = nanbuf((B * tps, Kcat), T)
    call("mmae_patchify_gather", _lib.dt(T), nmod, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(ch, ctypes.c_void_p),
         ctypes.cast(co, ctypes.c_void_p), onehot, Kcat, B, H, W, ps, ptr(tok_mod), ptr(tok_patch), tps, ptr(out), stream())
    torch.cuda.synchronize()
    return out


def check_patchify(images, col_offsets, onehot, Kcat, ps, tok_mod=None, tok_patch=None, tps=None, what=""):
    """fp32 bitwise equal to the gather, bf16 bitwise equal to the fp32 gather rounded to bf16; both reproducible."""
    H, W = images[0].shape[-2:]
    tps = tps or (H // ps) * (W // ps)
    ref = ref_gather(images, col_offsets, onehot, Kcat, ps, tok_mod, tok_patch, tps)
    for T in (F32, BF16):
        (out,) = twice(lambda: (run_patchify(T, images, col_offsets, onehot, Kcat, ps, tok_mod, tok_patch, tps),),
                       "patchify %s %s" % (what, T))
        assert_bitwise(out, ref.to(T), "patchify %s %s" % (what, T))


DENSE = [(C, ps, H, W) for C in (1, 3, 9) for ps in (4, 8, 16, 32) for H, W in ((64, 64), (64, 128), (128, 48 if ps != 32 else 64))]


@pytest.mark.parametrize("C,ps,H,W", DENSE, ids=["C%d-ps%d-%dx%d" % c for c in DENSE])
def test_patchify_unpatchify_dense_bitwise(C, ps, H, W):
    """Dense patchify (the encoder input and the backward of unpatchify) and unpatchify, square and non-square images."""
    gen = torch.Generator(device=DEV).manual_seed(C * 1000 + ps * 10 + H + W)
    B = 3
    P, K = (H // ps) * (W // ps), C * ps * ps
    img = torch.randn(B, C, H, W, device=DEV, generator=gen)
    check_patchify([img], [0], -1, K, ps, what="dense")
    for T in (F32, BF16):
        tok = torch.randn(B * P, K, device=DEV, generator=gen).to(T)

        def fwd():
            im = nanbuf((B, C, H, W))
            call("mmae_unpatchify", _lib.dt(T), B, C, H, W, ps, ptr(tok), ptr(im), stream())
            torch.cuda.synchronize()
            return (im,)
        (im,) = twice(fwd, "unpatchify")
        assert_bitwise(im, ref_unpatchify(tok.float(), B, C, H, W, ps), "unpatchify %s" % T)
        # autograd: the backward of unpatchify is a dense patchify into the token dtype
        g = torch.randn(B, C, H, W, device=DEV, generator=gen)

        def bwd():
            t = tok.clone().requires_grad_()
            ops.unpatchify(t, B, C, H, W, ps).backward(g)
            return (t.grad,)
        (gt,) = twice(bwd, "unpatchify backward")
        assert_bitwise(gt, ref_patches(g, ps).reshape(B * P, K).to(T), "unpatchify backward %s" % T)


def dropout_descriptors(B, M, P, N, gen):
    """The product's descriptors over masks_from_draws, one draw per sample, with per-sample modality dropout: in about a
    third of the samples one modality (drawn per sample) has a zero Dirichlet share and so no kept token."""
    alpha = torch.rand(B, M, generator=gen) + 0.05
    drop = torch.rand(B, generator=gen) < 0.35
    alpha[drop, torch.randint(0, M, (B,), generator=gen)[drop]] = 0.0
    alpha = alpha / alpha.sum(1, keepdim=True)
    mask_all, _, _ = ops.masks_from_draws(alpha.to(DEV), torch.rand(B, M, P, generator=gen).to(DEV),
                                          torch.rand(B, M * P, generator=gen).to(DEV), N)
    desc = ops.Descriptors(mask_all, B, M, P, N)
    assert int(desc.status[0]) == 0
    return mask_all, desc


@pytest.mark.parametrize("layout", ["three", "quad"])
def test_patchify_descriptor_mode_product_tables(layout):
    """The encoder's one-GEMM patch embedding input at the bench shape: B 256, 256 x 256, ps 16, P 256, N 384 kept tokens,
    tok_mod / tok_patch from the product's descriptors.  3 modalities (C 1/3/1, Kcat 1288) and the quad (C 2/4/1/9,
    Kcat 4104), column layout as multimae_crossattn builds it; the gathered rows match the mask."""
    B, P, N, ps, H = 256, 256, 384, 16, 256
    chans = (1, 3, 1) if layout == "three" else (2, 4, 1, 9)
    M = len(chans)
    gen = torch.Generator().manual_seed(7 + M)
    dgen = torch.Generator(device=DEV).manual_seed(8 + M)
    mask_all, desc = dropout_descriptors(B, M, P, N, gen)
    Ks = [c * ps * ps for c in chans]
    koff = [sum(Ks[:i]) for i in range(M)]
    onehot = sum(Ks)
    Kcat = onehot + ((M + 7) // 8) * 8
    assert Kcat == (1288 if layout == "three" else 4104)
    # the tables name exactly the kept (modality, patch) pairs of each sample
    tm, tp = desc.tok_mod.long().view(B, N), desc.tok_patch.long().view(B, N)
    kept = torch.zeros(B, M * P, dtype=torch.long, device=DEV)
    kept.scatter_(1, tm * P + tp, 1)
    assert torch.equal(kept, 1 - mask_all.expand(B, M * P)), "tok_mod / tok_patch do not name the kept patches"
    assert bool(((mask_all.view(B, M, P) == 0).sum((1, 2)) == N).all())
    assert bool(((mask_all.view(B, M, P) == 0).sum(2) == 0).any()), "no sample dropped a modality"
    images = [torch.randn(B, c, H, H, device=DEV, generator=dgen) for c in chans]
    check_patchify(images, koff, onehot, Kcat, ps, desc.tok_mod, desc.tok_patch, N, "descriptor %s" % layout)


HAND = [
    # (channels, col_offsets, onehot, Kcat, ps, H, W): gaps between slots, slots out of order, spare columns
    ((1, 3, 2), (784, 16, 400), 1000, 1024, 4, 32, 48),                # slots out of order with gaps, spare columns
    ((3, 1), (64, 8), -1, 128, 4, 16, 12),                              # no one-hot columns, gap columns 0..7 and 24..63
    ((2, 1, 3), (8, 40, 64), 0, 120, 4, 8, 16),                         # one-hot block first (not at the end)
    ((1, 2, 1, 3, 1, 2, 1, 1), tuple(8 + 64 * i for i in range(8)), 1000, 1032, 4, 16, 16),    # nmod 8, spare columns
    ((9, 4), (4096, 0), 2400, 6400, 16, 64, 32),                        # one-hot between the slots, wide rows
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_patchify_descriptor_mode_hand_made(case):
    """Column layouts the product never builds but the ABI accepts: gaps, out-of-order slots, a one-hot block first or
    between the slots, no one-hot block, spare columns, nmod 8; random tok_mod / tok_patch, N not a multiple of 4."""
    chans, koff, onehot, Kcat, ps, H, W = HAND[case]
    B, N = 3, 37
    P = (H // ps) * (W // ps)
    dgen = torch.Generator(device=DEV).manual_seed(60 + case)
    images = [torch.randn(B, c, H, W, device=DEV, generator=dgen) for c in chans]
    tok_mod = torch.randint(0, len(chans), (B * N,), dtype=torch.int32, device=DEV, generator=dgen)
    tok_patch = torch.randint(0, P, (B * N,), dtype=torch.int32, device=DEV, generator=dgen)
    for m in range(len(chans)):                                   # every modality at least once
        tok_mod[m] = m
    tok_patch[0], tok_patch[1] = 0, P - 1
    check_patchify(images, list(koff), onehot, Kcat, ps, tok_mod, tok_patch, N, "hand %d" % case)


# ------------------------------------------------------------------------------------------------ 2./3. masked losses
def make_mask(kind, B, P, gen):
    if kind == "none":
        return None
    if kind == "zeros":
        return torch.zeros(B, P, dtype=torch.long, device=DEV)
    m = (torch.rand(B, P, generator=gen) < 0.6).long()
    m[0, 0] = 1
    if B >= 3:
        m[1] = 0                                       # a sample with nothing masked: excluded from the nanmean
        m[2] = 1                                       # every patch masked
    return m.to(DEV)


def make_pred(form, B, C, H, W, ps, img):
    """The prediction as the kernel reads it: the (B,C,H,W) fp32 image or its (B*P, C*ps*ps) token form."""
    if form == "image":
        return img.contiguous()
    tok = ref_patches(img, ps).reshape(-1, C * ps * ps)
    return tok.to(BF16 if form == "tok_bf16" else F32).contiguous()


def pred_image64(form, pred, B, C, H, W, ps):
    """fp64 leaf of the prediction and the (B,C,H,W) image the reference sees."""
    leaf = pred.double().requires_grad_()
    return leaf, (leaf if form == "image" else ref_unpatchify(leaf, B, C, H, W, ps))


def run_loss(ce, form, pred, tgt, mask, B, C, H, W, ps, gloss, kind=0, smooth=0.0):
    """fwd + bwd through the C ABI, outputs NaN-prefilled.  -> loss stats (2,), den (B,), partial (B*P,), gpred."""
    P = (H // ps) * (W // ps)
    tok = int(form != "image")
    partial, den, stats = nanbuf(B * P), nanbuf(B), nanbuf(2)
    g = torch.tensor([gloss], dtype=F32, device=DEV)
    gp = nanbuf(tuple(pred.shape), pred.dtype)
    dt = _lib.dt(pred)
    if ce:
        call("mmae_masked_ce_loss_fwd", dt, tok, B, C, H, W, ps, ptr(pred), ptr(tgt), ptr(mask), smooth, ptr(partial),
             ptr(den), ptr(stats), stream())
        call("mmae_masked_ce_loss_bwd", dt, tok, B, C, H, W, ps, ptr(pred), ptr(tgt), ptr(mask), smooth, ptr(den),
             ptr(stats), ptr(g), ptr(gp), stream())
    else:
        call("mmae_masked_loss_fwd", dt, tok, kind, B, C, H, W, ps, ptr(pred), ptr(tgt), ptr(mask), ptr(partial), ptr(den),
             ptr(stats), stream())
        call("mmae_masked_loss_bwd", dt, tok, kind, B, C, H, W, ps, ptr(pred), ptr(tgt), ptr(mask), ptr(den), ptr(stats),
             ptr(g), ptr(gp), stream())
    torch.cuda.synchronize()
    return stats, den, partial, gp


def check_loss_case(ce, form, pred, tgt, mask, B, C, H, W, ps, gloss, ref_fn, what, kind=0, smooth=0.0):
    """Kernel vs fp64 reference (ref_fn(image64, mask) -> loss): loss, gradient, den, every output written, bitwise reruns."""
    P = (H // ps) * (W // ps)
    stats, den, partial, gp = twice(lambda: run_loss(ce, form, pred, tgt, mask, B, C, H, W, ps, gloss, kind, smooth), what)
    for t, nm in ((stats, "stats"), (den, "den"), (partial, "partial")):
        assert not bool(torch.isnan(t).any()), "%s: %s not fully written" % (what, nm)
    dens = (mask.sum(1).float() if mask is not None else torch.full((B,), float(P), device=DEV)) * (ps * ps)
    assert torch.equal(den, dens), what + ": den[b] is not the masked pixel count"
    T = BF16 if form == "tok_bf16" else F32
    if mask is not None and int(mask.sum()) == 0:            # the reference returns an integer 0 (no gradient)
        assert float(stats[0]) == 0.0 and float(stats[1]) == 0.0, what
        assert bool((gp == 0).all()), what + ": all-zero mask must give a zero gradient"
        return
    nvalid = B if mask is None else int((mask.sum(1) > 0).sum())
    assert float(stats[1]) == nvalid, what + ": n_valid"
    leaf, img = pred_image64(form, pred, B, C, H, W, ps)
    l = ref_fn(img, mask)
    (gloss * l).backward()
    close(stats[0], l, TIGHT[F32], what + " loss")
    ref_g = torch.nan_to_num(leaf.grad, nan=0.0)        # the reference's 0/0 for a sample with nothing masked: 0 here
    check_grad(T, gp, ref_g, what + " grad")


LOSS_SHAPES = [  # B, C, H, W, ps
    (256, 1, 256, 256, 16), (256, 3, 256, 256, 16),          # the bench shape: K = C*256 in 1 and 3 trips of the lane loop
    (6, 2, 64, 64, 16), (6, 4, 64, 64, 16),                  # the quad's C 2 and 4
    (5, 3, 32, 32, 4), (4, 3, 64, 64, 32),                   # K 48 < 256 (idle lanes), K 3072
    (4, 3, 64, 128, 16), (5, 2, 128, 48, 16), (3, 1, 48, 32, 8),   # non-square
    (4, 3, 16, 16, 16),                                      # P = 1
    (1, 3, 64, 64, 16), (257, 1, 32, 32, 8), (600, 2, 32, 64, 8),  # B 1; B > 256: the finish kernel's strided loop
]


@pytest.mark.parametrize("kind", [0, 1], ids=["mse", "l1"])
@pytest.mark.parametrize("B,C,H,W,ps", LOSS_SHAPES, ids=["B%d-C%d-%dx%d-ps%d" % s for s in LOSS_SHAPES])
def test_masked_pixel_loss_vs_fp64(B, C, H, W, ps, kind):
    """Masked MSE / L1 in the three forms (fp32 image, fp32 tokens, bf16 tokens) with a random mask (one sample with
    nothing masked, one with everything masked), no mask and an all-zero mask; gloss 1, 0.3 and -2.5 rotate over them."""
    P = (H // ps) * (W // ps)
    gen = torch.Generator().manual_seed(B * 7 + C * 131 + H * 3 + W + ps + kind)
    dgen = torch.Generator(device=DEV).manual_seed(B * 7 + C * 131 + H * 3 + W + ps + kind)
    img = torch.randn(B, C, H, W, device=DEV, generator=dgen)
    tgt = torch.randn(B, C, H, W, device=DEV, generator=dgen)
    kname = ("mse", "l1")[kind]
    for j, mk in enumerate(("random", "none", "zeros")):
        mask = make_mask(mk, B, P, gen)
        for i, form in enumerate(FORMS):
            pred = make_pred(form, B, C, H, W, ps, img)
            gloss = GLOSSES[(i + j) % 3]
            check_loss_case(False, form, pred, tgt, mask, B, C, H, W, ps, gloss,
                            lambda im, m: O.masked_loss(im, tgt.double(), m, kname, ps),
                            "%s %s mask=%s gloss %g" % (kname, form, mk, gloss), kind=kind)


@pytest.mark.parametrize("kind", [0, 1], ids=["mse", "l1"])
def test_masked_pixel_loss_norm_pix_through_criterion(kind):
    """norm_pix=True through MaskedMSELoss / MaskedL1Loss (forward and forward_tokens, fp32 and bf16 tokens, autograd with
    gloss 0.3) against oracle.masked_loss(norm_pix=True) in fp64, on a non-square image."""
    B, C, H, W, ps = 5, 3, 64, 96, 16
    P = (H // ps) * (W // ps)
    gen = torch.Generator().manual_seed(90 + kind)
    dgen = torch.Generator(device=DEV).manual_seed(91 + kind)
    img = torch.randn(B, C, H, W, device=DEV, generator=dgen)
    tgt = 3.0 * torch.randn(B, C, H, W, device=DEV, generator=dgen) + 1.0
    mask = make_mask("random", B, P, gen)
    crit = (MaskedMSELoss if kind == 0 else MaskedL1Loss)(patch_size=ps, norm_pix=True)
    for form in FORMS:
        pred = make_pred(form, B, C, H, W, ps, img)
        x = pred.clone().requires_grad_()
        l = crit(x, tgt, mask=mask) if form == "image" else crit.forward_tokens(x, tgt, mask=mask)
        (0.3 * l).backward()
        leaf, im = pred_image64(form, pred, B, C, H, W, ps)
        lr = O.masked_loss(im, tgt.double(), mask, ("mse", "l1")[kind], ps, norm_pix=True)
        (0.3 * lr).backward()
        close(l, lr, TIGHT[F32], "norm_pix %s loss" % form)
        check_grad(x.dtype, x.grad, torch.nan_to_num(leaf.grad, nan=0.0), "norm_pix %s grad" % form)


def ce_reference(C, ps, smooth, tgt):
    """oracle.masked_ce_loss, except that EVERY class id outside [0, C) is ignored: F.cross_entropy ignores only -100 (and
    raises on other out-of-range ids), while the kernel skips every out-of-range id (loss and gradient 0, the pixel still
    counted in the mask denominator) -- so those ids become -100 here."""
    t = tgt.clone()
    t[(t < 0) | (t >= C)] = -100

    def fn(im, m):
        return O.masked_ce_loss(im, t, m, ps, label_smoothing=smooth)
    return fn


def ce_inputs(B, C, H, W, dgen):
    """Logits spanning +-30, every logit of ~1/8 of the pixels shifted by +50; targets with -100, -1 and C sprinkled in."""
    logits = 60.0 * torch.rand(B, C, H, W, device=DEV, generator=dgen) - 30.0
    shift = torch.rand(B, 1, H, W, device=DEV, generator=dgen) < 0.125
    logits = logits + 50.0 * shift
    tgt = torch.randint(0, C, (B, H, W), device=DEV, generator=dgen)
    u = torch.rand(B, H, W, device=DEV, generator=dgen)
    tgt[u < 0.06] = -100
    tgt[(u >= 0.06) & (u < 0.09)] = -1
    tgt[(u >= 0.09) & (u < 0.12)] = C
    return logits, tgt


CE_SHAPES = [  # B, C, H, W, ps
    (4, 2, 64, 64, 16), (4, 9, 64, 64, 16), (3, 19, 32, 32, 16),
    (5, 9, 32, 32, 4), (3, 2, 64, 64, 32), (3, 19, 64, 64, 32),
    (4, 9, 64, 128, 16), (5, 2, 128, 48, 16), (3, 19, 48, 32, 4),
    (257, 9, 16, 16, 8),
    (16, 9, 256, 256, 16),                                   # the dnw bench shape at B 16
]


@pytest.mark.parametrize("B,C,H,W,ps", CE_SHAPES, ids=["B%d-C%d-%dx%d-ps%d" % s for s in CE_SHAPES])
def test_masked_ce_vs_fp64(B, C, H, W, ps):
    """Masked cross-entropy in the three forms, label smoothing 0 / 0.1 / 1.0, random / no / all-zero mask, gloss rotating
    over 1, 0.3, -2.5."""
    P = (H // ps) * (W // ps)
    gen = torch.Generator().manual_seed(B * 11 + C * 17 + H + W * 3 + ps)
    dgen = torch.Generator(device=DEV).manual_seed(B * 11 + C * 17 + H + W * 3 + ps)
    logits, tgt = ce_inputs(B, C, H, W, dgen)
    for j, (mk, smooth) in enumerate((("random", 0.0), ("random", 0.1), ("none", 1.0), ("random", 1.0), ("zeros", 0.1))):
        mask = make_mask(mk, B, P, gen)
        for i, form in enumerate(FORMS):
            pred = make_pred(form, B, C, H, W, ps, logits)
            gloss = GLOSSES[(i + j) % 3]
            check_loss_case(True, form, pred, tgt, mask, B, C, H, W, ps, gloss, ce_reference(C, ps, smooth, tgt),
                            "ce %s mask=%s smooth %g gloss %g" % (form, mk, smooth, gloss), smooth=smooth)


# ------------------------------------------------------------------------------------------------ 4. DINO
def run_dino(s, t, ts, tt, gloss):
    B, D = s.shape
    ws, loss, gs = nanbuf(B), nanbuf(1), nanbuf((B, D))
    g = torch.tensor([gloss], dtype=F32, device=DEV)
    call("mmae_dino_loss_fwd", B, D, ptr(s), ptr(t), ts, tt, ptr(ws), ptr(loss), stream())
    call("mmae_dino_loss_bwd", B, D, ptr(s), ptr(t), ts, tt, ptr(g), ptr(gs), stream())
    torch.cuda.synchronize()
    return ws, loss, gs


DINO_B = (1, 3, 5, 256, 1000)
DINO_D = (4, 32, 200, 256, 260, 768, 1020, 1024)


@pytest.mark.parametrize("temps", [(0.04, 0.1), (0.07, 0.2)], ids=["default", "tt0.07-ts0.2"])
@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
def test_dino_vs_fp64(T, temps):
    """B x D over 1..1000 x 4..1024 (chunks 1-3 of dino_row, a partial last chunk, mean_rows' strided loop), gloss 0.3.
    fp32: the C ABI on NaN-prefilled outputs.  bf16: ops.dino_loss with autograd (the gradient comes back in bf16, the
    teacher gets none).  Row 0 of the student is all zero when B > 1 (F.normalize's clamp: a gradient ~1e12, checked on
    its own scale)."""
    tt, ts = temps
    for B in DINO_B:
        for D in DINO_D:
            what = "dino %s B %d D %d" % (T, B, D)
            gen = torch.Generator(device=DEV).manual_seed(B * 10000 + D)
            s = torch.randn(B, D, device=DEV, generator=gen).to(T)
            t = torch.randn(B, D, device=DEV, generator=gen).to(T)
            if B > 1:
                s[0] = 0.0
            s64 = s.double().requires_grad_()
            lr = O.dino_loss(s64, t.double(), tt, ts)
            (0.3 * lr).backward()
            if T == F32:
                ws, loss, gs = twice(lambda: run_dino(s, t, ts, tt, 0.3), what)
                assert not bool(torch.isnan(ws).any()), what + ": row losses not all written"
            else:
                def via_ops():
                    sd, td = s.clone().requires_grad_(), t.clone().requires_grad_()
                    l = ops.dino_loss(sd, td, tt, ts)
                    (0.3 * l).backward()
                    assert td.grad is None, what + ": the teacher must not receive a gradient"
                    assert sd.grad.dtype == BF16
                    return l.detach().reshape(1), sd.grad
                loss, gs = twice(via_ops, what)
            close(loss[0], lr, TIGHT[F32], what + " loss")
            ref = s64.grad
            rows = torch.arange(1 if B > 1 else 0, B)
            check_grad(T, gs[rows.to(DEV)], ref[rows.to(DEV)], what + " grad")
            if B > 1:                                   # the zero row's gradient dwarfs the others: its own scale
                assert float(ref[0].abs().max()) > 1e4 * float(ref[rows.to(DEV)].abs().max())
                check_grad(T, gs[0], ref[0], what + " grad of the zero row")


# ------------------------------------------------------------------------------------------------ 5. hard negative
def run_hn(a, b, tau, beta, temp, gloss):
    B, D = a.shape
    ws = nanbuf(int(_lib.lib().mmae_hardneg_ws_floats(B, D)))
    loss, g1, g2 = nanbuf(1), nanbuf((B, D)), nanbuf((B, D))
    g = torch.tensor([gloss], dtype=F32, device=DEV)
    call("mmae_hardneg_loss_fwd", B, D, ptr(a), ptr(b), tau, beta, temp, ptr(ws), ptr(loss), stream())
    call("mmae_hardneg_loss_bwd", B, D, ptr(a), ptr(b), tau, beta, temp, ptr(ws), ptr(g), ptr(g1), ptr(g2), stream())
    torch.cuda.synchronize()
    return loss, g1, g2


def hn_raw_and_clamp(a, b, tau, beta, temp):
    """fp64 restatement of the 'hard' estimator's unclamped Ng per row and the clamp value (criterion.py:250-256)."""
    B = a.shape[0]
    out = torch.cat([F.normalize(a.double(), dim=1), F.normalize(b.double(), dim=1)])
    E = torch.exp(out @ out.t() / temp)
    j = torch.arange(2 * B)
    neg = (j[None, :] % B) != (j[:, None] % B)
    pos = E[j, (j + B) % (2 * B)]
    en = E.masked_select(neg.to(E.device)).view(2 * B, -1)
    imp = en ** beta
    rw = (imp * en).sum(1) / imp.mean(1)
    Nn = 2 * B - 2
    return (-tau * Nn * pos + rw) / (1 - tau), Nn * math.exp(-1 / temp)


def check_hn(a, b, est, tau, beta, temp, gloss, what):
    r1, r2 = a.double().cpu().requires_grad_(), b.double().cpu().requires_grad_()     # the oracle builds its masks on the CPU
    lr = O.hardneg_loss(r1, r2, tau_plus=tau, beta=beta, temperature=temp, estimator=est)
    (gloss * lr).backward()
    # the kernel runs 'easy' as the 'hard' expression at tau_plus 0, beta 0 (criterion.HardNegtive_loss)
    kt, kb = (tau, beta) if est == "hard" else (0.0, 0.0)
    loss, g1, g2 = twice(lambda: run_hn(a, b, kt, kb, temp, gloss), what)
    close(loss[0], lr, TIGHT[F32], what + " loss")
    close(g1, r1.grad, GRAD * TIGHT[F32], what + " g1")
    close(g2, r2.grad, GRAD * TIGHT[F32], what + " g2")


@pytest.mark.parametrize("tau", [0.5, 0.7, 0.9])
def test_hardneg_clamp_branch_mixed(tau):
    """Rows whose views are correlated (a large positive: the debiased Ng falls below N e^(-1/T) and is clamped, dNg = 0)
    next to anti-correlated rows (not clamped) in one batch; the fp64 restatement asserts both branches occur and that no
    row is within 1 % of the switch."""
    B, D, temp = 24, 64, 0.5
    gen = torch.Generator().manual_seed(int(tau * 100))
    a, n = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen)
    rho = torch.linspace(-0.9, 0.95, B)[torch.randperm(B, generator=gen)].view(B, 1)
    b = rho * a + (1 - rho * rho).sqrt() * n
    raw, clampv = hn_raw_and_clamp(a, b, tau, 1.0, temp)
    clamped = raw < clampv
    assert 0 < int(clamped.sum()) < 2 * B, "both branches must occur (%d of %d rows clamped)" % (int(clamped.sum()), 2 * B)
    assert float(((raw - clampv).abs() / clampv).min()) > 0.01, "a row sits at the clamp switch"
    check_hn(a.to(DEV), b.to(DEV), "hard", tau, 1.0, temp, 0.3, "hardneg tau %g" % tau)


@pytest.mark.parametrize("beta", [0.5, 2.0])
@pytest.mark.parametrize("est", ["hard", "easy"])
def test_hardneg_temperature_beta_gloss_minimum_batch(est, beta):
    """Temperature 0.2, beta 0.5 / 2, gloss -2.5 and 0.3, B 2 (the minimum: N = 2 negatives per row) and B 9, D 40."""
    gen = torch.Generator().manual_seed(int(beta * 10) + (est == "easy"))
    for B, gloss in ((2, -2.5), (9, 0.3)):
        a = torch.randn(B, 40, generator=gen)
        b = 0.5 * a + torch.randn(B, 40, generator=gen)
        check_hn(a.to(DEV), b.to(DEV), est, 0.1, beta, 0.2, gloss, "hardneg %s beta %g B %d" % (est, beta, B))


@pytest.mark.parametrize("est", ["hard", "easy"])
def test_hardneg_antipodal_negatives_at_the_clamp(est):
    """B 2 with o1 = [a, -a], o2 = [b, -2a]: row 0's two negatives are exactly antipodal to it, so its Ng equals
    N e^(-1/T) up to rounding and the kernel's clamp (applied to both estimators; the reference's 'easy' has none,
    criterion.py:257-258) may fire on rounding alone.  Its Ng gradient then vanishes in exact arithmetic (each negative's
    direction is normal to the sphere at the row), so the clamp must not change the gradient: checked against fp64."""
    gen = torch.Generator().manual_seed(5)
    D = 48
    a, b = torch.randn(D, generator=gen), torch.randn(D, generator=gen)
    o1, o2 = torch.stack([a, -a]), torch.stack([b, -2.0 * a])
    raw, clampv = hn_raw_and_clamp(o1, o2, 0.0 if est == "easy" else 0.1, 0.0 if est == "easy" else 1.0, 0.5)
    if est == "easy":
        assert abs(float(raw[0]) - clampv) <= 1e-12 * clampv
    for temp, gloss in ((0.5, 1.0), (0.2, -2.5)):
        check_hn(o1.to(DEV), o2.to(DEV), est, 0.1, 1.0, temp, gloss, "hardneg antipodal %s T %g" % (est, temp))
