"""GPU parity tests (run with `-m gpu` on an MI355X): every HIP kernel, called through the C ABI, against
  (a) the committed golden fixtures generated from the reference (tests/golden, oracle/make_golden.py), and
  (b) the CPU oracle (oracle/mmae_oracle.py) / an fp64 dense restatement on seeded random inputs at larger, ragged sizes.
Tolerances (north_star): fp32 1e-3, bf16 1e-2, relative to max|reference|; integer bookkeeping bit-exact."""
import math

import pytest
import torch

from oracle import mmae_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}
# fp32 kernels are far more accurate than the contract; a tighter internal bar catches indexing slips early
TIGHT = {torch.float32: 2e-4, torch.bfloat16: 1.5e-2}
# The contract's two gradient bars (tests/parity.py): a gradient is held to twice the output tolerance
# (fp32 2e-3, bf16 2e-2), a column sum over every row of the batch (dgamma, dbeta) to four times (one more reduction level).
GRAD, COLSUM = 2.0, 4.0


def close(a, b, tol, what=""):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert not torch.isnan(a).any(), what + ": NaN in result"
    if b.numel() == 0:
        return
    scale = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max())
    assert err <= tol * scale, "%s: max err %.3e, scale %.3e, tol %.1e" % (what, err, scale, tol)


def dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def load_module(mod, weights):
    missing, unexpected = mod.load_state_dict(weights, strict=True)
    assert not missing and not unexpected
    return mod.to(DEV)


def W(c):
    return {k[2:]: v for k, v in c.items() if k.startswith("w.")}


def check_param_grads(mod, c, tol, prefix="gw."):
    for n, p in mod.named_parameters():
        key = prefix + n
        if key in c:
            if p.grad is None:      # never reached by the graph: the reference reports an all-zero gradient
                assert float(c[key].abs().max()) == 0.0, n
                continue
            close(p.grad, c[key], tol, "grad " + n)


# ---------------------------------------------------------------------------------------------- golden: per-module
def test_layernorm_golden(g_ops):
    from incomplete_multimodal_fusion_amd.multimae.zorro_utils import LayerNorm
    c = g_ops.sub("layernorm")
    ln = LayerNorm(32).to(DEV)
    ln.gamma.data.copy_(c["gamma"])
    x = c["x"].to(DEV).requires_grad_()
    y = ln(x)
    close(y, c["y"], TIGHT[torch.float32], "y")
    y.backward(c["g"].to(DEV))
    close(x.grad, c["gx"], TIGHT[torch.float32], "gx")
    close(ln.gamma.grad, c["ggamma"], TIGHT[torch.float32], "ggamma")


@pytest.mark.parametrize("autocast", [False, True])
def test_attention_golden(g_ops, autocast):
    from incomplete_multimodal_fusion_amd.multimae.zorro_utils import Attention
    T = torch.bfloat16 if autocast else torch.float32
    tol = TIGHT[T]
    c = g_ops.sub("attn_self")
    attn = load_module(Attention(dim=32, dim_head=32, heads=2), W(c))
    x = c["x"].to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = attn(x, attn_mask=c["mask"].to(DEV))
    close(y, c["y"], tol, "self masked y")
    y.backward(c["g"].to(DEV).to(y.dtype))
    close(x.grad, c["gx"], tol, "gx")
    check_param_grads(attn, c, tol)
    # unmasked
    attn.zero_grad(); x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = attn(x)
    c2 = g_ops.sub("attn_self_nomask")
    close(y, c2["y"], tol, "self nomask y")
    y.backward(c["g"].to(DEV).to(y.dtype))
    close(x.grad, c2["gx"], tol, "gx nomask")
    # pool-style cross attention with a fully masked row (uniform attention) -------------------------------
    cp = g_ops.sub("attn_pool")
    attn.zero_grad()
    q = cp["q"].to(DEV).requires_grad_(); ctx = cp["ctx"].to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = attn(q, context=ctx, attn_mask=cp["mask"].to(DEV))
    close(y, cp["y"], tol, "pool y")
    y.backward(cp["g"].to(DEV).to(y.dtype))
    close(q.grad, cp["gq"], tol, "pool gq"); close(ctx.grad, cp["gctx"], tol, "pool gctx")
    check_param_grads(attn, cp, tol)
    # single query, no mask; and empty context -> zeros ----------------------------------------------------
    c1 = g_ops.sub("attn_cross1")
    q = c1["q"].to(DEV).requires_grad_(); ctx = c1["ctx"].to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = attn(q, context=ctx)
    close(y, c1["y"], tol, "cross1 y")
    y.backward(c1["g"].to(DEV).to(y.dtype))
    close(q.grad, c1["gq"], tol, "cross1 gq"); close(ctx.grad, c1["gctx"], tol, "cross1 gctx")
    y = attn(q, context=torch.zeros(2, 0, 32, device=DEV))
    close(y, g_ops.sub("attn_cross_empty")["y"], tol, "empty ctx")


@pytest.mark.parametrize("case", ["feedforward", "mlp", "block", "block_fusion"])
@pytest.mark.parametrize("autocast", [False, True])
def test_blocks_golden(g_ops, case, autocast):
    from incomplete_multimodal_fusion_amd.multimae import zorro_utils as Z
    T = torch.bfloat16 if autocast else torch.float32
    tol = TIGHT[T] * (2 if autocast else 1)
    c = g_ops.sub(case)
    mod = {"feedforward": lambda: Z.FeedForward(dim=32, mult=4),
           "mlp": lambda: Z.Mlp(in_features=32, hidden_features=128),
           "block": lambda: Z.Block(dim=32, dim_head=32, heads=2, ff_mult=4, norm_layer=Z.LayerNorm),
           "block_fusion": lambda: Z.Block_Fusion(dim=32, dim_head=32, heads=2, ff_mult=4, norm_layer=Z.LayerNorm)}[case]()
    mod = load_module(mod, W(c))
    x = c["x"].to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = mod(x, c["mask"].to(DEV)) if case == "block" else mod(x)
    close(y, c["y"], tol, case + " y")
    y.backward(c["g"].to(DEV).to(y.dtype))
    close(x.grad, c["gx"], tol, case + " gx")
    check_param_grads(mod, c, tol)


def test_adapters_golden(g_ops):
    from incomplete_multimodal_fusion_amd.multimae import FusionInputAdapter, PatchedInputAdapter, SpatialOutputAdapter
    tol = TIGHT[torch.float32]
    c = g_ops.sub("patched_input")
    pia = load_module(PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=8, dim_tokens=32, image_size=32), W(c))
    y = pia(c["x"].to(DEV))
    close(y, c["y"], tol, "patched y")
    y.backward(c["g"].to(DEV))
    close(pia.proj.weight.grad, c["gweight"], tol, "gweight"); close(pia.proj.bias.grad, c["gbias"], tol, "gbias")
    c = g_ops.sub("fusion_input")
    fia = load_module(FusionInputAdapter(num_channels=1, stride_level=1, patch_size_full=8, dim_tokens=32, image_size=32), W(c))
    close(fia(c["x"].to(DEV)), c["y"], 1e-6, "fusion adapter")
    c = g_ops.sub("spatial_output")
    soa = load_module(SpatialOutputAdapter(num_channels=3, stride_level=1, patch_size_full=8, dim_tokens_enc=32,
                                           dim_tokens=64, depth=2, num_heads=2, image_size=32, task="s2",
                                           context_tasks=["s1", "s2", "dem"]), W(c))
    enc = c["enc"].to(DEV).requires_grad_()
    y = soa(enc, {"image_size": (32, 32)}, None, None)
    close(y, c["y"], tol, "decoder y")
    y.backward(c["g"].to(DEV))
    close(enc.grad, c["genc"], tol, "genc")
    check_param_grads(soa, c, tol)
    for n, p in soa.named_parameters():          # cross-task embeddings and pos_emb never get a gradient
        if n.startswith("task_embeddings.") and not n.endswith(".s2"):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_masked_losses_golden(g_ops, kind):
    from incomplete_multimodal_fusion_amd.multimae import MaskedL1Loss, MaskedMSELoss
    cls = MaskedMSELoss if kind == "mse" else MaskedL1Loss
    tol = TIGHT[torch.float32]
    c = g_ops.sub("masked_" + kind)
    pred = c["pred"].to(DEV).requires_grad_(); tgt = c["tgt"].to(DEV); mask = c["mask"].to(DEV)
    l = cls(patch_size=8, stride=1)(pred, tgt, mask=mask)
    close(l, c["loss"], tol, "loss")
    l.backward()
    ref_g = torch.nan_to_num(c["gpred"], nan=0.0)       # reference: NaN grads for the sample with an empty mask row
    assert torch.isnan(c["gpred"][2]).all() and not torch.isnan(c["gpred"][:2]).any()
    close(pred.grad, ref_g, tol, "gpred")
    c2 = g_ops.sub("masked_%s_nomask" % kind)
    pred.grad = None
    l = cls(patch_size=8, stride=1)(pred, tgt, mask=None)
    close(l, c2["loss"], tol, "loss nomask"); l.backward(); close(pred.grad, c2["gpred"], tol, "gpred nomask")
    l0 = cls(patch_size=8, stride=1)(pred, tgt, mask=torch.zeros(3, 16, dtype=torch.long, device=DEV))
    assert float(l0) == 0.0
    c4 = g_ops.sub("masked_%s_normpix" % kind)
    pred.grad = None
    l = cls(patch_size=8, stride=1, norm_pix=True)(pred, tgt, mask=mask)
    close(l, c4["loss"], tol, "loss normpix"); l.backward()
    close(pred.grad, torch.nan_to_num(c4["gpred"], nan=0.0), tol, "gpred normpix")
    # fused token form == image form
    from incomplete_multimodal_fusion_amd import ops
    tok = torch.randn(3 * 16, 3 * 64, device=DEV, requires_grad=True)
    img = ops.unpatchify(tok, 3, 3, 32, 32, 8)
    li = cls(patch_size=8, stride=1)(img, tgt, mask=mask)
    (gi,) = torch.autograd.grad(li, tok)
    tok2 = tok.detach().clone().requires_grad_()
    lt = cls(patch_size=8, stride=1).forward_tokens(tok2, tgt, mask=mask)
    lt.backward()
    close(lt, li, 1e-6, "fused loss"); close(tok2.grad, gi, 1e-6, "fused grad")


def test_contrastive_golden(g_ops):
    from incomplete_multimodal_fusion_amd.multimae import HardNegtive_loss, dino_loss_func
    tol = TIGHT[torch.float32]
    c = g_ops.sub("dino")
    s = c["student"].to(DEV).requires_grad_(); t = c["teacher"].to(DEV).requires_grad_()
    l = dino_loss_func(s, t)
    close(l, c["loss"], tol, "dino"); l.backward()
    close(s.grad, c["gstudent"], tol, "dino gs")
    assert t.grad is None
    c = g_ops.sub("hardneg")
    o1 = c["out_1"].to(DEV).requires_grad_(); o2 = c["out_2"].to(DEV).requires_grad_()
    l = HardNegtive_loss()(o1, o2)
    close(l, c["loss"], tol, "hardneg"); l.backward()
    close(o1.grad, c["g1"], tol, "hardneg g1"); close(o2.grad, c["g2"], tol, "hardneg g2")
    e = g_ops.sub("hardneg_easy")                           # estimator='easy' (criterion.py:257-258) on the same inputs
    o1 = c["out_1"].to(DEV).requires_grad_(); o2 = c["out_2"].to(DEV).requires_grad_()
    l = HardNegtive_loss(estimator='easy')(o1, o2)
    close(l, e["loss"], tol, "hardneg easy"); l.backward()
    close(o1.grad, e["g1"], tol, "hardneg easy g1"); close(o2.grad, e["g2"], tol, "hardneg easy g2")
    with pytest.raises(Exception):
        HardNegtive_loss(estimator='medium')


@pytest.mark.parametrize("B,D", [(5, 48), (37, 200), (64, 1024), (256, 768)])
def test_hardneg_multi_block_vs_oracle_fp64(B, D):
    """The hard-negative head at sizes that span several Gram / gradient tiles (ragged: 2B and D not multiples of the 32 x 32 / 16 x 256
    tiles; BASELINE config 5's B = 64, D = 1024; the headline batch) against the oracle (criterion.py:233-268 restated) in fp64."""
    from incomplete_multimodal_fusion_amd.multimae import HardNegtive_loss
    from oracle import mmae_oracle as O
    g = torch.Generator().manual_seed(B * 1000 + D)
    a, b = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    b = 0.6 * a + 0.8 * b                                        # correlated views: positives above the negatives
    for est in ("hard", "easy"):
        r1, r2 = a.double().requires_grad_(), b.double().requires_grad_()
        lr = O.hardneg_loss(r1, r2, estimator=est); lr.backward()
        o1, o2 = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        l = HardNegtive_loss(estimator=est)(o1, o2); l.backward()
        close(l, lr, 1e-5, "hardneg %s loss" % est)
        close(o1.grad, r1.grad, 1e-4, "hardneg %s g1" % est); close(o2.grad, r2.grad, 1e-4, "hardneg %s g2" % est)
        o1b, o2b = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()          # bitwise reproducible (fixed summation orders)
        l2 = HardNegtive_loss(estimator=est)(o1b, o2b); l2.backward()
        assert torch.equal(l2, l) and torch.equal(o1b.grad, o1.grad) and torch.equal(o2b.grad, o2.grad)


# ---------------------------------------------------------------------------------------------- bookkeeping: bit exact
def test_masks_from_draws_bit_exact(g_masks):
    from incomplete_multimodal_fusion_amd import ops
    for name in g_masks.json("cases"):
        c = g_masks.sub(name)
        N, B, P = int(c["N"]), int(c["B"]), int(c["P"])
        mask_all, ids_keep, ids_restore = ops.masks_from_draws(c["dirichlet"].to(DEV), c["noise"][None].to(DEV),
                                                               c["noise_all"].to(DEV), N)
        ref_all = torch.cat([c["task_mask." + d] for d in O.DOMAINS], dim=1)
        assert torch.equal(mask_all.cpu().repeat(B, 1), ref_all), name
        assert torch.equal(ids_keep.cpu().repeat(B, 1), c["ids_keep"]), name
        assert torch.equal(ids_restore.cpu().repeat(B, 1), c["ids_restore"]), name
        # descriptors against the oracle's nonzero()-based bookkeeping
        d = ops.Descriptors(mask_all, B, 3, P, N)
        d.check()
        m_idx, types, zorro, pool = O.bookkeeping([mask_all[0, i * P:(i + 1) * P].cpu() for i in range(3)], P)
        lens = [len(i) for i in m_idx]
        assert d.enc_len.cpu().tolist() == [lens + [P]] * B
        assert d.tok_patch.cpu().view(B, N)[0].tolist() == torch.cat(m_idx).tolist()
        assert d.tok_mod.cpu().view(B, N)[-1].tolist() == types[:N].tolist()
        slot = d.slot_row.cpu().view(B, P, 4)
        for m in range(3):
            kept = torch.zeros(P, dtype=torch.bool); kept[m_idx[m]] = True
            assert ((slot[0, :, m] < B * N) == kept).all()
            assert (slot[B - 1, ~kept, m] == B * N + B * P + torch.arange(P)[~kept]).all()
        assert (slot[B - 1, :, 3] == B * N + (B - 1) * P + torch.arange(P)).all()


def test_masks_ties_are_stable():
    from incomplete_multimodal_fusion_amd import ops
    P, N = 16, 20
    noise = torch.zeros(1, 3, P); noise_all = torch.zeros(1, 3 * P)       # all ties
    dirichlet = torch.tensor([[0.5, 0.25, 0.25]])
    got = ops.masks_from_draws(dirichlet.to(DEV), noise.to(DEV), noise_all.to(DEV), N)
    exp = O.masks_from_draws(dirichlet, noise, noise_all, N)
    for a, b in zip(got, exp):
        assert torch.equal(a.cpu(), b)


# ---------------------------------------------------------------------------------------------- attention kernel, ragged
def dense_attention_ref(q, k, v, qseg, kseg, scale, empty_mode):
    """fp64 CPU restatement of the segment rule on per-sample row ranges; q,k,v (rows, H, dh) double with grad."""
    out = torch.zeros_like(q)
    B, nseg = qseg[0].shape
    for b in range(B):
        krows = torch.cat([torch.arange(kseg[0][b, s], kseg[0][b, s] + kseg[1][b, s]) for s in range(nseg)])
        ktype = torch.cat([torch.full((int(kseg[1][b, s]),), s) for s in range(nseg)])
        for s in range(nseg):
            qr = torch.arange(qseg[0][b, s], qseg[0][b, s] + qseg[1][b, s])
            if len(qr) == 0 or len(krows) == 0:
                continue
            allow = torch.ones(len(krows), dtype=torch.bool) if s == nseg - 1 else (ktype == s)
            if not allow.any():
                if empty_mode == 1:
                    continue
                sim = torch.zeros(q.shape[1], len(qr), len(krows), dtype=q.dtype)     # uniform, no grad to q/k
            else:
                sim = torch.einsum("ihd,jhd->hij", q[qr], k[krows]) * scale
                sim = sim.masked_fill(~allow[None, None, :], -1e300)
            p = torch.softmax(sim, dim=-1)
            out = out.index_add(0, qr, torch.einsum("hij,jhd->ihd", p, v[krows]))
    return out


# variant: kernel variant of csrc/mmae_internal.h (0 = what the product ABI runs: the 32x32x16 forward for dh 64; 2 = the
# 16x16x32 forward of round 1; 4 = 32x32x16 with 256-query tiles)
# H, hpb: heads, and how many of them ONE workgroup of the sample-head kernels walks (0 = the product's choice, which is 1 at
# these batch sizes).  The bench shape (B = 256, H = 8) runs hpb = 8: head loop, K/V ring prefetch ACROSS head boundaries;
# hpb 2 / 8 at H = 8 reach exactly that code here (forward + dK/dV with variant 0, the query-stationary dQ with variant 5).
HPB_CASES = [(torch.bfloat16, 64, v, 8, hpb) for v in (0, 5, 50) for hpb in (1, 2, 8)]       # 50: dQ + dK + dV fused (mha_sh_bwd_kernel)


@pytest.mark.parametrize("T,dh,variant,H,hpb", [(torch.float32, 64, 0, 3, 0), (torch.float32, 32, 0, 3, 0), (torch.bfloat16, 64, 0, 3, 0),
                                                (torch.bfloat16, 32, 0, 3, 0), (torch.bfloat16, 64, 2, 3, 0), (torch.bfloat16, 64, 4, 3, 0),
                                                (torch.bfloat16, 64, 5, 3, 0), (torch.bfloat16, 64, 23, 3, 0), (torch.bfloat16, 64, 50, 3, 0),
                                                (torch.bfloat16, 64, 55, 3, 0)] + HPB_CASES)     # 55: the fused backward forming its row constants itself
@pytest.mark.parametrize("empty_mode", [0, 1])
def test_mha_kernel_ragged_segments(T, dh, empty_mode, variant, H, hpb):
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(3)
    nseg = 4
    I = H * dh
    # per-sample different lengths, crossing 64-row tile boundaries, with empty segments (dropped modalities)
    qlens = torch.tensor([[70, 1, 130, 65], [0, 64, 63, 129], [5, 0, 0, 3]], dtype=torch.int32)
    klens = torch.tensor([[70, 0, 131, 65], [3, 64, 0, 200], [0, 0, 0, 0]], dtype=torch.int32)
    B = qlens.shape[0]

    def starts(lens, gap):
        st = torch.zeros_like(lens); r = 0
        for b in range(B):
            for s in range(nseg):
                st[b, s] = r; r += int(lens[b, s]) + gap
        return st, r
    qst, nq = starts(qlens, 0)
    kst, nk = starts(klens, 0)
    q = torch.randn(nq, I); kv = torch.randn(nk, 2 * I); g = torch.randn(nq, I)
    qd = q.to(DEV, T).requires_grad_(); kvd = kv.to(DEV, T).requires_grad_()
    qseg = ops.Segments(qst.to(DEV), qlens.to(DEV), int(qlens.sum(1).max()))
    kseg = ops.Segments(kst.to(DEV), klens.to(DEV), int(klens.sum(1).max()))
    scale = dh ** -0.5
    out = ops.mha_cross(qd, kvd, H, dh, qseg, kseg, scale, empty_mode, variant=variant, hpb=hpb)
    out.backward(g.to(DEV, T))
    # reference on what the kernel actually saw (bf16-rounded inputs), fp64
    q64 = qd.detach().cpu().double().reshape(nq, H, dh).requires_grad_()
    kv64 = kvd.detach().cpu().double()
    k64 = kv64[:, :I].reshape(nk, H, dh).clone().requires_grad_(); v64 = kv64[:, I:].reshape(nk, H, dh).clone().requires_grad_()
    ref = dense_attention_ref(q64, k64, v64, (qst, qlens), (kst, klens), scale, empty_mode)
    ref.backward(g.to(T).double().reshape(nq, H, dh))
    tol = 2e-5 if T == torch.float32 else 1e-2
    close(out, ref.reshape(nq, I), tol, "out")
    close(qd.grad, q64.grad.reshape(nq, I), tol * GRAD, "dq")
    close(kvd.grad[:, :I], k64.grad.reshape(nk, I), tol * GRAD, "dk")
    close(kvd.grad[:, I:], v64.grad.reshape(nk, I), tol * GRAD, "dv")


@pytest.mark.parametrize("T,variant,H,hpb", [(torch.float32, 0, 1, 0), (torch.bfloat16, 0, 1, 0), (torch.bfloat16, 2, 1, 0),
                                             (torch.bfloat16, 4, 1, 0), (torch.bfloat16, 5, 1, 0), (torch.bfloat16, 23, 1, 0)] +
                         [(torch.bfloat16, v, 8, hpb) for v in (0, 5) for hpb in (1, 2, 8)])
@pytest.mark.parametrize("shift", [0.0, -40.0])
def test_mha_online_softmax_rescale_branch(T, variant, shift, H, hpb):
    """Spike one key per tile so that the running max jumps at chosen tiles (forces the rescale path; the 32x32x16 forward
    defers the rescale until a row outgrows its reference by 2^6, so spikes below AND above that threshold are used).
    shift: every score of query 10 moved far below zero (a constant along the key axis: softmax unchanged) -- the running
    reference must follow the data, not sit at 0.  H = 8: every head has its own data and its own spike amplitudes (head h
    scales them by 1 + h / 4), walked hpb heads per workgroup (see HPB_CASES)."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(5)
    dh, n = 64, 300
    q = torch.randn(n, H, dh); k = torch.randn(n, H, dh) * 0.1; v = torch.randn(n, H, dh)
    for h in range(H):
        q10 = q[10, h]
        for j, amp in ((30, 1.5), (70, 4.0), (140, 9.0), (299, 20.0)):
            k[j, h] = q10 * (amp * (1 + h / 4)) / q10.norm()
        if shift:
            k[:, h] = k[:, h] + shift * dh ** 0.5 * q10[None] / (q10 @ q10)   # adds `shift` to every scaled score of query 10
    I = H * dh
    qkv = torch.cat([q.reshape(n, I), k.reshape(n, I), v.reshape(n, I)], dim=1).to(DEV, T).requires_grad_()
    seg = ops.Segments.dense(1, n, DEV)
    out = ops.mha_self(qkv, H, dh, seg, dh ** -0.5, variant=variant, hpb=hpb)
    out.sum().backward()
    x = qkv.detach().cpu().double().requires_grad_()
    qq, kk, vv = (x[:, i * I:(i + 1) * I].reshape(n, H, dh) for i in range(3))
    p = torch.softmax(torch.einsum("ihd,jhd->hij", qq, kk) * dh ** -0.5, dim=-1)
    ref = torch.einsum("hij,jhd->ihd", p, vv).reshape(n, I)
    ref.sum().backward()
    tol = 2e-5 if T == torch.float32 else 1e-2
    close(out, ref, tol, "out"); close(qkv.grad, x.grad, tol * GRAD, "grads")


def test_mha_fused_backward_long_schedule():
    """The fused backward's step table holds 2 x 64 entries (one lane each of two register sets): samples whose schedule runs past
    the first 64 steps -- many key passes, long segments -- against the fp64 restatement.  Sample 0: 5 passes, ~70 steps."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(9)
    H, dh, nseg = 2, 64, 3
    I = H * dh
    lens = torch.tensor([[520, 10, 500], [300, 333, 257]], dtype=torch.int32)
    B = lens.shape[0]
    st = torch.zeros_like(lens); r = 0
    for b in range(B):
        for s_ in range(nseg):
            st[b, s_] = r; r += int(lens[b, s_])
    seg = ops.Segments(st.to(DEV), lens.to(DEV), int(lens.sum(1).max()))
    assert _lib_fused_supported(B, H, nseg, seg.max_rows)
    qkv = torch.randn(r, 3 * I, device=DEV).to(torch.bfloat16)
    g = torch.randn(r, I, device=DEV).to(torch.bfloat16)
    x = qkv.clone().requires_grad_()
    out = ops.mha_self(x, H, dh, seg, dh ** -0.5, variant=50)
    out.backward(g)
    xs = x.detach().cpu().double()
    q64 = xs[:, :I].reshape(-1, H, dh).clone().requires_grad_()
    k64 = xs[:, I:2 * I].reshape(-1, H, dh).clone().requires_grad_()
    v64 = xs[:, 2 * I:].reshape(-1, H, dh).clone().requires_grad_()
    ref = dense_attention_ref(q64, k64, v64, (st, lens), (st, lens), dh ** -0.5, 0)
    ref.backward(g.cpu().double().reshape(-1, H, dh))
    close(out, ref.reshape(-1, I), 1e-2, "out")
    close(x.grad[:, :I], q64.grad.reshape(-1, I), 1e-2 * GRAD, "dq")
    close(x.grad[:, I:2 * I], k64.grad.reshape(-1, I), 1e-2 * GRAD, "dk")
    close(x.grad[:, 2 * I:], v64.grad.reshape(-1, I), 1e-2 * GRAD, "dv")


def _lib_fused_supported(B, H, nseg, max_rows):
    from incomplete_multimodal_fusion_amd import _lib
    return bool(_lib.lib().mmae_mha_bwd_fused_supported(_lib.BF16, 64, B, H, nseg, max_rows, max_rows))


def _dirichlet_segments(B, N, P, M, gen):
    """Per-sample segment lengths as the bench draws them: Dirichlet(1) shares of N kept tokens over M modalities (largest-remainder
    rounding so each row sums to N, capped at P) + P fusion rows.  -> (start, length) int32 (B, M + 1), rows packed per sample."""
    w = torch.distributions.Dirichlet(torch.ones(M)).sample((B,))
    lens = torch.floor(w * N).to(torch.int64)
    for b in range(B):
        while int(lens[b].sum()) < N:
            lens[b, int(torch.argmin(lens[b] - w[b] * N))] += 1
        while int(lens[b].max()) > P:                                   # a modality has only P patches
            i = int(lens[b].argmax()); ex = int(lens[b, i]) - P; lens[b, i] = P
            lens[b, int(lens[b].argmin())] += ex
    lens = torch.cat([lens, torch.full((B, 1), P, dtype=torch.int64)], dim=1).to(torch.int32)
    flat = lens.reshape(-1).to(torch.int64)
    start = (torch.cumsum(flat, 0) - flat).reshape(B, M + 1).to(torch.int32)
    return start, lens


@pytest.mark.parametrize("variant", [0, 5, 50])
def test_mha_bench_shape_dispatch_vs_fp64(variant):
    """The configuration bench.py runs: B = 256 samples x H = 8 heads x dh 64, every sample Dirichlet-ragged
    modality segments summing to 384 + 256 fusion rows, bf16, the PRODUCT dispatch (variant 0: one workgroup per sample walks all
    eight heads -- hpb = 8 by the library's own choice, K/V ring prefetched across head boundaries; forward = mha_sh_fwd_kernel,
    dK/dV = mha_sh_dkdv_kernel, dQ = the tile-per-block kernel; variant 5: the query-stationary dQ).  Checked against the fp64
    dense restatement of the segment rule on 12 samples: the first, the last, the most skewed split and 9 random ones -- outputs,
    dQ, dK, dV.  The other samples are held to finiteness and to the row-sum property of softmax (V = 1 column check below)."""
    from incomplete_multimodal_fusion_amd import ops
    gen = torch.manual_seed(41)
    B, H, dh, N, P, M = 256, 8, 64, 384, 256, 3
    I = H * dh
    st, ln = _dirichlet_segments(B, N, P, M, gen)
    rows = B * (N + P)
    assert int(ln.sum()) == rows and int(ln[:, :M].sum(1).min()) == N
    qkv = torch.randn(rows, 3 * I, device=DEV).to(torch.bfloat16)
    qkv[:, 2 * I] = 1.0                                        # v[:, head 0, dim 0] = 1: that output column must be exactly ~1
    g = torch.randn(rows, I, device=DEV).to(torch.bfloat16)
    x = qkv.clone().requires_grad_()
    seg = ops.Segments(st.to(DEV), ln.to(DEV), N + P)
    out = ops.mha_self(x, H, dh, seg, dh ** -0.5, variant=variant)
    out.backward(g)
    assert torch.isfinite(out.float()).all() and torch.isfinite(x.grad.float()).all()
    close(out[:, 0].float(), torch.ones(rows), 1e-2, "softmax rows sum to one (all samples)")
    skew = int((ln[:, :M].max(1).values).argmax())
    pick = sorted(set([0, B - 1, skew] + torch.randperm(B)[:9].tolist()))
    for b in pick:
        r0, r1 = int(st[b, 0]), int(st[b, 0]) + N + P
        xs = x.detach()[r0:r1].cpu().double()
        q64 = xs[:, :I].reshape(-1, H, dh).clone().requires_grad_()
        k64 = xs[:, I:2 * I].reshape(-1, H, dh).clone().requires_grad_()
        v64 = xs[:, 2 * I:].reshape(-1, H, dh).clone().requires_grad_()
        lst = (st[b:b + 1] - r0, ln[b:b + 1])
        ref = dense_attention_ref(q64, k64, v64, lst, lst, dh ** -0.5, 0)
        ref.backward(g[r0:r1].cpu().double().reshape(-1, H, dh))
        tag = " sample %d lens %s" % (b, ln[b].tolist())
        close(out[r0:r1], ref.reshape(-1, I), 1e-2, "out" + tag)
        close(x.grad[r0:r1, :I], q64.grad.reshape(-1, I), 1e-2 * GRAD, "dq" + tag)
        close(x.grad[r0:r1, I:2 * I], k64.grad.reshape(-1, I), 1e-2 * GRAD, "dk" + tag)
        close(x.grad[r0:r1, 2 * I:], v64.grad.reshape(-1, I), 1e-2 * GRAD, "dv" + tag)


# ---------------------------------------------------------------------------------------------- row kernels, big + odd sizes
@pytest.mark.parametrize("D", [768, 1024, 48])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_add_double_ln_vs_oracle(D, T):
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(1)
    r1, r2 = 37, 130
    x1 = torch.randn(r1, D); x2 = torch.randn(r2, D) * 3 + 1
    delta = torch.randn(r1 + r2, D).to(T)
    g1 = torch.rand(D) + 0.5; g2 = torch.rand(D) + 0.5; gy = torch.randn(r1 + r2, D).to(T); gup = torch.randn(r2, D)
    xs = [x1.to(DEV).requires_grad_(), x2.to(DEV).requires_grad_()]
    dd = delta.to(DEV).requires_grad_(); G1 = g1.to(DEV).requires_grad_(); G2 = g2.to(DEV).requires_grad_()
    (n1, n2), y = ops.parts_add_ln(xs, dd, [0, r1], G1, None, G2, None, out_dtype=T)
    (y.float() * gy.to(DEV).float()).sum().backward(retain_graph=True)
    (n2 * gup.to(DEV)).sum().backward()
    X = torch.cat([x1, x2]).double().requires_grad_(); Dl = delta.double().requires_grad_()
    A = g1.double().requires_grad_(); Bg = g2.double().requires_grad_()
    xn = X + Dl
    yr = O.zorro_layernorm(O.zorro_layernorm(xn, A), Bg)
    ((yr * gy.double()).sum() + (xn[r1:] * gup.double()).sum()).backward()
    tol = 2e-5 if T == torch.float32 else 1e-2
    close(y, yr, tol, "y"); close(torch.cat([n1, n2]), xn, 1e-6, "x_new")
    close(torch.cat([xs[0].grad, xs[1].grad]), X.grad, tol * GRAD, "gx"); close(dd.grad, Dl.grad, tol * GRAD, "gdelta")
    close(G1.grad, A.grad, tol * COLSUM, "dgamma1"); close(G2.grad, Bg.grad, tol * COLSUM, "dgamma2")


@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("dbl", [False, True])
def test_add_ln_with_bf16_copy_vs_oracle(D, dbl):
    """mmae_add_ln_fwd_cast (the final norm, multimae_crossattn.py:472): fp32 y and its bf16 copy from one pass; the backward takes
    the copy's bf16 gradient alone, the fp32 gradient alone, or both."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(11)
    r1, r2 = 70, 201
    x1 = torch.randn(r1, D); x2 = torch.randn(r2, D) * 2 - 1
    delta = torch.randn(r1 + r2, D).to(torch.bfloat16)
    g1 = torch.rand(D) + 0.5; g2 = (torch.rand(D) + 0.5) if dbl else None
    gy32 = torch.randn(r1 + r2, D); gyT = torch.randn(r1 + r2, D).to(torch.bfloat16)
    for use32, useT in ((False, True), (True, False), (True, True)):
        xs = [x1.to(DEV).requires_grad_(), x2.to(DEV).requires_grad_()]
        dd = delta.to(DEV).requires_grad_(); G1 = g1.to(DEV).requires_grad_()
        G2 = g2.to(DEV).requires_grad_() if dbl else None
        res = ops.parts_add_ln(xs, dd, [0, r1], G1, None, G2, None, out_dtype=torch.float32, cast_copy=True)
        assert len(res) == 3 and res[2].dtype == torch.bfloat16
        (n1, n2), y, yT = res
        assert torch.equal(yT, y.to(torch.bfloat16)), "the copy must be the rounded fp32 output"
        loss = 0
        if use32:
            loss = loss + (y * gy32.to(DEV)).sum()
        if useT:
            loss = loss + (yT.float() * gyT.to(DEV).float()).sum()
        loss.backward()
        X = torch.cat([x1, x2]).double().requires_grad_(); Dl = delta.double().requires_grad_()
        A = g1.double().requires_grad_(); Bg = g2.double().requires_grad_() if dbl else None
        xn = X + Dl
        yr = O.zorro_layernorm(xn, A)
        if dbl:
            yr = O.zorro_layernorm(yr, Bg)
        gtot = (gy32.double() if use32 else 0) + (gyT.double() if useT else 0)
        (yr * gtot).sum().backward()
        tag = "fp32 %s bf16 %s" % (use32, useT)
        close(y, yr, 2e-5, "y " + tag); close(torch.cat([n1, n2]), xn, 1e-6, "x_new " + tag)
        # the bf16-only case reads the gradient in bf16 (exact: it IS bf16); the mixed one sums in fp32 first
        close(torch.cat([xs[0].grad, xs[1].grad]), X.grad, 2e-5 * GRAD, "gx " + tag)
        close(dd.grad, Dl.grad, 1e-2 * GRAD, "gdelta " + tag)
        close(G1.grad, A.grad, 2e-5 * COLSUM, "dgamma1 " + tag)
        if dbl:
            close(G2.grad, Bg.grad, 2e-5 * COLSUM, "dgamma2 " + tag)


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_decoder_front_end_nodes_vs_torch(T):
    """ops.kv_ctx_projections (pool K/V over all rows + every decoder's proj_context over the tail rows, one node),
    ops.split_cols_f32 (column blocks + task embeddings) and ops.fork_gather_rows (pass-through + row gather, gradients merged
    by scatter-add) against the plain torch compositions they replace (multimae_crossattn.py:475-543,
    output_adapters_simple.py:166-176)."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(5)
    rows, r0, D, I2 = 96, 40, 64, 48
    n = rows - r0
    z = torch.randn(rows, D).to(T)
    wkv = torch.randn(I2, D) * 0.2
    wcs = [torch.randn(16, D) * 0.2 for _ in range(3)]; bcs = [torch.randn(16) for _ in range(3)]
    embs = [torch.randn(1, 1, 16), None, torch.randn(1, 1, 16)]
    idx = torch.tensor([5, 17, 5, 80, -1, 33, 17, 2], dtype=torch.int32)      # rows repeat across classes, unique within one
    filt = torch.tensor([0, 0, 1, 1, 1, 2, 2, 2], dtype=torch.int32)
    gkv_a = torch.randn(rows, I2).to(T); ggath = torch.randn(idx.numel(), I2).to(T)
    gouts = [torch.randn(n, 16) for _ in range(3)]

    def run(native):
        dev = DEV if native else "cpu"
        dtp = T if native else torch.float64
        zz = z.to(dev, dtp).requires_grad_()
        Wkv = wkv.to(dev, torch.float32 if native else dtp).requires_grad_()
        Wc = [w.to(dev, torch.float32 if native else dtp).requires_grad_() for w in wcs]
        Bc = [b.to(dev, torch.float32 if native else dtp).requires_grad_() for b in bcs]
        Em = [None if e is None else e.to(dev, torch.float32 if native else dtp).requires_grad_() for e in embs]
        if native:
            kv, c = ops.kv_ctx_projections(zz, r0, n, Wkv, Wc, Bc)
            xs = ops.split_cols_f32(c, [16, 16, 16], Em)
            kv2, gath = ops.fork_gather_rows(kv, idx.to(dev), filt=filt.to(dev), nfilt=3)
        else:
            kv = zz @ Wkv.t()
            xs = []
            for w, b, e in zip(Wc, Bc, Em):
                x = zz[r0:] @ w.t() + b
                xs.append(x if e is None else x + e.reshape(1, -1))
            kv2 = kv
            gath = torch.stack([kv[i] if i >= 0 else torch.zeros_like(kv[0]) for i in idx.tolist()])
        loss = (kv2.double() * gkv_a.to(dev).double()).sum() + (gath.double() * ggath.to(dev).double()).sum()
        for x, g in zip(xs, gouts):
            loss = loss + (x.double() * g.to(dev).double()).sum()
        loss.backward()
        return kv, gath, xs, zz.grad, Wkv.grad, [w.grad for w in Wc], [b.grad for b in Bc], [None if e is None else e.grad for e in Em]

    a, b = run(True), run(False)
    tol = TOL[T]
    close(a[0], b[0], tol, "kv"); close(a[1], b[1], tol, "gathered")
    for i in range(3):
        close(a[2][i], b[2][i], tol, "ctx %d" % i)
        close(a[5][i], b[5][i], tol * GRAD, "d proj_context.weight %d" % i)
        close(a[6][i], b[6][i], tol * GRAD, "d proj_context.bias %d" % i)
        if embs[i] is not None:
            close(a[7][i], b[7][i], tol * GRAD, "d task embedding %d" % i)
    close(a[3], b[3], tol * GRAD, "dz"); close(a[4], b[4], tol * GRAD, "d to_kv.weight")


@pytest.mark.parametrize("F", [2048, 85])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_geglu_gelu(F, T):
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(2)
    h = torch.randn(77, 2 * F).to(T); g = torch.randn(77, F).to(T)
    hd = h.to(DEV).requires_grad_()
    out = ops.geglu(hd); out.backward(g.to(DEV))
    hr = h.double().requires_grad_()
    ref = O.gelu_erf(hr[:, F:]) * hr[:, :F]; ref.backward(g.double())
    tol = 1e-5 if T == torch.float32 else 1e-2
    close(out, ref, tol, "geglu"); close(hd.grad, hr.grad, tol, "geglu grad")
    xd = h.to(DEV).requires_grad_(); y = ops.gelu(xd); y.backward(torch.ones_like(y))
    xr = h.double().requires_grad_(); yr = O.gelu_erf(xr); yr.sum().backward()
    close(y, yr, tol, "gelu"); close(xd.grad, xr.grad, tol, "gelu grad")


def test_patchify_unpatchify_roundtrip_exact():
    """Size-independent property at the full tile size: unpatchify(patchify_dense(x)) == x bit for bit, and
    patchify_gather picks exactly the kept patches (integer-exact data movement)."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(0)
    B, H, Wd, ps = 3, 256, 256, 16
    imgs = [torch.randn(B, c, H, Wd, device=DEV) for c in (1, 3, 1)]
    for im in imgs:
        C = im.shape[1]
        tok = ops.patchify_gather([im], [0], -1, C * ps * ps, ps, None, None, 256, torch.float32)
        ref = im.reshape(B, C, 16, ps, 16, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * 256, C * ps * ps)
        assert torch.equal(tok, ref)
        assert torch.equal(ops.unpatchify(tok, B, C, H, Wd, ps), im)
    N = 40
    tok_mod = torch.randint(0, 3, (B * N,), dtype=torch.int32, device=DEV)
    tok_patch = torch.randint(0, 256, (B * N,), dtype=torch.int32, device=DEV)
    Ks = [256, 768, 256]; koff = [0, 256, 1024]; Kcat = 1280 + 8
    pc = ops.patchify_gather(imgs, koff, 1280, Kcat, ps, tok_mod, tok_patch, N, torch.float32)
    for r in (0, 17, B * N - 1):
        b, m, p = r // N, int(tok_mod[r]), int(tok_patch[r])
        py, px = (p // 16) * ps, (p % 16) * ps
        exp = torch.zeros(Kcat, device=DEV)
        exp[koff[m]:koff[m] + Ks[m]] = imgs[m][b, :, py:py + ps, px:px + ps].reshape(-1)
        exp[1280 + m] = 1.0
        assert torch.equal(pc[r], exp)


@pytest.mark.parametrize("dh", [64, 32])
def test_mha_bf16_fast_path_matches_generic_kernels(dh):
    """The bf16 fast path (transpose reads, exp2 softmax, prefetch) and the generic dtype-templated kernels are two
    implementations of the same contract: same inputs, bf16-level agreement on outputs and all gradients."""
    from incomplete_multimodal_fusion_amd import _lib, ops
    torch.manual_seed(9)
    H, nseg, B = 2, 4, 3
    I = H * dh
    lens = torch.tensor([[100, 37, 0, 256], [64, 1, 191, 256], [0, 0, 128, 256]], dtype=torch.int32)
    st = torch.zeros_like(lens); r = 0
    for b in range(B):
        for s_ in range(nseg):
            st[b, s_] = r; r += int(lens[b, s_])
    seg = ops.Segments(st.to(DEV), lens.to(DEV), int(lens.sum(1).max()))
    qkv = torch.randn(r, 3 * I, device=DEV).to(torch.bfloat16)
    g = torch.randn(r, I, device=DEV).to(torch.bfloat16)
    res = []
    # -1: generic dtype-templated kernels (csrc/mmae_internal.h), 0: bf16 fast path (dh 64: 32x32x16 forward), 2: the round-1
    # 16x16x32 forward, 4: 256-query tiles, 5: sample-head dQ, 50 / 55: fused backward (the table in csrc/mmae_internal.h)
    for variant in ((-1, 0, 2, 4, 5, 50, 55) if dh == 64 else (-1, 0)):
        x = qkv.clone().requires_grad_()
        out = ops.mha_self(x, H, dh, seg, dh ** -0.5, variant=variant)
        out.backward(g)
        res.append((out.float(), x.grad.float()))
    for i in range(1, len(res)):
        close(res[i][0], res[0][0], 1e-2, "out"); close(res[i][1], res[0][1], 2e-2, "grads")


def test_mha_unknown_variant_is_rejected():
    """The variant numbers of csrc/mmae_internal.h are -1, 0, 2, 4, 5, 23, 50 and 55.  Every other number -- the retired experiment
    builds and anything never defined -- is an argument error of both *_variant entry points, raised before a kernel is launched,
    with or without the heads-per-workgroup bits.  One 64-row segment: whatever a library without the check ran was a valid launch."""
    import ctypes
    from incomplete_multimodal_fusion_amd import _lib, ops
    from incomplete_multimodal_fusion_amd._lib import MmaeLibraryError, dt, ptr, stream
    torch.manual_seed(11)
    B, H, dh, n = 1, 1, 64, 64
    I = H * dh
    seg = ops.Segments.dense(B, n, DEV)
    qkv = torch.randn(n, 3 * I, device=DEV).to(torch.bfloat16)
    for v in (1, 3, 6, 7, 8, 9, 18, 22, 30, 31, 32, 35, 40, 41, 45, 51, 52, 53, 54, 99):
        with pytest.raises(MmaeLibraryError):
            ops.mha_self(qkv, H, dh, seg, dh ** -0.5, variant=v)
    with pytest.raises(MmaeLibraryError):
        ops.mha_self(qkv, H, dh, seg, dh ** -0.5, variant=7, hpb=1)
    # backward: the tensors of a valid variant-0 forward, then one direct call with a retired number
    out = torch.empty(n, I, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(H, n, dtype=torch.float32, device=DEV)
    es = qkv.element_size()
    col = lambda t, c: ctypes.c_void_p(t.data_ptr() + c * es)
    _lib.call("mmae_mha_fwd_variant", dt(qkv), dh, B, H, seg.nseg, col(qkv, 0), col(qkv, I), col(qkv, 2 * I), ptr(out), ptr(lse),
              qkv.stride(0), qkv.stride(0), qkv.stride(0), out.stride(0), n, ptr(seg.start), ptr(seg.length), ptr(seg.start),
              ptr(seg.length), n, n, dh ** -0.5, 0, 0, stream())
    gout = torch.randn(n, I, device=DEV).to(torch.bfloat16)
    gqkv = torch.zeros_like(qkv)
    ws = torch.empty(_lib.lib().mmae_mha_bwd_fused_ws_floats(B, H, seg.nseg, n, n), dtype=torch.float32, device=DEV)
    with pytest.raises(MmaeLibraryError):
        _lib.call("mmae_mha_bwd_variant", dt(qkv), dh, B, H, seg.nseg, col(qkv, 0), col(qkv, I), col(qkv, 2 * I), ptr(out), ptr(gout),
                  ptr(lse), ptr(ws), col(gqkv, 0), col(gqkv, I), col(gqkv, 2 * I), qkv.stride(0), qkv.stride(0), qkv.stride(0),
                  out.stride(0), gout.stride(0), gqkv.stride(0), gqkv.stride(0), gqkv.stride(0), n, ptr(seg.start), ptr(seg.length),
                  ptr(seg.start), ptr(seg.length), n, n, dh ** -0.5, 0, 51, stream())
    torch.cuda.synchronize()


def test_colsum_bias_gradient_kernel():
    """mmae_colsum (bias gradients of the decoder / Mlp linears): fp32 sums of bf16 / fp32 matrices, strided rows, sizes that
    do not fill a block; and the fallback for widths the 16-byte lanes cannot take."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(20)
    for rows, cols, dt_ in ((65536, 768, torch.bfloat16), (1000, 256, torch.bfloat16), (37, 1024, torch.float32),
                            (5000, 2304, torch.bfloat16), (64, 85, torch.float32)):
        x = torch.randn(rows, cols, device=DEV).to(dt_)
        close(ops.colsum(x), x.double().sum(0), 1e-5 if dt_ == torch.float32 else 2e-5, "colsum %s" % ((rows, cols, dt_),))
    wide = torch.randn(512, 1024, device=DEV).to(torch.bfloat16)
    view = wide[:, 256:768]                                             # row stride 1024, 512 columns
    close(ops.colsum(view), view.double().sum(0), 2e-5, "strided colsum")
    # through ops.linear: bias gradient == column sum of the upstream gradient
    w = torch.nn.Parameter(torch.randn(256, 128, device=DEV)); b = torch.nn.Parameter(torch.zeros(256, device=DEV))
    xin = torch.randn(4096, 128, device=DEV, dtype=torch.bfloat16)
    g = torch.randn(4096, 256, device=DEV, dtype=torch.bfloat16)
    ops.linear(xin, w, b).backward(g)
    close(b.grad, g.double().sum(0), 2e-5, "bias grad")


@pytest.mark.parametrize("D,T,n0", [(768, torch.bfloat16, 333), (768, torch.float32, 333), (1024, torch.bfloat16, 333),
                                    (192, torch.float32, 333), (768, torch.bfloat16, 0), (768, torch.bfloat16, 5000)])
def test_dual_double_layernorm_equals_two_passes(D, T, n0):
    """parts_add_ln(dual=...) + parts_add_ln(y_into=...) -- the modality rows normalised with two gamma pairs in ONE pass, the
    second matrix completed by a later call -- against the two-pass composition it replaces: same outputs, same gradients for the
    residual parts, the delta and all four gammas."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(D)
    n1, n2 = 150, 16                       # n0 = 0: no kept modality token at all; 5000: more rows than the persistent grid
    mk = lambda *s: torch.randn(*s, device=DEV)
    x0, x1, x2 = mk(n0, D), mk(n1, D), mk(n2, D)
    delta = mk(n0 + n1, D).to(T)
    f = mk(n1, D).to(T)
    ga = [torch.rand(D, device=DEV) + 0.5 for _ in range(2)]
    gb = [torch.rand(D, device=DEV) + 0.5 for _ in range(2)]
    w_z, w_zb = mk(n0 + n1 + n2, D), mk(n0 + n1, D)
    w0, w1 = mk(n0, D), mk(n1, D)

    def run(dual):
        leaves = [t.clone().requires_grad_() for t in (x0, x1, x2, delta, f, *ga, *gb)]
        a0, a1, a2, dl, ff, ga1, ga2, gb1, gb2 = leaves
        if dual:
            zb = torch.empty(n0 + n1, D, dtype=T, device=DEV)
            (y0, y1, _), z, zb = ops.parts_add_ln([a0, a1, a2], dl, [0, n0, -1], ga1, None, ga2, None, out_dtype=T,
                                                  dual=(0, gb1, gb2, zb, 0))
            (y1b,), zb = ops.parts_add_ln([y1], ff, [0], gb1, None, gb2, None, out_dtype=T, y_into=(zb, n0))
        else:
            (y0, y1, _), z = ops.parts_add_ln([a0, a1, a2], dl, [0, n0, -1], ga1, None, ga2, None, out_dtype=T)
            (y0, y1b), zb = ops.parts_add_ln([y0, y1], ff, [-1, 0], gb1, None, gb2, None, out_dtype=T)
        loss = (z.float() * w_z).sum() + (zb.float() * w_zb).sum() + (y0 * w0).sum() + (y1b * w1).sum()
        loss.backward()
        return [z, zb, y0, y1b] + [t.grad for t in leaves]
    got, ref = run(True), run(False)
    names = ["z", "zb", "x0_new", "x1_new", "dx0", "dx1", "dx2", "ddelta", "df", "dga1", "dga2", "dgb1", "dgb2"]
    tol = 2e-2 if T == torch.bfloat16 else 2e-5          # bf16: the two compositions round gdelta / outputs at the same places
    for n, a, b in zip(names, got, ref):
        if a is None or b is None:                       # an empty part has no gradient in either composition
            assert a is None and b is None, n
            continue
        close(a, b, 1e-6 if n in ("z", "zb", "x0_new", "x1_new") else tol, n)


# ---------------------------------------------------------------------------------------------- row kernels at the bench's scale
# the persistent multi-row loops of add_ln_{fwd,bwd}[_dual]_fast_kernel / add_ln_fwd_cast (768-block grid, several
# rows per wave, gamma in LDS) and the one-pass GEGLU grids only run at bench-scale row counts.  Checker: the oracle's fp64
# zorro_layernorm composition (zorro_utils.py:103-110 twice, :238-239 with :176 / :124) evaluated on the CPU in row chunks (rows are
# independent; the gamma gradients are summed over the chunks), compared chunk by chunk so no full-size fp64 tensor is ever held.
CH = 16384


def _ln_pair_ref_chunks(x, delta, gammas, gys, gup, r0, r1):
    """One chunk of rows [r0, r1): x fp32, delta bf16 or None, gammas = [(g1, g2 or None), ...] (one pair per normalised output),
    gys = upstream gradients of those outputs (or None), gup = upstream gradient of x_new (or None).
    -> (x_new, [y_i], gx, per-pair (dg1, dg2)) in fp64."""
    X = x[r0:r1].double().requires_grad_()
    xn = X if delta is None else X + delta[r0:r1].double()
    leaves, ys, loss = [], [], 0
    for (g1, g2), gy in zip(gammas, gys):
        a = g1.double().requires_grad_(); b = None if g2 is None else g2.double().requires_grad_()
        y = O.zorro_layernorm(xn, a)
        if b is not None:
            y = O.zorro_layernorm(y, b)
        ys.append(y.detach()); leaves.append((a, b))
        if gy is not None:
            loss = loss + (y * gy[r0:r1].double()).sum()
    if gup is not None:
        loss = loss + (xn * gup[r0:r1].double()).sum()
    loss.backward()
    return xn.detach(), ys, X.grad, [(a.grad, None if b is None else b.grad) for a, b in leaves]


@pytest.mark.parametrize("rows_mod,rows_fus,D", [(98304, 65536, 768), (40000, 25536, 1024)])
def test_add_double_ln_bench_scale_vs_oracle(rows_mod, rows_fus, D):
    """The encoder's residual pass as the bench runs it: two parts (B*N modality rows, B*P fusion rows; 163 840 x 768 at ViT-B with
    B = 256, 65 536 x 1024 for ViT-L), bf16 delta and output, both residual outputs consumed -- forward + backward."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(21)
    rows = rows_mod + rows_fus
    x = torch.randn(rows, D) * 2 + 0.3
    delta = torch.randn(rows, D).to(torch.bfloat16)
    g1 = torch.rand(D) + 0.5; g2 = torch.rand(D) + 0.5
    gy = torch.randn(rows, D).to(torch.bfloat16); gup = torch.randn(rows, D)
    xs = [x[:rows_mod].to(DEV).requires_grad_(), x[rows_mod:].to(DEV).requires_grad_()]
    dd = delta.to(DEV).requires_grad_(); G1 = g1.to(DEV).requires_grad_(); G2 = g2.to(DEV).requires_grad_()
    (n1, n2), y = ops.parts_add_ln(xs, dd, [0, rows_mod], G1, None, G2, None, out_dtype=torch.bfloat16)
    gupd = gup.to(DEV)
    ((y.float() * gy.to(DEV).float()).sum() + (n1 * gupd[:rows_mod]).sum() + (n2 * gupd[rows_mod:]).sum()).backward()
    xn_d = torch.cat([n1, n2]).detach().cpu(); y_d = y.detach().float().cpu()
    gx_d = torch.cat([xs[0].grad, xs[1].grad]).cpu(); gd_d = dd.grad.float().cpu()
    dg1 = torch.zeros(D, dtype=torch.float64); dg2 = torch.zeros(D, dtype=torch.float64)
    for r0 in range(0, rows, CH):
        r1 = min(rows, r0 + CH)
        xn, (yr,), gx, ((a, b),) = _ln_pair_ref_chunks(x, delta, [(g1, g2)], [gy], gup, r0, r1)
        tag = " rows %d..%d" % (r0, r1)
        close(xn_d[r0:r1], xn, 1e-6, "x_new" + tag); close(y_d[r0:r1], yr, 1e-2, "y" + tag)
        close(gx_d[r0:r1], gx, 1e-2 * GRAD, "gx" + tag); close(gd_d[r0:r1], gx, 1e-2 * GRAD, "gdelta" + tag)
        dg1 += a; dg2 += b
    close(G1.grad, dg1, 1e-2 * COLSUM, "dgamma1"); close(G2.grad, dg2, 1e-2 * COLSUM, "dgamma2")


def test_dual_double_ln_bench_scale_vs_oracle():
    """The modality rows of one layer normalised with BOTH gamma pairs in one pass (mmae_add_ln_fwd_dual / _bwd_dual) at 98 304 rows,
    the second matrix completed with the 65 536 fusion rows by parts_add_ln(y_into=...) -- the call pattern of
    multimae_crossattn.py's layer loop at B = 256 -- against the fp64 composition, forward and backward."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(22)
    D, n0, n1 = 768, 98304, 65536
    T = torch.bfloat16
    x0 = torch.randn(n0, D) * 1.5; x1 = torch.randn(n1, D) - 0.2
    delta = torch.randn(n0 + n1, D).to(T); f = torch.randn(n1, D).to(T)
    ga = [torch.rand(D) + 0.5 for _ in range(2)]; gb = [torch.rand(D) + 0.5 for _ in range(2)]
    w_z = torch.randn(n0 + n1, D).to(T); w_zb = torch.randn(n0 + n1, D).to(T)
    w0 = torch.randn(n0, D); w1 = torch.randn(n1, D)
    a0, a1 = x0.to(DEV).requires_grad_(), x1.to(DEV).requires_grad_()
    dl, ff = delta.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
    GA = [g.to(DEV).requires_grad_() for g in ga]; GB = [g.to(DEV).requires_grad_() for g in gb]
    zb = torch.empty(n0 + n1, D, dtype=T, device=DEV)
    (y0, y1), z, zb = ops.parts_add_ln([a0, a1], dl, [0, n0], GA[0], None, GA[1], None, out_dtype=T, dual=(0, GB[0], GB[1], zb, 0))
    (y1b,), zb = ops.parts_add_ln([y1], ff, [0], GB[0], None, GB[1], None, out_dtype=T, y_into=(zb, n0))
    loss = (z.float() * w_z.to(DEV).float()).sum() + (zb.float() * w_zb.to(DEV).float()).sum() + (y0 * w0.to(DEV)).sum() + \
        (y1b * w1.to(DEV)).sum()
    loss.backward()
    got = {k: v.detach().float().cpu() for k, v in dict(z=z, zb=zb, y0=y0, y1b=y1b, da0=a0.grad, da1=a1.grad, ddl=dl.grad, dff=ff.grad).items()}
    acc = [torch.zeros(D, dtype=torch.float64) for _ in range(4)]
    # modality rows: x0 + delta -> pair A (into z) and pair B (into zb); residual output y0 consumed with w0
    for r0 in range(0, n0, CH):
        r1 = min(n0, r0 + CH)
        xn, (ya, yb), gx, ((a1_, a2_), (b1_, b2_)) = _ln_pair_ref_chunks(x0, delta[:n0], [(ga[0], ga[1]), (gb[0], gb[1])],
                                                                         [w_z[:n0], w_zb[:n0]], w0, r0, r1)
        tag = " modality rows %d..%d" % (r0, r1)
        close(got["y0"][r0:r1], xn, 1e-6, "x_new" + tag); close(got["z"][r0:r1], ya, 1e-2, "z" + tag); close(got["zb"][r0:r1], yb, 1e-2, "zb" + tag)
        close(got["da0"][r0:r1], gx, 1e-2 * GRAD, "dx0" + tag); close(got["ddl"][r0:r1], gx, 1e-2 * GRAD, "ddelta" + tag)
        for t, g in zip(acc, (a1_, a2_, b1_, b2_)):
            t += g
    # fusion rows: y1 = x1 + delta -> pair A (into z); y1b = y1 + f -> pair B (into zb); y1b consumed with w1
    for r0 in range(0, n1, CH):
        r1 = min(n1, r0 + CH)
        X = x1[r0:r1].double().requires_grad_(); Dl = delta[n0 + r0:n0 + r1].double().requires_grad_(); F = f[r0:r1].double().requires_grad_()
        lv = [g.double().requires_grad_() for g in (*ga, *gb)]
        yy1 = X + Dl
        za = O.zorro_layernorm(O.zorro_layernorm(yy1, lv[0]), lv[1])
        yy1b = yy1 + F
        zbb = O.zorro_layernorm(O.zorro_layernorm(yy1b, lv[2]), lv[3])
        ((za * w_z[n0 + r0:n0 + r1].double()).sum() + (zbb * w_zb[n0 + r0:n0 + r1].double()).sum() + (yy1b * w1[r0:r1].double()).sum()).backward()
        tag = " fusion rows %d..%d" % (r0, r1)
        close(got["y1b"][r0:r1], yy1b, 1e-6, "x_new" + tag)
        close(got["z"][n0 + r0:n0 + r1], za, 1e-2, "z" + tag); close(got["zb"][n0 + r0:n0 + r1], zbb, 1e-2, "zb" + tag)
        close(got["da1"][r0:r1], X.grad, 1e-2 * GRAD, "dx1" + tag); close(got["ddl"][n0 + r0:n0 + r1], Dl.grad, 1e-2 * GRAD, "ddelta" + tag)
        close(got["dff"][r0:r1], F.grad, 1e-2 * GRAD, "df" + tag)
        for t, g in zip(acc, lv):
            t += g.grad
    for nm, G, r in zip(("dga1", "dga2", "dgb1", "dgb2"), (*GA, *GB), acc):
        close(G.grad, r, 1e-2 * COLSUM, nm)


def test_add_ln_cast_copy_bench_scale_vs_oracle():
    """mmae_add_ln_fwd_cast at 163 840 x 768 (the final norm at B = 256): fp32 y + its bf16 copy, the copy's bf16 gradient alone."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(23)
    D, ra, rb = 768, 98304, 65536
    rows = ra + rb
    x = torch.randn(rows, D) * 2 - 0.5
    delta = torch.randn(rows, D).to(torch.bfloat16)
    g1 = torch.rand(D) + 0.5
    gyT = torch.randn(rows, D).to(torch.bfloat16)
    xs = [x[:ra].to(DEV).requires_grad_(), x[ra:].to(DEV).requires_grad_()]
    dd = delta.to(DEV).requires_grad_(); G1 = g1.to(DEV).requires_grad_()
    res = ops.parts_add_ln(xs, dd, [0, ra], G1, None, None, None, out_dtype=torch.float32, cast_copy=True)
    assert len(res) == 3 and res[2].dtype == torch.bfloat16
    (_, _), y, yT = res
    assert torch.equal(yT, y.to(torch.bfloat16)), "the copy must be the rounded fp32 output"
    (yT.float() * gyT.to(DEV).float()).sum().backward()
    y_d = y.detach().cpu(); gx_d = torch.cat([xs[0].grad, xs[1].grad]).cpu(); gd_d = dd.grad.float().cpu()
    dg1 = torch.zeros(D, dtype=torch.float64)
    for r0 in range(0, rows, CH):
        r1 = min(rows, r0 + CH)
        _, (yr,), gx, ((a, _),) = _ln_pair_ref_chunks(x, delta, [(g1, None)], [gyT], None, r0, r1)
        tag = " rows %d..%d" % (r0, r1)
        close(y_d[r0:r1], yr, 2e-5, "y" + tag); close(gx_d[r0:r1], gx, 2e-5 * GRAD, "gx" + tag)
        close(gd_d[r0:r1], gx, 1e-2 * GRAD, "gdelta" + tag)
        dg1 += a
    close(G1.grad, dg1, 2e-5 * COLSUM, "dgamma1")


def test_geglu_bench_scale_vs_oracle():
    """GEGLU forward / backward at 163 840 x 2 048 (FeedForward of the encoder blocks at B = 256; zorro_utils.py:115-118), bf16,
    against the exact-erf fp64 formula in row chunks -- every row of the one-pass grid, incl. the tail block."""
    from incomplete_multimodal_fusion_amd import ops
    torch.manual_seed(24)
    rows, F = 163840, 2048
    h = (torch.randn(rows, 2 * F, device=DEV) * 1.5).to(torch.bfloat16)
    g = torch.randn(rows, F, device=DEV).to(torch.bfloat16)
    hd = h.clone().requires_grad_()
    out = ops.geglu(hd); out.backward(g)
    for r0 in range(0, rows, CH):
        r1 = min(rows, r0 + CH)
        hr = h[r0:r1].cpu().double().requires_grad_()
        ref = O.gelu_erf(hr[:, F:]) * hr[:, :F]
        ref.backward(g[r0:r1].cpu().double())
        close(out[r0:r1], ref, 1e-2, "geglu rows %d..%d" % (r0, r1)); close(hd.grad[r0:r1], hr.grad, 1e-2, "geglu grad rows %d..%d" % (r0, r1))
