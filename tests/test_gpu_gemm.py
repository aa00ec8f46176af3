"""The hand-written persistent GEMM (csrc/gemm.hip: mmae_gemm_nt, mmae_gemm_geglu) against plain torch references.

Numerics bar: bf16 operands, fp32 accumulation, bf16 result -- compared with the SAME product evaluated by torch in fp32 from the bf16
operands (the kernel's only freedom is the summation order and the final rounding): max-abs error within 1e-2 of max|ref| (north_star's
bf16 bar), and within ~1.5 bf16 ulps of the result's own magnitude element-wise for the bulk (mean error check).  Shapes cover: M tails
(partial last tile), one tile per workgroup and many, the minimum K (6 K-tiles) and long K, N of 1..16 tiles (every XCD-order branch),
leading dimensions larger than the row (column blocks of wider matrices), and the encoder's own projection shapes."""
import pytest
import torch

from tests.test_gpu_kernels import DEV, close

pytestmark = pytest.mark.gpu


def _operands(M, N, K, lda=None, ldw=None, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lda, ldw = lda or K, ldw or K
    a = (torch.rand(M, lda, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    w = (torch.rand(N, ldw, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    return a[:, :K], w[:, :K]


SHAPES = [(256, 256, 384), (1000, 512, 512), (2597, 768, 768), (4096, 1536, 768), (8192, 768, 2048), (5000, 256, 4096),
          (66000, 2304, 384), (70016, 768, 512), (16384, 4096, 768), (9999, 2560, 1024)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_nt_matches_fp32_reference(M, N, K):
    from incomplete_multimodal_fusion_amd import _lib, ops
    a, w = _operands(M, N, K, seed=M + N + K)
    assert _lib.lib().mmae_gemm_nt_supported(M, N, K, a.stride(0), w.stride(0), N)
    y = ops.gemm_nt(a, w)
    ref = a.float() @ w.float().t()
    close(y, ref, 1e-2, "gemm %s" % ((M, N, K),))
    # the bulk is at rounding level: bf16 has 8 significand bits -> relative error <= 2^-9 per element after one rounding
    err = (y.float() - ref).abs()
    assert float((err / (ref.abs() + 1e-3)).median()) < 4e-3
    assert torch.equal(y, y.clone()) and torch.isfinite(y.float()).all()
    # bitwise reproducible (fixed tile order and summation order, no atomics)
    assert torch.equal(ops.gemm_nt(a, w), y)


# every forward / input-gradient projection of the bench step (ViT-B, B = 256: 163 840 encoder rows, 65 536 fusion rows, 164 096 key rows)
_R, _RF, _RK = 256 * 640, 256 * 256, 256 * 640 + 256
BENCH_SHAPES = [(_R, 1536, 768), (_R, 768, 512), (_R, 768, 2048), (_RK, 1024, 768), (_RF, 512, 768), (_RF, 768, 512), (_RF, 768, 2048),
                (_R, 768, 1536), (_R, 512, 768), (_R, 2048, 768), (_R, 768, 4096), (_RK, 768, 1024), (_RF, 2048, 768), (_RF, 768, 4096)]


@pytest.mark.parametrize("M,N,K", BENCH_SHAPES)
def test_gemm_nt_bench_shapes(M, N, K):
    """The persistent kernel at the sizes the benchmark runs (640+ M-panels: every workgroup walks several tiles, the XCD chunking and the
    rolled epilogue across tile seams are all exercised): row blocks from the start, the middle, every XCD's share and the end of the
    output against the fp32 product of the same bf16 operands."""
    from incomplete_multimodal_fusion_amd import ops
    a, w = _operands(M, N, K, seed=N + K)
    y = ops.gemm_nt(a, w)
    wt = w.float().t()
    starts = sorted({0, 256, M // 8 + 37, M // 3, M // 2 - 129, 5 * (M // 8) + 1000, M - 3 * 256 - 5, M - 300})
    for r0 in starts:
        close(y[r0:r0 + 300], a[r0:r0 + 300].float() @ wt, 1e-2, "rows %d.. of %s" % (r0, (M, N, K)))
    assert torch.isfinite(y.float()).all()
    assert torch.equal(ops.gemm_nt(a, w), y), "bitwise reproducible"


@pytest.mark.parametrize("M", [_R, _RF])
def test_gemm_geglu_bench_shapes(M):
    """FeedForward[1] + GEGLU at the bench rows (F = 2048, K = 768): h and the product on sampled row blocks."""
    from incomplete_multimodal_fusion_amd import ops
    from oracle import mmae_oracle as O
    F, K = 2048, 768
    a, w1 = _operands(M, 2 * F, K, seed=M)
    h = torch.empty(M, 2 * F, device=DEV, dtype=torch.bfloat16)
    g = torch.empty(M, F, device=DEV, dtype=torch.bfloat16)
    ops.gemm_geglu(a, w1, h, g)
    wt = w1.float().t()
    for r0 in sorted({0, M // 8 + 37, M // 2 - 129, 5 * (M // 8) + 1000, M - 300}):
        ref_h = a[r0:r0 + 300].float() @ wt
        close(h[r0:r0 + 300], ref_h, 1e-2, "h rows %d" % r0)
        h64 = ref_h.double()
        close(g[r0:r0 + 300], O.gelu_erf(h64[:, F:]) * h64[:, :F], 1e-2, "g rows %d" % r0)
    assert torch.isfinite(h.float()).all() and torch.isfinite(g.float()).all()


def test_gemm_nt_leading_dimensions_and_output_view():
    """Operands that are column blocks of wider matrices (lda / ldw > K) and an output written into a column block (ldc > N): the untouched
    columns of the output matrix must stay untouched."""
    from incomplete_multimodal_fusion_amd import ops
    M, N, K = 3000, 512, 768
    a, w = _operands(M, N, K, lda=K + 64, ldw=K + 8, seed=5)
    big = torch.full((M, N + 256), 7.0, device=DEV, dtype=torch.bfloat16)
    out = big[:, 128:128 + N]
    assert out.data_ptr() % 8 == 0
    ops.gemm_nt(a, w, out=out)
    close(out, a.float() @ w.float().t(), 1e-2, "strided gemm")
    assert float((big[:, :128].float() - 7).abs().max()) == 0.0 and float((big[:, 128 + N:].float() - 7).abs().max()) == 0.0


def test_gemm_nt_rejects_unsupported_shapes():
    from incomplete_multimodal_fusion_amd import _lib, ops
    lib = _lib.lib()
    assert not lib.mmae_gemm_nt_supported(1024, 300, 768, 768, 768, 300)          # N not a multiple of 256
    assert not lib.mmae_gemm_nt_supported(1024, 256, 320, 320, 320, 256)          # K below six K-tiles
    assert not lib.mmae_gemm_nt_supported(1024, 256, 448, 448, 448, 256)          # K not a multiple of 128
    assert not lib.mmae_gemm_nt_supported(1 << 20, 4096, 768, 768, 768, 4096)     # byte offsets beyond 32 bits
    a, w = _operands(512, 300, 768)
    with pytest.raises(_lib.MmaeLibraryError):
        ops.gemm_nt(a, w)
    # the dispatcher falls back to the library GEMM instead
    close(ops.matmul_nt(a, w), a.float() @ w.float().t(), 1e-2, "fallback")


@pytest.mark.parametrize("M,F,K", [(256, 128, 384), (3001, 256, 768), (16384, 2048, 768), (40000, 1024, 512)])
def test_gemm_geglu_matches_separate_path(M, F, K):
    """FeedForward[1] + GEGLU in one kernel (zorro_utils.py:115-126): h against the fp32 product, g against (a) the exact-erf formula on
    the kernel's own bf16 h -- the contract: g is what mmae_geglu_fwd computes from h -- and (b) the fp64 composition from scratch."""
    from incomplete_multimodal_fusion_amd import _lib, ops
    from oracle import mmae_oracle as O
    a, w1 = _operands(M, 2 * F, K, seed=M + F)
    assert _lib.lib().mmae_gemm_geglu_supported(M, F, K, a.stride(0), w1.stride(0), 2 * F, F)
    h = torch.full((M, 2 * F), float("nan"), device=DEV, dtype=torch.bfloat16)
    g = torch.full((M, F), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.gemm_geglu(a, w1, h, g)
    ref_h = a.float() @ w1.float().t()
    close(h, ref_h, 1e-2, "h")
    sep = ops.geglu(h)                                               # the separate kernel on the same h
    assert float((g.float() - sep.float()).abs().max()) <= 2 ** -7 * max(float(sep.float().abs().max()), 1e-6), "g vs geglu(h)"
    # the epilogue's GELU form (csrc/gemm.hip gm_gelu) is within 2.6e-5 of the separate kernel's for every bf16 gate
    # (tools/probes/gelu_form_check.py): element by element the two products differ by that times |val| plus one rounding step
    d = (g.float() - sep.float()).abs()
    bound = 2 ** -7 * sep.float().abs() + 3e-5 * h[:, :F].float().abs() + 1e-30
    assert bool((d <= bound).all()), float((d / bound).max())
    # (no bit-identity count: with this test's wide gates (std ~9) a good share of the products pairs a tail gate with a large val, where
    # the two forms legitimately round differently; the elementwise bound above is the contract)
    h64 = ref_h.double()
    close(g, O.gelu_erf(h64[:, F:]) * h64[:, :F], 1e-2, "g vs fp64")


def test_gemm_geglu_epilogue_gelu_over_every_bf16_gate():
    """The FF1 + GEGLU epilogue's GELU (csrc/gemm.hip gm_gelu, the fitted-sigmoid form: x * sigma(x (c0 + c1 x^2 + c2 x^4)), a documented
    deviation from the reference's erf GELU, DSI-MM/zorro_utils.py:115-118) evaluated ON THE DEVICE for EVERY finite bf16 gate: row m
    of A carries bf16 bit pattern m in column 0 and 1.0 in column 1, the gate rows of W1 pick column 0, the val rows column 1 -- so
    the accumulator of (m, gate) is exactly that bf16 value, val is exactly 1 and the stored product is bf16(gelu(gate)).
    Contract asserted against the fp64 erf form:
      * |g - gelu_erf(x)| <= 2.6e-5 + half a bf16 ulp of the result, for all 65 280 finite patterns (incl. +-0 and denormals);
      * where |gelu| >= 0.02 (everything that is not lost in the rounding of a sum of such products) the stored value is within ONE
        bf16 ulp of the correctly rounded erf form, and bit-identical to it for >= 99 % of those inputs;
      * sign / limits: gelu(+-0) = +-0 or 0, x >= 9: g == x (the factor is 1), x <= -9: |g| <= 2.1e-11 (exactly -0 from -9.6 on);
      * h carries the operands unchanged (val 1, gate x; denormal gates may be flushed to zero by the matrix core).
    Non-finite gates (128 NaN + 2 inf patterns) cannot be driven through a GEMM without poisoning the other columns of their row
    (inf * 0); the epilogue's x * rcp(1 + exp2(x p(min(x^2, 81)))) gives NaN -> NaN, +inf -> +inf, -inf -> NaN -- what the erf form
    0.5 x (1 + erf) gives -- stated here, not asserted through the kernel."""
    from incomplete_multimodal_fusion_amd import ops
    F, K, M = 128, 384, 65536
    bits = torch.arange(M, dtype=torch.int32, device=DEV).to(torch.int16)
    x = bits.view(torch.bfloat16)
    finite = torch.isfinite(x.float())
    assert int(finite.sum()) == 65280
    a = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    a[:, 0] = torch.where(finite, x, torch.zeros_like(x))
    a[:, 1] = 1.0
    w1 = torch.zeros(2 * F, K, device=DEV, dtype=torch.bfloat16)
    w1[:F, 1] = 1.0                                                   # val rows
    w1[F:, 0] = 1.0                                                   # gate rows
    h = torch.full((M, 2 * F), float("nan"), device=DEV, dtype=torch.bfloat16)
    g = torch.full((M, F), float("nan"), device=DEV, dtype=torch.bfloat16)
    ops.gemm_geglu(a, w1, h, g)
    xf = torch.where(finite, x, torch.zeros_like(x)).double()
    assert bool((h[:, :F].float() == 1.0).all())
    denorm = (xf.abs() > 0) & (xf.abs() < 2.0 ** -126)
    hg = h[:, F:].double()
    assert bool(((hg == xf[:, None]) | (denorm[:, None] & (hg == 0))).all()), "h must carry the gate unchanged"
    assert bool((g == g[:, :1]).all()), "every column evaluates the same function"
    got = g[:, 0].double()
    gate = hg[:, 0]                                                   # what the epilogue saw (a flushed denormal is 0)
    ref = 0.5 * gate * (1.0 + torch.erf(gate * 2.0 ** -0.5))
    ref_bf = ref.float().to(torch.bfloat16).double()
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7), torch.tensor(2.0 ** -133, dtype=torch.float64, device=DEV))
    err = (got - ref).abs()
    assert bool((err[finite] <= 2.6e-5 + 0.5 * ulp[finite] + 1e-30).all()), float((err - 0.5 * ulp)[finite].max())
    big = finite & (ref.abs() >= 0.02)
    off = ((got - ref_bf).abs() / ulp)[big]
    assert int(big.sum()) > 2000 and float(off.max()) <= 1.0 + 1e-9, float(off.max())
    same = float((off == 0).double().mean())
    assert same >= 0.99, same
    print("gelu epilogue: %d gates with |gelu| >= 0.02, %d differ from the correctly rounded erf form (by one ulp); max abs err %.3g"
          % (int(big.sum()), int((off != 0).sum()), float(err[finite].max())))
    zero = finite & (gate == 0)
    assert bool((got[zero] == 0).all())
    hi, lo = finite & (gate >= 9), finite & (gate <= -9)
    assert bool((got[hi] == gate[hi]).all()) and bool((got[lo].abs() <= 2.1e-11).all())


@pytest.mark.parametrize("rows,N,Kin", [(128, 256, 256), (4096, 512, 256), (10000, 768, 512), (163840, 768, 512), (65536, 4096, 768),
                                         (40037, 1536, 768), (164096, 1024, 768), (20000, 768, 2048)])
def test_gemm_tn_weight_gradient_matches_fp32_reference(rows, N, Kin):
    """dW = G^T X (autograd of nn.Linear): transposing LDS reads, split-K over workgroups, fp32 slabs summed in a fixed order.  Row counts
    that are not multiples of the 64-row K-tile or of the split size (zero-filled tails), one to 48 output tiles, 1 to 42 splits."""
    from incomplete_multimodal_fusion_amd import _lib, ops
    g = torch.Generator(device=DEV).manual_seed(rows + N)
    G = (torch.rand(rows, N, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    X = (torch.rand(rows, Kin, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    assert _lib.lib().mmae_gemm_tn_supported(rows, N, Kin, N, Kin)
    out = ops.gemm_tn(G, X)
    ref = G.double().t() @ X.double()
    close(out, ref, 1e-3, "wgrad %s" % ((rows, N, Kin),))              # fp32 accumulation and output: far inside the bf16 bar
    assert torch.equal(ops.gemm_tn(G, X), out), "bitwise reproducible"
    # written in place into a destination view (the optimizer engine's flat gradient buffer)
    flat = torch.full((N * Kin + 16,), 3.0, device=DEV)
    view = flat[8:8 + N * Kin].view(N, Kin)
    if view.data_ptr() % 16 == 0:
        ops.gemm_tn(G, X, out=view)
        assert torch.equal(view, out) and float(flat[:8].min()) == 3.0 and float(flat[-8:].min()) == 3.0


def test_gemm_tn_strided_operands():
    from incomplete_multimodal_fusion_amd import _lib, ops
    rows, N, Kin = 9000, 512, 768
    g = torch.Generator(device=DEV).manual_seed(3)
    Gw = (torch.rand(rows, 3 * N + 8, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)       # a column block of a fused qkv gradient
    Xw = (torch.rand(rows, Kin + 40, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    G, X = Gw[:, N:2 * N], Xw[:, :Kin]
    assert _lib.lib().mmae_gemm_tn_supported(rows, N, Kin, G.stride(0), X.stride(0)) and G.data_ptr() % 16 == 0
    close(ops.gemm_tn(G, X), G.double().t() @ X.double(), 1e-3, "strided wgrad")


# ------------------------------------------------------------------------------------------------ zero-padded FeedForward (ViT-L's ffi = 2730)
def _ff_engine(D, F, seed=0):
    from incomplete_multimodal_fusion_amd.engine import FlatAdamW
    torch.manual_seed(seed)
    w1 = torch.nn.Parameter(torch.randn(2 * F, D, device=DEV) * D ** -0.5)
    w2 = torch.nn.Parameter(torch.randn(D, F, device=DEV) * F ** -0.5)
    return w1, w2, FlatAdamW([w1, w2], lr=1e-2, betas=(0.9, 0.95), weight_decay=0.0)


@pytest.mark.parametrize("D,F", [(128, 90), (512, 300), (1024, 2730)])
def test_padded_ff_shadows_match_the_weights(D, F):
    """engine.FlatAdamW.padded_ff: the zero-padded / transposed bf16 copies (mmae_pad_copy_bf16_batched, element-granular edges:
    2730 % 8 = 2) hold exactly the shadow's values in their payload and zeros in the pads -- at registration and after an update."""
    w1, w2, eng = _ff_engine(D, F)
    pf = eng.padded_ff(w1, w2)
    Fp = pf.Fp
    assert Fp % 256 == 0 and Fp >= F and Fp - F < 256

    def check():
        s1, s2 = w1._mmae_shadow, w2._mmae_shadow
        e1 = torch.zeros(2 * Fp, D, dtype=torch.bfloat16, device=DEV); e1[:F] = s1[:F]; e1[Fp:Fp + F] = s1[F:]
        e2 = torch.zeros(D, Fp, dtype=torch.bfloat16, device=DEV); e2[:, :F] = s2
        assert torch.equal(pf.w1p, e1) and torch.equal(pf.w2p, e2)
        assert torch.equal(pf.w1pt, e1.t().contiguous()) and torch.equal(pf.w2pt, e2.t().contiguous())
    check()
    w1.grad = torch.randn_like(w1); w2.grad = torch.randn_like(w2)
    eng._on_grad(w1); eng._on_grad(w2)
    before = pf.w1p.clone()
    eng.step()
    assert not torch.equal(pf.w1p, before)
    check()


@pytest.mark.parametrize("rows,D,F", [(4096, 512, 300), (6000, 1024, 2730), (8229, 512, 512)])
def test_feedforward_geglu_own_gemm_padded_and_unpadded_vs_fp64_and_library_path(rows, D, F, monkeypatch):
    """ops.feedforward_geglu on the own kernels (gemm8p; asserted engaged) against the fp64 composition of zorro_utils.py:115-128 and
    against the library path at the exact width -- output, input gradient and both weight gradients (written in place into the flat
    buffer at the EXACT shapes).  F = 300 / 2730 fit none of the own GEMM's tiles: the padded path, on the engine's padded copies.
    F = 512 needs no padding: the unpadded branch (the ViT-B product path) through the autograd node, every projection inside the own
    kernel's shape rules (N % 256 == 0, 128 GEGLU pairs; K >= 384, K % 128 == 0), 8229 rows ending in a partial M-tile."""
    from incomplete_multimodal_fusion_amd import ops
    w1, w2, eng = _ff_engine(D, F, 1)
    y = (torch.randn(rows, D, device=DEV) * 0.7).to(torch.bfloat16).requires_grad_(True)
    df = (torch.randn(rows, D, device=DEV) * 0.5).to(torch.bfloat16)

    def run(min_tiles, own):
        monkeypatch.setattr(ops, "_OWN_GEMM_MIN_TILES", min_tiles)
        monkeypatch.setattr(ops, "OWN_GEMM", own)
        eng.zero_grad(); y.grad = None
        before = dict(ops.CALLS)
        f = ops.feedforward_geglu(y, w1, w2)
        f.backward(df)
        eng.grad_norm()                                                 # flushes deferred split-K sums
        calls = {k: ops.CALLS[k] - before[k] for k in before}
        assert w1.grad is not None and w2.grad is not None
        return f.detach().float(), y.grad.detach().float(), w1._mmae_grad.clone(), w2._mmae_grad.clone(), calls
    f_p, dy_p, g1_p, g2_p, calls = run(0, 1)
    assert calls["mmae_gemm_geglu"] == 1 and calls["mmae_gemm_nt"] == 3, calls
    f_l, dy_l, g1_l, g2_l, calls_l = run(1 << 30, 0)
    assert calls_l["mmae_gemm_geglu"] == 0 and calls_l["mmae_gemm_nt"] == 0
    # fp64 reference on the bf16-rounded operands the GPU paths read
    yd = y.detach().double().cpu().requires_grad_(True)
    a1 = w1._mmae_shadow.double().cpu().requires_grad_(True); a2 = w2._mmae_shadow.double().cpu().requires_grad_(True)
    h = yd @ a1.t()
    val, gate = h[:, :F], h[:, F:]
    fr = (val * torch.nn.functional.gelu(gate)) @ a2.t()
    fr.backward(df.double().cpu())

    def rel(a, b):
        return float((a.double().cpu() - b).norm() / b.norm())
    for name, got_p, got_l, ref in (("f", f_p, f_l, fr.detach()), ("dy", dy_p, dy_l, yd.grad), ("dW1", g1_p, g1_l, a1.grad), ("dW2", g2_p, g2_l, a2.grad)):
        ep, el = rel(got_p, ref), rel(got_l, ref)
        assert ep < 1.2e-2 and ep < 1.5 * el + 1e-3, (name, ep, el)       # bf16 intermediates (h, g, dg, dh): same rounding points in both paths


def test_matmul_nt_destination_that_the_own_kernel_cannot_write_falls_back(monkeypatch, capsys):
    """own_gemm_ok() validates the DESTINATION too -- a 4-byte aligned or strided `out` view must take the library path
    instead of raising MMAE_ERR_ARG from the committed own kernel; and a projection that is big enough for the own kernel but beyond
    its 31-bit byte offsets says so once on stderr instead of falling back silently."""
    from incomplete_multimodal_fusion_amd import ops
    monkeypatch.setattr(ops, "_OWN_GEMM_MIN_TILES", 0)
    M, N, K = 1024, 256, 512
    a, w = _operands(M, N, K, seed=9)
    ref = a.float() @ w.float().t()
    before = ops.CALLS["mmae_gemm_nt"]
    big = torch.zeros(M, N + 6, device=DEV, dtype=torch.bfloat16)
    out = big[:, 2:2 + N]                                            # 4-byte aligned base, row stride N + 6
    assert out.data_ptr() % 8 != 0 and not ops.own_gemm_ok(a, w, out)
    ops.matmul_nt(a, w, out=out)
    close(out, ref, 1e-2, "library fallback into a misaligned view")
    assert ops.CALLS["mmae_gemm_nt"] == before
    good = torch.zeros(M, N + 8, device=DEV, dtype=torch.bfloat16)[:, 4:4 + N]       # 8-byte aligned, strided: the own kernel takes it
    assert ops.own_gemm_ok(a, w, good)
    ops.matmul_nt(a, w, out=good)
    close(good, ref, 1e-2, "own kernel into a strided view")
    assert ops.CALLS["mmae_gemm_nt"] == before + 1
    # beyond the 31-bit offsets (5.7 GB operand; uninitialised: only the dispatch decision is tested, nothing is launched)
    ops._WARNED.clear()
    huge = torch.empty(700000, 4096, device=DEV, dtype=torch.bfloat16)
    wbig = torch.empty(768, 4096, device=DEV, dtype=torch.bfloat16)
    assert not ops.own_gemm_ok(huge, wbig) and not ops.own_gemm_ok(huge, wbig)
    err = capsys.readouterr().err
    assert err.count("31-bit") == 1, err
