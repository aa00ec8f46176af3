"""The elementwise, row-routing and column-sum kernels of csrc/rowops.hip at their edges, through the C ABI.

  mmae_gelu_fwd / _bwd, mmae_geglu_fwd / _bwd     vs fp64 (Phi = erfc(-x/sqrt2)/2, phi = exp(-x^2/2)/sqrt(2 pi))
  mmae_scale_rows, mmae_gather_rows, mmae_scatter_rows     bitwise vs the same single fp32 operation in torch
  mmae_colsum                                     integer-valued inputs: equal to the int64 column sum in any summation order
  ops.gather_rows / ops.fork_gather_rows          gradients vs an fp64 index_add on the CPU

Guard bands: every tensor a kernel sees (`Band`) lives inside a larger allocation filled with a signalling-NaN bit pattern
(0x7FA5 / 0x7FA5A5A5) that no arithmetic and no copy of these inputs produces.  After each call everything outside the
logical output -- the pads before and after, the columns between W and the row stride, the scatter rows no index names --
must hold its earlier bits, and every input must be unchanged.  All pointers stay inside the allocation they come from.
Only the elementwise kernels get bases that are not 16-byte aligned (one element past an aligned address: their V = 1
kernels); gather / scatter bases stay 4-element aligned and colsum bases 16-byte aligned, as those entry points assume.

GELU bounds.  The kernels' formula (Abramowitz-Stegun 7.1.26, one exp2 and one reciprocal) evaluated on the CPU in fp32 with
exact exp2 and division differs from the fp64 reference by at most
    3.7e-7 (x Phi) and 2.7e-7 (Phi + x phi) over every finite bf16 value,
    4.2e-7 and 3.1e-7 over 2M fp32 values (randn * 3 and uniform(-12, 12)).
The hardware exp2 and rcp are good to about one ulp each, so the kernels get about 5x that: |err| <= 2e-6 for gelu and
1.5e-6 for gelu' at |x| <= 16; beyond 16 the exponential underflows and the results are exact (x and 1, or 0 and 0).
bf16 results are held to the interval bf16(ref - t) <= out <= bf16(ref + t), so rounding costs nothing extra; fp32 results
get 2^-22 |ref| on top for their own roundings.
Measured on an MI355X (fp32 kernels, |x| <= 16, linspace(-16, 16, .) and every finite bf16 value; printed by
test_gelu_fwd / test_gelu_bwd):
    gelu  (x Phi):        max |err| = 4.14e-7 (3.69e-7 over the bf16 values): 0.21 of the bound
    gelu' (Phi + x phi):  max |err| = 2.63e-7 (2.29e-7 over the bf16 values): 0.18 of the bound
i.e. the hardware exp2 and rcp cost nothing measurable over the exact-arithmetic figures above.
"""
import ctypes
import math

import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib, ops
from incomplete_multimodal_fusion_amd._lib import call, dt, ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="fp32")]
SENT = {BF16: 0x7FA5, F32: 0x7FA5A5A5}           # signalling NaNs: arithmetic only ever returns quiet ones
IBITS = {BF16: torch.int16, F32: torch.int32}
PAD = 64                                           # guard elements on either side (keeps 16-byte alignment for both types)
GELU_TOL, DGELU_TOL, U32 = 2e-6, 1.5e-6, 2.0 ** -22


def bits(t):
    return t.view(IBITS[t.dtype])


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Band:
    """A (rows, W) tensor of type T at row stride `stride`, `off` elements past a 16-byte aligned address, inside an
    allocation pre-filled with the sentinel.  `fill` (a (rows, W) tensor) makes it an input or a destination with earlier
    contents; without it the logical region holds the sentinel too (an output every element of which must be written)."""

    def __init__(self, T, rows, W, stride=None, off=0, fill=None):
        self.T, self.rows, self.W = T, rows, W
        self.stride = W if stride is None else stride
        assert self.stride >= W
        self.pre = PAD + off
        self.buf = torch.full((self.pre + rows * self.stride + PAD,), SENT[T], dtype=IBITS[T], device=DEV).view(T)
        self.t = self.buf[self.pre:self.pre + rows * self.stride].view(rows, self.stride)[:, :W]
        if fill is not None:
            self.t.copy_(fill.reshape(rows, W).to(DEV))
        self.snap = self.buf.clone()
        self.addr = self.buf.data_ptr() + self.pre * self.buf.element_size()      # (an empty view's data_ptr() is null)
        self.p = ctypes.c_void_p(self.addr)

    def outside(self):
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        m[self.pre:self.pre + self.rows * self.stride].view(self.rows, self.stride)[:, :self.W] = False
        return m

    def assert_guard(self, what):
        """Everything outside the logical (rows, W) region still holds the bits it had before the call."""
        m = self.outside()
        assert torch.equal(bits(self.buf)[m], bits(self.snap)[m]), what + ": wrote outside its logical region"

    def assert_unchanged(self, what):
        assert torch.equal(bits(self.buf), bits(self.snap)), what + ": an input (or its surroundings) was modified"

    def assert_all_written(self, what):
        assert not bool((bits(self.t) == SENT[self.T]).any()), what + ": sentinel left inside the output"


def vec(T):
    return 8 if T == BF16 else 4


def all_finite_bf16():
    """Every finite bf16 value (65280 = 8 * 8160 of them), in bit-pattern order: -0 ... -max, +0 ... +max."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    v = v[torch.isfinite(v)]
    assert v.numel() == 65280
    return v


def gelu_ref(x64):
    """-> (x Phi(x), Phi(x) + x phi(x)) in fp64, tail-accurate."""
    Phi = 0.5 * torch.erfc(-x64 / math.sqrt(2.0))
    phi = torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi)
    return x64 * Phi, Phi + x64 * phi


def assert_within(out, ref, tol, what, x=None):
    """out (type T) against the fp64 `ref` with the fp64 per-element tolerance `tol`: bf16 in interval form
    bf16(ref - tol) <= out <= bf16(ref + tol) (round to nearest, compared as floats), fp32 as |out - ref| <= tol."""
    out, ref, tol = out.reshape(-1), ref.reshape(-1), tol.reshape(-1)
    o = out.double()
    assert not bool(torch.isnan(o).any()), what + ": NaN in the result"
    if out.dtype == BF16:
        ok = ((ref - tol).to(BF16).double() <= o) & (o <= (ref + tol).to(BF16).double())
    else:
        ok = (o - ref).abs() <= tol
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError("%s: %d of %d outside the bound; first at %d: got %.9g, ref %.9g, tol %.3g%s" % (
            what, int((~ok).sum()), ok.numel(), i, float(o[i]), float(ref[i]), float(tol[i]),
            "" if x is None else ", x %.9g" % float(x.reshape(-1)[i])))


# ================================================================================================ 1. gelu / geglu vs fp64
def gelu_inputs(T, case):
    """-> (x, off): the values and the element offset of every base pointer."""
    if case == "bf16set-vector":                  # n = 65280, a multiple of 8 and of 4: V = 8 / 4 kernels
        return all_finite_bf16().to(T), 0
    if case == "bf16set-scalar-misaligned":       # same n, bases one element past 16-byte alignment: V = 1 kernels
        return all_finite_bf16().to(T), 1
    if case == "bf16set-scalar-n65279":           # n % V != 0: V = 1 kernels
        v = all_finite_bf16()
        return torch.cat([v[:12345], v[12346:]]).to(T), 0
    n = int(case.split("-n")[1])                  # fp32 grid: the EW_U = 2 tail states (vector) or n % 4 == 1 (scalar)
    return torch.linspace(-16.0, 16.0, n, dtype=torch.float64).to(T), 0


def _lin(k):
    return 4 * (512 * 3 + k)


GELU_CASES = [pytest.param(BF16, c, id="bf16-" + c) for c in
              ("bf16set-vector", "bf16set-scalar-misaligned", "bf16set-scalar-n65279")]
GELU_CASES += [pytest.param(F32, c, id="fp32-" + c) for c in
               ("bf16set-vector", "bf16set-scalar-misaligned", "bf16set-scalar-n65279",
                "vector-lastblock-empty-n%d" % _lin(0), "vector-lastblock-1vec-n%d" % _lin(1),
                "vector-lastblock-u0-short-n%d" % _lin(255), "vector-lastblock-u0-full-n%d" % _lin(256),
                "vector-lastblock-u1-1vec-n%d" % _lin(257), "scalar-n%d" % (4 * 512 * 3 + 1))]


@pytest.mark.parametrize("T,case", GELU_CASES)
def test_gelu_fwd(T, case):
    x, off = gelu_inputs(T, case)
    n = x.numel()
    X, Y = Band(T, 1, n, off=off, fill=x), Band(T, 1, n, off=off)
    call("mmae_gelu_fwd", dt(T), n, X.p, Y.p, stream())
    what = "gelu_fwd %s" % case
    X.assert_unchanged(what); Y.assert_guard(what); Y.assert_all_written(what)
    x64, y = X.t.reshape(-1).double(), Y.t.reshape(-1)
    ref, _ = gelu_ref(x64)
    tol = torch.full_like(ref, GELU_TOL) + (U32 * ref.abs() if T == F32 else 0.0)
    assert_within(y, ref, tol, what, x64)
    big, neg = x64 > 16, x64 < -16
    assert torch.equal(y[big], X.t.reshape(-1)[big]), what + ": gelu(x) != x beyond 16"
    assert bool((y[neg] == 0).all()), what + ": gelu(x) != 0 below -16"
    if T == F32:
        near = x64.abs() <= 16
        print("MEASURED gelu fwd %s: max |err| at |x| <= 16 = %.3e" % (case, float((y.double() - ref)[near].abs().max())))


@pytest.mark.parametrize("gkind", ["g1", "grand"])
@pytest.mark.parametrize("T,case", GELU_CASES)
def test_gelu_bwd(T, case, gkind):
    x, off = gelu_inputs(T, case)
    n = x.numel()
    g = torch.ones(n) if gkind == "g1" else torch.randn(n, generator=gen(3))
    X, G, DX = Band(T, 1, n, off=off, fill=x), Band(T, 1, n, off=off, fill=g.to(T)), Band(T, 1, n, off=off)
    call("mmae_gelu_bwd", dt(T), n, X.p, G.p, DX.p, stream())
    what = "gelu_bwd %s %s" % (case, gkind)
    X.assert_unchanged(what); G.assert_unchanged(what); DX.assert_guard(what); DX.assert_all_written(what)
    x64, g64, dx = X.t.reshape(-1).double(), G.t.reshape(-1).double(), DX.t.reshape(-1)
    _, d = gelu_ref(x64)
    ref = g64 * d
    tol = (DGELU_TOL + (U32 * d.abs() if T == F32 else 0.0)) * g64.abs()
    assert_within(dx, ref, tol, what, x64)
    big, neg = x64 > 16, x64 < -16
    assert torch.equal(dx[big], G.t.reshape(-1)[big]), what + ": gelu'(x) != 1 beyond 16"
    assert bool((dx[neg] == 0).all()), what + ": gelu'(x) != 0 below -16"
    if T == F32 and gkind == "g1":
        near = x64.abs() <= 16
        print("MEASURED gelu bwd %s: max |err| at |x| <= 16 = %.3e" % (case, float((dx.double() - ref)[near].abs().max())))


@pytest.mark.parametrize("off,n", [pytest.param(0, 4096, id="vector"), pytest.param(1, 4096, id="scalar-misaligned"),
                                   pytest.param(0, 4093, id="scalar-n4093")])
@pytest.mark.parametrize("T", TYPES)
def test_gelu_nan_stays_in_place(T, off, n):
    """NaN in -> NaN out at the same position and nowhere else (forward: x; backward: x or g)."""
    x = torch.randn(n, generator=gen(5)) * 3
    g = torch.randn(n, generator=gen(6))
    nan_x = torch.zeros(n, dtype=torch.bool); nan_x[[0, 7, 8, 511, 2048, n - 1]] = True
    nan_g = torch.zeros(n, dtype=torch.bool); nan_g[[1, 8, 1000, n - 2]] = True
    x[nan_x] = float("nan"); g[nan_g] = float("nan")
    X, G, Y, DX = Band(T, 1, n, off=off, fill=x.to(T)), Band(T, 1, n, off=off, fill=g.to(T)), Band(T, 1, n, off=off), Band(T, 1, n, off=off)
    call("mmae_gelu_fwd", dt(T), n, X.p, Y.p, stream())
    call("mmae_gelu_bwd", dt(T), n, X.p, G.p, DX.p, stream())
    X.assert_unchanged("gelu nan"); G.assert_unchanged("gelu nan"); Y.assert_guard("gelu nan"); DX.assert_guard("gelu nan")
    Y.assert_all_written("gelu nan"); DX.assert_all_written("gelu nan")
    assert torch.equal(torch.isnan(Y.t.reshape(-1)).cpu(), nan_x), "gelu_fwd: NaN positions moved"
    assert torch.equal(torch.isnan(DX.t.reshape(-1)).cpu(), nan_x | nan_g), "gelu_bwd: NaN positions moved"


# (rows, F, offset of out / dh in elements, dispatch path)
GEGLU_SHAPES = [
    pytest.param(1, 8, 0, id="1x8-vector-shift-oneblock"),
    pytest.param(3, 8, 0, id="3x8-vector-shift"),
    pytest.param(64, 64, 0, id="64x64-vector-shift-pow2-per-row"),
    pytest.param(33, 40, 0, id="33x40-vector-divide"),
    pytest.param(7, 85, 0, id="7x85-scalar-F%V-divide"),
    pytest.param(129, 520, 0, id="129x520-vector-divide-multiblock-partial"),
    pytest.param(64, 64, 1, id="64x64-scalar-misaligned-out"),
]


def gate_grid(T):
    """linspace(-18, 18) and every finite bf16 value up to 32 in magnitude, in T: the tails, zero and the denormals."""
    v = all_finite_bf16().double()
    return torch.cat([torch.linspace(-18.0, 18.0, 4099, dtype=torch.float64), v[v.abs() <= 32]]).to(T)


def geglu_inputs(T, rows, F):
    """h (rows, 2F): value half random with entries exactly 1.0 and 0.0, gate half the dense grid cycled at a stride coprime
    to its length (so a shape of 8 elements already sees both tails); g random."""
    grid = gate_grid(T)
    i = torch.arange(rows * F, dtype=torch.int64)
    gate = grid[(i * 1031) % grid.numel()].reshape(rows, F)
    val = torch.randn(rows, F, generator=gen(11))
    pick = torch.rand(rows, F, generator=gen(12))
    val[pick < 0.125] = 1.0; val[pick > 0.875] = 0.0
    g = torch.randn(rows, F, generator=gen(13))
    return torch.cat([val.to(T), gate], dim=1), g.to(T)


@pytest.mark.parametrize("rows,F,off", GEGLU_SHAPES)
@pytest.mark.parametrize("T", TYPES)
def test_geglu_fwd(T, rows, F, off):
    h, _ = geglu_inputs(T, rows, F)
    H, OUT = Band(T, rows, 2 * F, fill=h), Band(T, rows, F, off=off)
    call("mmae_geglu_fwd", dt(T), rows, F, H.p, OUT.p, stream())
    what = "geglu_fwd (%d, %d) off %d" % (rows, F, off)
    H.assert_unchanged(what); OUT.assert_guard(what); OUT.assert_all_written(what)
    val, gate = H.t[:, :F].double(), H.t[:, F:].double()
    ref = val * gelu_ref(gate)[0]
    assert_within(OUT.t, ref, GELU_TOL * val.abs() + U32 * ref.abs(), what, gate)


@pytest.mark.parametrize("rows,F,off", GEGLU_SHAPES)
@pytest.mark.parametrize("T", TYPES)
def test_geglu_bwd(T, rows, F, off):
    h, g = geglu_inputs(T, rows, F)
    H, G, DH = Band(T, rows, 2 * F, fill=h), Band(T, rows, F, fill=g), Band(T, rows, 2 * F, off=off)
    call("mmae_geglu_bwd", dt(T), rows, F, H.p, G.p, DH.p, stream())
    what = "geglu_bwd (%d, %d) off %d" % (rows, F, off)
    H.assert_unchanged(what); G.assert_unchanged(what); DH.assert_guard(what); DH.assert_all_written(what)
    val, gate, g64 = H.t[:, :F].double(), H.t[:, F:].double(), G.t.double()
    y, d = gelu_ref(gate)
    ref_val, ref_gate = g64 * y, g64 * val * d
    assert_within(DH.t[:, :F], ref_val, GELU_TOL * g64.abs() + U32 * ref_val.abs(), what + " dval", gate)
    assert_within(DH.t[:, F:], ref_gate, DGELU_TOL * (g64 * val).abs() + U32 * ref_gate.abs(), what + " dgate", gate)


@pytest.mark.parametrize("rows,F,off", [pytest.param(33, 40, 0, id="vector"), pytest.param(7, 85, 0, id="scalar")])
@pytest.mark.parametrize("T", TYPES)
def test_geglu_bwd_halves_not_swapped(T, rows, F, off):
    """value = 1, gate = 0: dval = g * gelu(0) = 0 and dgate = g * gelu'(0) = g / 2, both exact -- and different."""
    h = torch.cat([torch.ones(rows, F), torch.zeros(rows, F)], dim=1).to(T)
    g = torch.randn(rows, F, generator=gen(17)).to(T)
    H, G, DH = Band(T, rows, 2 * F, fill=h), Band(T, rows, F, fill=g), Band(T, rows, 2 * F, off=off)
    call("mmae_geglu_bwd", dt(T), rows, F, H.p, G.p, DH.p, stream())
    DH.assert_guard("geglu halves")
    assert bool((DH.t[:, :F] == 0).all()), "dval half is not zero"
    assert torch.equal(DH.t[:, F:], (G.t.float() * 0.5).to(T)), "dgate half is not g / 2"


# ================================================================================================ 2. scale / gather / scatter
def row_scales(rows):
    """0, 1, 1 / keep (keep = 0.9) and a negative value, starting at 1 / keep so that one row already scales."""
    s = torch.tensor([1.0 / 0.9, 0.0, 1.0, -1.75], dtype=torch.float32)
    return s[torch.arange(rows) % 4].to(DEV)


# the geglu shapes with W for F; also in place (out is x: every element is read and written by the same lane, so a caller may
# scale a gradient it owns without a second tensor) wherever out has no offset of its own
SCALE_CASES = [pytest.param(*p.values, False, id=p.id + "-out") for p in GEGLU_SHAPES]
SCALE_CASES += [pytest.param(*p.values, True, id=p.id + "-inplace") for p in GEGLU_SHAPES if p.values[2] == 0]


@pytest.mark.parametrize("rows,W,off,inplace", SCALE_CASES)
@pytest.mark.parametrize("T", TYPES)
def test_scale_rows(T, rows, W, off, inplace):
    x = torch.randn(rows, W, generator=gen(21)).to(T)
    s = row_scales(rows)
    X = Band(T, rows, W, fill=x)
    OUT = X if inplace else Band(T, rows, W, off=off)
    ref = (X.t.float() * s[:, None]).to(T)
    s0 = s.clone()
    call("mmae_scale_rows", dt(T), rows, W, X.p, ptr(s), OUT.p, stream())
    what = "scale_rows (%d, %d) off %d %s" % (rows, W, off, "in place" if inplace else "")
    OUT.assert_guard(what)
    if not inplace:
        X.assert_unchanged(what)
    assert torch.equal(s, s0), what + ": the scales were modified"
    assert torch.equal(bits(OUT.t), bits(ref)), what + ": not bitwise x * scale"


def gather_indices(rows, nsrc):
    """The last source row, -1, the first row, repeats of both, then random rows with one in eight -1."""
    head = [nsrc - 1, -1, 0, 0, nsrc - 1]
    idx = torch.randint(0, nsrc, (rows,), generator=gen(31), dtype=torch.int32)
    idx[torch.rand(rows, generator=gen(32)) < 0.125] = -1
    k = min(rows, len(head))
    idx[:k] = torch.tensor(head[:k], dtype=torch.int32)
    return idx.to(DEV)


GATHER_W = [pytest.param(4, id="W4-one-lane"), pytest.param(8, id="W8-two-lanes"), pytest.param(252, id="W252-one-trip-short"),
            pytest.param(256, id="W256-one-trip-full"), pytest.param(260, id="W260-column-loop-2nd-trip-one-lane"),
            pytest.param(1028, id="W1028-column-loop-5-trips")]
NSRC = 37


def check_gather(T, W, rows, src_stride=None, out_stride=None, off=0):
    src = torch.randn(NSRC, W, generator=gen(33)).to(T)
    SRC, OUT = Band(T, NSRC, W, stride=src_stride, off=off, fill=src), Band(T, rows, W, stride=out_stride, off=off)
    idx = gather_indices(rows, NSRC)
    idx0 = idx.clone()
    call("mmae_gather_rows", dt(T), rows, W, SRC.p, SRC.stride, ptr(idx), OUT.p, OUT.stride, stream())
    what = "gather_rows W %d rows %d strides %s %s" % (W, rows, src_stride, out_stride)
    SRC.assert_unchanged(what); OUT.assert_guard(what)
    assert torch.equal(idx, idx0), what + ": the indices were modified"
    ref = torch.zeros(rows, W, dtype=T, device=DEV)
    ok = idx >= 0
    ref[ok] = SRC.t[idx[ok].long()]
    assert torch.equal(bits(OUT.t), bits(ref)), what + ": not a bitwise copy of the indexed rows"
    assert bool((bits(OUT.t)[~ok] == 0).all()), what + ": a -1 row is not all zero bits"


@pytest.mark.parametrize("W", GATHER_W)
@pytest.mark.parametrize("T", TYPES)
def test_gather_rows(T, W):
    """rows 1, 3, 5, 1001: the last block has 1, 3, 1, 1 live waves; 4: none idle."""
    for rows in (1, 3, 4, 5, 1001):
        check_gather(T, W, rows)


@pytest.mark.parametrize("T", TYPES)
def test_gather_rows_strided(T):
    """src and out are column slices, 4 elements into rows of wider tensors (strides > W), W = 260 (column loop)."""
    check_gather(T, 260, 5, src_stride=272, out_stride=268, off=4)
    check_gather(T, 260, 1001, src_stride=272, out_stride=268, off=4)


NDST, SROWS = 300, 203          # 203 = 4 * 50 + 3: the last block has an idle wave


def scatter_plan(filtered):
    """-> (idx, filt): 203 rows into 300 destination rows.  Without a filter the non-negative indices are unique; with one
    they are unique within each of three classes and repeat across them.  Rows 0 and 299 are named, -1 occurs."""
    if not filtered:
        idx = torch.randperm(NDST, generator=gen(41))[:SROWS].to(torch.int32)
        idx[0], idx[1], idx[2] = 0, NDST - 1, -1
        idx[3:][idx[3:] == 0] = -1; idx[3:][idx[3:] == NDST - 1] = -1
        idx[torch.arange(SROWS) % 9 == 5] = -1
        return idx.to(DEV), None
    filt = (torch.randperm(SROWS, generator=gen(42)) % 3).to(torch.int32)
    idx = torch.empty(SROWS, dtype=torch.int32)
    for f in range(3):
        rows_f = (filt == f).nonzero().reshape(-1)
        pick = torch.randperm(NDST - 2, generator=gen(43 + f))[:rows_f.numel()].to(torch.int32) + 1       # 1 .. 298, unique
        pick[0], pick[1], pick[2] = 0, NDST - 1, -1                                                        # in every class
        idx[rows_f] = pick
    return idx.to(DEV), filt.to(DEV)


def scatter_reference(T, dst0, src, idx, filt, accumulate):
    """The passes the wrappers run (ops._GatherRows / _ForkGatherRows backward), restated with torch indexing."""
    ref = dst0.clone()
    passes = [(None, accumulate)] if filt is None else [(f, 1 if (accumulate or f > 0) else 0) for f in range(3)]
    for f, acc in passes:
        sel = idx >= 0 if f is None else (idx >= 0) & (filt == f)
        d = idx[sel].long()
        ref[d] = (ref[d].float() + src[sel].float()).to(T) if acc else src[sel]
    return ref, passes


def check_scatter(T, W, accumulate, filtered, src_stride=None, dst_stride=None, off=0):
    src = torch.randn(SROWS, W, generator=gen(47)).to(T)
    old = torch.randn(NDST, W, generator=gen(48)).to(T)
    idx, filt = scatter_plan(filtered)
    # earlier contents: random values wherever a pass reads them (accumulate, or the later class passes); the sentinel for a
    # plain overwrite, so that the rows no index names are seen to keep it
    SRC = Band(T, SROWS, W, stride=src_stride, off=off, fill=src)
    DST = Band(T, NDST, W, stride=dst_stride, off=off, fill=old if (accumulate or filtered) else None)
    ref, passes = scatter_reference(T, DST.t.clone(), SRC.t, idx, filt, accumulate)
    idx0 = idx.clone()
    for f, acc in passes:
        call("mmae_scatter_rows", dt(T), SROWS, W, SRC.p, SRC.stride, ptr(idx), DST.p, DST.stride, acc,
             None if f is None else ptr(filt), 0 if f is None else f, stream())
    what = "scatter_rows W %d accumulate %d filter %s strides %s %s" % (W, accumulate, filtered, src_stride, dst_stride)
    SRC.assert_unchanged(what); DST.assert_guard(what)
    assert torch.equal(idx, idx0), what + ": the indices were modified"
    named = torch.zeros(NDST, dtype=torch.bool, device=DEV)
    named[idx[idx >= 0].long()] = True
    assert 0 < int(named.sum()) < NDST and bool(named[0]) and bool(named[NDST - 1])
    before = DST.snap[DST.pre:DST.pre + NDST * DST.stride].view(NDST, DST.stride)[:, :W]
    assert torch.equal(bits(DST.t)[~named], bits(before)[~named]), what + ": a row no index names changed"
    assert torch.equal(bits(DST.t), bits(ref)), what + ": differs from the per-class restatement"


@pytest.mark.parametrize("filtered", [False, True], ids=["nofilter", "filter3"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("W", GATHER_W)
@pytest.mark.parametrize("T", TYPES)
def test_scatter_rows(T, W, accumulate, filtered):
    check_scatter(T, W, accumulate, filtered)


@pytest.mark.parametrize("filtered", [False, True], ids=["nofilter", "filter3"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("T", TYPES)
def test_scatter_rows_strided(T, accumulate, filtered):
    """src and dst are column slices, 4 elements into rows of wider tensors (strides > W), W = 260 (column loop)."""
    check_scatter(T, 260, accumulate, filtered, src_stride=268, dst_stride=272, off=4)


# ---- through autograd: ~300 index rows over a 128-row source at W = 260 (the column loop), fp64 index_add on the CPU
AG_SRC, AG_W = 128, 260


def autograd_plan(filtered):
    """300 index rows.  Unfiltered: 120 distinct source rows at random positions, -1 elsewhere.  Filtered: three classes of 100
    rows, each naming 90 distinct source rows (so rows repeat across classes) and ten -1."""
    if not filtered:
        idx = torch.full((300,), -1, dtype=torch.int32)
        idx[torch.randperm(300, generator=gen(51))[:120]] = torch.randperm(AG_SRC, generator=gen(52))[:120].to(torch.int32)
        return idx, None
    filt = (torch.randperm(300, generator=gen(53)) % 3).to(torch.int32)
    idx = torch.full((300,), -1, dtype=torch.int32)
    for f in range(3):
        rows_f = (filt == f).nonzero().reshape(-1)
        idx[rows_f[:90]] = torch.randperm(AG_SRC, generator=gen(54 + f))[:90].to(torch.int32)
    return idx, filt


def check_autograd_grad(T, got, ref, roundings, what):
    """All gradient terms are positive, so every partial sum is below |ref|.  fp32: exact up to the order of at most four terms
    (three roundings of 2^-24 each) -> 2^-22 |ref|.  bf16 (8 significant bits, unit roundoff 2^-8): one rounding, 2^-8 of a
    partial sum <= |ref| (1 + 2^-8)^k, for each pass that adds -> roundings * 2^-8 * (1 + 2^-6) |ref|."""
    got, ref = got.detach().double().cpu(), ref.double()
    tol = (U32 if T == F32 else roundings * 2.0 ** -8 * (1 + 2.0 ** -6)) * ref.abs()
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), "%s: %d elements off, worst %.3g" % (what, int(bad.sum()), float(((got - ref).abs() - tol).max()))


def positive(shape, seed, T):
    return (torch.rand(shape, generator=gen(seed)) + 0.5).to(T)


@pytest.mark.parametrize("filtered", [False, True], ids=["unique", "filter3-three-accumulate-passes"])
@pytest.mark.parametrize("T", TYPES)
def test_gather_rows_autograd(T, filtered):
    idx, filt = autograd_plan(filtered)
    src, G = torch.randn(AG_SRC, AG_W, generator=gen(57)).to(T), positive((300, AG_W), 58, T)
    s = src.to(DEV).requires_grad_()
    out = ops.gather_rows(s, idx.to(DEV), unique=not filtered, filt=None if filt is None else filt.to(DEV), nfilt=3 if filtered else 0)
    out.backward(G.to(DEV))
    ok = idx >= 0
    ref_out = torch.zeros(300, AG_W, dtype=T); ref_out[ok] = src[idx[ok].long()]
    assert torch.equal(bits(out.detach().cpu()), bits(ref_out)), "gather_rows forward"
    ref = torch.zeros(AG_SRC, AG_W, dtype=torch.float64).index_add_(0, idx[ok].long(), G[ok].double())
    check_autograd_grad(T, s.grad, ref, 3 if filtered else 0, "gather_rows grad (filtered %s)" % filtered)


@pytest.mark.parametrize("filtered", [False, True], ids=["unique", "filter3"])
@pytest.mark.parametrize("fresh", [True, False], ids=["fresh-grad-in-place", "grad-copied"])
@pytest.mark.parametrize("T", TYPES)
def test_fork_gather_rows_autograd(T, fresh, filtered):
    idx, filt = autograd_plan(filtered)
    src, G, A = torch.randn(AG_SRC, AG_W, generator=gen(61)).to(T), positive((300, AG_W), 62, T), positive((AG_SRC, AG_W), 63, T)
    s = src.to(DEV).requires_grad_()
    through, out = ops.fork_gather_rows(s, idx.to(DEV), None if filt is None else filt.to(DEV), 3 if filtered else 0, fresh)
    Ad = A.to(DEV)
    ((through * Ad).sum() + (out * G.to(DEV)).sum()).backward()
    ok = idx >= 0
    ref_out = torch.zeros(300, AG_W, dtype=T); ref_out[ok] = src[idx[ok].long()]
    assert torch.equal(bits(out.detach().cpu()), bits(ref_out)), "fork_gather_rows forward"
    assert torch.equal(bits(Ad.cpu()), bits(A)), "fork_gather_rows: the other consumer's operand was modified"
    ref = A.double().index_add_(0, idx[ok].long(), G[ok].double())
    check_autograd_grad(T, s.grad, ref, 3 if filtered else 1, "fork_gather_rows grad (fresh %s, filtered %s)" % (fresh, filtered))


# ================================================================================================ 3. colsum
def colsum_rows_per_block(rows, cols, V):
    """csrc/rowops.hip colsum_rows_per_block, restated: at most 256 partial rows, at least 16 loads per thread."""
    cg = cols // V
    rpi = 256 // cg if cg <= 256 else 1
    return max((rows + 255) // 256, 16 * rpi), rpi


def colsum_blocks(rows, cols, V):
    rpb, _ = colsum_rows_per_block(rows, cols, V)
    return max(1, -(-rows // rpb))


def run_colsum(T, x, cols, ld=None, col_off=0):
    """x (rows, ld) -> (out, second out): mmae_colsum of the `cols` columns from `col_off` on, called twice on the same
    workspace; guards around out and the workspace, the input unchanged."""
    rows = x.shape[0]
    ld = cols if ld is None else ld
    X = Band(T, rows, ld, fill=x)
    nws = int(_lib.lib().mmae_colsum_ws_floats(rows, cols))
    assert nws == 256 * cols
    OUT, WS = Band(F32, 1, cols), Band(F32, 1, nws)
    xp = ctypes.c_void_p(X.addr + col_off * X.buf.element_size())
    assert xp.value % 16 == 0
    call("mmae_colsum", dt(T), rows, cols, xp, ld, OUT.p, WS.p, stream())
    first = OUT.t.reshape(-1).clone()
    call("mmae_colsum", dt(T), rows, cols, xp, ld, OUT.p, WS.p, stream())
    what = "colsum %s (%d, %d) ld %d" % (T, rows, cols, ld)
    X.assert_unchanged(what); OUT.assert_guard(what); WS.assert_guard(what); OUT.assert_all_written(what)
    assert torch.equal(bits(first), bits(OUT.t.reshape(-1))), what + ": the second call differs"
    return first


def int_matrix(rows, ld, seed):
    return torch.randint(-8, 9, (rows, ld), generator=gen(seed), dtype=torch.int8)


def check_colsum_exact(T, rows, cols, nb, ld=None, col_off=0):
    V = vec(T)
    assert colsum_blocks(rows, cols, V) == nb, "the case does not reach the intended number of partial rows"
    xi = int_matrix(rows, cols if ld is None else ld, 71)
    out = run_colsum(T, xi.to(T), cols, ld, col_off)
    ref = xi[:, col_off:col_off + cols].sum(0, dtype=torch.int64)
    assert torch.equal(out.cpu().to(torch.int64), ref) and bool((out == out.round()).all()), \
        "colsum %s (%d, %d): not the integer column sum (%d columns differ)" % (T, rows, cols, int((out.cpu().double() != ref.double()).sum()))


# (T, cols, rows, nb): nb = number of partial rows (blocks of stage 1) that finish adds; rows = rows_per_block * nb or fewer
COLSUM_CASES = [
    # cg = 1: 256 rows in flight, rows_per_block 4096
    (BF16, 8, 300, 1, "cg1-rpi256"), (BF16, 8, 5000, 2, "cg1-rpi256"), (F32, 4, 65541, 17, "cg1-rpi256-finish-tail-2nd-trip"),
    # cg = 12: rpi 21, threads 252..255 idle, rows_per_block 336
    (F32, 48, 5376, 16, "cg12-rpi21-idle-threads"), (F32, 48, 37968, 113, "cg12-rpi21-idle-threads-finish-unrolled-once"),
    # cg = 96: rpi 2, 64 idle threads, rows_per_block 32
    (BF16, 768, 4096, 128, "cg96-rpi2-finish-unrolled-no-tail"), (BF16, 768, 4097, 129, "cg96-rpi2-finish-unrolled-plus-tail"),
    (BF16, 768, 6400, 200, "cg96-rpi2"), (BF16, 768, 8192, 256, "cg96-rpi2-full-workspace"),
    # cg = 256: the last width of the rows-in-flight branch (rpi 1), rows_per_block 16
    (F32, 1024, 272, 17, "cg256-branch-boundary"), (F32, 1024, 1800, 113, "cg256-branch-boundary-short-last-block"),
    # cg > 256: one column group per thread and trip
    (F32, 1028, 31, 2, "cg257-wide-branch-2nd-trip-one-thread"), (F32, 1028, 2060, 129, "cg257-wide-branch"),
    (BF16, 2304, 13, 1, "cg288-wide-branch"), (BF16, 2304, 256, 16, "cg288-wide-branch"),
    (BF16, 2304, 3200, 200, "cg288-wide-branch"), (BF16, 2304, 4096, 256, "cg288-wide-branch-full-workspace"),
]
# rows 0, 1, 15, 16, 17 at a narrow (rows_per_block 4096) and a wide (rows_per_block 16) shape
COLSUM_CASES += [(BF16, 8, r, 1, "cg1-few-rows") for r in (0, 1, 15, 16, 17)]
COLSUM_CASES += [(F32, 1028, r, 2 if r == 17 else 1, "cg257-few-rows") for r in (0, 1, 15, 16, 17)]


@pytest.mark.parametrize("T,cols,rows,nb", [
    pytest.param(T, cols, rows, nb, id="%s-cols%d-rows%d-nb%d-%s" % ("bf16" if T == BF16 else "fp32", cols, rows, nb, path))
    for T, cols, rows, nb, path in COLSUM_CASES])
def test_colsum_exact(T, cols, rows, nb):
    check_colsum_exact(T, rows, cols, nb)


@pytest.mark.parametrize("T", TYPES)
def test_colsum_rows0_writes_zero_bits(T):
    out = run_colsum(T, torch.zeros(0, 8 * vec(T), dtype=T), 8 * vec(T))
    assert bool((bits(out) == 0).all())


@pytest.mark.parametrize("T", TYPES)
def test_colsum_column_slice(T):
    """ld > cols: 512 columns from column 256 of a 1024-wide tensor (cg = 64 / 128, rpi = 4 / 2); nb = 16 / 32."""
    check_colsum_exact(T, 1000, 512, 16 if T == BF16 else 32, ld=1024, col_off=256)


def test_colsum_large():
    """(65536, 768) bf16: rows_per_block 256, nb = 256 -- the bench's bias-gradient shape; a single dropped row fails."""
    check_colsum_exact(BF16, 65536, 768, 256)


@pytest.mark.parametrize("T,cols,rows", [pytest.param(F32, 48, 5000, id="fp32-cols48-cg12"), pytest.param(BF16, 768, 4097, id="bf16-cols768-cg96"),
                                         pytest.param(F32, 1028, 2060, id="fp32-cols1028-wide-branch")])
def test_colsum_random_floats(T, cols, rows):
    """Not the main check: random floats against the fp64 sum, per column within (depth + 1) 2^-24 sum_r |x[r, c]|."""
    V = vec(T)
    rpb, rpi = colsum_rows_per_block(rows, cols, V)
    nb = colsum_blocks(rows, cols, V)
    # additions on the longest path to one output: a thread of stage 1 adds ceil(rows_per_block / rpi) rows to its accumulator,
    # the strip's rpi accumulators are added one after the other; in finish the longest chain is s0 (at most ceil(nb / 16)
    # partial rows), then 3 levels of the s0..s7 tree and the 16 row groups one after the other
    depth = -(-rpb // rpi) + rpi + -(-nb // 16) + 3 + 16
    x = torch.randn(rows, cols, generator=gen(81)).to(T)
    out = run_colsum(T, x, cols).cpu().double()
    ref, mag = x.double().sum(0), x.double().abs().sum(0)
    err, tol = (out - ref).abs(), (depth + 1) * 2.0 ** -24 * mag
    assert bool((err <= tol).all()), "colsum random: worst err / tol %.3g (depth %d)" % (float((err / tol).max()), depth)
