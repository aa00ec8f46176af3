"""Modality attention of Block_Fusion (csrc/modattn.hip) against a plain fp64 restatement, on every dispatch path.

For every (sample, patch) row the fusion query attends over the row's ns = M+1 slots; `slot_row[row, s]` names the kv row
slot s reads, kv = [token rows | fusion rows | P shared mask-embedding rows].  mmae_modattn_fwd / _bwd dispatch to 46
kernel instantiations, all launched here:
  fast  <T, DH, NS>  forward and backward, I == 512 and 2 <= ns <= 5:    2 dtypes x 2 head dims x 4 slot counts x 2 = 32
  generic forward <T, DH> (every other I / ns):                                                            4
  generic backward <T, DH, NCH> (NCH = 1: I <= 512, NCH = 2: 512 < I <= 1024):                              8
  finish <T>: the per-sample-group fp32 slabs of the shared rows summed in fixed order:                      2
The reference (`ref_modattn`) gathers the slot rows into a dense (rows, ns, 2I) fp64 tensor, runs per-head softmax
attention with torch, takes dq and the gathered rows' gradient from autograd and index_adds the latter into the kv rows
(a shared row collects every sample and slot that names it).  `oracle_route` is a second, independent construction for the
descriptor-driven cases: all_tokens built as the oracle builds it (mask_embedding cloned, kept tokens scattered in, the
fusion slot last).

Tolerances (tests/test_gpu_kernels.py): fp32 TIGHT of max|ref| for out, dq and the token rows of dkv, COLSUM x TIGHT for
the shared rows (each a sum over up to B*M slot gradients).  bf16: the inputs are exact in fp64 and the kernels accumulate
in fp32 and round once, so every ELEMENT is held to 2^-8 |ref| + 2^-12 max|ref|."""
import random

import pytest
import torch

from incomplete_multimodal_fusion_amd import _lib, ops
from incomplete_multimodal_fusion_amd._lib import call, ptr, stream
from oracle import mmae_oracle as O
from tests.test_gpu_kernels import COLSUM, TIGHT, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -30000.0            # padding-column sentinel (exact in fp32 and bf16)
PATTERNS = ("random", "all_masked", "none", "drop", "mixed")


# ------------------------------------------------------------------------------------------------ slot tables
def kept_pattern(pattern, B, P, M, gen):
    """(B, P, M) bool: True -> the slot reads its own token row, False -> the patch's shared mask-embedding row."""
    kept = torch.rand(B, P, M, generator=gen) < 0.5
    if M == 0:
        return kept
    if pattern == "all_masked":            # patch 0: every modality slot masked in every sample (M copies of one row)
        kept[:, 0, :] = False
    elif pattern == "none":
        kept[:] = True
    elif pattern == "drop":                # modality 0 dropped entirely
        kept[:, :, 0] = False
    elif pattern == "mixed":               # the last patch kept in even samples, masked in odd ones
        kept[0::2, -1, :] = True
        kept[1::2, -1, :] = False
    return kept


def make_slots(kept, spare=0, gen=None):
    """Slot table over kv = [token rows (shuffled, plus `spare` rows no slot names) | B*P fusion rows | P shared rows].
    -> slot (B*P, ns) int32 (host), kv row count, shared_base, the unnamed token rows."""
    B, P, M = kept.shape
    T = int(kept.sum())
    perm = torch.randperm(T + spare, generator=gen)
    fus_base = T + spare
    shared_base = fus_base + B * P
    slot = torch.empty(B, P, M + 1, dtype=torch.long)
    mod = (shared_base + torch.arange(P)).view(1, P, 1).repeat(B, 1, M)
    mod[kept] = perm[:T]
    slot[..., :M] = mod
    slot[..., M] = fus_base + torch.arange(B * P).view(B, P)
    return slot.view(B * P, M + 1).to(torch.int32), shared_base + P, shared_base, perm[T:]


# ------------------------------------------------------------------------------------------------ fp64 references
def _attend(q, slots, H, dh, scale):
    r, ns, I2 = slots.shape
    I = I2 // 2
    k = slots[..., :I].reshape(r, ns, H, dh)
    v = slots[..., I:].reshape(r, ns, H, dh)
    a = torch.softmax(torch.einsum("rhd,rshd->rhs", q.reshape(r, H, dh), k) * scale, dim=-1)
    return torch.einsum("rhs,rshd->rhd", a, v).reshape(r, I)


def ref_modattn(q, kv, slot, gout, H, dh, scale, chunk=4096):
    """fp64 on q's device, in row chunks (the dense gather of the bench shape is ~2 GB).  -> out, dq, dkv."""
    rows, ns = slot.shape
    I = H * dh
    kv64 = kv.double()
    out = torch.empty(rows, I, dtype=torch.float64, device=q.device)
    dq = torch.empty_like(out)
    dkv = torch.zeros(kv.shape[0], 2 * I, dtype=torch.float64, device=q.device)
    slot = slot.to(q.device).long()
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        idx = slot[r0:r1]
        qc = q[r0:r1].double().requires_grad_()
        g = kv64[idx].requires_grad_()
        o = _attend(qc, g, H, dh, scale)
        o.backward(gout[r0:r1].double())
        out[r0:r1] = o.detach()
        dq[r0:r1] = qc.grad
        dkv.index_add_(0, idx.reshape(-1), g.grad.reshape(-1, 2 * I))
    return out, dq, dkv


def oracle_route(q, kv, gout, mask_all, B, M, P, N, H, dh, scale):
    """fp64, independent of slot_row: per sample, all_tokens as oracle/mmae_oracle.py builds it (mask_embedding cloned,
    the sample's packed kept tokens of modality m scattered to its kept patches, the fusion tokens as the last slot),
    attention of the fusion query over the M+1 slots, autograd back to the kv rows."""
    I = H * dh
    kv64 = kv.double().cpu().requires_grad_()
    q64 = q.double().cpu().requires_grad_()
    shared_base = B * N + B * P
    me = kv64[shared_base:shared_base + P]
    outs = []
    for b in range(B):
        mask = mask_all[0 if mask_all.shape[0] == 1 else b].cpu().view(M, P)
        tokens = kv64[b * N:(b + 1) * N]
        slots, off = [], 0
        for m in range(M):
            ix = (mask[m] == 0).nonzero(as_tuple=True)[0]
            f = me.clone()
            f[ix] = tokens[off:off + len(ix)]
            off += len(ix)
            slots.append(f)
        slots.append(kv64[B * N + b * P:B * N + (b + 1) * P])
        all_tokens = torch.stack(slots, dim=1)                      # (P, M+1, 2I)
        outs.append(_attend(q64[b * P:(b + 1) * P], all_tokens, H, dh, scale))
    out = torch.cat(outs)
    out.backward(gout.double().cpu())
    return out.detach(), q64.grad, kv64.grad


# ------------------------------------------------------------------------------------------------ the kernels through the C ABI
def padded(rows, cols, pad, T, value=None):
    """(storage with `pad` sentinel columns, the (rows, cols) view handed to the kernel)."""
    buf = torch.full((rows, cols + pad), SENT, dtype=T, device=DEV)
    v = buf[:, :cols]
    if value is None:
        v.fill_(float("nan"))
    else:
        v.copy_(value)
    return buf, v


def run_modattn(q, kv, slot, gout, B, P, dh, shared_base, pads=(0,) * 6, backward_twice=False):
    """mmae_modattn_fwd + _bwd on operands with padded row strides (q, kv, out, dout, dq, dkv); out, dq and dkv start as
    NaN.  Asserts every padding column still holds the sentinel.  -> out, dq, dkv (views), and a second dkv / dq when
    backward_twice."""
    T = q.dtype
    rows, I = q.shape
    ns = slot.shape[1]
    nkv = kv.shape[0]
    assert rows == B * P and kv.shape[1] == 2 * I and nkv >= shared_base + P
    assert int(slot.min()) >= 0 and int(slot.max()) < nkv              # the kernels trust slot_row: check before launching
    slot = slot.to(DEV).contiguous()
    scale = dh ** -0.5
    qb, qv = padded(rows, I, pads[0], T, q)
    kvb, kvv = padded(nkv, 2 * I, pads[1], T, kv)
    ob, ov = padded(rows, I, pads[2], T)
    gb, gv = padded(rows, I, pads[3], T, gout)
    call("mmae_modattn_fwd", _lib.dt(T), dh, B, P, ns, I, ptr(qv), qb.stride(0), ptr(kvv), kvb.stride(0), ptr(slot),
         ptr(ov), ob.stride(0), scale, stream())
    ws = torch.empty(_lib.lib().mmae_modattn_bwd_nsplit(B) * P * 2 * I, dtype=torch.float32, device=DEV)
    res, bufs = [], [(qb, pads[0], "q"), (kvb, pads[1], "kv"), (ob, pads[2], "out"), (gb, pads[3], "dout")]
    for _ in range(2 if backward_twice else 1):
        dqb, dqv = padded(rows, I, pads[4], T)
        dkb, dkv = padded(nkv, 2 * I, pads[5], T)
        call("mmae_modattn_bwd", _lib.dt(T), dh, B, P, ns, I, ptr(qv), qb.stride(0), ptr(kvv), kvb.stride(0), ptr(slot),
             ptr(gv), gb.stride(0), ptr(dqv), dqb.stride(0), ptr(dkv), dkb.stride(0), shared_base, scale, ptr(ws), stream())
        res += [dqv, dkv]
        bufs += [(dqb, pads[4], "dq"), (dkb, pads[5], "dkv")]
    torch.cuda.synchronize()
    for buf, pad, name in bufs:
        assert bool((buf[:, buf.shape[1] - pad:] == SENT).all()), "padding columns of %s overwritten" % name
    return (ov,) + tuple(res)


def assert_bf16(got, ref, what):
    """Elementwise: |got - ref| <= 2^-8 |ref| + 2^-12 max|ref| (fp32 accumulation, one rounding to bf16)."""
    got = got.double().cpu(); ref = ref.double().cpu()
    assert not torch.isnan(got).any(), what + ": NaN in result"
    if ref.numel() == 0:
        return
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -12 * max(float(ref.abs().max()), 1e-30)
    ratio = float(((got - ref).abs() / bound).max())
    assert ratio <= 1.0, "%s: worst element at %.2fx the bf16 bound" % (what, ratio)


def check(T, got, ref, named, shared, what):
    """got / ref: (out, dq, dkv).  named: kv rows below shared_base that some slot names; shared: the P shared rows."""
    (o, dq, dkv), (ro, rdq, rdkv) = got, ref
    dkv, rdkv = dkv.double().cpu(), rdkv.cpu()
    parts = [("out", o, ro, 1.0), ("dq", dq, rdq, 1.0), ("dkv token/fusion rows", dkv[named], rdkv[named], 1.0),
             ("dkv shared rows", dkv[shared], rdkv[shared], COLSUM)]
    for name, a, b, f in parts:
        if T == torch.float32:
            close(a, b, TIGHT[T] * f, "%s %s" % (what, name))
        else:
            assert_bf16(a, b, "%s %s" % (what, name))


def rand_inputs(rows, nkv, I, T, gen):
    q = torch.randn(rows, I, generator=gen).to(T)
    kv = torch.randn(nkv, 2 * I, generator=gen).to(T)
    gout = torch.randn(rows, I, generator=gen).to(T)
    return q.to(DEV), kv.to(DEV), gout.to(DEV)


def run_and_check(T, I, dh, kept, gen, pads=(0,) * 6, spare=0, what=""):
    """One random case on the product's row layout: kernel vs fp64 reference; unnamed rows keep their NaN.
    -> (out, dq, dkv), slot, kv."""
    B, P, _ = kept.shape
    slot, nkv, shared_base, unnamed = make_slots(kept, spare, gen)
    q, kv, gout = rand_inputs(B * P, nkv, I, T, gen)
    got = run_modattn(q, kv, slot, gout, B, P, dh, shared_base, pads)
    ref = ref_modattn(q, kv, slot, gout, I // dh, dh, dh ** -0.5)
    named = torch.ones(shared_base, dtype=torch.bool)
    named[unnamed] = False
    check(T, got, ref, named.nonzero(as_tuple=True)[0], torch.arange(shared_base, nkv), what)
    if len(unnamed):
        assert bool(torch.isnan(got[2].cpu()[unnamed]).all()), what + ": an unnamed kv row was written (the caller owns it)"
    return got, slot, kv


# ------------------------------------------------------------------------------------------------ 1. dispatch matrix
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_modattn_dispatch_matrix(T, dh):
    """I in {64, 192, 512, 576, 1024} x ns 1..8 at small B, P: the fast kernels (I == 512, ns 2..5), the generic forward and
    both generic backwards (I = 576: the second 512-column chunk only partly active), the finish kernel.  Slot patterns,
    padded strides and unnamed rows rotate over the cases."""
    gen = torch.Generator().manual_seed(1000 + dh + (T == torch.bfloat16))
    pad_sets = [(0, 0, 0, 0, 0, 0), (8, 24, 16, 8, 24, 8), (24, 8, 8, 16, 8, 24)]
    case = 0
    for I in (64, 192, 512, 576, 1024):
        for ns in range(1, 9):
            B, P = (3, 7) if case % 2 else (5, 4)
            kept = kept_pattern(PATTERNS[case % len(PATTERNS)], B, P, ns - 1, gen)
            what = "I %d ns %d %s" % (I, ns, PATTERNS[case % len(PATTERNS)])
            (o, dq, dkv), slot, kv = run_and_check(T, I, dh, kept, gen, pad_sets[case % 3], spare=case % 3, what=what)
            if ns == 1:
                # one slot: out = v of the fusion row, dq = dk = 0, dv = dout -- exact
                fr = slot[:, 0].long().to(DEV)
                assert torch.equal(o, kv[fr][:, I:]), what
                assert bool((dq == 0).all()) and bool((dkv[fr][:, :I] == 0).all()), what
            case += 1


# ------------------------------------------------------------------------------------------------ 2. batch and nsplit
BATCH = [(1, 7), (3, 7), (31, 7), (32, 7), (33, 7), (64, 7), (100, 7), (256, 7), (513, 7), (600, 7),
         (1, 1), (33, 1), (600, 1), (3, 256), (64, 256), (513, 256)]


@pytest.mark.parametrize("B,P", BATCH, ids=["B%d-P%d" % bp for bp in BATCH])
def test_modattn_batch_and_nsplit(B, P):
    """nsplit = clamp(B / 32, 1, 16) sample groups per patch: 1, 2, 3, 8 and 16 (below and at the clamp), B not a multiple
    of 4 or 32.  Fast path (I 512, ns 4, dh 64) in fp32 and bf16; at P = 7 also the generic path (I 576, ns 6, dh 32).
    The backward runs twice and must be bitwise equal (fixed-order slab sum, no atomics)."""
    gen = torch.Generator().manual_seed(B * 1000 + P)
    cases = [(torch.float32, 512, 4, 64), (torch.bfloat16, 512, 4, 64)]
    if P == 7:
        cases.append((torch.float32, 576, 6, 32))
    for T, I, ns, dh in cases:
        kept = kept_pattern("random", B, P, ns - 1, gen)
        slot, nkv, shared_base, _ = make_slots(kept, 0, gen)
        q, kv, gout = rand_inputs(B * P, nkv, I, T, gen)
        o, dq, dkv, dq2, dkv2 = run_modattn(q, kv, slot, gout, B, P, dh, shared_base, (8, 8, 0, 0, 8, 8), backward_twice=True)
        assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), "backward not bitwise deterministic at B %d" % B
        ref = ref_modattn(q, kv, slot, gout, I // dh, dh, dh ** -0.5)
        check(T, (o, dq, dkv), ref, torch.arange(shared_base), torch.arange(shared_base, nkv),
              "B %d P %d I %d %s" % (B, P, I, T))


# ------------------------------------------------------------------------------------------------ 3. descriptor-driven cases
def draws(R, M, P, gen, drop=False):
    alpha = torch.rand(R, M, generator=gen) + 0.05
    if drop:
        alpha[:, 0] = 0.0
    return (alpha / alpha.sum(1, keepdim=True), torch.rand(R, M, P, generator=gen), torch.rand(R, M * P, generator=gen))


def product_descriptors(B, M, P, N, R, gen, drop=False):
    d, n, na = draws(R, M, P, gen, drop)
    mask_all, _, _ = ops.masks_from_draws(d.to(DEV), n.to(DEV), na.to(DEV), N)
    desc = ops.Descriptors(mask_all, B, M, P, N)
    assert int(desc.status[0]) == 0
    return mask_all, desc


def assert_slot_contract(desc, mask_all, B, M, P, N):
    """slot_row <-> kernel contract: every row in [0, shared_base) named exactly once, a masked slot of (b, p) names
    shared_base + p, the fusion slot of (b, p) names B*N + b*P + p."""
    slot = desc.slot_row.cpu().long().view(B, P, M + 1)
    sb = desc.shared_base
    assert sb == B * N + B * P
    mask = mask_all.cpu().view(-1, M, P).transpose(1, 2).expand(B, P, M)       # (B, P, M), 1 = masked
    mod = slot[..., :M]
    shared = (sb + torch.arange(P)).view(1, P, 1).expand(B, P, M)
    assert torch.equal(mod[mask == 1], shared[mask == 1]), "a masked slot does not name its patch's shared row"
    assert bool((mod[mask == 0] < B * N).all()), "a kept slot does not name a token row"
    assert torch.equal(slot[..., M], B * N + torch.arange(B * P).view(B, P)), "fusion slot"
    named = slot.reshape(-1)
    named = named[named < sb]
    assert torch.equal(torch.bincount(named, minlength=sb), torch.ones(sb, dtype=torch.long)), \
        "a row below shared_base is named zero or several times"
    for b in range(B):                                  # kept tokens of a sample are packed in [b*N, (b+1)*N)
        rows = mod[b][mask[b] == 0]
        assert bool(((rows >= b * N) & (rows < (b + 1) * N)).all())


def test_descriptor_slot_contract_fuzzed():
    rng = random.Random(17)
    gen = torch.Generator().manual_seed(18)
    for case in range(40):
        M = rng.randint(1, 7); P = rng.choice([1, 4, 16, 49, 64, 256]); B = rng.choice([1, 2, 5, 33])
        R = rng.choice([1, B])
        N = rng.randint(1, M * P)
        mask_all, desc = product_descriptors(B, M, P, N, R, gen, drop=rng.random() < 0.3 and M > 1)
        assert_slot_contract(desc, mask_all, B, M, P, N)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_modattn_product_tables_oracle_route(T, per_sample):
    """Small shapes (B 5, P 16, M 3 and M 2 with a dropped modality) on the product's descriptor tables: kernel vs the
    slot-table gather AND vs the oracle's own all_tokens construction; every q / kv row comes back finite."""
    gen = torch.Generator().manual_seed(21 + per_sample)
    for M, drop, I, dh in ((3, False, 512, 64), (2, True, 512, 32), (4, False, 192, 64), (6, False, 576, 64)):
        B, P, N = 5, 16, 5 * M
        mask_all, desc = product_descriptors(B, M, P, N, B if per_sample else 1, gen, drop)
        assert_slot_contract(desc, mask_all, B, M, P, N)
        nkv = desc.shared_base + P
        q, kv, gout = rand_inputs(B * P, nkv, I, T, gen)
        got = run_modattn(q, kv, desc.slot_row, gout, B, P, dh, desc.shared_base, (0, 8, 0, 0, 0, 16))
        for t in got:
            assert bool(torch.isfinite(t).all()), "every row of out / dq / dkv must be written"
        ref = ref_modattn(q, kv, desc.slot_row, gout, I // dh, dh, dh ** -0.5)
        ref2 = oracle_route(q, kv, gout, mask_all, B, M, P, N, I // dh, dh, dh ** -0.5)
        for a, b, nm in zip(ref, ref2, ("out", "dq", "dkv")):
            assert torch.allclose(a.cpu(), b, rtol=1e-12, atol=1e-12), "gather and oracle construction disagree: " + nm
        what = "M %d I %d dh %d" % (M, I, dh)
        check(T, got, ref2, torch.arange(desc.shared_base), torch.arange(desc.shared_base, nkv), what)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per_sample"])
def test_modattn_bench_shape(per_sample):
    """The flagship shape: B 256, P 256, N 384, M 3 (ns 4), I 512 (8 x 64), bf16, slot_row from the product's descriptors
    over masks_from_draws; nsplit 8.  Every row finite, backward bitwise deterministic, elementwise bf16 bound."""
    B, M, P, N, I, dh, T = 256, 3, 256, 384, 512, 64, torch.bfloat16
    gen = torch.Generator().manual_seed(31 + per_sample)
    mask_all, desc = product_descriptors(B, M, P, N, B if per_sample else 1, gen)
    assert_slot_contract(desc, mask_all, B, M, P, N)
    nkv = desc.shared_base + P
    q, kv, gout = rand_inputs(B * P, nkv, I, T, gen)
    o, dq, dkv, dq2, dkv2 = run_modattn(q, kv, desc.slot_row, gout, B, P, dh, desc.shared_base, backward_twice=True)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), "backward not bitwise deterministic"
    for t in (o, dq, dkv):
        assert bool(torch.isfinite(t).all())
    ref = ref_modattn(q, kv, desc.slot_row, gout, I // dh, dh, dh ** -0.5)
    check(T, (o, dq, dkv), ref, torch.arange(desc.shared_base), torch.arange(desc.shared_base, nkv), "bench shape")


def test_modattn_block_fusion_layout_shared_rows_zero():
    """Block_Fusion.forward's layout (zorro_utils.py): every slot a real row, P unnamed zero rows appended as the shared rows.
    The finish kernel must write those rows as exact zeros (the caller's dkv starts as NaN here)."""
    gen = torch.Generator().manual_seed(41)
    for T, I, ns, dh, B, n in ((torch.float32, 512, 4, 64, 40, 7), (torch.bfloat16, 192, 6, 32, 70, 5)):
        slot = torch.arange(B * n * ns, dtype=torch.int32).view(B * n, ns)
        nkv = B * n * ns + n
        q, kv, gout = rand_inputs(B * n, nkv, I, T, gen)
        kv[B * n * ns:] = 0
        o, dq, dkv = run_modattn(q, kv, slot, gout, B, n, dh, B * n * ns, (0, 0, 0, 0, 0, 8))
        assert bool((dkv[B * n * ns:] == 0).all()), "shared rows of the padded layout must be exactly 0"
        ref = ref_modattn(q, kv, slot, gout, I // dh, dh, dh ** -0.5)
        check(T, (o, dq, dkv), ref, torch.arange(B * n * ns), torch.arange(B * n * ns, nkv), "block fusion layout")


# ------------------------------------------------------------------------------------------------ 4. numerics
def logit_inputs(mode, B, P, ns, I, dh, T, gen):
    """q, kv whose per-head scores are set by column 0 of each head: q[.., 0] = 1, k[.., 0] = t / scale, the other columns
    small, so score(row, slot) = t[slot row, head] + O(0.05).  span: t ~ U(-100, 100); shift+100 / shift-100: t = +-100 + U(-4, 4)
    (fp32 exp overflows above ~88 and flushes below ~-87: a kernel that skipped the max subtraction returns inf / NaN);
    ties: q is zero outside column 0 and every kv row has the same column 0, so all ns scores of a row are bitwise equal
    (the other K columns differ, so dq = sum_s ds_s k_s is not identically 0)."""
    kept = kept_pattern("random", B, P, ns - 1, gen)
    slot, nkv, shared_base, _ = make_slots(kept, 0, gen)
    H, scale = I // dh, dh ** -0.5
    q = 0.05 * torch.randn(B * P, H, dh, generator=gen)
    q[..., 0] = 1.0
    kv = torch.randn(nkv, 2, H, dh, generator=gen)
    kv[:, 0] *= 0.05
    if mode == "span":
        t = 200 * torch.rand(nkv, H, generator=gen) - 100
    elif mode == "ties":
        q[..., 1:] = 0.0
        t = torch.full((nkv, H), 3.0)
    else:
        t = (100.0 if mode == "shift+100" else -100.0) + 8 * torch.rand(nkv, H, generator=gen) - 4
    kv[:, 0, :, 0] = t / scale
    q, kv = q.reshape(B * P, I).to(T), kv.reshape(nkv, 2 * I).to(T)
    gout = torch.randn(B * P, I, generator=gen).to(T)
    return q.to(DEV), kv.to(DEV), gout.to(DEV), slot, nkv, shared_base


@pytest.mark.parametrize("mode", ["span", "shift+100", "shift-100", "ties"])
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_modattn_extreme_logits(T, mode):
    """Scores spanning +-100, a uniform +-100 shift of every score of a row, exactly tied scores: fast (I 512, ns 4 / 5)
    and generic (I 576 ns 7, I 192 ns 3) forward and backward against fp64."""
    gen = torch.Generator().manual_seed(51)
    for I, ns, dh, B in ((512, 4, 64, 9), (512, 5, 32, 40), (576, 7, 64, 9), (192, 3, 32, 40)):
        P = 6
        q, kv, gout, slot, nkv, shared_base = logit_inputs(mode, B, P, ns, I, dh, T, gen)
        got = run_modattn(q, kv, slot, gout, B, P, dh, shared_base, (0, 8, 0, 0, 0, 8))
        ref = ref_modattn(q, kv, slot, gout, I // dh, dh, dh ** -0.5)
        what = "%s I %d ns %d dh %d" % (mode, I, ns, dh)
        check(T, got, ref, torch.arange(shared_base), torch.arange(shared_base, nkv), what)
        if mode == "ties":                                # equal weights: out = mean of the slots' V rows
            vmean = kv[slot.long().to(DEV)][..., I:].double().mean(1)
            close(got[0], vmean, TIGHT[T], what + " uniform weights")


# ------------------------------------------------------------------------------------------------ 5. the fast paths inside the model
def _seeded_backbone(seed):
    from incomplete_multimodal_fusion_amd.multimae import FusionInputAdapter, PatchedInputAdapter, TokenTypes
    from incomplete_multimodal_fusion_amd.multimae.multimae_big_imcomplete import ViTBaseline
    torch.manual_seed(seed)
    chans, size = (("s1", 1), ("s2", 3), ("dem", 1)), 128
    ia = {d: PatchedInputAdapter(num_channels=c, stride_level=1, patch_size_full=16, image_size=size) for d, c in chans}
    ia["fusion"] = FusionInputAdapter(num_channels=1, stride_level=1, patch_size_full=16, image_size=size)
    m = ViTBaseline(input_adapters=ia, output_adapters=None, num_fusion_tokens=(size // 16) ** 2,
                    return_token_types=(TokenTypes.S1, TokenTypes.S2, TokenTypes.DEM, TokenTypes.FUSION),
                    dim_tokens=768, depth=4, dim_head=64, heads=8, in_domains=[c[0] for c in chans], pretrained=None)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("gamma"):
                p.add_(0.1 * torch.randn_like(p))
        m.mask_embedding.add_(0.05 * torch.randn_like(m.mask_embedding))
    return m, chans, size


def _subset_seed(domains, k):
    """The first `random` seed whose forward_features draw (ViTBaseline: random.sample(in_domains, randint(1, 3))) has k
    modalities -> (seed, present in in_domains order)."""
    for seed in range(100):
        random.seed(seed)
        sub = random.sample(domains, random.randint(1, 3))
        if len(sub) == k:
            return seed, [d for d in domains if d in sub]
    raise AssertionError("no seed")


@pytest.mark.parametrize("k", [1, 2], ids=["one_modality", "two_modalities"])
def test_downstream_backbone_missing_modalities_fp32(k):
    """ViTBaseline (D 768, 8 x 64 heads, depth 4, 128 px, P 64) in training mode with a 1- or 2-modality subset: Block_Fusion
    runs modattn with ns = 2 / 3 at I = 512 -- the only product use of fast NS 2 and 3.  Taps and every parameter gradient
    against oracle.backbone_forward_features on the CPU (fp32: 1e-3, gradients 2e-3)."""
    from tests import parity
    model, chans, size = _seeded_backbone(60 + k)
    domains = [c[0] for c in chans]
    seed, present = _subset_seed(domains, k)
    gen = torch.Generator().manual_seed(70 + k)
    B, P = 2, (size // 16) ** 2
    x = {d: torch.randn(B, c, size, size, generator=gen) for d, c in chans}
    N = int(len(present) * P * 0.9)
    masks, left = {}, N
    for i, d in enumerate(present):
        keep = left if i == len(present) - 1 else min(P, N // len(present))
        left -= keep
        row = torch.ones(P, dtype=torch.long); row[torch.randperm(P, generator=gen)[:keep]] = 0
        masks[d] = row[None].repeat(B, 1)
    state = {k_: v.detach().clone() for k_, v in model.state_dict().items()}
    p = parity.leaf_params(state)
    ref = O.backbone_forward_features(p, {d: x[d] for d in present}, present, masks, N, 8)
    sum((o * o).mean() for o in ref).backward()
    model.to(DEV).train()
    model.zero_grad()
    random.seed(seed)
    outs, _, _ = model.forward_features({d: v.to(DEV) for d, v in x.items()}, task_masks={d: masks[d].to(DEV) for d in present})
    assert [d for d in model.in_domains if d in model.incomplete_domains] == present
    assert len(outs) == 4
    for i, (o, r) in enumerate(zip(outs, ref)):
        close(o, r, 1e-3, "tap%d" % i)
    sum((o * o).mean() for o in outs).backward()
    n = 0
    for name, prm in model.named_parameters():
        if name in p and p[name].grad is not None:
            assert prm.grad is not None, name
            close(prm.grad, p[name].grad, 2e-3, "grad " + name)
            n += 1
    assert n > 20 and p["mask_embedding"].grad is not None


def test_quad_small_fp32_step_fast_ns5():
    """One fp32 4-modality pretraining step at I = 512 (Small preset: D 384, 8 heads of 64): fast <float, 64, 5>, which the
    rest of the suite runs only in bf16 at B = 2.  Every output, loss and gradient against the oracle at the 1e-3 contract."""
    from tests.test_gpu_quad import _quad_step
    _quad_step("small", 64, 3, (7, 5, 0, 9), "fp32", "hardneg", 61, decoder_dim=64, decoder_depth=1, decoder_num_heads=2)
