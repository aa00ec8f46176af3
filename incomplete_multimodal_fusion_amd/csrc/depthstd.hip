// Truncated depth standardisation (gfx950): the `--standardize_depth` switch of the reference trainer.
//
// Reference arithmetic replaced (pretraining/pretrain_mmae.py:452-458; pretrain_mmae_my.py:468-474), per sample b of the DSM:
//   s = sort(x[b].flatten()) ; s = s[int(0.1 n) : int(0.9 n)] ; y[b] = (x[b] - mean(s)) / sqrt(var(s, correction 1) + 1e-6)
// without sorting.  One 1024-thread workgroup per sample:
//   1. the two order statistics t_lo = key at rank k_lo and t_hi = key at rank k_hi - 1 by a 4 x 8-bit MSB radix select over
//      order-preserving uint32 keys (NaN canonicalised to +NaN first: it ranks above +inf, where torch.sort puts it), with
//      per-wave private LDS histograms;
//   2. the slice's sum relative to the pivot x(t_lo): every value strictly between the two keys counts once, the copies of t_lo /
//      t_hi count as many times as they fill slots of the slice (which copies a sort puts there does not change the sum; -0.0 and
//      +0.0 may rank either way, both add 0);
//   3. the unbiased variance as a second pass over the same weighted selection, then y = ((x - pivot) - d) / sqrtf(var + eps),
//      d = mean - pivot, in correctly rounded fp32 division / square root.
// Every reduction is a fixed-order tree (no float atomics): bitwise reproducible.  n <= 64 Ki (the 256 x 256 tile): the sample
// lives in VGPRs, one HBM read and one write; larger n re-reads the sample from L2 / MALL in every pass.
#include "common.hpp"
#include "mmae_hip.h"

#define DS_THREADS 1024
#define DS_WAVES (DS_THREADS / WAVE)
#define DS_ITEMS 64                                  // register-resident path: n <= DS_THREADS * DS_ITEMS
#define DS_BINS 256

__device__ __forceinline__ unsigned ds_key(float x) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0x7fc00000u;                     // every NaN -> +NaN: above +inf
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ds_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// One histogram increment per active lane (slot < 0: none).  The lanes sharing the first lane's slot are added by ONE atomic: DSM
// values are concentrated, so in the top digits most of a wave falls into one or two bins; the others add 1 each.
__device__ __forceinline__ void ds_hist_add(unsigned* h, int slot, int lane) {
    const unsigned long long act = __ballot(slot >= 0);
    if (act == 0) return;
    const int leader = __builtin_ctzll(act);
    const int s0 = __builtin_amdgcn_readlane(slot, leader);
    const unsigned long long same = __ballot(slot == s0);
    if (lane == leader) atomicAdd(h + s0, (unsigned)__popcll(same));
    else if (slot >= 0 && slot != s0) atomicAdd(h + slot, 1u);
}

// fixed-order block sum: wave butterfly, lane 0's value per wave, the 16 wave sums in wave order (the same value in every thread)
__device__ __forceinline__ float ds_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < DS_WAVES; ++i) t += red[i];
    return t;
}

template <bool REG>
__global__ __launch_bounds__(DS_THREADS) void trunc_std_kernel(long n, unsigned k_lo, unsigned k_hi, float eps,
                                                               const float* __restrict__ x, float* __restrict__ y,
                                                               float* __restrict__ mean_out, float* __restrict__ std_out) {
    __shared__ unsigned hist[DS_WAVES * 2 * DS_BINS];   // per wave: [target 0 | target 1] x 256 bins (32 KB)
    __shared__ unsigned tot[2 * DS_BINS];
    __shared__ unsigned sel[2][3];                      // per target: digit, residual rank, count of the digit's bin
    __shared__ float red[DS_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const float* xs = x + (long)blockIdx.x * n;
    float* ys = y + (long)blockIdx.x * n;

    // keys, 0 = no element (no float maps to 0: it would be a NaN, and every NaN was canonicalised)
    unsigned v[REG ? DS_ITEMS : 1];
    if (REG) {
        // clamped addresses, no branches: all 64 loads are in flight at once
        const int last = (int)n - 1;
        float t[DS_ITEMS];
#pragma unroll
        for (int j = 0; j < DS_ITEMS; ++j) t[j] = xs[min(j * DS_THREADS + tid, last)];
#pragma unroll
        for (int j = 0; j < DS_ITEMS; ++j) v[j] = j * DS_THREADS + tid <= last ? ds_key(t[j]) : 0u;
    }
    // f(key, index) over the sample; wave-uniform control flow (ds_hist_add ballots inside it)
    auto visit = [&](auto&& f) {
        if (REG) {
            // the keys as the compiler sees them change between visits: nothing derived from them (compare masks, decoded values)
            // is kept alive from one pass to the next -- 64 of those do not fit beside the keys
#pragma unroll
            for (int j = 0; j < DS_ITEMS; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
            for (int j = 0; j < DS_ITEMS; ++j) f(v[j], j * DS_THREADS + tid);
        } else {
            for (long base = 0; base < n; base += DS_THREADS) {
                const long i = base + tid;
                f(i < n ? ds_key(xs[i]) : 0u, i);
            }
        }
    };

    // ---- 1. radix select of the keys at ranks k_lo and k_hi - 1 (target 0 / 1) ----
    // The visited slots past n carry key 0, below every real key: they are counted like values and skipped by the ranks.
    const unsigned pad = (unsigned)((REG ? (long)DS_THREADS * DS_ITEMS : (n + DS_THREADS - 1) / DS_THREADS * DS_THREADS) - n);
    unsigned pre0 = 0, pre1 = 0, r0 = k_lo + pad, r1 = k_hi - 1 + pad, c0 = 0;
    unsigned* hw = hist + wave * 2 * DS_BINS;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass == 0 ? 0u : ~0u << (shift + 8);
        const bool same = pre0 == pre1;                 // one shared prefix: histogram 0 serves both targets
        for (int i = tid; i < DS_WAVES * 2 * DS_BINS; i += DS_THREADS) hist[i] = 0;
        __syncthreads();
        visit([&](unsigned k, long) {
            const unsigned hk = k & himask;
            const int d = (int)((k >> shift) & (DS_BINS - 1));
            const int slot = hk == pre0 ? d : (!same && hk == pre1 ? DS_BINS + d : -1);
            ds_hist_add(hw, slot, lane);
        });
        __syncthreads();
        if (tid < 2 * DS_BINS) {
            unsigned s = 0;
            for (int w = 0; w < DS_WAVES; ++w) s += hist[w * 2 * DS_BINS + tid];
            tot[tid] = s;
        }
        __syncthreads();
        if (wave < 2) {                                  // wave t finds the bin holding target t's residual rank
            const unsigned* t = tot + (same ? 0 : wave * DS_BINS);
            const unsigned r = wave ? r1 : r0;
            unsigned c[4], loc = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = t[lane * 4 + q]; loc += c[q]; }
            unsigned inc = loc;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const unsigned u = __shfl_up(inc, o);
                if (lane >= o) inc += u;
            }
            unsigned before = inc - loc;
            if (before <= r && r < inc) {                // exactly one lane: r < number of keys under the prefix
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (r < before + c[q]) {
                        sel[wave][0] = lane * 4 + q; sel[wave][1] = r - before; sel[wave][2] = c[q];
                        break;
                    }
                    before += c[q];
                }
            }
        }
        __syncthreads();
        pre0 |= sel[0][0] << shift; r0 = sel[0][1]; c0 = sel[0][2];
        pre1 |= sel[1][0] << shift; r1 = sel[1][1];
    }
    // t_lo = pre0 fills w_lo = c0 - r0 slots of the slice, t_hi = pre1 fills w_hi = r1 + 1 (the whole slice when they are equal)
    const bool one = pre0 == pre1;
    const float L = (float)(k_hi - k_lo);
    const float xlo = ds_val(pre0), xhi = ds_val(pre1);
    const float piv = isfinite(xlo) ? xlo : 0.f;
    const float wlo = (float)(c0 - r0), whi = (float)(r1 + 1);

    // ---- 2. mean relative to the pivot ----
    float s = 0.f;
    visit([&](unsigned k, long) {                        // (key 0 is below every pre0)
        if (k > pre0 && k < pre1) s += ds_val(k) - piv;
    });
    s = ds_block_sum(s, red);
    const float S = one ? L * (xlo - piv) : s + wlo * (xlo - piv) + whi * (xhi - piv);
    const float d = S / L;                               // mean - pivot

    // ---- 3. unbiased variance over the same selection, then normalise ----
    float q = 0.f;
    visit([&](unsigned k, long) {
        if (k > pre0 && k < pre1) { const float e = (ds_val(k) - piv) - d; q += e * e; }
    });
    q = ds_block_sum(q, red);
    const float elo = (xlo - piv) - d, ehi = (xhi - piv) - d;
    const float Q = one ? L * (elo * elo) : q + wlo * (elo * elo) + whi * (ehi * ehi);
    const float sd = sqrtf(Q / (L - 1.f) + eps);
    visit([&](unsigned k, long i) {
        if (k != 0) ys[i] = ((ds_val(k) - piv) - d) / sd;
    });
    if (tid == 0) {
        if (mean_out) mean_out[blockIdx.x] = piv + d;
        if (std_out) std_out[blockIdx.x] = sd;
    }
}

extern "C" int mmae_trunc_standardize(int B, long n, long k_lo, long k_hi, float eps, const float* x, float* y, float* mean,
                                      float* stdv, void* stream) {
    if (!x || !y || B < 1 || n > 0x7fffffffL || k_lo < 0 || k_hi > n || k_hi - k_lo < 2) return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n <= (long)DS_THREADS * DS_ITEMS)
        MMAE_LAUNCH(trunc_std_kernel<true>, dim3(B), dim3(DS_THREADS), 0, st, n, (unsigned)k_lo, (unsigned)k_hi, eps, x, y, mean, stdv);
    else
        MMAE_LAUNCH(trunc_std_kernel<false>, dim3(B), dim3(DS_THREADS), 0, st, n, (unsigned)k_lo, (unsigned)k_hi, eps, x, y, mean, stdv);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}
