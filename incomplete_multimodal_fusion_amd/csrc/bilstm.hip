// Two-step bidirectional LSTM + attention pooling (gfx950): the BiLSTM fusion of the S2+DSM model.
//
// Reference arithmetic replaced (pretraining/multimae/multimae_lstm_s2dsm.py:428-434 with DSI-MM/zorro_utils.py:261-299): every
// pair (modality token x0, fusion row x1) is a length-2 sequence through nn.LSTM(D, D, bidirectional) (h0 = c0 = 0, gate order
// i, f, g, o), y_t = h_t^fwd + h_t^rev, s_t = w . tanh(y_t) + b, alpha = softmax(s_0, s_1), r = alpha_0 y_0 + alpha_1 y_1.
//
// The GEMMs stay outside (ops.bilstm2_attn_pool): G = [x0; x1] . [W_ih_fwd; W_ih_rev]^T is (2R, 8D) -- row j (x0) holds fwd@t0 in
// columns [0, 4D) and rev@t0 in [4D, 8D), row R + j (x1) fwd@t1 and rev@t1 -- and the recurrent products Hf = h_fwd@t0 . W_hh_fwd^T,
// Hr = h_rev@t1 . W_hh_rev^T are (R, 4D).  bsum (8D) fp32 = [b_ih + b_hh fwd | b_ih + b_hh rev].  Here:
//   cell1      step 1 of both directions (fwd@t0, rev@t1), c_prev = 0: c = i g, h = o tanh(c) -> h in the GEMM dtype, c / h fp32
//   cell2_pool step 2 (fwd@t1, rev@t0) and the attention pooling, one wave per row: r (R, D) fp32 and alpha (R, 2)
// and their backward kernels.  Cell math is fp32 in both dtypes; sigmoid / tanh saturate without inf or NaN.  The reductions
// over rows (dw, db of the pooling) go through per-wave partials in a fixed row -> wave map and a fixed-order second pass: no
// float atomics, bitwise reproducible.
#include "common.hpp"
#include "mmae_hip.h"

#define BL_THREADS 256
#define BL_WAVES_MAX 1024                    // waves of the pooling backward: its workspace is BL_WAVES_MAX * (D + 1) floats

__device__ __forceinline__ float bl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }   // expf(+1e4) = inf -> 0: no NaN

// One LSTM cell from the four pre-activations (i, f, g, o) and c_prev: gates, c, h.
struct Cell {
    float i, f, g, o, c, tc, h;
    __device__ __forceinline__ void run(float ai, float af, float ag, float ao, float c_prev) {
        i = bl_sigmoid(ai); f = bl_sigmoid(af); g = tanhf(ag); o = bl_sigmoid(ao);
        c = f * c_prev + i * g;
        tc = tanhf(c);
        h = o * tc;
    }
};

// pre-activation of gate q (0..3) at column k: G column block `col0` of row `row`, + bsum, (+ recurrent term)
template <typename T>
__device__ __forceinline__ float bl_pre(const T* G, long row, int D, int col0, int q, int k, const float* bsum) {
    return to_f(G[row * 8L * D + col0 + q * D + k]) + bsum[col0 + q * D + k];
}

// ---- step 1 -------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BL_THREADS) void bilstm_cell1_fwd_kernel(int R, int D, const T* __restrict__ G,
                                                                      const float* __restrict__ bsum, T* __restrict__ hf,
                                                                      T* __restrict__ hr, float* __restrict__ c1,
                                                                      float* __restrict__ h1) {
    const long e = (long)blockIdx.x * BL_THREADS + threadIdx.x, n = (long)R * D;
    if (e >= n) return;
    const long j = e / D;
    const int k = (int)(e - j * D);
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {                 // fwd@t0 (row j, cols [0,4D)), rev@t1 (row R+j, cols [4D,8D))
        const long row = dir ? R + j : j;
        const int col0 = dir * 4 * D;
        Cell s;
        s.run(bl_pre(G, row, D, col0, 0, k, bsum), bl_pre(G, row, D, col0, 1, k, bsum), bl_pre(G, row, D, col0, 2, k, bsum),
              bl_pre(G, row, D, col0, 3, k, bsum), 0.f);
        (dir ? hr : hf)[e] = from_f<T>(s.h);
        c1[dir * n + e] = s.c;
        h1[dir * n + e] = s.h;
    }
}

// dh = dh (GEMM path, T) + dh1 (pooling path, fp32); dc = dc1 + dh o (1 - tanh^2 c); gate gradients of step 1 into dG (the forget
// gate multiplies c_prev = 0: its gradient is exactly 0).
template <typename T>
__global__ __launch_bounds__(BL_THREADS) void bilstm_cell1_bwd_kernel(int R, int D, const T* __restrict__ G,
                                                                      const float* __restrict__ bsum, const T* __restrict__ dhf,
                                                                      const T* __restrict__ dhr, const float* __restrict__ dc1,
                                                                      const float* __restrict__ dh1, T* __restrict__ dG) {
    const long e = (long)blockIdx.x * BL_THREADS + threadIdx.x, n = (long)R * D;
    if (e >= n) return;
    const long j = e / D;
    const int k = (int)(e - j * D);
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const long row = dir ? R + j : j;
        const int col0 = dir * 4 * D;
        Cell s;
        s.run(bl_pre(G, row, D, col0, 0, k, bsum), 0.f, bl_pre(G, row, D, col0, 2, k, bsum),
              bl_pre(G, row, D, col0, 3, k, bsum), 0.f);
        const float dh = to_f((dir ? dhr : dhf)[e]) + dh1[dir * n + e];
        const float dc = dc1[dir * n + e] + dh * s.o * (1.f - s.tc * s.tc);
        T* d = dG + row * 8L * D + col0 + k;
        d[0] = from_f<T>(dc * s.g * s.i * (1.f - s.i));
        d[D] = from_f<T>(0.f);
        d[2 * D] = from_f<T>(dc * s.i * (1.f - s.g * s.g));
        d[3 * D] = from_f<T>(dh * s.tc * s.o * (1.f - s.o));
    }
}

// ---- step 2 + attention pooling: one wave per row, NPL columns per lane (k = lane + 64 q) ---------------------------------------
template <typename T>
struct Step2 {
    const T* G; const T* Hf; const T* Hr; const float* bsum; const float* c1; const float* h1;
    int R, D;
    // step-2 cell of direction dir at row j, column k: fwd@t1 (G row R+j, cols [0,4D), + Hf), rev@t0 (G row j, cols [4D,8D), + Hr)
    __device__ __forceinline__ void cell(Cell& s, int dir, long j, int k) const {
        const long row = dir ? j : R + j;
        const int col0 = dir * 4 * D;
        const T* H = (dir ? Hr : Hf) + j * 4L * D + k;
        s.run(bl_pre(G, row, D, col0, 0, k, bsum) + to_f(H[0]), bl_pre(G, row, D, col0, 1, k, bsum) + to_f(H[D]),
              bl_pre(G, row, D, col0, 2, k, bsum) + to_f(H[2 * D]), bl_pre(G, row, D, col0, 3, k, bsum) + to_f(H[3 * D]),
              c1[(long)dir * R * D + j * D + k]);
    }
};

template <typename T, int NPL>
__global__ __launch_bounds__(BL_THREADS) void bilstm_cell2_pool_fwd_kernel(Step2<T> a, const float* __restrict__ w,
                                                                           const float* __restrict__ b, float* __restrict__ r,
                                                                           float* __restrict__ alpha) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long j = (long)blockIdx.x * (BL_THREADS / WAVE) + threadIdx.x / WAVE;
    if (j >= a.R) return;                                // wave-uniform
    const int D = a.D;
    const long n = (long)a.R * D;
    float y0[NPL], y1[NPL], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int k = lane + q * WAVE;
        y0[q] = y1[q] = 0.f;
        if (k < D) {
            Cell f, v;
            a.cell(f, 0, j, k);                          // h_fwd@t1
            a.cell(v, 1, j, k);                          // h_rev@t0
            y0[q] = a.h1[j * D + k] + v.h;               // h_fwd@t0 + h_rev@t0
            y1[q] = f.h + a.h1[n + j * D + k];           // h_fwd@t1 + h_rev@t1
            s0 += w[k] * tanhf(y0[q]);
            s1 += w[k] * tanhf(y1[q]);
        }
    }
    s0 = wave_sum(s0) + b[0];
    s1 = wave_sum(s1) + b[0];
    const float m = fmaxf(s0, s1), e0 = expf(s0 - m), e1 = expf(s1 - m);
    const float a0 = e0 / (e0 + e1), a1 = e1 / (e0 + e1);
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int k = lane + q * WAVE;
        if (k < D) r[j * D + k] = a0 * y0[q] + a1 * y1[q];
    }
    if (lane == 0) { alpha[2 * j] = a0; alpha[2 * j + 1] = a1; }
}

// Backward of the above.  Per row: d alpha_t = dr . y_t, ds_t = alpha_t (d alpha_t - sum alpha d alpha),
// dy_t = alpha_t dr + ds_t w (1 - tanh^2 y_t); dw += sum_t ds_t tanh(y_t), db += ds_0 + ds_1 (per-wave partials in ws);
// y_0 = h_fwd@t0 + h_rev@t0 and y_1 = h_fwd@t1 + h_rev@t1 hand dy to the step-1 outputs (dh1) and to the step-2 cells, whose gate
// gradients go to dG (and, identical, to dHf / dHr: the recurrent GEMMs' outputs) and whose c_prev gradient goes to dc1.
template <typename T, int NPL>
__global__ __launch_bounds__(BL_THREADS) void bilstm_cell2_pool_bwd_kernel(Step2<T> a, const float* __restrict__ w,
                                                                           const float* __restrict__ alpha,
                                                                           const float* __restrict__ dr, T* __restrict__ dG,
                                                                           T* __restrict__ dHf, T* __restrict__ dHr,
                                                                           float* __restrict__ dc1, float* __restrict__ dh1,
                                                                           float* __restrict__ ws) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int gw = blockIdx.x * (BL_THREADS / WAVE) + threadIdx.x / WAVE, nw = gridDim.x * (BL_THREADS / WAVE);
    const int D = a.D;
    const long n = (long)a.R * D;
    float dw[NPL], db = 0.f;
#pragma unroll
    for (int q = 0; q < NPL; ++q) dw[q] = 0.f;
    for (long j = gw; j < a.R; j += nw) {                // fixed row -> wave map: the partials do not depend on timing
        const float a0 = alpha[2 * j], a1 = alpha[2 * j + 1];
        float y0[NPL], y1[NPL], g[NPL], p0 = 0.f, p1 = 0.f;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int k = lane + q * WAVE;
            y0[q] = y1[q] = g[q] = 0.f;
            if (k < D) {
                Cell f, v;
                a.cell(f, 0, j, k);
                a.cell(v, 1, j, k);
                y0[q] = a.h1[j * D + k] + v.h;
                y1[q] = f.h + a.h1[n + j * D + k];
                g[q] = dr[j * D + k];
                p0 += g[q] * y0[q];
                p1 += g[q] * y1[q];
            }
        }
        p0 = wave_sum(p0);
        p1 = wave_sum(p1);
        const float dot = a0 * p0 + a1 * p1;
        const float ds0 = a0 * (p0 - dot), ds1 = a1 * (p1 - dot);
        db += ds0 + ds1;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int k = lane + q * WAVE;
            if (k >= D) continue;
            const float t0 = tanhf(y0[q]), t1 = tanhf(y1[q]);
            dw[q] += ds0 * t0 + ds1 * t1;
            const float dy0 = a0 * g[q] + ds0 * w[k] * (1.f - t0 * t0);
            const float dy1 = a1 * g[q] + ds1 * w[k] * (1.f - t1 * t1);
            dh1[j * D + k] = dy0;                        // into h_fwd@t0
            dh1[n + j * D + k] = dy1;                    // into h_rev@t1
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {          // fwd@t1 takes dy1, rev@t0 takes dy0
                Cell s;
                a.cell(s, dir, j, k);
                const float dh = dir ? dy0 : dy1;
                const float cp = a.c1[dir * n + j * D + k];
                const float dc = dh * s.o * (1.f - s.tc * s.tc);
                const float gi = dc * s.g * s.i * (1.f - s.i);
                const float gf = dc * cp * s.f * (1.f - s.f);
                const float gg = dc * s.i * (1.f - s.g * s.g);
                const float go = dh * s.tc * s.o * (1.f - s.o);
                dc1[dir * n + j * D + k] = dc * s.f;
                const long row = dir ? j : a.R + j;
                T* d = dG + row * 8L * D + dir * 4 * D + k;
                T* h = (dir ? dHr : dHf) + j * 4L * D + k;
                d[0] = h[0] = from_f<T>(gi);
                d[D] = h[D] = from_f<T>(gf);
                d[2 * D] = h[2 * D] = from_f<T>(gg);
                d[3 * D] = h[3 * D] = from_f<T>(go);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int k = lane + q * WAVE;
        if (k < D) ws[(long)gw * (D + 1) + k] = dw[q];
    }
    if (lane == 0) ws[(long)gw * (D + 1) + D] = db;
}

// dw[k] = sum over waves of ws[wave][k] in wave order, db = the same for column D
__global__ __launch_bounds__(BL_THREADS) void bilstm_pool_reduce_kernel(int nw, int D, const float* __restrict__ ws,
                                                                        float* __restrict__ dw, float* __restrict__ db) {
    for (int k = blockIdx.x * BL_THREADS + threadIdx.x; k <= D; k += gridDim.x * BL_THREADS) {
        float s = 0.f;
        for (int i = 0; i < nw; ++i) s += ws[(long)i * (D + 1) + k];
        if (k < D) dw[k] = s;
        else db[0] = s;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static inline bool bl_al(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool bl_args(int dtype, int R, int D) {
    return (dtype == MMAE_F32 || dtype == MMAE_BF16) && R > 0 && D >= 32 && D <= 1024 && D % 32 == 0;
}
static inline int bl_npl(int D) { return D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : D <= 512 ? 8 : D <= 768 ? 12 : 16; }

extern "C" int mmae_bilstm_cell1_fwd(int dtype, int R, int D, const void* G, const float* bsum, void* hf, void* hr, float* c1,
                                     float* h1, void* stream) {
    if (!bl_args(dtype, R, D) || !bl_al(G) || !bl_al(bsum) || !bl_al(hf) || !bl_al(hr) || !bl_al(c1) || !bl_al(h1)) return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(cdiv((long)R * D, BL_THREADS));
    if (dtype == MMAE_BF16)
        MMAE_LAUNCH(bilstm_cell1_fwd_kernel<bf16>, grid, dim3(BL_THREADS), 0, st, R, D, (const bf16*)G, bsum, (bf16*)hf, (bf16*)hr, c1, h1);
    else
        MMAE_LAUNCH(bilstm_cell1_fwd_kernel<float>, grid, dim3(BL_THREADS), 0, st, R, D, (const float*)G, bsum, (float*)hf, (float*)hr, c1, h1);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

extern "C" int mmae_bilstm_cell1_bwd(int dtype, int R, int D, const void* G, const float* bsum, const void* dhf, const void* dhr,
                                     const float* dc1, const float* dh1, void* dG, void* stream) {
    if (!bl_args(dtype, R, D) || !bl_al(G) || !bl_al(bsum) || !bl_al(dhf) || !bl_al(dhr) || !bl_al(dc1) || !bl_al(dh1) || !bl_al(dG))
        return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(cdiv((long)R * D, BL_THREADS));
    if (dtype == MMAE_BF16)
        MMAE_LAUNCH(bilstm_cell1_bwd_kernel<bf16>, grid, dim3(BL_THREADS), 0, st, R, D, (const bf16*)G, bsum, (const bf16*)dhf,
                    (const bf16*)dhr, dc1, dh1, (bf16*)dG);
    else
        MMAE_LAUNCH(bilstm_cell1_bwd_kernel<float>, grid, dim3(BL_THREADS), 0, st, R, D, (const float*)G, bsum, (const float*)dhf,
                    (const float*)dhr, dc1, dh1, (float*)dG);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

template <typename T>
static int bl_pool_fwd(int npl, dim3 grid, hipStream_t st, Step2<T> a, const float* w, const float* b, float* r, float* alpha) {
#define BL_FWD(N) MMAE_LAUNCH((bilstm_cell2_pool_fwd_kernel<T, N>), grid, dim3(BL_THREADS), 0, st, a, w, b, r, alpha)
    switch (npl) {
        case 1: BL_FWD(1); break;
        case 2: BL_FWD(2); break;
        case 4: BL_FWD(4); break;
        case 8: BL_FWD(8); break;
        case 12: BL_FWD(12); break;
        default: BL_FWD(16); break;
    }
#undef BL_FWD
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

template <typename T>
static int bl_pool_bwd(int npl, dim3 grid, hipStream_t st, Step2<T> a, const float* w, const float* alpha, const float* dr,
                       void* dG, void* dHf, void* dHr, float* dc1, float* dh1, float* ws) {
#define BL_BWD(N) MMAE_LAUNCH((bilstm_cell2_pool_bwd_kernel<T, N>), grid, dim3(BL_THREADS), 0, st, a, w, alpha, dr, (T*)dG, (T*)dHf, \
                              (T*)dHr, dc1, dh1, ws)
    switch (npl) {
        case 1: BL_BWD(1); break;
        case 2: BL_BWD(2); break;
        case 4: BL_BWD(4); break;
        case 8: BL_BWD(8); break;
        case 12: BL_BWD(12); break;
        default: BL_BWD(16); break;
    }
#undef BL_BWD
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

extern "C" int mmae_bilstm_cell2_pool_fwd(int dtype, int R, int D, const void* G, const void* Hf, const void* Hr, const float* bsum,
                                          const float* c1, const float* h1, const float* w, const float* b, float* r, float* alpha,
                                          void* stream) {
    if (!bl_args(dtype, R, D) || !bl_al(G) || !bl_al(Hf) || !bl_al(Hr) || !bl_al(bsum) || !bl_al(c1) || !bl_al(h1) || !bl_al(w) ||
        !b || !bl_al(r) || !bl_al(alpha))
        return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(cdiv(R, BL_THREADS / WAVE));
    const int npl = bl_npl(D);
    if (dtype == MMAE_BF16)
        return bl_pool_fwd<bf16>(npl, grid, st, Step2<bf16>{(const bf16*)G, (const bf16*)Hf, (const bf16*)Hr, bsum, c1, h1, R, D}, w, b,
                                 r, alpha);
    return bl_pool_fwd<float>(npl, grid, st, Step2<float>{(const float*)G, (const float*)Hf, (const float*)Hr, bsum, c1, h1, R, D}, w,
                              b, r, alpha);
}

extern "C" int mmae_bilstm_cell2_pool_bwd(int dtype, int R, int D, const void* G, const void* Hf, const void* Hr, const float* bsum,
                                          const float* c1, const float* h1, const float* w, const float* alpha, const float* dr,
                                          void* dG, void* dHf, void* dHr, float* dc1, float* dh1, float* ws, float* dw, float* db,
                                          void* stream) {
    if (!bl_args(dtype, R, D) || !bl_al(G) || !bl_al(Hf) || !bl_al(Hr) || !bl_al(bsum) || !bl_al(c1) || !bl_al(h1) || !bl_al(w) ||
        !bl_al(alpha) || !bl_al(dr) || !bl_al(dG) || !bl_al(dHf) || !bl_al(dHr) || !bl_al(dc1) || !bl_al(dh1) || !bl_al(ws) ||
        !bl_al(dw) || !db)
        return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // rows per wave ~ R / 1024 at large R; the row -> wave map depends on R only (fixed-order partial sums)
    const int nblk = cdiv(R, BL_THREADS / WAVE) < BL_WAVES_MAX / (BL_THREADS / WAVE) ? cdiv(R, BL_THREADS / WAVE)
                                                                                      : BL_WAVES_MAX / (BL_THREADS / WAVE);
    const int npl = bl_npl(D);
    int rc;
    if (dtype == MMAE_BF16)
        rc = bl_pool_bwd<bf16>(npl, dim3(nblk), st, Step2<bf16>{(const bf16*)G, (const bf16*)Hf, (const bf16*)Hr, bsum, c1, h1, R, D},
                               w, alpha, dr, dG, dHf, dHr, dc1, dh1, ws);
    else
        rc = bl_pool_bwd<float>(npl, dim3(nblk), st, Step2<float>{(const float*)G, (const float*)Hf, (const float*)Hr, bsum, c1, h1, R,
                                D}, w, alpha, dr, dG, dHf, dHr, dc1, dh1, ws);
    if (rc != MMAE_OK) return rc;
    MMAE_LAUNCH(bilstm_pool_reduce_kernel, dim3(cdiv(D + 1, BL_THREADS)), dim3(BL_THREADS), 0, st, nblk * (BL_THREADS / WAVE), D, ws, dw,
                db);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}
