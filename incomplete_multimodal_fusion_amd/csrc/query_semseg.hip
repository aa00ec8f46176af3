// Mask2Former semantic inference on the device (gfx950): bilinear resize of the query masks, sigmoid, softmax of the class logits
// and the query-mixing einsum in one kernel, with the argmax, the confusion matrix or the dice sums taken from its registers.
//
// Reference composition replaced (downstream/semantic_segmentation/maskformer_train_seg.py:258-274, 287-308; repeated in
// mask2former_infer_seg.py:185-259 and in instance_segmentation/maskformer_train_{seg,ins,ins_vit}.py, mask2former_infer{,2json}.py):
//   mask_pred = F.interpolate(pred_masks, size=(H, W), mode="bilinear", align_corners=False)       (B,Q,h,w) -> (B,Q,H,W)
//   semseg    = einsum("bqc,bqhw->bchw", softmax(pred_logits, -1)[..., 1:], mask_pred.sigmoid())   (B,K,H,W)
//   conf_mat.add_batch(target, semseg.cpu().max(1)[1] + 1)   |   _get_dice(semseg[0], onehot(target[0])[1:])
// which writes and re-reads the (B,Q,H,W) upsampled masks three times.  Here the low-resolution masks are read once per output
// tile and nothing of size (B,Q,H,W) exists.
//   query_kernel<KB, MODE>: 256 threads own one 16 x 16 output tile at a time, a contiguous range of tiles per workgroup.
//     - class weights: softmax over all K1 columns (precise expf, division), column void_index removed, (Q, KB) floats in LDS with
//       zero padding, recomputed only when the workgroup moves on to another sample;
//     - the tile's low-resolution footprint (6 x 6 per query at ratio 4) is staged through LDS in chunks of queries with scalar
//       loads (rows are not 16-byte aligned when w is odd), widened to fp32; a footprint above QS_FOOT_MAX values (ratios below
//       ~2.3: identity, downsampling), whose values would serve few taps each, is not staged: the four taps are read from global
//       memory, with no barrier in the query loop;
//     - per pixel and query: ATen's align_corners=False taps on the mask LOGITS (the source index as ONE fma,
//       fmaf(y + 0.5f, scale, -0.5f), where ATen multiplies and subtracts, and y0 clamped to h - 1; see qs_tap), sigmoid 1 / (1 + expf(-m)), then KB fma into
//       register accumulators, queries in ascending order.  VALU on purpose: bf16 MFMA would round the sigmoid and move argmax
//       decisions, and ~Q*K fma per pixel are far from mattering.
//     MODE 0 writes the scores and / or argmax + offset; MODE 1 counts (gt, pred) pairs in the LDS histogram of confhist.hpp;
//     MODE 2 reduces p*t, p, t per class over the tile in a fixed order (wave butterflies, then the four waves in order) into
//     the workspace.  All three run the same accumulation code: their scores agree bit for bit.
//   dice_finalize_kernel: one thread per (sample, class, sum) adds the tile partials in fp64 in tile order.  No float atomics.
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage; scratch 0 in all twelve instantiations), VGPRs MODE 0 / 1 / 2:
//   KB 8: 81 / 89 / 87    KB 16: 96 / 98 / 97    KB 32: 114 / 114 / 113    KB 64: 154 / 152 / 155    (5 / 4-5 / 4 / 3 waves per SIMD)
#include "common.hpp"
#include "confhist.hpp"
#include "mmae_hip.h"

#define QS_THREADS 256
#define QS_TILE 16
#define QS_STAGE 4096                                // floats of the footprint staging buffer (16 KB)
#define QS_FOOT_MAX 64                               // largest staged footprint per query: every staged value serves 16 taps or more,
                                                     // and a chunk holds 64 queries or more
#define QS_AHEAD 4                                   // queries whose taps are in flight ahead of the unstaged loop
#define QS_MAX_Q 256
#define QS_MAX_K 64
#define QS_MAX_KC 128
#define QS_MAX_GRID 1024                             // 4 workgroups per CU; more tiles than that: several per workgroup.  A counting
                                                     // workgroup ends with up to Kc*Kc same-address atomics (segmetrics.hip)

struct QsDesc {
    const void* logits; const void* masks; const long long* tgt;
    float* scores; long long* labels; long long* conf; float* ws;
    long long ignore_label;
    float sy, sx;
    int Q, K1, K, h, w, H, W, void_index, logit_bf16, mask_bf16, offset, Kc, ntx, tiles_per_sample, ntiles, per;
};

__device__ __forceinline__ float qs_ld(const void* p, long i, int is_bf16) {
    return is_bf16 ? (float)reinterpret_cast<const bf16*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// ATen's area_pixel_compute_source_index(scale, y, align_corners=false) and the two taps, with two differences: the index is one
// explicit fma, max(fmaf(y + 0.5f, scale, -0.5f), 0), not ATen's rounded product minus 0.5f (at most one rounding apart; equal at
// integer ratios) -- every caller rounds alike, whatever the compiler contracts, and the result is monotone in y, so the taps of a
// tile's pixels lie inside the taps of its first and last pixel; and i0 is clamped to n - 1, which the formula reaches only through
// rounding and where lam then weighs the same value twice.
__device__ __forceinline__ void qs_tap(int y, float scale, int n, int& i0, int& i1, float& lam) {
    const float src = fmaxf(fmaf((float)y + 0.5f, scale, -0.5f), 0.f);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    lam = src - (float)i0;
}

// softmax(pred_logits[b, q, :]) without column void_index -> wts[q*KB + j], j < K, zeros up to KB.  One thread per query.
template <int KB> __device__ __forceinline__ void qs_weights(const QsDesc& d, int b, float* wts) {
    for (int q = threadIdx.x; q < d.Q; q += QS_THREADS) {
        const long base = ((long)b * d.Q + q) * d.K1;
        float mx = qs_ld(d.logits, base, d.logit_bf16);
        for (int c = 1; c < d.K1; ++c) mx = fmaxf(mx, qs_ld(d.logits, base + c, d.logit_bf16));
        float sum = 0.f;
        for (int c = 0; c < d.K1; ++c) sum += expf(qs_ld(d.logits, base + c, d.logit_bf16) - mx);
        int j = 0;
        for (int c = 0; c < d.K1; ++c) {
            if (c == d.void_index) continue;
            wts[q * KB + j++] = expf(qs_ld(d.logits, base + c, d.logit_bf16) - mx) / sum;
        }
        for (; j < KB; ++j) wts[q * KB + j] = 0.f;
    }
}

template <int KB>
__device__ __forceinline__ void qs_mix(float (&acc)[KB], const float* wr, float m00, float m01, float m10, float m11, float ly,
                                       float lx) {
    const float m = (1.f - ly) * ((1.f - lx) * m00 + lx * m01) + ly * ((1.f - lx) * m10 + lx * m11);
    const float s = 1.f / (1.f + expf(-m));
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = fmaf(wr[k], s, acc[k]);
}

// The mask dtype is chosen outside the loops: a branch around every load would keep the loads of one trip from overlapping.
// Footprint of n / fsz queries, rows of fw values -> stage; m points at its first value.
template <typename TM>
__device__ __forceinline__ void qs_stage(float* stage, const TM* m, int n, int fsz, int fw, long plane, int w) {
    for (int i = threadIdx.x; i < n; i += QS_THREADS) {
        const int q = i / fsz, e = i - q * fsz, fy = e / fw, fx = e - fy * fw;
        stage[i] = (float)m[(long)q * plane + (long)fy * w + fx];
    }
}

// The unstaged query loop: the four taps of every query straight from global memory; m points at the sample's first mask.  The
// taps of the next QS_AHEAD queries are loaded before the current ones are used: without that the loop waits for every query's
// loads in turn.  Past the last query the loads repeat it (in bounds) and are not used.
template <int KB, typename TM>
__device__ __forceinline__ void qs_direct(float (&acc)[KB], const float* wts, const TM* m, long plane, int Q, long g00, long g01,
                                          long g10, long g11, float ly, float lx) {
    TM cur[QS_AHEAD][4], nxt[QS_AHEAD][4];
#pragma unroll
    for (int j = 0; j < QS_AHEAD; ++j) {
        const TM* p = m + (long)min(j, Q - 1) * plane;
        cur[j][0] = p[g00]; cur[j][1] = p[g01]; cur[j][2] = p[g10]; cur[j][3] = p[g11];
    }
    for (int q0 = 0; q0 < Q; q0 += QS_AHEAD) {
#pragma unroll
        for (int j = 0; j < QS_AHEAD; ++j) {
            const TM* p = m + (long)min(q0 + QS_AHEAD + j, Q - 1) * plane;
            nxt[j][0] = p[g00]; nxt[j][1] = p[g01]; nxt[j][2] = p[g10]; nxt[j][3] = p[g11];
        }
#pragma unroll
        for (int j = 0; j < QS_AHEAD; ++j)
            if (q0 + j < Q)
                qs_mix<KB>(acc, wts + (q0 + j) * KB, (float)cur[j][0], (float)cur[j][1], (float)cur[j][2], (float)cur[j][3], ly, lx);
#pragma unroll
        for (int j = 0; j < QS_AHEAD; ++j) {
            cur[j][0] = nxt[j][0]; cur[j][1] = nxt[j][1]; cur[j][2] = nxt[j][2]; cur[j][3] = nxt[j][3];
        }
    }
}

template <int KB, int MODE>
__global__ __launch_bounds__(QS_THREADS) void query_kernel(QsDesc d) {
    extern __shared__ float qs_lds[];
    float* wts = qs_lds;                                              // (Q, KB)
    float* stage = wts + d.Q * KB;                                    // QS_STAGE
    unsigned* hist = reinterpret_cast<unsigned*>(stage + QS_STAGE);   // MODE 1: (Kc, Kc)
    float* red = stage + QS_STAGE;                                    // MODE 2: (4 waves, KB, 3)
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int tx = tid & (QS_TILE - 1), ty = tid / QS_TILE;
    if (MODE == 1) sm_hist_clear<QS_THREADS>(hist, d.Kc);
    const int t_end = (int)min((long)(blockIdx.x + 1) * d.per, (long)d.ntiles);      // the product can pass 2^31 when ntiles is near it
    int cur_b = -1;
    for (int t = blockIdx.x * d.per; t < t_end; ++t) {               // block-uniform: every barrier below is reached by all
        const int b = t / d.tiles_per_sample, r = t - b * d.tiles_per_sample;
        const int tyi = r / d.ntx, txi = r - tyi * d.ntx;
        if (b != cur_b) {
            __syncthreads();                                          // the previous sample's readers are done
            qs_weights<KB>(d, b, wts);
            __syncthreads();
            cur_b = b;
        }
        const int Y = tyi * QS_TILE + ty, X = txi * QS_TILE + tx;
        const bool valid = Y < d.H && X < d.W;
        int y0, y1, x0, x1, fy0, fy1, fx0, fx1, u;
        float ly, lx, lu;
        qs_tap(min(Y, d.H - 1), d.sy, d.h, y0, y1, ly);               // a thread off the image repeats the edge pixel, unused
        qs_tap(min(X, d.W - 1), d.sx, d.w, x0, x1, lx);
        qs_tap(tyi * QS_TILE, d.sy, d.h, fy0, u, lu);                 // the footprint: rows [fy0, fy1] x columns [fx0, fx1]
        qs_tap(min(tyi * QS_TILE + QS_TILE - 1, d.H - 1), d.sy, d.h, u, fy1, lu);
        qs_tap(txi * QS_TILE, d.sx, d.w, fx0, u, lu);
        qs_tap(min(txi * QS_TILE + QS_TILE - 1, d.W - 1), d.sx, d.w, u, fx1, lu);
        const int fh = fy1 - fy0 + 1, fw = fx1 - fx0 + 1;
        const bool staged = fh <= QS_FOOT_MAX && fw <= QS_FOOT_MAX && fh * fw <= QS_FOOT_MAX;
        const long plane = (long)d.h * d.w, mbase = (long)b * d.Q * plane;
        float acc[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) acc[k] = 0.f;
        if (staged) {
            const int fsz = fh * fw, qc = min(d.Q, QS_STAGE / fsz);
            const int o00 = (y0 - fy0) * fw + (x0 - fx0), o01 = (y0 - fy0) * fw + (x1 - fx0);
            const int o10 = (y1 - fy0) * fw + (x0 - fx0), o11 = (y1 - fy0) * fw + (x1 - fx0);
            for (int q0 = 0; q0 < d.Q; q0 += qc) {
                const int n = min(qc, d.Q - q0);
                __syncthreads();                                      // the previous chunk's (or tile's) readers are done
                const long o = mbase + (long)q0 * plane + (long)fy0 * d.w + fx0;
                if (d.mask_bf16) qs_stage<bf16>(stage, reinterpret_cast<const bf16*>(d.masks) + o, n * fsz, fsz, fw, plane, d.w);
                else qs_stage<float>(stage, reinterpret_cast<const float*>(d.masks) + o, n * fsz, fsz, fw, plane, d.w);
                __syncthreads();
                for (int q = 0; q < n; ++q) {
                    const float* s = stage + q * fsz;
                    qs_mix<KB>(acc, wts + (q0 + q) * KB, s[o00], s[o01], s[o10], s[o11], ly, lx);
                }
            }
        } else {
            const long g00 = (long)y0 * d.w + x0, g01 = (long)y0 * d.w + x1, g10 = (long)y1 * d.w + x0, g11 = (long)y1 * d.w + x1;
            if (d.mask_bf16) qs_direct<KB, bf16>(acc, wts, reinterpret_cast<const bf16*>(d.masks) + mbase, plane, d.Q, g00, g01, g10, g11, ly, lx);
            else qs_direct<KB, float>(acc, wts, reinterpret_cast<const float*>(d.masks) + mbase, plane, d.Q, g00, g01, g10, g11, ly, lx);
        }
        // argmax over the K kept classes, the rule of argmax_confusion_kernel: lowest index among equal maxima, first NaN wins
        float best = acc[0];
        int idx = 0;
#pragma unroll
        for (int k = 1; k < KB; ++k) {
            const bool take = k < d.K && (acc[k] > best || (acc[k] != acc[k] && best == best));
            best = take ? acc[k] : best;
            idx = take ? k : idx;
        }
        const long pix = ((long)b * d.H + min(Y, d.H - 1)) * d.W + min(X, d.W - 1);
        if (MODE == 0) {
            if (valid) {
                if (d.scores) {
                    const long HW = (long)d.H * d.W;
                    float* sp = d.scores + (long)b * d.K * HW + (long)Y * d.W + X;
#pragma unroll
                    for (int k = 0; k < KB; ++k)
                        if (k < d.K) sp[(long)k * HW] = acc[k];
                }
                if (d.labels) d.labels[pix] = (long long)idx + d.offset;
            }
        } else if (MODE == 1) {
            const long long g = d.tgt[pix];
            sm_hist_add(hist, valid ? sm_bin(g, (long long)idx + d.offset, d.Kc, d.ignore_label) : -1, lane);
        } else {
            const long long c = d.tgt[pix] - d.offset;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k < d.K) {                                        // block-uniform
                    const float p = valid ? acc[k] : 0.f, tt = (valid && c == k) ? 1.f : 0.f;
                    const float s0 = wave_sum(p * tt), s1 = wave_sum(p), s2 = wave_sum(tt);
                    if (lane == 0) {
                        float* o = red + (wave * KB + k) * 3;
                        o[0] = s0; o[1] = s1; o[2] = s2;
                    }
                }
            }
            __syncthreads();
            if (tid < d.K * 3) {
                const int W3 = KB * 3;
                d.ws[(long)t * d.K * 3 + tid] = ((red[tid] + red[W3 + tid]) + red[2 * W3 + tid]) + red[3 * W3 + tid];
            }
            __syncthreads();                                          // red is rewritten by the next tile
        }
    }
    if (MODE == 1) sm_hist_flush<QS_THREADS>(hist, d.Kc, d.conf);
}

// sums[(b*K + k)*3 + j] = the tile partials of sample b in tile order, in fp64.
__global__ __launch_bounds__(QS_THREADS) void dice_finalize_kernel(int n, int K, int tiles_per_sample, const float* __restrict__ ws,
                                                                   double* __restrict__ sums) {
    const int i = blockIdx.x * QS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int b = i / (K * 3), e = i - b * (K * 3);
    const float* p = ws + (long)b * tiles_per_sample * K * 3 + e;
    double s = 0.0;
    for (int t = 0; t < tiles_per_sample; ++t) s += (double)p[(long)t * K * 3];
    sums[i] = s;
}

static bool qs_shape_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W < (1L << 31); }

// Validates the arguments the three entry points share and fills the descriptor; false: MMAE_ERR_ARG.
static bool qs_desc(QsDesc& d, int logit_dtype, int mask_dtype, int B, int Q, int K1, int h, int w, int H, int W,
                    const void* pred_logits, const void* pred_masks, int void_index) {
    if ((logit_dtype != MMAE_F32 && logit_dtype != MMAE_BF16) || (mask_dtype != MMAE_F32 && mask_dtype != MMAE_BF16)) return false;
    if (!qs_shape_ok(B, H, W) || h < 1 || w < 1 || (long)h * w >= (1L << 31)) return false;
    if (Q < 1 || Q > QS_MAX_Q || K1 < 1 || void_index < -1 || void_index >= K1) return false;
    const int K = K1 - (void_index >= 0 ? 1 : 0);
    if (K < 1 || K > QS_MAX_K || !pred_logits || !pred_masks) return false;
    d = QsDesc{};
    d.logits = pred_logits; d.masks = pred_masks;
    d.sy = (float)h / (float)H; d.sx = (float)w / (float)W;
    d.Q = Q; d.K1 = K1; d.K = K; d.h = h; d.w = w; d.H = H; d.W = W; d.void_index = void_index;
    d.logit_bf16 = logit_dtype == MMAE_BF16; d.mask_bf16 = mask_dtype == MMAE_BF16;
    d.ntx = cdiv(W, QS_TILE);
    d.tiles_per_sample = d.ntx * cdiv(H, QS_TILE);
    d.ntiles = B * d.tiles_per_sample;
    d.per = cdiv(d.ntiles, QS_MAX_GRID);
    return true;
}

template <int KB, int MODE> static int qs_launch_kb(const QsDesc& d, hipStream_t st) {
    const size_t lds = ((size_t)d.Q * KB + QS_STAGE + (MODE == 1 ? (size_t)d.Kc * d.Kc : MODE == 2 ? 4 * KB * 3 : 0)) * sizeof(float);
    // more than 64 KB of dynamic LDS (Q * KB and Kc near their limits) is a per-device opt-in of the function
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(query_kernel<KB, MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return MMAE_ERR_LAUNCH;
    MMAE_LAUNCH((query_kernel<KB, MODE>), dim3(cdiv(d.ntiles, d.per)), dim3(QS_THREADS), lds, st, d);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

// The accumulators live in registers: the class loop is unrolled to a compile-time bound.
template <int MODE> static int qs_launch(const QsDesc& d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d.K <= 8) return qs_launch_kb<8, MODE>(d, st);
    if (d.K <= 16) return qs_launch_kb<16, MODE>(d, st);
    if (d.K <= 32) return qs_launch_kb<32, MODE>(d, st);
    return qs_launch_kb<64, MODE>(d, st);
}

extern "C" int mmae_query_semseg(int logit_dtype, int mask_dtype, int B, int Q, int K1, int h, int w, int H, int W,
                                 const void* pred_logits, const void* pred_masks, int void_index, float* scores, long long* labels,
                                 int label_offset, void* stream) {
    QsDesc d;
    if (!qs_desc(d, logit_dtype, mask_dtype, B, Q, K1, h, w, H, W, pred_logits, pred_masks, void_index)) return MMAE_ERR_ARG;
    if (!scores && !labels) return MMAE_ERR_ARG;
    d.scores = scores; d.labels = labels; d.offset = label_offset;
    return qs_launch<0>(d, stream);
}

extern "C" int mmae_query_confusion(int logit_dtype, int mask_dtype, int B, int Q, int K1, int h, int w, int H, int W,
                                    const void* pred_logits, const void* pred_masks, int void_index, const long long* target, int Kc,
                                    int pred_offset, long ignore_label, long long* conf, void* stream) {
    QsDesc d;
    if (!qs_desc(d, logit_dtype, mask_dtype, B, Q, K1, h, w, H, W, pred_logits, pred_masks, void_index)) return MMAE_ERR_ARG;
    if (Kc < 1 || Kc > QS_MAX_KC || !target || !conf) return MMAE_ERR_ARG;
    d.tgt = target; d.conf = conf; d.Kc = Kc; d.offset = pred_offset; d.ignore_label = (long long)ignore_label;
    return qs_launch<1>(d, stream);
}

extern "C" long mmae_query_dice_ws_floats(int B, int K1, int H, int W) {
    if (!qs_shape_ok(B, H, W) || K1 < 1 || K1 > QS_MAX_K + 1) return MMAE_ERR_ARG;
    return (long)B * cdiv(H, QS_TILE) * cdiv(W, QS_TILE) * K1 * 3;
}

extern "C" int mmae_query_dice(int logit_dtype, int mask_dtype, int B, int Q, int K1, int h, int w, int H, int W,
                               const void* pred_logits, const void* pred_masks, int void_index, const long long* target,
                               int label_offset, float* ws, double* sums, void* stream) {
    QsDesc d;
    if (!qs_desc(d, logit_dtype, mask_dtype, B, Q, K1, h, w, H, W, pred_logits, pred_masks, void_index)) return MMAE_ERR_ARG;
    if (!target || !ws || !sums) return MMAE_ERR_ARG;
    d.tgt = target; d.ws = ws; d.offset = label_offset;
    const int rc = qs_launch<2>(d, stream);
    if (rc != MMAE_OK) return rc;
    const int n = B * d.K * 3;
    MMAE_LAUNCH(dice_finalize_kernel, dim3(cdiv(n, QS_THREADS)), dim3(QS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), n, d.K,
                d.tiles_per_sample, ws, sums);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}
