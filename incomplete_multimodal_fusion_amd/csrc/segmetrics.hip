// Segmentation metrics on the device (gfx950): fused argmax + confusion matrix, and the scores read off it.
//
// Reference compositions replaced (downstream/semantic_segmentation/utils/metrics.py:7-86, driven from
// maskformer_train_seg.py:243-281; the pretraining side takes preds['dnw'].argmax(1), pretraining/infer_mmae_my.py:256):
//   pred.argmax(1) -> .cpu().numpy() -> per 64x64 image: pred[gt != 0], gt[gt != 0] -> sklearn confusion_matrix(labels=arange(K))
//   -> state += ; get_aa / get_sa / get_IoU / get_mIoU from the float64 state.
// Here the logits are read once, in the image form or in the decoder's token-major form (the two forms of the masked losses,
// imageops.hip), the target once; no argmax map, no compaction, no host copy.
//   argmax_confusion_kernel: one wave per (sample, patch) row, lanes cover 4 consecutive pixels each and keep a running
//     (max, index) per pixel over the classes; the (gt, pred) pairs go into a per-workgroup K x K uint32 histogram in LDS;
//     workgroups walk the rows with a grid-stride loop over a bounded grid and add their non-zero bins to the int64 matrix
//     once, at the end.  Integer adds commute: the counts are exact and do not depend on scheduling.
//   label_confusion_kernel: the same histogram over two flat label arrays (ConfMatrix.add_batch: argmax taken elsewhere).
//   confusion_scores_kernel: one workgroup; integer row / column sums, one fp64 division per score.
// A launch counts fewer than 2^31 pixels, so a 32-bit LDS bin cannot wrap.
#include "common.hpp"
#include "confhist.hpp"
#include "mmae_hip.h"

#define SM_THREADS 1024                              // 16 waves share one LDS histogram: few workgroups, few flushes
#define SM_WAVES (SM_THREADS / WAVE)
#define SM_MAX_K 128
#define SM_MAX_GRID 512                              // 2 workgroups per CU (8 waves per SIMD); more rows than that: the grid-stride loop.
                                                     // Every workgroup ends with up to K*K same-address global atomics, which serialise
                                                     // in L2 (~9 ns each): 2048 workgroups of 256 threads measured 18 us slower

typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <typename T> __device__ __forceinline__ f32x4 sm_ld4(const T* p);
template <> __device__ __forceinline__ f32x4 sm_ld4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 sm_ld4<bf16>(const bf16* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

struct ArgmaxDesc {
    const void* pred; const long long* tgt; const long long* mask; long long* conf;
    long rows; int P, C, H, W, ps, K, pred_offset; long long ignore_label;
};

// torch.argmax's rule on the CPU: the lowest index among equal maxima; a NaN beats every number and the first NaN wins; a row of
// all -inf gives 0 (the running best starts at class 0 and is replaced only by a strictly greater value or by the first NaN).
template <typename T, bool TOKENS>
__global__ __launch_bounds__(SM_THREADS) void argmax_confusion_kernel(ArgmaxDesc d) {
    extern __shared__ unsigned sm_hist[];
    sm_hist_clear<SM_THREADS>(sm_hist, d.K);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int ps2 = d.ps * d.ps, nw = d.W / d.ps;
    const long HW = (long)d.H * d.W;
    const int y0 = (4 * lane) / d.ps, x0 = (4 * lane) % d.ps;         // the first trip's pixel: the same in every row
    // rows = B*P <= B*H*W / 16 < 2^27: 32-bit row arithmetic (a 64-bit division costs more than a row's compares)
    for (int r = blockIdx.x * SM_WAVES + wave; r < (int)d.rows; r += gridDim.x * SM_WAVES) {
        if (d.mask && d.mask[r] == 0) continue;                       // wave-uniform: one row per wave
        const int b = r / d.P, patch = r - b * d.P;
        const int pr = patch / nw, py = pr * d.ps, px = (patch - pr * nw) * d.ps;
        for (int base = 0; base < ps2; base += 4 * WAVE) {            // wave-uniform trip count (sm_hist_add ballots)
            const int pix = base + 4 * lane;
            const bool on = pix < ps2;
            int idx[4] = {0, 0, 0, 0};
            long long g[4] = {0, 0, 0, 0};
            if (on) {
                const int y = base ? pix / d.ps : y0, x = base ? pix - (pix / d.ps) * d.ps : x0;
                const long io = (long)(py + y) * d.W + px + x;        // offset inside one (H, W) plane
                const long long* tp = d.tgt + (long)b * HW + io;
                const i64x2 t0 = *reinterpret_cast<const i64x2*>(tp), t1 = *reinterpret_cast<const i64x2*>(tp + 2);
                g[0] = t0[0]; g[1] = t0[1]; g[2] = t1[0]; g[3] = t1[1];
                const T* tok = reinterpret_cast<const T*>(d.pred) + (long)r * ((long)d.C * ps2) + pix;
                const float* img = reinterpret_cast<const float*>(d.pred) + (long)b * d.C * HW + io;
                f32x4 best = TOKENS ? sm_ld4<T>(tok) : sm_ld4<float>(img);
#pragma unroll 4
                for (int c = 1; c < d.C; ++c) {
                    const f32x4 v = TOKENS ? sm_ld4<T>(tok + (long)c * ps2) : sm_ld4<float>(img + (long)c * HW);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool take = v[j] > best[j] || (v[j] != v[j] && best[j] == best[j]);
                        best[j] = take ? v[j] : best[j];
                        idx[j] = take ? c : idx[j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                sm_hist_add(sm_hist, on ? sm_bin(g[j], (long long)idx[j] + d.pred_offset, d.K, d.ignore_label) : -1, lane);
        }
    }
    sm_hist_flush<SM_THREADS>(sm_hist, d.K, d.conf);
}

__global__ __launch_bounds__(SM_THREADS) void label_confusion_kernel(long n, const long long* __restrict__ gt,
                                                                     const long long* __restrict__ pred, int K,
                                                                     long long ignore_label, long long* conf) {
    extern __shared__ unsigned sm_hist[];
    sm_hist_clear<SM_THREADS>(sm_hist, K);
    const int lane = threadIdx.x & (WAVE - 1);
    for (long base = (long)blockIdx.x * SM_THREADS; base < n; base += (long)gridDim.x * SM_THREADS) {   // block-uniform
        const long i = base + threadIdx.x;
        sm_hist_add(sm_hist, i < n ? sm_bin(gt[i], pred[i], K, ignore_label) : -1, lane);
    }
    sm_hist_flush<SM_THREADS>(sm_hist, K, conf);
}

// out[0] mIoU, [1] AA, [2] overall accuracy, [3] existing classes, [4, 4+K) per-class IoU, [4+K, 4+2K) per-class recall.
// Sums of counts are integers (exact); each score is one correctly rounded fp64 division; the three means add their K terms
// in class order.
__global__ __launch_bounds__(SM_MAX_K) void confusion_scores_kernel(int K, const long long* __restrict__ conf,
                                                                   double* __restrict__ out) {
    __shared__ long long s_row[SM_MAX_K], s_diag[SM_MAX_K];
    __shared__ double s_iou[SM_MAX_K], s_rec[SM_MAX_K];
    const int i = threadIdx.x;
    if (i < K) {
        long long row = 0, col = 0;
        for (int j = 0; j < K; ++j) { row += conf[(long)i * K + j]; col += conf[(long)j * K + i]; }
        const long long dg = conf[(long)i * K + i], uni = row + col - dg;
        const double iou = uni != 0 ? (double)dg / (double)uni : 0.0;
        const double rec = row != 0 ? (double)dg / (double)row : 0.0;
        s_row[i] = row; s_diag[i] = dg; s_iou[i] = iou; s_rec[i] = rec;
        out[4 + i] = iou;
        out[4 + K + i] = rec;
    }
    __syncthreads();
    if (i == 0) {
        long long total = 0, trace = 0;
        int existing = 0;
        double si = 0.0, sr = 0.0;
        for (int j = 0; j < K; ++j) {
            total += s_row[j]; trace += s_diag[j]; existing += s_row[j] > 0;
            si += s_iou[j]; sr += s_rec[j];
        }
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        out[0] = si / (double)K;
        out[1] = existing ? sr / (double)existing : nan;
        out[2] = total != 0 ? (double)trace / (double)total : nan;
        out[3] = (double)existing;
    }
}

static bool sm_k_ok(int K) { return K >= 1 && K <= SM_MAX_K; }
static bool sm_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int mmae_argmax_confusion(int pred_dtype, int pred_is_tokens, int B, int C, int H, int W, int patch,
                                     const void* pred, const long long* target, const long long* mask, int K, int pred_offset,
                                     long ignore_label, long long* conf, void* stream) {
    if (pred_dtype != MMAE_F32 && pred_dtype != MMAE_BF16) return MMAE_ERR_ARG;
    if (!pred_is_tokens && pred_dtype != MMAE_F32) return MMAE_ERR_ARG;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || patch <= 0 || (patch % 4) || (H % patch) || (W % patch)) return MMAE_ERR_ARG;
    if (!sm_k_ok(K) || pred_offset < 0) return MMAE_ERR_ARG;
    const long HW = (long)H * W;
    if (HW >= (1L << 31) || (long)B * HW >= (1L << 31)) return MMAE_ERR_ARG;
    if (!pred || !target || !conf || !sm_al16(pred) || !sm_al16(target)) return MMAE_ERR_ARG;
    const int P = (H / patch) * (W / patch);
    ArgmaxDesc d{pred, target, mask, conf, (long)B * P, P, C, H, W, patch, K, pred_offset, (long long)ignore_label};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long wgs = (d.rows + SM_WAVES - 1) / SM_WAVES;
    dim3 grid((unsigned)(wgs < SM_MAX_GRID ? wgs : SM_MAX_GRID)), blk(SM_THREADS);
    const size_t lds = (size_t)K * K * sizeof(unsigned);
    if (!pred_is_tokens) MMAE_LAUNCH((argmax_confusion_kernel<float, false>), grid, blk, lds, st, d);
    else if (pred_dtype == MMAE_BF16) MMAE_LAUNCH((argmax_confusion_kernel<bf16, true>), grid, blk, lds, st, d);
    else MMAE_LAUNCH((argmax_confusion_kernel<float, true>), grid, blk, lds, st, d);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

extern "C" int mmae_label_confusion(long n, const long long* gt, const long long* pred, int K, long ignore_label,
                                    long long* conf, void* stream) {
    if (n < 1 || n >= (1L << 31) || !sm_k_ok(K) || !gt || !pred || !conf) return MMAE_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long wgs = (n + SM_THREADS - 1) / SM_THREADS;
    dim3 grid((unsigned)(wgs < SM_MAX_GRID ? wgs : SM_MAX_GRID)), blk(SM_THREADS);
    MMAE_LAUNCH(label_confusion_kernel, grid, blk, (size_t)K * K * sizeof(unsigned), st, n, gt, pred, K, (long long)ignore_label,
                conf);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}

extern "C" int mmae_confusion_scores(int K, const long long* conf, double* out, void* stream) {
    if (!sm_k_ok(K) || !conf || !out) return MMAE_ERR_ARG;
    MMAE_LAUNCH(confusion_scores_kernel, dim3(1), dim3(SM_MAX_K), 0, reinterpret_cast<hipStream_t>(stream), K, conf, out);
    MMAE_CHECK_LAUNCH();
    return MMAE_OK;
}
