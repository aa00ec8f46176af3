/* mmae_internal.h -- NOT part of the product ABI (include/mmae_hip.h).  Test / tuning entry points of libmmae_hip.so:
 * the attention launchers with the kernel variant as a PER-CALL argument (no process-global state, so concurrent streams
 * and threads cannot change each other's kernel).  Consumers: tests/ (generic-vs-fast-path agreement) and
 * tools/bench_attn.py (A/B of tilings inside one process).
 *
 * `variant` is -1 or, in bits 0..7, one of the numbers below; every other number returns MMAE_ERR_ARG before anything is launched.
 * fp32 always runs the generic kernels of mha.hip, head_dim 32 its own bf16 kernels; the table is bf16, head_dim 64
 * (mha_bf16.hip: mha_bf16_fwd / mha_bf16_bwd hold the routing and every fallback):
 *
 *   variant | forward                                             | backward
 *   --------+-----------------------------------------------------+-------------------------------------------------------------
 *     -1    | generic dtype-templated kernels of mha.hip          | same
 *      0    | what mmae_mha_fwd runs: mha_sh_fwd_kernel where     | what mmae_mha_bwd runs: dQ mha_bf16_bwd_dq_kernel; dK/dV
 *           | mha_sh_applicable, else mha_bf16_fwd32_kernel<1>    | mha_sh_dkdv_kernel where supported and max_k_rows >= 128,
 *           |                                                     | else mha_bf16_bwd_dkdv_kernel
 *      2    | mha_bf16_fwd_kernel (16x16x32, 128-query tiles)     | tile-per-block dQ and dK/dV
 *      4    | mha_bf16_fwd32_kernel<2> (256-query tiles)          | tile-per-block dQ and dK/dV
 *      5    | mha_sh_fwd_kernel unconditionally                   | mha_sh_dq_kernel and mha_sh_dkdv_kernel where supported (no
 *           |                                                     | 128-row threshold), else the tile-per-block kernels
 *     23    | as 0                                                | dQ mha_bf16_bwd_dq_heads_kernel; dK/dV as 0
 *     50    | as 0                                                | mha_rowconst_kernel + mha_sh_bwd_kernel (dQ + dK + dV fused; the
 *           |                                                     | product entry is mmae_mha_bwd_fused) where
 *           |                                                     | mha_sh_fused_supported, else as 0
 *     55    | as 0                                                | mha_sh_bwd_kernel forming the row constants itself, no pre-pass
 *           |                                                     | (correct results; did not pay in the step); else as 0
 *
 * Variants 50 and 55 need delta_ws sized by mmae_mha_bwd_fused_ws_floats (include/mmae_hip.h).
 * Bits 8..11 of a positive variant: heads ONE workgroup of the sample-head kernels (mha_sh.hip) walks, a divisor of H -- the product
 * path picks it from (B, H) (all H heads once B >= 256); tests force 1 / 2 / H at small B to reach the head loop, the cross-head
 * K/V prefetch and the ring accounting of the bench configuration.  0 = product choice. */
#ifndef MMAE_INTERNAL_H
#define MMAE_INTERNAL_H
#ifdef __cplusplus
extern "C" {
#endif
int mmae_mha_fwd_variant(int dtype, int head_dim, int B, int H, int nseg, const void* q, const void* k, const void* v, void* out,
                         float* lse, long q_stride, long k_stride, long v_stride, long o_stride, long q_rows_total,
                         const int* q_seg_start, const int* q_seg_len, const int* k_seg_start, const int* k_seg_len,
                         int max_q_rows, int max_k_rows, float scale, int empty_mode, int variant, void* stream);
int mmae_mha_bwd_variant(int dtype, int head_dim, int B, int H, int nseg, const void* q, const void* k, const void* v,
                         const void* out, const void* dout, const float* lse, float* delta_ws, void* dq, void* dk, void* dv,
                         long q_stride, long k_stride, long v_stride, long o_stride, long do_stride, long dq_stride,
                         long dk_stride, long dv_stride, long q_rows_total, const int* q_seg_start, const int* q_seg_len,
                         const int* k_seg_start, const int* k_seg_len, int max_q_rows, int max_k_rows, float scale,
                         int empty_mode, int variant, void* stream);
/* bench.py's event-bracket calibration: a streaming copy of n_bytes (multiple of 16) under its own kernel name. */
int mmae_debug_stream_copy(long n_bytes, const void* src, void* dst, void* stream);
#ifdef __cplusplus
}
#endif
#endif
