// The per-workgroup K x K confusion histogram in LDS shared by segmetrics.hip and query_semseg.hip: (gt, pred) pairs are counted
// into uint32 bins by LDS atomics and the non-zero bins are added to the int64 matrix once, when the workgroup ends.  Integer adds
// commute: the counts are exact and do not depend on scheduling.  NT: threads of the workgroup.
#pragma once
#include "common.hpp"

// Bin of one (gt, pred) pair, -1 when the pair is dropped: gt == ignore_label, or either label outside [0, K).
__device__ __forceinline__ int sm_bin(long long g, long long p, int K, long long ignore_label) {
    const bool ok = g != ignore_label && g >= 0 && g < (long long)K && p >= 0 && p < (long long)K;
    return ok ? (int)g * K + (int)p : -1;
}

// One histogram increment per lane (bin < 0: none); wave-uniform control flow required.  Class maps are smooth: most of a wave
// falls into the bin of its first active lane, and those lanes are added by ONE LDS atomic; the others add 1 each.
__device__ __forceinline__ void sm_hist_add(unsigned* h, int bin, int lane) {
    const unsigned long long act = __ballot(bin >= 0);
    if (act == 0) return;
    const int leader = __builtin_ctzll(act);
    const int b0 = __builtin_amdgcn_readlane(bin, leader);
    const unsigned long long same = __ballot(bin == b0);
    if (lane == leader) atomicAdd(h + b0, (unsigned)__popcll(same));
    else if (bin >= 0 && bin != b0) atomicAdd(h + bin, 1u);
}

template <int NT> __device__ __forceinline__ void sm_hist_clear(unsigned* h, int K) {
    for (int i = threadIdx.x; i < K * K; i += NT) h[i] = 0u;
    __syncthreads();
}

template <int NT> __device__ __forceinline__ void sm_hist_flush(const unsigned* h, int K, long long* conf) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += NT) {
        const unsigned v = h[i];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(conf) + i, (unsigned long long)v);
    }
}
