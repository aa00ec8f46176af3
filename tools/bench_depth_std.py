#!/usr/bin/env python
"""Micro-benchmark of the truncated depth standardisation (mmae_trunc_standardize, csrc/depthstd.hip) against the reference's
formulation (pretrain_mmae.py:452-458: torch.sort, slice, mean / var, normalise) in the same process, HIP events.
Bytes moved: 2 * B * n * 4 (one read, one write: the register-resident path's floor; n > 64 Ki re-reads the sample per pass).
`--lib` points the binding at another build of libmmae_hip.so for A/B runs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def timeit(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def torch_formulation(x):
    B = x.shape[0]
    s = torch.sort(x.reshape(B, -1), dim=1)[0]
    n = s.shape[1]
    s = s[:, int(0.1 * n):int(0.9 * n)]
    return (x - s.mean(dim=1)[:, None, None, None]) / torch.sqrt(s.var(dim=1)[:, None, None, None] + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    from incomplete_multimodal_fusion_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from incomplete_multimodal_fusion_amd import ops
    dev = "cuda:0"
    rows = []
    for side in (256, 1024):
        for B in (64, 256):
            n = side * side
            x = (300.0 + 25.0 * torch.randn(B, 1, side, side, device=dev))     # a DSM-like tile: metres, concentrated
            t_k = timeit(lambda: ops.trunc_standardize(x), args.iters)
            t_t = timeit(lambda: torch_formulation(x), max(5, args.iters // 3), warm=2)
            err = float((ops.trunc_standardize(x) - torch_formulation(x)).abs().max())
            gb = 2 * B * n * 4
            rows.append({"B": B, "n": n, "kernel_us": round(t_k, 1), "kernel_GBps": round(gb / t_k / 1e3, 1),
                         "torch_sort_us": round(t_t, 1), "speedup": round(t_t / t_k, 2), "max_abs_diff": err})
            print("B=%4d n=%8d  kernel %9.1f us (%7.1f GB/s)   torch sort %10.1f us   x%.1f   max|diff| %.2e" %
                  (B, n, t_k, gb / t_k / 1e3, t_t, t_t / t_k, err), flush=True)
            del x
            torch.cuda.empty_cache()
    print(json.dumps({"bench": "depth_std", "lib": os.path.basename(_lib.LIB_PATH), "rows": rows}))


if __name__ == "__main__":
    main()
