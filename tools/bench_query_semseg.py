#!/usr/bin/env python
"""Micro-benchmark of the fused Mask2Former evaluation call (mmae_query_confusion, csrc/query_semseg.hip) against the reference's
composition on the same device (maskformer_train_seg.py:258-270): F.interpolate(bilinear) -> softmax[..., 1:] -> sigmoid -> einsum
-> max(1)[1] + 1 in torch, in the dtype of the inputs, then the count by ops.label_confusion -- the path a user of
metrics.ConfMatrix had before this kernel (the reference's own .cpu() + sklearn count is not charged to it).  HIP events around a
window of about 0.3 s per path and shape (thousands of calls at the small shapes), after warm-up.  The reference's shape: B = 30,
K1 = 10, 64 x 64 masks; Q = 10 (the active config) and 100; labels at 64 x 64 and 256 x 256; fp32 and bf16.  Bytes: the algorithmic floor, masks and logits once + 8 B per target pixel.  `moved`: label pairs that
the two paths count in different bins (near-ties decided by summation order; bf16: the composition rounds every stage to bf16,
the kernel only widens the inputs).
Per-kernel split: run this file under `rocprofv3 --kernel-trace --stats` in a run of its own.
`--lib` points the binding at another build of libmmae_hip.so for A/B runs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def timeit(fn, seconds=0.3, warm=5):
    """us per call over a timed window of about `seconds`: the call count comes from a short pilot, so that a 20 us call is timed
    over as long a window as a 2 ms one."""
    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n = max(20, int(seconds * 1e6 / max(window(10), 1.0)))
    return window(n), n


def torch_composition(ops, lg, mk, tgt, K, conf=None):
    up = F.interpolate(mk, size=tgt.shape[-2:], mode="bilinear", align_corners=False)
    semseg = torch.einsum("bqc,bqhw->bchw", F.softmax(lg, dim=-1)[..., 1:], up.sigmoid())
    return ops.label_confusion(tgt, semseg.max(1)[1] + 1, K, conf=conf, ignore_label=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--seconds", type=float, default=0.3, help="timed window per path and shape")
    ap.add_argument("--batch", type=int, default=30)
    args = ap.parse_args()
    from incomplete_multimodal_fusion_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from incomplete_multimodal_fusion_amd import ops
    dev = "cuda:0"
    B, K1, side = args.batch, 10, 64
    rows = []
    for Q in (10, 100):
        for out in (64, 256):
            gen = torch.Generator(device=dev).manual_seed(Q + out)
            lg32 = 2 * torch.randn(B, Q, K1, device=dev, generator=gen)
            mk32 = 3 * torch.randn(B, Q, side, side, device=dev, generator=gen)
            tgt = torch.randint(0, K1, (B, out, out), device=dev, generator=gen)
            for name, dtype, esz in (("fp32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
                lg, mk = lg32.to(dtype), mk32.to(dtype)
                conf = torch.zeros(K1, K1, dtype=torch.int64, device=dev)
                t_k, n_k = timeit(lambda: ops.query_confusion(lg, mk, tgt, K1, conf=conf), args.seconds)
                t_t, n_t = timeit(lambda: torch_composition(ops, lg, mk, tgt, K1, conf=conf), args.seconds)
                diff = ops.query_confusion(lg, mk, tgt, K1) - torch_composition(ops, lg, mk, tgt, K1)
                moved = int(diff.abs().sum()) // 2
                floor = (lg.numel() + mk.numel()) * esz + tgt.numel() * 8
                rows.append({"B": B, "Q": Q, "out": out, "dtype": name, "kernel_us": round(t_k, 1), "floor_MB": round(floor / 1e6, 2),
                             "kernel_GBps": round(floor / t_k / 1e3, 1), "torch_us": round(t_t, 1), "speedup": round(t_t / t_k, 2),
                             "moved": moved, "pixels": tgt.numel(), "calls": [n_k, n_t]})
                print("B=%d Q=%3d %3d^2 -> %3d^2 %s  kernel %8.1f us (%6.1f GB/s of the %.2f MB floor)   torch %9.1f us   x%.1f   "
                      "moved %d of %d" % (B, Q, side, out, name, t_k, floor / t_k / 1e3, floor / 1e6, t_t, t_t / t_k, moved,
                                          tgt.numel()), flush=True)
            del lg32, mk32, tgt
            torch.cuda.empty_cache()
    print(json.dumps({"bench": "query_semseg", "lib": os.path.basename(_lib.LIB_PATH), "rows": rows}))


if __name__ == "__main__":
    main()
