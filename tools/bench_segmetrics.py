#!/usr/bin/env python
"""Micro-benchmark of the fused argmax + confusion matrix (mmae_argmax_confusion, csrc/segmetrics.hip) against the same result
composed from torch ops on the same device (argmax(1), patch-mask upsampling, gt*K + pred, bincount), HIP events after warm-up.
The dnw configuration: C = K = 9, 256 x 256 tiles, patch 16, B = 256 and 64; fp32 logit image and bf16 decoder tokens; with and
without a patch mask.  Bytes: the algorithmic floor, logits once + 8 B per target pixel + 8 B per mask entry (a masked run still
counts every logit: the floor of the unmasked problem is the yardstick for both).  The torch composition works on the logit IMAGE
in both layouts -- for tokens it is charged nothing for the unpatchify it would need first.
Per-kernel split: run this file under `rocprofv3 --kernel-trace --stats` in a run of its own.
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


def torch_composition(img, tgt, mask, K, ps):
    B, C, H, W = img.shape
    idx = tgt * K + img.argmax(1)
    if mask is None:
        return torch.bincount(idx.reshape(-1), minlength=K * K).reshape(K, K)
    up = mask.view(B, H // ps, W // ps).repeat_interleave(ps, 1).repeat_interleave(ps, 2) == 1
    return torch.bincount(idx[up], minlength=K * K).reshape(K, K)          # the boolean index synchronises with the host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 64])
    args = ap.parse_args()
    from incomplete_multimodal_fusion_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from incomplete_multimodal_fusion_amd import ops
    dev = "cuda:0"
    C = K = 9
    side, ps = 256, 16
    P = (side // ps) ** 2
    rows = []
    for B in args.batches:
        gen = torch.Generator(device=dev).manual_seed(B)
        img = torch.randn(B, C, side, side, device=dev, generator=gen)
        tgt = torch.randint(0, K, (B, side, side), device=dev, generator=gen)
        mask = (torch.rand(B, P, device=dev, generator=gen) < 0.75).long()                 # 3/4 of the patches predicted
        tok = img.view(B, C, side // ps, ps, side // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * P, C * ps * ps).bfloat16().contiguous()
        img_bf = ops.unpatchify(tok, B, C, side, side, ps).float()                         # the image the bf16 tokens stand for
        for layout, pred, ref_img, esz in (("image_f32", img, img, 4), ("tokens_bf16", (tok, C), img_bf, 2)):
            for m in (None, mask):
                conf = torch.zeros(K, K, dtype=torch.int64, device=dev)
                t_k = timeit(lambda: ops.argmax_confusion(pred, tgt, m, K, ps, conf=conf), args.iters)
                t_t = timeit(lambda: torch_composition(ref_img, tgt, m, K, ps), max(5, args.iters // 3), warm=2)
                same = bool(torch.equal(ops.argmax_confusion(pred, tgt, m, K, ps), torch_composition(ref_img, tgt, m, K, ps)))
                floor = B * side * side * (C * esz + 8) + B * P * 8
                rows.append({"B": B, "layout": layout, "mask": m is not None, "kernel_us": round(t_k, 1),
                             "floor_GB": round(floor / 1e9, 3), "kernel_GBps": round(floor / t_k / 1e3, 1),
                             "torch_us": round(t_t, 1), "speedup": round(t_t / t_k, 2), "equal": same})
                print("B=%4d %-11s mask=%-5s  kernel %9.1f us (%7.1f GB/s of the %.3f GB floor)   torch %10.1f us   x%.1f   equal %s" %
                      (B, layout, m is not None, t_k, floor / t_k / 1e3, floor / 1e9, t_t, t_t / t_k, same), flush=True)
        del img, tgt, mask, tok, img_bf
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "segmetrics", "lib": os.path.basename(_lib.LIB_PATH), "rows": rows}))


if __name__ == "__main__":
    main()
