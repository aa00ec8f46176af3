"""Time the S2+DSM BiLSTM fusion at the driver's shape (R = B*N = 100 * 256 = 25600 sequences, D = 192): the native op
(ops.bilstm2_attn_pool: three GEMMs + csrc/bilstm.hip cell kernels), forward + backward under bf16 autocast, against
torch.nn.LSTM(bidirectional) + the attention pooling in torch on the same GPU; then the whole PretrainStep of the driver's
configuration (tiny preset, 256^2 tiles, N = 256, hard-negative head, flat engine) in samples/s.  Prints one JSON line.
FLOPs and bytes are counted from shapes (GEMM: 2 m n k; cell kernels: the bytes they must move) so that a share of peak can be
stated: the cell kernels are bandwidth-bound.

    python tools/bench_bilstm.py [--R 25600] [--D 192] [--iters 50] [--batch 100] [--steps 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from incomplete_multimodal_fusion_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X
BF16_PEAK = 2.5e15         # dense bf16 MFMA FLOP/s, MI355X


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=25600)
    ap.add_argument("--D", type=int, default=192)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    R, D, dev = a.R, a.D, "cuda"
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(D, D, 1, bidirectional=True, batch_first=True).to(dev)
    att = torch.nn.Linear(D, 1).to(dev)
    params = [getattr(lstm, n) for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_ih_l0_reverse',
                                         'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')]
    x0 = torch.randn(R, D, device=dev, requires_grad=True)
    x1 = torch.randn(R, D, device=dev, requires_grad=True)
    dr = torch.randn(R, D, device=dev)

    def native():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            r = ops.bilstm2_attn_pool(x0, x1, params, att.weight, att.bias)
        r.backward(dr)

    def native_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            ops.bilstm2_attn_pool(x0, x1, params, att.weight, att.bias)

    def reference():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y, _ = lstm(torch.stack([x0, x1], dim=1))
            y = y[:, :, :D] + y[:, :, D:]
            alpha = torch.softmax(att(torch.tanh(y)).squeeze(2), dim=1).unsqueeze(1)
            r = alpha.bmm(y.to(alpha.dtype)).squeeze(1)
        r.backward(dr.to(r.dtype))

    t_nat = timed(native, a.iters)
    t_nat_fwd = timed(native_fwd, a.iters)
    t_ref = timed(reference, a.iters)
    # GEMM FLOPs: input projection (2R x 8D x D) + two recurrent (R x 4D x D); backward = 2x (dgrad + wgrad)
    gemm_fwd = 2 * (2 * R) * (8 * D) * D + 2 * 2 * R * (4 * D) * D
    # cell-kernel bytes (bf16 GEMM operands, fp32 state): cell1 fwd reads 2 x 3 gate blocks of G, writes h (bf16) + c, h (fp32);
    # cell2 fwd reads 2 x 4 gate blocks of G and of Hf / Hr, c1, h1, writes r
    e = R * D
    cell_fwd = e * (2 * 3 * 2 + 2 * 2 + 2 * 8) + e * (2 * 4 * 2 + 2 * 4 * 2 + 2 * 8 + 4)
    cell_bwd = e * (2 * 4 * 2 + 2 * 4 * 2 + 2 * 8 + 4 + 8 + 2 * 4 * 2 * 2 + 2 * 8) + e * (2 * 3 * 2 + 2 * 2 + 2 * 8 + 2 * 4 * 2)
    out = {"R": R, "D": D, "native_fwd_bwd_ms": round(t_nat, 4), "native_fwd_ms": round(t_nat_fwd, 4),
           "torch_lstm_fwd_bwd_ms": round(t_ref, 4), "speedup_vs_torch": round(t_ref / t_nat, 3),
           "gemm_gflop_fwd": round(gemm_fwd / 1e9, 2), "gemm_gflop_bwd": round(2 * gemm_fwd / 1e9, 2),
           "cell_gb_fwd": round(cell_fwd / 1e9, 3), "cell_gb_bwd": round(cell_bwd / 1e9, 3),
           "floor_ms_fwd_bwd": round(1e3 * max(3 * gemm_fwd / BF16_PEAK, (cell_fwd + cell_bwd) / HBM_PEAK), 4)}
    out["share_of_floor"] = round(out["floor_ms_fwd_bwd"] / t_nat, 3)

    # the driver's whole step
    from incomplete_multimodal_fusion_amd.engine import FlatAdamW
    from incomplete_multimodal_fusion_amd.pretrain import PretrainStep, get_model
    model = get_model("tiny", in_domains=("s2", "dem"), input_size=256, fusion="bilstm").to(dev).train()
    opt = FlatAdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, exclude=model.never_used_parameters())
    step = PretrainStep(model, opt, 256, contra="hardneg", clip_grad=1.0)
    B = a.batch
    x = {"s2": torch.randn(B, 3, 256, 256, device=dev), "dem": torch.randn(B, 1, 256, 256, device=dev)}
    t_step = timed(lambda: step(x), a.steps)
    out.update(step_batch=B, step_ms=round(t_step, 3), samples_per_s=round(B / t_step * 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
