"""Generate tests/golden/s2dsm_tiny*.npz: the reference's S2+DSM BiLSTM-fusion model (pretraining/multimae/multimae_lstm_s2dsm.py,
what pretraining/pretrain_mmae_s2dsm.py:181-241 builds) at a tiny size, under its driver's loss (:469-496: masked MSE for s2,
masked L1 for dem, NoWeightingStrategy, HardNegtive_loss over (s2, dem), (s2, fusion), (dem, fusion)).

The reference is imported at generation time only, through oracle/ref_loader.py's stub-package binding (the `multimae`
package object pointing at the reference directory, the canonical downstream zorro_utils bound as multimae.zorro_utils).  The
fixture holds arrays, the JSON configuration and the ordered state-dict key list -- no program text.

    python tools/make_golden_s2dsm.py            # (re)write the fixture files
    python tools/make_golden_s2dsm.py --check    # regenerate in memory; exit 1 unless the committed files are reproduced

Reproducible by construction: fixed seeds, single-threaded torch (the order of every CPU reduction is then fixed), .npz
containers written with a fixed entry timestamp, and the host requirement below, so the same arrays give the same file bytes.

Host requirement.  torch's CPU libraries pick their kernels by the host's instruction set, and different kernels round
differently.  The files were written with MKL on its AVX2 code path and oneDNN without native bf16 / AMX instructions; both are
pinned here before torch loads (HOST_PINS), which is a no-op on such a host and restores that arithmetic on a newer one:
  * the model file (seeded initialisation: RNG + MKL vector math) and the bf16-autocast file (its GEMMs and the LSTM run in oneDNN)
    then regenerate bit for bit also on a host with native bf16 / AMX units, and --check compares them bit for bit;
  * the two fp32 result files go through MKL's sgemm, whose blocking -- and with it the summation order -- is chosen per CPU
    vendor and model inside the AVX2 path and cannot be pinned.  They regenerate bit for bit on the host family that wrote them;
    elsewhere --check holds their float arrays to the fp32 rounding bound of differences(), everything else in them exactly.
"""
import argparse
import importlib
import io
import json
import os
import sys
import types
import zipfile

HOST_PINS = {"MKL_ENABLE_INSTRUCTIONS": "AVX2", "ONEDNN_MAX_CPU_ISA": "AVX512_CORE"}
for _k, _v in HOST_PINS.items():          # read once, when the libraries load: before `import torch`
    os.environ[_k] = _v

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# four files, each under the 1 MiB limit of a committed file: the model and its inputs, the fp32 result of each mask case, and the
# CPU bf16-autocast run of both cases (the anchor of tests/parity.compare, stored as float16: it only sizes the reference's own
# bf16 error, which is ~10x the float16 rounding)
FILES = ("s2dsm_tiny.npz", "s2dsm_tiny_both.npz", "s2dsm_tiny_nodem.npz", "s2dsm_tiny_bf16.npz")
CFG = dict(dim_tokens=32, depth=2, dim_head=32, heads=2, image_size=64, patch_size=16, decoder_dim=32, decoder_depth=1,
           decoder_heads=1, B=4)
CHANNELS = (("s2", 3), ("dem", 1))
CASES = {                      # kept patches per modality (row 0 of the masks drives the batch, :402-406)
    "both": {"s2": [0, 1, 2, 5, 7, 9, 14], "dem": [1, 2, 3, 4, 9, 12, 15]},   # 1, 2, 9 kept by both: two fusion rows each
    "nodem": {"s2": [0, 3, 4, 6, 8, 10, 11, 13], "dem": []},                  # one modality keeps nothing
}


def load_s2dsm():
    """-> (reference namespace of ref_loader.load(), the multimae_lstm_s2dsm module), imported unmodified."""
    ref = ref_loader.load()
    saved = {k: v for k, v in sys.modules.items() if k == "multimae" or k.startswith("multimae.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("multimae")
    pkg.__path__ = [ref_loader.MM]
    sys.modules["multimae"] = pkg
    sys.modules["multimae.zorro_utils"] = ref.zu
    sys.modules["multimae.multimae_utils"] = ref.mu
    try:
        mod = importlib.import_module("multimae.multimae_lstm_s2dsm")
    finally:
        for k in [k for k in sys.modules if k == "multimae" or k.startswith("multimae.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return ref, mod


def build(ref, mod):
    c = CFG
    T = ref.zu.TokenTypes
    ia = {d: ref.ia.PatchedInputAdapter(num_channels=ch, stride_level=1, patch_size_full=c["patch_size"],
                                        image_size=c["image_size"]) for d, ch in CHANNELS}
    oa = {d: ref.oa.SpatialOutputAdapter(num_channels=ch, stride_level=1, patch_size_full=c["patch_size"],
                                         dim_tokens=c["decoder_dim"], depth=c["decoder_depth"], num_heads=c["decoder_heads"],
                                         use_task_queries=True, task=d, context_tasks=[d for d, _ in CHANNELS], use_xattn=True)
          for d, ch in CHANNELS}
    ia["fusion"] = ref.ia.FusionInputAdapter(num_channels=1, stride_level=1, patch_size_full=c["patch_size"],
                                             image_size=c["image_size"])
    return mod.MultiMAE(input_adapters=ia, output_adapters=oa, num_global_tokens=1, dim_tokens=c["dim_tokens"], depth=c["depth"],
                        dim_head=c["dim_head"], heads=c["heads"], ff_mult=4,
                        num_fusion_tokens=(c["image_size"] // c["patch_size"]) ** 2,
                        return_token_types=(T.S2, T.DEM, T.FUSION), drop_path_rate=0.0, norm_layer=ref.zu.LayerNorm)


def npy(t, dtype=np.float32):
    if isinstance(t, torch.Tensor):
        a = t.detach().float().cpu().numpy()
        if dtype == np.float16:
            assert np.isfinite(a).all() and np.abs(a).max(initial=0) < 6e4
        return a.astype(dtype)
    return np.asarray(t)


def step(ref, model, x, masks, N, bf16):
    fns = {"s2": ref.cr.MaskedMSELoss(patch_size=16, stride=1), "dem": ref.cr.MaskedL1Loss(patch_size=16, stride=1)}
    hn = ref.cr.HardNegtive_loss()
    model.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        preds, tm, pooled, ori, fus = model(x, task_masks=masks, num_encoded_tokens=N)
        task_losses = {t: fns[t](preds[t].float(), x[t], mask=masks.get(t, None)) for t in preds}
        f = [t.squeeze(1) for t in torch.chunk(pooled, 3, dim=1)]
        loss_contra = hn(f[0], f[1]) + hn(f[0], f[2]) + hn(f[1], f[2])
        loss = sum(task_losses.values()) + loss_contra
    loss.backward()
    out = {}
    for d in preds:
        out["pred/" + d] = preds[d]
        out["loss/" + d] = task_losses[d]
    out.update(pooled=pooled, ori_tokens=ori, fusion_tokens=fus, loss_contra=loss_contra, loss=loss)
    for n, p in model.named_parameters():
        if p.grad is not None:
            out["grad/" + n] = p.grad
    return out


def generate():
    ref, mod = load_s2dsm()
    # HardNegtive_loss moves its negative mask with `.cuda()` (criterion.py:242): a no-op for this CPU run only
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        return _generate(ref, mod)
    finally:
        torch.Tensor.cuda = orig_cuda


def _generate(ref, mod):
    torch.manual_seed(5101)
    model = build(ref, mod)
    gen = torch.Generator().manual_seed(5102)
    with torch.no_grad():                         # move every parameter off its initial value so that the fixture pins all terms
        for _, p in model.named_parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=gen) * (p.abs().mean() + 0.1))
    model.train()
    B, P = CFG["B"], (CFG["image_size"] // CFG["patch_size"]) ** 2
    x = {d: torch.randn(B, ch, CFG["image_size"], CFG["image_size"], generator=gen) for d, ch in CHANNELS}
    bag = {"config": np.array(json.dumps(CFG)), "keys": np.array(list(model.state_dict().keys()))}
    bags = {FILES[0]: bag, FILES[3]: {}}
    for k, v in model.state_dict().items():
        bag["state/" + k] = npy(v)
    for d in x:
        bag["x/" + d] = npy(x[d])
    for cname, keep in CASES.items():
        masks = {}
        for d, idx in keep.items():
            row = torch.ones(P, dtype=torch.long)
            row[torch.tensor(idx, dtype=torch.long)] = 0
            masks[d] = row[None].repeat(B, 1)
        N = sum(len(v) for v in keep.values())
        cb = bags["s2dsm_tiny_%s.npz" % cname] = {}
        cb["N"] = np.array(N)
        for d in masks:
            cb["mask/" + d] = npy(masks[d]).astype(np.int64)
        for k, v in step(ref, model, x, masks, N, False).items():
            cb[k] = npy(v)
        for k, v in step(ref, model, x, masks, N, True).items():
            bags[FILES[3]]["case_%s/%s" % (cname, k)] = npy(v, np.float16)
    return {name: npz_bytes(bags[name]) for name in FILES}


def npz_bytes(bag) -> bytes:
    """np.savez_compressed's container (one deflated .npy entry per array; np.load reads it) with a fixed entry timestamp: the
    same arrays always give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in bag.items():
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with z.open(zi, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    return buf.getvalue()


FP32_RESULT_FILES = FILES[1:3]       # the files behind MKL's sgemm (see the module docstring); the other two compare bit for bit
FP32_RTOL, FP32_ATOL = 1e-5, 1e-7


def differences(committed: bytes, fresh: bytes, fp32_rounding: bool = False):
    """-> list of "name: why" for the arrays that are not bitwise identical (or exist on one side only).
    fp32_rounding (the two fp32 result files only): a float array also passes when max |difference| <= 1e-5 of its largest
    magnitude + 1e-7.  1e-5 is 84 fp32 ulps: every value is behind some ten reductions of up to ~1e3 terms, each off by a few
    ulps between two summation orders, and it is 100x below the 1e-3 at which the tests read these files.  1e-7 is one ulp of the
    O(1) terms that cancel in Attention_LSTM's bias gradient, which is 0 in exact arithmetic and rounding noise in any run."""
    a, b = np.load(io.BytesIO(committed)), np.load(io.BytesIO(fresh))
    out = ["%s: only in one file" % k for k in sorted(set(a.files) ^ set(b.files))]
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            out.append("%s: %s%s vs %s%s" % (k, x.dtype, x.shape, y.dtype, y.shape))
        elif x.tobytes() != y.tobytes():
            if x.dtype.kind != "f":
                out.append("%s: values differ" % k)
                continue
            d = np.abs(x.astype(np.float64) - y.astype(np.float64)).max()
            lim = FP32_RTOL * np.abs(x.astype(np.float64)).max() + FP32_ATOL if fp32_rounding else 0.0
            if not d <= lim:
                out.append("%s: values differ (max abs %s, allowed %s)" % (k, d, lim))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare every array with the committed fixture (see the module docstring)")
    a = ap.parse_args()
    torch.set_num_threads(1)          # single-threaded reductions: a fixed summation order
    data = generate()
    if a.check:
        bad = 0
        for name, b in data.items():
            with open(os.path.join(GOLDEN, name), "rb") as f:
                diff = differences(f.read(), b, fp32_rounding=name in FP32_RESULT_FILES)
            print(name + ":", "reproduced" if not diff else "DIFFERS: " + "; ".join(diff[:8]))
            bad += bool(diff)
        sys.exit(1 if bad else 0)
    for name, b in data.items():
        assert len(b) < 1 << 20, (name, len(b))
        with open(os.path.join(GOLDEN, name), "wb") as f:
            f.write(b)
        print("wrote", name, len(b), "bytes")


if __name__ == "__main__":
    main()
