"""The S2+DSM BiLSTM-fusion model (multimae_lstm_s2dsm.MultiMAE) against what the REFERENCE computed
(tests/golden/s2dsm_tiny*.npz, tools/make_golden_s2dsm.py), plus its random-mask, per-sample-mask and PretrainStep paths."""
import pytest
import torch

from tests import parity
from tests.conftest import Golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
DOMS = ("s2", "dem")
DB = "grad/attn_lstm.attention.attention.bias"


@pytest.fixture(scope="module")
def g_model():
    return Golden("s2dsm_tiny.npz")


def _native(cfg):
    from incomplete_multimodal_fusion_amd.multimae import FusionInputAdapter, PatchedInputAdapter, SpatialOutputAdapter
    from incomplete_multimodal_fusion_amd.multimae import multimae_lstm_s2dsm as ms
    from incomplete_multimodal_fusion_amd.multimae.zorro_utils import TokenTypes as T
    kw = dict(stride_level=1, patch_size_full=cfg["patch_size"], image_size=cfg["image_size"])
    chans = (("s2", 3), ("dem", 1))
    ia = {d: PatchedInputAdapter(num_channels=c, **kw) for d, c in chans}
    oa = {d: SpatialOutputAdapter(num_channels=c, stride_level=1, patch_size_full=cfg["patch_size"], dim_tokens=cfg["decoder_dim"],
                                  depth=cfg["decoder_depth"], num_heads=cfg["decoder_heads"], use_task_queries=True, task=d,
                                  context_tasks=list(DOMS), use_xattn=True) for d, c in chans}
    ia["fusion"] = FusionInputAdapter(num_channels=1, **kw)
    return ms.MultiMAE(input_adapters=ia, output_adapters=oa, dim_tokens=cfg["dim_tokens"], depth=cfg["depth"],
                       dim_head=cfg["dim_head"], heads=cfg["heads"], ff_mult=4,
                       num_fusion_tokens=(cfg["image_size"] // cfg["patch_size"]) ** 2, return_token_types=(T.S2, T.DEM, T.FUSION))


def _loaded(g_model):
    model = _native(g_model.json("config"))
    model.load_state_dict(g_model.sub("state"), strict=True)
    return model.to(DEV).train()


def test_state_dict_strict_loads_in_reference_order(g_model):
    model = _native(g_model.json("config"))
    assert list(model.state_dict().keys()) == [str(k) for k in g_model.z["keys"]]
    model.load_state_dict(g_model.sub("state"), strict=True)


@pytest.mark.parametrize("case", ["both", "nodem"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("fused", [False, True])
def test_s2dsm_model_matches_reference_fixture(g_model, case, mode, fused):
    """One step under the driver's loss (task losses + HardNegtive_loss over (s2, dem), (s2, fus), (dem, fus)): every output, the
    loss and every parameter gradient against the reference -- fp32 at 1e-3, bf16 against the reference's own CPU bf16 run."""
    model = _loaded(g_model)
    c = Golden("s2dsm_tiny_%s.npz" % case)
    x = {k: v.to(DEV) for k, v in g_model.sub("x").items()}
    masks = {d: c.t("mask/" + d).to(DEV) for d in DOMS}
    autocast = mode == "bf16"
    got = parity.native_step_flat(model, x, masks, int(c.t("N")), autocast, fused=fused, contra="hardneg", domains=DOMS)
    ref = {k: torch.from_numpy(c.z[k].copy()).double() for k in c.z.files if k not in ("N",) and not k.startswith("mask/")}
    assert sum(1 for k in ref if k.startswith("grad/")) > 50 and "grad/attn_lstm.lstm.weight_hh_l0_reverse" in ref
    # Attention_LSTM's bias gradient is mathematically zero (the 2-way softmax is shift invariant): both sides hold rounding noise,
    # so it is held to an absolute bound against the scale of its weight's gradient instead of a relative one
    db, dw = got.pop(DB), got["grad/attn_lstm.attention.attention.weight"]
    ref.pop(DB)
    assert float(db.abs().max()) <= 1e-3 * float(dw.abs().mean()), (float(db.abs().max()), float(dw.abs().mean()))
    anchor, pred_l2 = None, None
    if autocast:
        a = Golden("s2dsm_tiny_bf16.npz")
        anchor = {k: v.double() for k, v in a.sub("case_" + case).items()}
        # prediction images, strict clause: 1e-2 relative L2, or 1.5x what bf16 costs the reference's own arithmetic on this image
        # (the decoders of this model read bf16-rounded encoder rows AND the learned tokens of unkept patches)
        pred_l2 = max([1e-2] + [1.5 * parity._l2rel(anchor[k], ref[k]) for k in ref if k.startswith("pred/")])
    parity.compare(got, ref, anchor, tol=1e-2 if autocast else 1e-3, pred_l2_tol=pred_l2)


def test_random_masks_reproduce_through_explicit_masks(g_model):
    model = _loaded(g_model)
    x = {k: v.to(DEV) for k, v in g_model.sub("x").items()}
    torch.manual_seed(3)
    with torch.no_grad():
        out = model(x, num_encoded_tokens=12)
        again = model(x, task_masks=out[1], num_encoded_tokens=12)
    for d in DOMS:
        assert torch.equal(out[0][d], again[0][d]), d
    for i in (2, 3, 4):
        assert torch.equal(out[i], again[i]), i


@pytest.fixture(scope="module")
def plain_bf16(g_model):
    """The bf16 forward of case `both` without options, shared (and left unchanged) by the two option tests below; they reach this
    model through the pooling and decoder stages it shares with multimae_crossattn.  -> (call(**options), its plain result)."""
    model = _loaded(g_model)
    c = Golden("s2dsm_tiny_both.npz")
    x = {k: v.to(DEV) for k, v in g_model.sub("x").items()}
    masks = {d: c.t("mask/" + d).to(DEV) for d in DOMS}

    def call(**options):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(x, task_masks=masks, num_encoded_tokens=int(c.t("N")), **options)
    return call, call()


def _same_but(out, plain, preds=DOMS, others=(2, 3, 4)):
    for d in preds:
        assert torch.equal(out[0][d], plain[0][d]), d
    for i in others:
        assert torch.equal(out[i], plain[i]), i


def test_return_token_indices_select_rows_of_the_pooled_tokens(plain_bf16):
    """`return_token_indices=(0, 2)`: rows 0 and 2 of the plain call's pooled tokens, exactly; nothing else moves."""
    call, plain = plain_bf16
    out = call(return_token_indices=(0, 2))
    assert plain[2].shape[1] == 3 and out[2].shape[1] == 2
    assert torch.equal(out[2], plain[2][:, [0, 2]])
    _same_but(out, plain, others=(3, 4))


def test_fp32_output_adapter_agrees_with_its_bf16_run(plain_bf16):
    """`fp32_output_adapters=['dem']`: the dem decoder leaves the autocast region and reads the fp32 fusion grid, so it differs
    from its bf16 run by what bf16 costs one decoder -- held to the bound this file holds a bf16 prediction image to against the
    fp32 reference: 1e-2 relative L2, or 1.5x what bf16 costs the reference's own arithmetic on it.  Everything else: exact."""
    call, plain = plain_bf16
    out = call(fp32_output_adapters=["dem"])
    _same_but(out, plain, preds=("s2",))
    c, anchor = Golden("s2dsm_tiny_both.npz"), Golden("s2dsm_tiny_bf16.npz").sub("case_both")
    tol = max(1e-2, 1.5 * parity._l2rel(anchor["pred/dem"].double(), torch.from_numpy(c.z["pred/dem"].copy()).double()))
    err = parity._l2rel(out[0]["dem"].double(), plain[0]["dem"].double())
    print("fp32 dem adapter vs bf16 run: rel L2 %.3e (bound %.3e)" % (err, tol))
    assert out[0]["dem"].dtype == torch.float32 and torch.isfinite(out[0]["dem"]).all()
    assert 0.0 < err <= tol, (err, tol)


def test_per_sample_masks_match_single_sample_runs(g_model):
    """per_sample_masks=True: every sample uses its own mask row (tok_patch is per row) -- the same as running each sample alone."""
    model = _loaded(g_model)
    x = {k: v.to(DEV) for k, v in g_model.sub("x").items()}
    B, P, N = x["s2"].shape[0], 16, 10
    g = torch.Generator().manual_seed(4)
    masks = {d: torch.ones(B, P, dtype=torch.long) for d in DOMS}
    for b in range(B):
        k = int(torch.randint(0, N + 1, (1,), generator=g))
        masks["s2"][b, torch.randperm(P, generator=g)[:k]] = 0
        masks["dem"][b, torch.randperm(P, generator=g)[:N - k]] = 0
    masks = {d: m.to(DEV) for d, m in masks.items()}
    model.per_sample_masks = True
    with torch.no_grad():
        out = model(x, task_masks=masks, num_encoded_tokens=N)
        model.per_sample_masks = False
        for b in range(B):
            one = model({d: v[b:b + 1] for d, v in x.items()}, task_masks={d: m[b:b + 1] for d, m in masks.items()},
                        num_encoded_tokens=N)
            for d in DOMS:
                torch.testing.assert_close(out[0][d][b:b + 1], one[0][d], rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(out[2][b:b + 1], one[2], rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(out[4][b:b + 1], one[4], rtol=1e-4, atol=1e-5)


def _driver_step(B=8, size=256):
    from incomplete_multimodal_fusion_amd.engine import FlatAdamW
    from incomplete_multimodal_fusion_amd.pretrain import PretrainStep, get_model
    torch.manual_seed(21)
    model = get_model("tiny", in_domains=DOMS, input_size=size, fusion="bilstm").to(DEV).train()
    opt = FlatAdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, exclude=model.never_used_parameters())
    step = PretrainStep(model, opt, 256, contra="hardneg", clip_grad=1.0)
    gen = torch.Generator().manual_seed(22)
    x = {"s2": torch.randn(B, 3, size, size, generator=gen).to(DEV), "dem": torch.randn(B, 1, size, size, generator=gen).to(DEV)}
    return model, opt, step, x


def test_pretrain_step_driver_configuration_runs():
    """The driver's configuration (tiny preset, 256^2 tiles, N = 256, hard-negative head) through PretrainStep and the flat engine."""
    model, opt, step, x = _driver_step()
    for _ in range(3):
        out = step(x)
        assert torch.isfinite(out["loss"]) and torch.isfinite(out["loss_contra"])
    assert not opt.last_step_skipped()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert model.attn_lstm.lstm.weight_hh_l0_reverse._mmae_grad.abs().sum() > 0


def test_pretrain_step_captured_matches_eager():
    """PretrainStep.capture on the S2+DSM model: replays on fixed masks match the eager step (as tests/test_gpu_graph.py checks the
    headline model)."""
    from incomplete_multimodal_fusion_amd.engine import FlatAdamW
    from incomplete_multimodal_fusion_amd.pretrain import PretrainStep, get_model
    size, B = 128, 4
    gen = torch.Generator().manual_seed(31)
    x = {"s2": torch.randn(B, 3, size, size, generator=gen).to(DEV), "dem": torch.randn(B, 1, size, size, generator=gen).to(DEV)}
    P = (size // 16) ** 2
    masks = {d: torch.ones(B, P, dtype=torch.long) for d in DOMS}
    masks["s2"][:, :20] = 0
    masks["dem"][:, 10:34] = 0
    masks = {d: m.to(DEV) for d, m in masks.items()}
    runs = []
    for captured in (False, True):
        torch.manual_seed(32)
        model = get_model("tiny", in_domains=DOMS, input_size=size, decoder_dim=64, decoder_depth=1, decoder_num_heads=2,
                          fusion="bilstm").to(DEV).train()
        model.depth = 2; model.blocks = model.blocks[:2]
        opt = FlatAdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, exclude=model.never_used_parameters())
        step = PretrainStep(model, opt, 44, contra="hardneg")
        if captured:
            step.capture(x, task_masks=masks, warmup=2)
            losses = [float(step.replay(x, task_masks=masks)["loss"]) for _ in range(3)]
        else:
            losses = [float(step(x, task_masks=masks)["loss"]) for _ in range(5)][2:]
        runs.append((losses, [p.detach().clone() for p in model.parameters()]))
    (le, pe), (lc, pc) = runs
    for a, b in zip(le, lc):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (le, lc)
    for a, b in zip(pe, pc):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
