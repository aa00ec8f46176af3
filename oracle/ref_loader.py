"""TEST INFRASTRUCTURE ONLY -- loader for the *actual* reference implementation.

Only usable in the build container, where the read-only reference checkout lives at
/root/reference.  It is used by `oracle/make_golden.py` to generate the committed fixtures in
`tests/golden/`; no test imports it.  Nothing in the product package imports this file.

Why a custom loader:
  * pretraining/multimae/__init__.py imports .multimae -> .zorro_utils, and
    pretraining/multimae/zorro_utils.py:255 has a U+FF1A character (SyntaxError), so the package
    cannot be imported as committed.
  * downstream/instance_segmentation/modeling/multimae/zorro_utils.py is the same file with the
    working Block_Fusion (lines 249, 255) -- it is what the checkpoints are loaded with.
We therefore register an empty `multimae` package object whose __path__ points at the reference
directory (skipping its __init__), bind the downstream zorro_utils as `multimae.zorro_utils`, and
import the remaining reference modules unmodified.
"""
import importlib
import importlib.util
import os
import sys
import types

REF_ROOT = os.environ.get("MMAE_REFERENCE_ROOT", "/root/reference")
MM = os.path.join(REF_ROOT, "pretraining", "multimae")
DSI_MM = os.path.join(REF_ROOT, "downstream", "instance_segmentation", "modeling", "multimae")


def available() -> bool:
    return os.path.isfile(os.path.join(MM, "multimae_crossattn.py")) and os.path.isfile(
        os.path.join(DSI_MM, "zorro_utils.py"))


_cache = None


def load():
    """Returns a namespace with the reference modules: zu, mc, ia, oa, cr, mu."""
    global _cache
    if _cache is not None:
        return _cache
    if not available():
        raise RuntimeError("reference checkout not present at %s" % REF_ROOT)
    saved = {k: v for k, v in sys.modules.items() if k == "multimae" or k.startswith("multimae.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("multimae")
    pkg.__path__ = [MM]
    sys.modules["multimae"] = pkg
    spec = importlib.util.spec_from_file_location("multimae.zorro_utils", os.path.join(DSI_MM, "zorro_utils.py"))
    zu = importlib.util.module_from_spec(spec)
    sys.modules["multimae.zorro_utils"] = zu
    spec.loader.exec_module(zu)
    ns = types.SimpleNamespace(
        zu=zu,
        mu=importlib.import_module("multimae.multimae_utils"),
        cr=importlib.import_module("multimae.criterion"),
        ia=importlib.import_module("multimae.input_adapters"),
        oa=importlib.import_module("multimae.output_adapters_simple"),
        mc=importlib.import_module("multimae.multimae_crossattn"),
    )
    # Leave no `multimae.*` entries behind: the product package has a sub-package of the same name
    # (incomplete_multimodal_fusion_amd.multimae) and tests must never pick up the reference by accident.
    for k in [k for k in sys.modules if k == "multimae" or k.startswith("multimae.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    _cache = ns
    return ns


def build_reference_model(ref, *, dim_tokens, depth, dim_head, heads, image_size, patch_size=16,
                          channels=(("s1", 1), ("s2", 3), ("dem", 1)),
                          decoder_dim=256, decoder_depth=2, decoder_heads=8, drop_path_rate=0.0, decoder_drop_path_rate=0.0):
    """Builds reference adapters + MultiMAE the way pretraining/pretrain_mmae.py:193-246 does,
    with free sizes (the class takes arbitrary dims; the factories only fix presets)."""
    from functools import partial
    T = ref.zu.TokenTypes
    in_domains = [c[0] for c in channels]
    input_adapters = {
        d: ref.ia.PatchedInputAdapter(num_channels=c, stride_level=1, patch_size_full=patch_size,
                                      image_size=image_size)
        for d, c in channels
    }
    output_adapters = {
        d: ref.oa.SpatialOutputAdapter(num_channels=c, stride_level=1, patch_size_full=patch_size,
                                       dim_tokens=decoder_dim, depth=decoder_depth,
                                       num_heads=decoder_heads, use_task_queries=True, task=d,
                                       context_tasks=list(in_domains), use_xattn=True, drop_path_rate=decoder_drop_path_rate)
        for d, c in channels
    }
    input_adapters["fusion"] = ref.ia.FusionInputAdapter(num_channels=1, stride_level=1,
                                                         patch_size_full=patch_size,
                                                         image_size=image_size)
    num_patches = (image_size // patch_size) ** 2
    model = ref.mc.MultiMAE(input_adapters=input_adapters, output_adapters=output_adapters,
                            num_global_tokens=1, dim_tokens=dim_tokens, depth=depth,
                            dim_head=dim_head, heads=heads, ff_mult=4,
                            num_fusion_tokens=num_patches,
                            return_token_types=(T.S1, T.S2, T.DEM, T.FUSION),
                            drop_path_rate=drop_path_rate, norm_layer=ref.zu.LayerNorm)
    return model


_ds_cache = None


def load_downstream():
    """The downstream backbone (downstream/instance_segmentation/modeling/multimae/multimae_big_imcomplete.py, SURVEY 8f
    row f4) with its sibling modules, imported unmodified through a stub package whose __path__ is that directory."""
    global _ds_cache
    if _ds_cache is not None:
        return _ds_cache
    if not available():
        raise RuntimeError("reference checkout not present at %s" % REF_ROOT)
    saved = {k: v for k, v in sys.modules.items() if k == "multimae" or k.startswith("multimae.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("multimae")
    pkg.__path__ = [DSI_MM]
    sys.modules["multimae"] = pkg
    ns = types.SimpleNamespace(
        zu=importlib.import_module("multimae.zorro_utils"),
        ia=importlib.import_module("multimae.input_adapters"),
        big=importlib.import_module("multimae.multimae_big_imcomplete"),
    )
    for k in [k for k in sys.modules if k == "multimae" or k.startswith("multimae.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    _ds_cache = ns
    return ns


def build_downstream_backbone(ds, *, dim_tokens, depth, dim_head, heads, image_size, patch_size=16,
                              channels=(("s1", 1), ("s2", 3), ("dem", 1))):
    """ViTBaseline built the way ViTMAE() does (multimae_big_imcomplete.py:756-797), free sizes, no pretrained file."""
    T = ds.zu.TokenTypes
    ia = {d: ds.ia.PatchedInputAdapter(num_channels=c, stride_level=1, patch_size_full=patch_size, image_size=image_size)
          for d, c in channels}
    ia["fusion"] = ds.ia.FusionInputAdapter(num_channels=1, stride_level=1, patch_size_full=patch_size, image_size=image_size)
    return ds.big.ViTBaseline(input_adapters=ia, output_adapters=None, num_fusion_tokens=(image_size // patch_size) ** 2,
                              return_token_types=(T.S1, T.S2, T.DEM, T.FUSION), drop_path_rate=0.0,
                              dim_tokens=dim_tokens, depth=depth, dim_head=dim_head, heads=heads, ff_mult=4,
                              norm_layer=ds.zu.LayerNorm, in_domains=[c[0] for c in channels], frozen_stages=11,
                              pretrained="/nonexistent")


_aux_cache = None


def load_aux():
    """Reference pieces outside the `multimae` package that the step shell / 4-modality driver use, loaded by file path:
      tb  = pretraining/utils/task_balancing.py        (imports torch only)
      ns  = pretraining/utils/native_scaler.py         (cosine_scheduler; its `from torch._six import inf` needs torch 1.x:
            a placeholder module object named torch._six carrying `inf` is registered for the import and removed again)
      dfc = pretraining/utils/multimodal_dfc2023.py    (normalisation constants / functions; imports rasterio and cv2 at
            the top, both absent here: NEVER-CALLED placeholder module objects are registered for the import only, so
            only the functions that touch neither -- normalization, normalize_rgb/sar/dem -- may be called)
      ia  = pretraining/multimae/input_adapters.py     (SemSegInputAdapter), cr = criterion.py (MaskedCrossEntropyLoss, DINOLoss)
    """
    global _aux_cache
    if _aux_cache is not None:
        return _aux_cache
    ref = load()
    UT = os.path.join(REF_ROOT, "pretraining", "utils")

    def by_path(name, path, placeholders=()):
        added = []
        for mod_name, attrs in placeholders:
            if mod_name not in sys.modules:
                m = types.ModuleType(mod_name)
                for k, v in attrs.items():
                    setattr(m, k, v)
                sys.modules[mod_name] = m
                added.append(mod_name)
        try:
            spec = importlib.util.spec_from_file_location(name, path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            for mod_name in added:
                del sys.modules[mod_name]
        return mod
    ns = types.SimpleNamespace(
        tb=by_path("_ref_task_balancing", os.path.join(UT, "task_balancing.py")),
        ns=by_path("_ref_native_scaler", os.path.join(UT, "native_scaler.py"), [("torch._six", {"inf": float("inf")})]),
        dfc=by_path("_ref_multimodal_dfc2023", os.path.join(UT, "multimodal_dfc2023.py"), [("rasterio", {}), ("cv2", {})]),
        ia=ref.ia, cr=ref.cr)
    _aux_cache = ns
    return ns


_quad_cache = None


def load_quad():
    """The reference's own 4-modality model (pretraining/multimae/multimae_quadruplet.py with zorro_utils_quadruplet.py; what
    pretraining/pretrain_mmae_my.py:35-36 imports), imported unmodified through the stub package of load().
    zorro_utils_quadruplet.py:12-13 imports `beartype` (absent in this image) and never uses it: a placeholder module object
    (identity decorator; beartype.typing = typing) is registered for the import only and removed again."""
    global _quad_cache
    if _quad_cache is not None:
        return _quad_cache
    ref = load()
    import typing
    saved = {k: v for k, v in sys.modules.items() if k == "multimae" or k.startswith("multimae.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("multimae")
    pkg.__path__ = [MM]
    sys.modules["multimae"] = pkg
    sys.modules["multimae.multimae_utils"] = ref.mu
    added = []
    if "beartype" not in sys.modules:
        bt = types.ModuleType("beartype")
        bt.beartype = lambda f: f
        bt.typing = typing
        sys.modules["beartype"], sys.modules["beartype.typing"] = bt, typing
        added = ["beartype", "beartype.typing"]
    try:
        ns = types.SimpleNamespace(zq=importlib.import_module("multimae.zorro_utils_quadruplet"),
                                   mq=importlib.import_module("multimae.multimae_quadruplet"),
                                   ia=ref.ia, oa=ref.oa, cr=ref.cr)
    finally:
        for k in added:
            del sys.modules[k]
        for k in [k for k in sys.modules if k == "multimae" or k.startswith("multimae.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    _quad_cache = ns
    return ns


QUAD_CHANNELS = (("s1", 2), ("s2", 4), ("dem", 1), ("dnw", 9))


def build_reference_quad_model(q, *, dim_tokens, depth, dim_head, heads, image_size, patch_size=16, num_classes=9,
                               dim_class_emb=64, decoder_dim=256, decoder_depth=2, decoder_heads=8):
    """Adapters + multimae_quadruplet.MultiMAE the way pretraining/pretrain_mmae_my.py:46-81, :196-255 builds them
    (s1 2ch, s2 4ch, dem 1ch, dnw class map with a SemSegInputAdapter and a num_classes-channel output adapter), free sizes."""
    T = q.zq.TokenTypes
    doms = [c[0] for c in QUAD_CHANNELS]
    ia = {d: q.ia.PatchedInputAdapter(num_channels=c, stride_level=1, patch_size_full=patch_size, image_size=image_size)
          for d, c in QUAD_CHANNELS[:3]}
    ia["dnw"] = q.ia.SemSegInputAdapter(num_classes=num_classes, dim_class_emb=dim_class_emb, interpolate_class_emb=False,
                                        stride_level=1, patch_size_full=patch_size, image_size=image_size)
    oa = {d: q.oa.SpatialOutputAdapter(num_channels=(num_classes if d == "dnw" else c), stride_level=1,
                                       patch_size_full=patch_size, dim_tokens=decoder_dim, depth=decoder_depth,
                                       num_heads=decoder_heads, use_task_queries=True, task=d, context_tasks=list(doms),
                                       use_xattn=True) for d, c in QUAD_CHANNELS}
    ia["fusion"] = q.ia.FusionInputAdapter(num_channels=1, stride_level=1, patch_size_full=patch_size, image_size=image_size)
    return q.mq.MultiMAE(input_adapters=ia, output_adapters=oa, num_global_tokens=1, dim_tokens=dim_tokens, depth=depth,
                         dim_head=dim_head, heads=heads, ff_mult=4, num_fusion_tokens=(image_size // patch_size) ** 2,
                         return_token_types=(T.S1, T.S2, T.DEM, T.DNW, T.FUSION), drop_path_rate=0.0,
                         norm_layer=q.zq.LayerNorm)
