"""Strengthening of the oracle pin: the oracle against a run of the ACTUAL reference on a seeded configuration that the
other fixtures do not cover (3 encoder layers of width 16 with 2 heads of 8, 2 decoder layers of width 8 with 2 heads, 32 x 32
tiles in 8 x 8 patches, every trainable parameter drawn at random), and against the reference's own generate_random_masks for
20 seeds.  oracle/make_golden.py (gen_vs_reference) recorded what the reference computed -- outputs, loss, gradients, mask
draws -- and its fixed buffers in tests/golden/vs_reference.npz; the parameters, inputs and masks it ran on are redrawn here
by the same seeded vsref_inputs()."""
import json

import torch

from oracle import mmae_oracle as O
from oracle.make_golden import vsref_inputs
from tests.conftest import Golden


def test_random_config_forward_backward_matches_reference():
    g = Golden("vs_reference.npz")
    cfg = g.json("config")
    state, x, masks = vsref_inputs(g.json("layout"))
    state.update(g.sub("buffer"))
    N = cfg["N"]
    p = {k: v.clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("pos_emb") and not k.endswith("beta"))
         for k, v in state.items()}
    out_o, (tl_o, lc_o, loss_o) = O.train_step_loss(p, x, masks, N, cfg["heads"], cfg["decoder_heads"], cfg["patch_size"])
    loss_o.backward()
    loss = float(g.t("loss"))
    assert abs(loss - float(loss_o)) < 1e-5 * max(1.0, abs(loss))
    for d in O.DOMAINS:
        assert torch.allclose(g.t("pred/" + d), out_o[0][d], atol=2e-5)
    for i in (2, 3, 4, 5, 6, 7):
        assert torch.allclose(g.t("out/%d" % i), out_o[i], atol=2e-5), i
    for name in g.json("no_grad"):
        assert p[name].grad is None, name
    names = g.json("grad_names")
    grads = torch.split(g.t("grads"), [p[n].numel() for n in names])
    assert sum(t.numel() for t in grads) == g.t("grads").numel()
    for name, grad in zip(names, grads):
        assert torch.allclose(grad.view_as(p[name]), p[name].grad, atol=3e-5, rtol=1e-4), name
    assert len(names) > 100


def test_random_mask_draws_match_reference_rng_order():
    """Same seed -> the oracle's injected-draw bookkeeping reproduces generate_random_masks of the reference."""
    from torch.distributions.dirichlet import Dirichlet
    g = Golden("vs_reference.npz")
    P, N, B = (int(v) for v in g.z["draws_shape"])
    ref = {k: v.long() for k, v in g.sub("draws").items()}
    assert ref["task_mask"].shape[0] == 20
    for seed in range(20):
        torch.manual_seed(seed)
        d = Dirichlet(torch.Tensor([1.0] * 3)).sample((1,))
        noise = torch.stack([torch.rand(1, P) for _ in range(3)], dim=1)
        na = torch.rand(1, 3 * P)
        mask_all, k, r = O.masks_from_draws(d, noise, na, N)
        assert torch.equal(mask_all.repeat(B, 1), ref["task_mask"][seed])
        assert torch.equal(k.repeat(B, 1), ref["ids_keep"][seed]) and torch.equal(r.repeat(B, 1), ref["ids_restore"][seed])
