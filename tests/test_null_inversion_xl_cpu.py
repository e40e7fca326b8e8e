"""Host side of SD-XL null-text inversion and the edit_image_xl command: the recorded oracle run, the parser defaults, the
new exported symbols, the dry-run sizing of the pooled-gradient buffer, the sweep's length check and the refusal to run
without a GPU."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import edit_image_xl as EX
from sliders_conceptmod_amd import null_inversion_xl as NX
from tests import null_inversion_xl_refs as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smi_unet_pooled_grad_bytes", "smi_unet_pooled_grad_attach", "smi_unet_pooled_grad", "smi_unet_backward_cond")


def test_new_symbols_are_declared_exported_and_documented():
    hdr = open(os.path.join(ROOT, "include", "smi.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for s in NEW_SYMBOLS:
        assert s in _native.EXPORTED_SYMBOLS and f"{s}(" in hdr and s in design, s
        assert hasattr(_native.lib(), s)


def _sizes(cfg, sites, shape):
    cc = _native.make_config(cfg, torch.float16)
    arr, _keep = _native.make_sites(sites)
    out = {}
    for fn in ("smi_workspace_bytes", "smi_arena_bytes", "smi_unet_ctx_grad_bytes", "smi_unet_pooled_grad_bytes"):
        v = C.c_size_t(0)
        _native.check(getattr(_native.lib(), fn)(C.byref(cc), arr, len(sites), *shape, C.byref(v)), fn)
        out[fn] = v.value
    w = C.c_size_t(0)
    _native.check(_native.lib().smi_weights_bytes(C.byref(cc), arr, len(sites), C.byref(w)), "smi_weights_bytes")
    out["smi_weights_bytes"] = w.value
    return out


def test_the_sizing_calls_are_dry_runs_that_leave_the_other_sizes_alone():
    import sliders_conceptmod_amd.unet as PU
    from oracle import unet_ref as OU
    cfg = PU.UNetConfig(**dataclasses.asdict(OU.tiny_sdxl_config()))
    big, again, small = _sizes(cfg, [], (2, 2, 16, 16, 77)), _sizes(cfg, [], (2, 2, 16, 16, 77)), _sizes(cfg, [], (1, 1, 8, 8, 77))
    assert big == again  # asking for the pooled size in between changes nothing
    n_temb = sum(2 * p.numel() for n, p in PU.UNet2DConditionModel(cfg).named_parameters() if n.endswith("time_emb_proj.weight"))
    # at least the transposed grouped time_emb_proj copy (16-bit), and a saved-pass arena no smaller than the context's
    assert big["smi_unet_pooled_grad_bytes"] > n_temb
    assert n_temb < small["smi_unet_pooled_grad_bytes"] < big["smi_unet_pooled_grad_bytes"]
    assert small["smi_weights_bytes"] == big["smi_weights_bytes"]
    # an SD-1.x UNet has no pooled embedding: an error that says so, not a size
    cfg1 = PU.UNetConfig(**dataclasses.asdict(OU.tiny_sd1x_config()))
    cc = _native.make_config(cfg1, torch.float16)
    arr, _keep = _native.make_sites([])
    v = C.c_size_t(0)
    with pytest.raises(_native.SmiError, match="no added conditioning"):
        _native.check(_native.lib().smi_unet_pooled_grad_bytes(C.byref(cc), arr, 0, 2, 2, 16, 16, 77, C.byref(v)), "bytes")


def test_recorded_oracle_run_is_reproducible():
    """The first timestep of tests/golden/null_inversion_xl_oracle.json, recomputed, with the pooled optimisation on and off."""
    from tests.ctx_grad_refs import plain_oracle
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", N.GOLDEN)))
    ou = plain_oracle(N.MODEL)
    args = N.recipe(ou.cfg.cross_attention_dim, N.pooled_dim(ou.cfg))
    for key, on in (("losses_pooled_off", False), ("losses_pooled_on", True)):
        losses, ts = N.oracle_null_optimization(ou, *args, optimize_pooled=on, only_first=True)
        assert ts == golden["timesteps"][:1]
        np.testing.assert_allclose(losses[0], golden[key][0], rtol=1e-4)
        assert len(golden[key]) == N.STEPS and all(len(l) == N.INNER for l in golden[key])
    off, on = golden["losses_pooled_off"], golden["losses_pooled_on"]
    assert off[0][0] == on[0][0]  # the first step starts from the same embeddings
    gap = (off[0][-1] - on[0][-1]) / off[0][-1]
    print(f"first timestep, last loss: pooled off {off[0][-1]:.4f} on {on[0][-1]:.4f} ({100 * gap:.1f} % lower)")
    assert gap > 0.03
    assert all(b[-1] < a[-1] for a, b in zip(off, on))


def test_parser_defaults():
    a = EX.build_parser().parse_args(["--image", "a.jpg", "--prompt", "p", "--model_name", "m.pt", "--save_path", "o"])
    assert (a.scales, a.start_noise, a.ddim_steps, a.guidance_scale, a.num_inner_steps, a.early_stop_epsilon) == \
        ("0,2,4", 500, 50, 7.5, 10, 1e-5)
    assert a.offsets == "0,0,0,0" and a.vae_dtype is None and not a.unfused and not a.no_null_pooled
    assert a.image_size == 1024 and a.pretrained_model == "synthetic://sdxl" and not hasattr(a, "base")
    assert EX.parse_offsets("1, 2,3,4") == (1, 2, 3, 4)
    with pytest.raises(ValueError, match="cuda"):
        EX.edit(EX.build_parser().parse_args(["--image", "a", "--prompt", "p", "--model_name", "m", "--save_path", "o",
                                              "--device", "cpu"]))


def test_old_refusals_name_the_new_class_and_command():
    from sliders_conceptmod_amd import edit_image as E
    with pytest.raises(ValueError, match="SD-1.x") as ei:
        E.edit(E.build_parser().parse_args(["--image", "a", "--prompt", "p", "--model_name", "m", "--save_path", "o",
                                            "--base", "xl"]))
    assert "edit_image_xl" in str(ei.value)


class _Sched:
    def __init__(self, n):
        self.n = n

    def set_timesteps(self, n):
        self.timesteps = torch.arange(n)


def test_sweep_refuses_a_pooled_list_of_the_wrong_length():
    from sliders_conceptmod_amd import train_util as TU
    te, lat = torch.zeros(2, 77, 8), torch.zeros(1, 4, 8, 8)
    added = (torch.zeros(2, 8), torch.zeros(2, 6))
    unconds = [te[:1]] * 4
    with pytest.raises(ValueError, match="unconditional pooled embeddings for 4 steps"):
        TU.slider_sweep_latents(None, None, _Sched(4), lat, te, 1.0, 500, 7.5, 4, added_cond=added, uncond_per_step=unconds,
                                uncond_pooled_per_step=[added[0][:1]] * 3)
    with pytest.raises(ValueError, match="goes with uncond_per_step and added_cond"):
        TU.slider_sweep_latents(None, None, _Sched(4), lat, te, 1.0, 500, 7.5, 4, added_cond=added,
                                uncond_pooled_per_step=[added[0][:1]] * 4)


def test_null_inversion_xl_needs_the_gpu():
    import sliders_conceptmod_amd.unet as PU
    from oracle import unet_ref as OU
    from tests.null_inversion_refs import ddim_scheduler
    unet = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(OU.tiny_sdxl_config()))).half()
    with pytest.raises(_native.SmiError, match="runs only on an MI355X"):
        NX.NullInversionXL(unet, ddim_scheduler())
