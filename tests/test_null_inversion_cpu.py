"""Host side of null-text inversion and the edit_image command: exported symbols, argument parsing, output paths, load_512
against a NumPy restatement, the DDIM step coefficients against the notebook's formulas, the recorded oracle run, and the
refusal to run without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import edit_image as E
from sliders_conceptmod_amd import null_inversion as NI
from tests import null_inversion_refs as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smi_unet_ctx_grad_bytes", "smi_unet_ctx_grad_attach", "smi_unet_ctx_grad", "smi_unet_backward_ctx",
               "smi_nulltext_loss", "smi_op_cast_f32")


def test_new_symbols_are_declared_exported_and_documented():
    hdr = open(os.path.join(ROOT, "include", "smi.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for s in NEW_SYMBOLS:
        assert s in _native.EXPORTED_SYMBOLS and f"{s}(" in hdr and s in design, s
        assert hasattr(_native.lib(), s)


def test_ctx_grad_sizing_is_a_dry_run_and_leaves_the_other_sizes_alone():
    import ctypes as C
    import dataclasses
    import sliders_conceptmod_amd.unet as PU
    from oracle import unet_ref as OU
    cfg = PU.UNetConfig(**dataclasses.asdict(OU.tiny_sd1x_config()))
    cc = _native.make_config(cfg, torch.float16)
    arr, _keep = _native.make_sites([])
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_unet_ctx_grad_bytes(C.byref(cc), arr, 0, 2, 2, 16, 16, 77, C.byref(out)), "bytes")
    n_kv = sum(2 * p.numel() for n, p in PU.UNet2DConditionModel(cfg).named_parameters()
               if ".attn2.to_k." in n or ".attn2.to_v." in n)
    assert out.value > n_kv  # at least the transposed k|v copy (16-bit)
    small = C.c_size_t(0)
    _native.check(_native.lib().smi_unet_ctx_grad_bytes(C.byref(cc), arr, 0, 1, 1, 8, 8, 77, C.byref(small)), "bytes")
    assert n_kv < small.value < out.value


def test_parser_defaults_and_helpers():
    a = E.build_parser().parse_args(["--image", "a.jpg", "--prompt", "p", "--model_name", "m.pt", "--save_path", "o"])
    assert (a.scales, a.start_noise, a.ddim_steps, a.guidance_scale, a.num_inner_steps, a.early_stop_epsilon) == \
        ("0,2,4", 500, 50, 7.5, 10, 1e-5)
    assert a.offsets == "0,0,0,0" and a.vae_dtype is None and a.base == "1.4" and not a.unfused
    assert E.parse_offsets("1, 2,3,4") == (1, 2, 3, 4)
    for bad in ("1,2,3", "1,2,3,-4"):
        with pytest.raises(ValueError):
            E.parse_offsets(bad)
    rec, per, strip = E.output_paths("out", "age", [0, 0.5, 2], "/x/y/photo.jpeg")
    assert rec == os.path.join("out", "age", "reconstruction.png")
    assert per == [os.path.join("out", "age", d, "photo.png") for d in ("0", "half", "2")]
    assert strip == os.path.join("out", "age", "all", "photo.png")
    with pytest.raises(ValueError, match="SD-1.x"):
        E.edit(E.build_parser().parse_args(["--image", "a", "--prompt", "p", "--model_name", "m", "--save_path", "o",
                                            "--base", "xl"]))


def numpy_load(image, left, right, top, bottom, size):
    """load_512 restated: the offset clamps, the crop, the centre square, then PIL's default resize"""
    from PIL import Image
    h, w, _ = image.shape
    left = min(left, w - 1)
    right = min(right, w - left - 1)
    top = min(top, h - left - 1)
    bottom = min(bottom, h - top - 1)
    image = image[top:h - bottom, left:w - right]
    h, w, _ = image.shape
    s = min(h, w)
    oy, ox = (h - s) // 2, (w - s) // 2
    return np.array(Image.fromarray(np.ascontiguousarray(image[oy:oy + s, ox:ox + s])).resize((size, size)))


@pytest.mark.parametrize("shape,offsets", [((48, 80), (0, 0, 0, 0)), ((80, 48), (3, 5, 7, 2)), ((64, 64), (10, 0, 0, 20)),
                                           ((40, 40), (100, 100, 100, 100))])
def test_load_512(tmp_path, shape, offsets):
    from PIL import Image
    img = np.random.default_rng(1).integers(0, 256, shape + (4,), dtype=np.uint8)  # RGBA: the alpha plane is dropped
    want = numpy_load(img[:, :, :3], *offsets, 32)
    assert np.array_equal(NI.load_512(img[:, :, :3], *offsets, size=32), want) and want.shape == (32, 32, 3)
    Image.fromarray(img).save(tmp_path / "a.png")
    assert np.array_equal(NI.load_512(str(tmp_path / "a.png"), *offsets, size=32), want)
    assert NI.load_512(img[:, :, :3]).shape == (512, 512, 3)


def test_step_coefficients_are_the_notebooks_next_and_prev_step():
    s = N.ddim_scheduler(50)
    a = s.alphas_cumprod.double()
    x, e = torch.randn(7, dtype=torch.float64), torch.randn(7, dtype=torch.float64)
    for t in (981, 501, 1, 0):
        # prev_step
        pt = t - 1000 // 50
        a_t, a_p = a[t], (a[pt] if pt >= 0 else s.final_alpha_cumprod.double())
        want = a_p ** 0.5 * (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5 + (1 - a_p) ** 0.5 * e
        cx, ce = NI.step_coefficients(s, t, False)
        torch.testing.assert_close(cx * x + ce * e, want, rtol=1e-12, atol=1e-12)
        # next_step
        ct = min(t - 1000 // 50, 999)
        a_c, a_n = (a[ct] if ct >= 0 else s.final_alpha_cumprod.double()), a[t]
        want = a_n ** 0.5 * (x - (1 - a_c) ** 0.5 * e) / a_c ** 0.5 + (1 - a_n) ** 0.5 * e
        cx, ce = NI.step_coefficients(s, t, True)
        torch.testing.assert_close(cx * x + ce * e, want, rtol=1e-12, atol=1e-12)


def test_recorded_oracle_run_is_reproducible():
    """The first timestep of tests/golden/null_inversion_oracle.json, recomputed (the whole run takes four times as long)."""
    from tests.ctx_grad_refs import plain_oracle
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", N.GOLDEN)))
    ou = plain_oracle("tiny_sd1x")
    losses, ts = N.oracle_null_optimization(ou, *N.recipe(ou.cfg.cross_attention_dim), only_first=True)
    assert ts == golden["timesteps"][:1]
    np.testing.assert_allclose(losses[0], golden["losses"][0], rtol=1e-4)
    falls = [(l[0] - l[-1]) / l[0] for l in golden["losses"]]
    assert all(f > 0.01 for f in falls[:3]) and 0 < falls[3] < 0.01


def test_null_inversion_needs_the_gpu():
    import dataclasses
    import sliders_conceptmod_amd.unet as PU
    from oracle import unet_ref as OU
    unet = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(OU.tiny_sd1x_config()))).half()
    with pytest.raises(_native.SmiError, match="runs only on an MI355X"):
        NI.NullInversion(unet, N.ddim_scheduler())


def test_the_inversion_loops_are_defined_once():
    """NullInversionXL reuses NullInversion's loops: a second definition in either module is the fork coming back."""
    import ast
    import inspect
    from sliders_conceptmod_amd import null_inversion_xl as NX
    names = ("_null_optimization_fused", "_null_optimization_autograd", "ddim_loop", "image2latent", "latent2image")
    defined = [n.name for mod in (NI, NX) for n in ast.walk(ast.parse(inspect.getsource(mod)))
               if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
    for name in names:
        assert defined.count(name) == 1, f"def {name}: {defined.count(name)} definitions"
        assert getattr(NX.NullInversionXL, name) is getattr(NI.NullInversion, name)
