"""The Flux sweep on a real MI355X: diffusion_flux on tiny_flux against the restated loop of tests/flux_refs.py, and the
`generate_images --base flux` command on synthetic://tiny_flux."""
import numpy as np
import pytest
import torch

import flux_refs as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dynamic", [False, True], ids=["static_shift", "dynamic_shift"])
def test_diffusion_flux_against_the_restated_loop(dynamic):
    """Four steps, one transformer pass each; the bar is 2 x the distance of the storage-dtype twin's loop from the float64
    loop, on the same inputs (the accumulation of tests/test_sd3_sweep_gpu.py).  dynamic: a guidance_embeds model under the
    scheduler's exponential shift (FLUX.1-dev's kind), else the schnell kind."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import model_util as MU
    from sliders_conceptmod_amd import train_util as TU
    dt = torch.float16
    cfg = M.tiny_flux_config(guidance_embeds=dynamic)
    model = M.init_synthetic_(M.FluxTransformer2DModel(cfg), seed=3)
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(2, 16, 8, 6, generator=g)
    te = torch.randn(1, 9, 64, generator=g).to(dt).repeat(2, 1, 1)
    pooled = torch.randn(1, 32, generator=g).to(dt).repeat(2, 1)
    sd = {k: v.to(dt) for k, v in model.state_dict().items()}
    sched = MU.FlowMatchEulerDiscreteScheduler(1000, 3.0 if dynamic else 1.0, use_dynamic_shifting=dynamic)
    mu = F.calculate_shift(4 * 3) if dynamic else None
    gs = [3.5, 3.5] if dynamic else None

    def loop(twin):
        fn = lambda x, t: F.forward(sd, cfg, x, [t] * x.shape[0], gs, te, pooled, dt=twin)
        return F.sweep_loop(fn, lat, 4, mu=mu)
    ref = loop(None)
    bar = 2.0 * F.rel_l2(loop(dt), ref)
    model = model.to("cuda", dt)
    got = TU.diffusion_flux(None, model, sched, lat.cuda(), te.cuda(), pooled.cuda(), guidance_scale=3.5, num_inference_steps=4)
    err = F.rel_l2(got.cpu(), ref)
    print(f"diffusion_flux ({'dynamic' if dynamic else 'static'} shift), 4 steps: rel-L2 {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    # one step returns the stepped latents; start / total select the slice
    one = TU.predict_noise_flux(None, model, sched, sched.timesteps[0], lat.cuda(), te.cuda(), pooled.cuda(), guidance_scale=3.5)
    rest = TU.diffusion_flux(None, model, sched, one, te.cuda(), pooled.cuda(), guidance_scale=3.5, start_timesteps=1,
                             total_timesteps=4, num_inference_steps=4)
    assert torch.equal(rest, got)


def test_generate_images_flux_command(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from PIL import Image
    from sliders_conceptmod_amd import generate_images as G
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import model_util as MU
    _t, _e, model, _s = MU.load_models_flux("synthetic://tiny_flux")
    torch.manual_seed(2)
    net = L.LoRANetwork(model, rank=4, alpha=4.0, delimiter="-", train_method="full")  # the reference trainer's module set and keys
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0, 0.5)
    slider = tmp_path / "age_flux.pt"
    net.save_weights(slider, torch.float32)
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\na portrait of a dog,12,1\n")
    common = ["--prompts_path", str(prompts), "--pretrained_model", "synthetic://tiny_flux", "--base", "flux", "--image_size",
              "64", "--num_samples", "1", "--ddim_steps", "3", "--t5_tokens", "5", "--start_noise", "900"]
    G.main(["--model_name", str(slider), "--save_path", str(tmp_path / "out"), "--scales=-2,0,2"] + common)
    folder = tmp_path / "out" / "age_flux"
    for case in (0, 1):
        for d in ("-2", "0", "2", "all"):
            assert (folder / d / f"{case}_0.png").exists()
    assert Image.open(folder / "all" / "0_0.png").size == (3 * 64, 64)
    G.main(["--save_path", str(tmp_path / "out0"), "--scales=0"] + common)  # no slider file: the frozen network
    img = lambda p: np.asarray(Image.open(p))
    for case in (0, 1):
        base = img(tmp_path / "out0" / "frozen" / "0" / f"{case}_0.png")
        assert np.array_equal(img(folder / "0" / f"{case}_0.png"), base), "scale 0 == a sweep without the file"
        assert not np.array_equal(img(folder / "2" / f"{case}_0.png"), base)
        assert not np.array_equal(img(folder / "2" / f"{case}_0.png"), img(folder / "-2" / f"{case}_0.png"))
