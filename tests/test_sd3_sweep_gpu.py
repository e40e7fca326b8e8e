"""The SD3 sweep on a real MI355X: predict_noise_sd3 / diffusion_sd3 on tiny_sd3 against the restated loop of
tests/mmdit_refs.py, the 16-channel VAE decoder without post_quant_conv against the existing decoder reference, and the
`generate_images --base sd3` command on synthetic://tiny_sd3."""
import os

import numpy as np
import pytest
import torch

import mmdit_refs as R
import vae_decoder_ref as VR

pytestmark = pytest.mark.gpu


def test_diffusion_sd3_against_the_restated_loop():
    """Four CFG steps; the bar is 2 x the distance of the storage-dtype twin's loop from the float64 loop, on the same inputs."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import mmdit as M
    from sliders_conceptmod_amd import model_util as MU
    from sliders_conceptmod_amd import train_util as TU
    dt = torch.float16
    cfg = M.tiny_sd3_config()
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=3)
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(2, 16, 8, 6, generator=g)
    u, c = torch.randn(1, 9, 64, generator=g).to(dt), torch.randn(1, 9, 64, generator=g).to(dt)
    up, cp = torch.randn(1, 64, generator=g).to(dt), torch.randn(1, 64, generator=g).to(dt)
    te, pooled = TU.concat_embeddings_sd3(u, c, 2), TU.concat_embeddings_sd3(up, cp, 2)
    sd = {k: v.to(dt) for k, v in model.state_dict().items()}

    def loop(twin):
        fn = lambda x2, t: R.forward(sd, cfg, x2, [t] * x2.shape[0], te, pooled, dt=twin)
        return R.sweep_loop(fn, lat, 4, 5.0)
    ref = loop(None)
    bar = 2.0 * R.rel_l2(loop(dt), ref)
    sched = MU.FlowMatchEulerDiscreteScheduler()
    sched.set_timesteps(4)
    model = model.to("cuda", dt)
    got = TU.diffusion_sd3(model, sched, lat.cuda(), te.cuda(), pooled.cuda(), guidance_scale=5.0)
    err = R.rel_l2(got.cpu(), ref)
    print(f"diffusion_sd3, 4 steps: rel-L2 {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    # one step returns the stepped latents; start / total select the slice
    one = TU.predict_noise_sd3(model, sched, sched.timesteps[0], lat.cuda(), te.cuda(), pooled.cuda(), guidance_scale=5.0)
    rest = TU.diffusion_sd3(model, sched, one, te.cuda(), pooled.cuda(), guidance_scale=5.0, start_timesteps=1, total_timesteps=4)
    assert torch.equal(rest, got)


# the bars of the 4-channel decoder at this tiny configuration (tests/test_vae_decoder_gpu.py TINY_BARS): the network is the
# same but for conv_in reading 16 instead of 4 of its 64 padded input channels, and one 1x1 mix fewer
VAE_BARS = {torch.float16: 2.4e-3, torch.bfloat16: 2.0e-2}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vae_decoder_16_channels_without_post_quant_conv(dtype):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import vae as PV
    from sliders_conceptmod_amd import vae_decoder as PD
    cfg = PV.VAEConfig(latent_channels=16, block_out_channels=(64, 128, 128, 128), norm_num_groups=16, scaling_factor=1.5305,
                       shift_factor=0.0609, use_post_quant_conv=False)
    ref = VR.init_synthetic_(VR.AutoencoderKLDecoderRef(cfg), seed=7).eval()
    d = PD.AutoencoderKLDecoder(cfg)
    assert not any(k.startswith("post_quant_conv") for k in d.state_dict())
    d.load_state_dict({k: v for k, v in ref.state_dict().items() if not k.startswith("post_quant_conv")})
    d = d.to("cuda", dtype).requires_grad_(False).eval()
    z = torch.randn(2, 16, 4, 4, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = ref.decoder(z)  # no post_quant_conv
    got = d.decode(z.cuda()).sample
    err = float((got.cpu() - want).norm() / want.norm())
    print(f"16-channel decoder {dtype}: rel-L2 {err:.3e}, bar {VAE_BARS[dtype]:.1e}")
    assert tuple(got.shape) == (2, 3, 32, 32) and err <= VAE_BARS[dtype]
    rgb = d.decode_to_uint8(z.cuda())
    assert torch.equal(rgb.cpu(), VR.to_uint8(got.cpu()))


def test_generate_images_sd3_command(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from PIL import Image
    from sliders_conceptmod_amd import generate_images as G
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import model_util as MU
    _t, _e, model, _s = MU.load_models_sd3("synthetic://tiny_sd3")
    torch.manual_seed(2)
    net = L.LoRANetwork(model, rank=4, alpha=4.0, train_method="full")  # the four projections the reference's class adapts
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0, 0.5)
    slider, zeroed = tmp_path / "age_sd3.pt", tmp_path / "zeroed" / "age_sd3.pt"
    net.save_weights(slider, torch.float32)
    with torch.no_grad():
        net.flat[net._n_down:].zero_()
    os.makedirs(zeroed.parent)
    net.save_weights(zeroed, torch.float32)
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\na portrait of a dog,12,1\n")
    common = ["--prompts_path", str(prompts), "--pretrained_model", "synthetic://tiny_sd3", "--base", "sd3", "--image_size",
              "64", "--num_samples", "1", "--ddim_steps", "3", "--t5_tokens", "3", "--start_noise", "900"]
    G.main(["--model_name", str(slider), "--save_path", str(tmp_path / "out"), "--scales=-2,0,2"] + common)
    folder = tmp_path / "out" / "age_sd3"
    for case in (0, 1):
        for d in ("-2", "0", "2", "all"):
            assert (folder / d / f"{case}_0.png").exists()
    assert Image.open(folder / "all" / "0_0.png").size == (3 * 64, 64)
    G.main(["--model_name", str(zeroed), "--save_path", str(tmp_path / "out0"), "--scales=2"] + common)
    img = lambda p: np.asarray(Image.open(p))
    for case in (0, 1):
        base = img(tmp_path / "out0" / "age_sd3" / "2" / f"{case}_0.png")
        assert np.array_equal(img(folder / "0" / f"{case}_0.png"), base), "scale 0 == a sweep with lora_up zeroed"
        assert not np.array_equal(img(folder / "2" / f"{case}_0.png"), base)
        assert not np.array_equal(img(folder / "2" / f"{case}_0.png"), img(folder / "-2" / f"{case}_0.png"))
