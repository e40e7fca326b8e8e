"""`python -m sliders_conceptmod_amd.generate_images` end to end on the synthetic tiny SD-1.x / SD-XL models: the PNG files
it writes, their pixels against `decode_to_uint8(slider_sweep_latents(...))` recomputed through the API in the eval
scripts' draw order (E/generate_images_sd1.py:145-200), and what the slider scale does to them."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALES = (-1, 0, 1)


def save_lora(model, path, seed):
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    _, _, unet, _ = MU.load_models(f"synthetic://{model}", xl=model.endswith("xl"))
    torch.manual_seed(seed)
    net = L.LoRANetwork(unet, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn")
    with torch.no_grad():
        net.flat_up.copy_(torch.randn(net.flat_up.shape, generator=torch.Generator().manual_seed(seed)) * 0.05)
    net.save_weights(str(path))
    return path


def run_cli(model, lora, prompts, out):
    from sliders_conceptmod_amd import generate_images as G
    G.main(["--model_name", str(lora), "--prompts_path", str(prompts), "--save_path", str(out),
            "--pretrained_model", f"synthetic://{model}", "--base", "xl" if model.endswith("xl") else "1.4",
            "--image_size", "64", "--num_samples", "2", "--ddim_steps", "3", "--scales=" + ",".join(map(str, SCALES))])


def recompute(model, lora, prompt, seed):
    """The eval loop through the public API, written out: the expected uint8 images [scale][n, h, w, 3]."""
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    from sliders_conceptmod_amd import train_util as TU
    xl = model.endswith("xl")
    _, enc, unet, sched = MU.load_models(f"synthetic://{model}", "ddim" if xl else "lms", xl=xl)
    unet = unet.to("cuda", torch.float16).requires_grad_(False).eval()
    net = L.LoRANetwork(unet, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn").to("cuda")
    net.load_state_dict(torch.load(str(lora), weights_only=True))
    vae = MU.load_vae_decoder(f"synthetic://{model}", xl=xl).to("cuda", torch.bfloat16 if xl else torch.float16)
    if xl:
        c, u = enc.encode(prompt), enc.encode("")
        te = TU.concat_embeddings(u[0], c[0], 2).to("cuda", torch.float16)
        pooled = TU.concat_embeddings(u[1], c[1], 2).to("cuda", torch.float16)
        added = (pooled, TU.get_add_time_ids(64, 64).to("cuda").repeat(4, 1))
    else:
        te = TU.concat_embeddings(enc.encode(""), enc.encode(prompt), 2).to("cuda", torch.float16)
        added = None
    out = []
    for scale in SCALES:
        sched.set_timesteps(3)
        g = torch.manual_seed(seed)
        lat = torch.randn((2, 4, 8, 8), generator=g) * sched.init_noise_sigma
        lat = TU.slider_sweep_latents(unet, net, sched, lat.cuda(), te, scale, 750 if xl else 850, 7.5, 3, added_cond=added)
        out.append(vae.decode_to_uint8(lat.float() / vae.config.scaling_factor).cpu().numpy())
    return out


@pytest.mark.parametrize("model", ["tiny_sd1x", "tiny_sdxl"])
def test_generate_images_cli(tmp_path, model):
    from PIL import Image
    prompts = tmp_path / "prompts.csv"
    with open(prompts, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["prompt", "evaluation_seed", "case_number"])
        w.writerow(["a photo of a person", 42, 0])
        w.writerow(["a dog, running", 7, 1])
    loras = [save_lora(model, tmp_path / f"lora{i}.pt", seed) for i, seed in enumerate((1, 2))]
    outs = [tmp_path / "out0", tmp_path / "out1"]
    for lora, out in zip(loras, outs):
        run_cli(model, lora, prompts, out)
    imgs = {}
    for k, (lora, out) in enumerate(zip(loras, outs)):
        name = os.path.splitext(os.path.basename(lora))[0]
        for case, (prompt, seed) in enumerate((("a photo of a person", 42), ("a dog, running", 7))):
            want = recompute(model, lora, prompt, seed) if k == 0 or case == 0 else None
            for num in range(2):
                for i, s in enumerate(SCALES):
                    p = out / name / str(s) / f"{case}_{num}.png"
                    assert p.exists(), p
                    a = np.asarray(Image.open(p))
                    assert a.shape == (64, 64, 3)
                    imgs[(k, case, num, s)] = a
                    if want is not None:
                        assert np.array_equal(a, want[i][num]), (k, case, num, s)
                strip = np.asarray(Image.open(out / name / "all" / f"{case}_{num}.png"))
                assert strip.shape == (64, 64 * len(SCALES), 3)
                assert np.array_equal(strip[:, 64:128], imgs[(k, case, num, 0)])
    for case in range(2):
        for num in range(2):
            # scale 0: the adaptor is off throughout -- the LoRA file must not matter; +-1: it must
            assert np.array_equal(imgs[(0, case, num, 0)], imgs[(1, case, num, 0)])
            for s in (-1, 1):
                assert not np.array_equal(imgs[(0, case, num, s)], imgs[(1, case, num, s)])
                assert not np.array_equal(imgs[(0, case, num, s)], imgs[(0, case, num, 0)])
