"""`python -m sliders_conceptmod_amd.compose_images` end to end on the synthetic tiny SD-1.x model: two LoRA files written by
LoRANetwork.save_weights, a 2 x 2 grid of scales, the files it writes, and the (0, 0) cell against `generate_images` of slider
A alone at scale 0 (a row of zero multipliers is the adaptor-off pass bit for bit, tests/test_compose_engine_gpu.py)."""
import csv

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODEL = "tiny_sd1x"


def save_lora(path, seed, method, rank):
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    _, _, unet, _ = MU.load_models(f"synthetic://{MODEL}")
    torch.manual_seed(seed)
    net = L.LoRANetwork(unet, rank=rank, multiplier=1.0, alpha=1.0, train_method=method)
    with torch.no_grad():
        net.flat_up.copy_(torch.randn(net.flat_up.shape, generator=torch.Generator().manual_seed(seed)) * 0.05)
    net.save_weights(str(path))
    return path


def test_compose_images_cli(tmp_path):
    from PIL import Image
    from sliders_conceptmod_amd import compose_images as CI
    from sliders_conceptmod_amd import generate_images as G
    prompts = tmp_path / "prompts.csv"
    with open(prompts, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["prompt", "evaluation_seed", "case_number"])
        w.writerow(["a photo of a person", 42, 3])
    a = save_lora(tmp_path / "age.pt", 1, "noxattn", 4)
    b = save_lora(tmp_path / "smile.pt", 2, "xattn", 8)
    common = ["--prompts_path", str(prompts), "--pretrained_model", f"synthetic://{MODEL}", "--base", "1.4",
              "--image_size", "64", "--num_samples", "1", "--ddim_steps", "4"]
    out = tmp_path / "grid"
    CI.main(["--model_name", str(a), "--model_name", str(b), "--scales=0,2", "--scales=0,2", "--save_path", str(out)] + common)
    cells = [(0, 0), (0, 2), (2, 0), (2, 2)]
    imgs = {}
    for sa, sb in cells:
        p = out / "age+smile" / f"{sa}_{sb}" / "3_0.png"
        assert p.exists(), p
        imgs[sa, sb] = np.asarray(Image.open(p))
        assert imgs[sa, sb].shape == (64, 64, 3)
    for i, c in enumerate(cells):
        for d in cells[i + 1:]:
            assert not np.array_equal(imgs[c], imgs[d]), (c, d)
    # all/: the 2-D grid, rows slider A, columns slider B
    grid = np.asarray(Image.open(out / "age+smile" / "all" / "3_0.png"))
    assert grid.shape == (128, 128, 3)
    for (sa, sb) in cells:
        y, x = 64 * (sa // 2), 64 * (sb // 2)
        assert np.array_equal(grid[y:y + 64, x:x + 64], imgs[sa, sb])
    # (0, 0) = generate_images of slider A at scale 0, same seed
    single = tmp_path / "single"
    G.main(["--model_name", str(a), "--scales=0", "--save_path", str(single)] + common)
    want = np.asarray(Image.open(single / "age" / "0" / "3_0.png"))
    assert np.array_equal(imgs[0, 0], want)
