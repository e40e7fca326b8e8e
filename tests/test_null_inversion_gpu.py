"""Null-text inversion on the engine (sliders_conceptmod_amd/null_inversion.py): the fused route and the autograd route
against the recorded CPU oracle run of the same recipe (tests/null_inversion_refs.py, tests/golden/null_inversion_oracle.json:
tiny_sd1x, 8 x 8 latents, 4 DDIM steps, 5 inner steps, early stop disabled, guidance 7.5, seeded embeddings), the per-step
unconditional embeddings in slider_sweep_latents, and the `edit_image` command end to end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctx_grad_refs as R
from tests import null_inversion_refs as N

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", N.GOLDEN)))


def make_inversion(fused, dtype=torch.float16):
    from sliders_conceptmod_amd.null_inversion import NullInversion
    ocfg, _ou, pu = R.build_plain_pair("tiny_sd1x", dtype)
    inv = NullInversion(pu, N.ddim_scheduler(), num_ddim_steps=N.STEPS, guidance_scale=N.GUIDANCE, fused=fused)
    x0, uncond, cond = N.recipe(ocfg.cross_attention_dim)
    inv.context = torch.cat([uncond, cond]).cuda()
    return inv, x0.cuda()


_RUNS = {}


def run(fused, fresh=False):
    """(losses, embeddings, timesteps) of one route on the recipe; computed once and left unchanged (fresh: a run of its
    own, not kept)"""
    if fresh or fused not in _RUNS:
        inv, x0 = make_inversion(fused)
        latents = inv.ddim_loop(x0)
        assert len(latents) == N.STEPS + 1
        embs = inv.null_optimization(latents, N.INNER, N.NO_EARLY_STOP)
        got = (inv.losses, embs, [int(t) for t in inv.scheduler.timesteps])
        if fresh:
            return got
        _RUNS[fused] = got
    return _RUNS[fused]


@pytest.mark.parametrize("fused", [True, False])
def test_losses_fall_where_the_reference_falls(fused):
    losses, embs, ts = run(fused)
    assert ts == GOLDEN["timesteps"] and len(losses) == N.STEPS and len(embs) == N.STEPS
    falling = []
    for t, got, ref in zip(ts, losses, GOLDEN["losses"]):
        print(f"fused={fused} t={t}: engine {['%.5f' % v for v in got]}")
        print(f"fused={fused} t={t}: oracle {['%.5f' % v for v in ref]}")
        assert len(got) == N.INNER and all(np.isfinite(got))
        if (ref[0] - ref[-1]) / ref[0] > 0.01:
            falling.append(t)
            assert got[-1] < got[0], f"t={t}: loss {got[0]:.5f} -> {got[-1]:.5f} does not fall (oracle {ref[0]:.5f} -> {ref[-1]:.5f})"
    assert falling == ts[:3]  # the last timestep moves by 0.15 % in the reference: nothing is asserted on it
    for e in embs:
        assert e.shape == (1, 77, 64) and e.dtype == torch.float32 and torch.isfinite(e).all()
    assert not torch.equal(embs[0], embs[1])


def test_routes_agree_on_the_first_loss():
    """Same forward kernels on the same operands; only the fp32 sum of the loss differs."""
    a, b = run(True)[0][0][0], run(False)[0][0][0]
    print(f"first loss: fused {a:.8f} autograd {b:.8f} oracle {GOLDEN['losses'][0][0]:.8f}")
    assert abs(a - b) <= 1e-5 * abs(b)


def test_two_fused_runs_give_equal_bits():
    a, b = run(True), run(True, fresh=True)
    assert isinstance(a[1], list) and len(a[1]) == len(b[1]) == N.STEPS
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("fused", [True, False])
def test_early_stop_ends_the_inner_loop(fused):
    inv, x0 = make_inversion(fused)
    latents = inv.ddim_loop(x0)
    inv.null_optimization(latents, N.INNER, 1e9)  # above any loss: one inner step per timestep
    assert [len(l) for l in inv.losses] == [1] * N.STEPS


def test_sweep_with_per_step_copies_of_one_embedding_is_the_plain_sweep():
    from sliders_conceptmod_amd import train_util as TU
    from tests.test_engine_gpu import build_pair
    ocfg, _ou, _onet, pu, pnet = build_pair("tiny_sd1x", torch.float16)
    g = torch.Generator().manual_seed(4)
    te = torch.randn(2, 77, ocfg.cross_attention_dim, generator=g).cuda().half()
    lat = torch.randn(1, 4, 8, 8, generator=g).cuda()
    sched = N.ddim_scheduler()
    plain = TU.slider_sweep_latents(pu, pnet, sched, lat, te, 2.0, 500, 7.5, N.STEPS)
    same = TU.slider_sweep_latents(pu, pnet, sched, lat, te, 2.0, 500, 7.5, N.STEPS,
                                   uncond_per_step=[te[:1].float().clone() for _ in range(N.STEPS)])
    assert torch.equal(plain, same)
    other = TU.slider_sweep_latents(pu, pnet, sched, lat, te, 2.0, 500, 7.5, N.STEPS,
                                    uncond_per_step=[te[:1].float() * (1 + 0.1 * k) for k in range(N.STEPS)])
    assert not torch.equal(plain, other)
    with pytest.raises(ValueError, match="unconditional embeddings"):
        TU.slider_sweep_latents(pu, pnet, sched, lat, te, 2.0, 500, 7.5, N.STEPS, uncond_per_step=[te[:1]])


def test_sdxl_is_refused():
    from sliders_conceptmod_amd._native import SmiError
    from sliders_conceptmod_amd.null_inversion import NullInversion
    _ocfg, _ou, pu = R.build_plain_pair("tiny_sdxl", torch.float16)
    with pytest.raises(SmiError, match="SD-XL"):
        NullInversion(pu, N.ddim_scheduler())


def test_edit_image_cli(tmp_path):
    from PIL import Image
    from sliders_conceptmod_amd import edit_image as E
    from tests.test_generate_gpu import save_lora
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(tmp_path / "photo.png")
    lora = save_lora("tiny_sd1x", tmp_path / "slider.pt", 1)
    out = tmp_path / "out"
    E.main(["--image", str(tmp_path / "photo.png"), "--prompt", "photo of a person", "--model_name", str(lora),
            "--save_path", str(out), "--pretrained_model", "synthetic://tiny_sd1x", "--image_size", "64",
            "--ddim_steps", "4", "--num_inner_steps", "2", "--scales=0,2"])
    folder = out / "slider"
    names = sorted(str(p.relative_to(folder)) for p in folder.rglob("*.png"))
    assert names == ["0/photo.png", "2/photo.png", "all/photo.png", "reconstruction.png"]
    rec = np.asarray(Image.open(folder / "reconstruction.png"))
    s0, s2 = (np.asarray(Image.open(folder / s / "photo.png")) for s in ("0", "2"))
    strip = np.asarray(Image.open(folder / "all" / "photo.png"))
    assert rec.shape == s0.shape == s2.shape == (64, 64, 3) and strip.shape == (64, 128, 3)
    assert np.array_equal(strip[:, :64], s0) and np.array_equal(strip[:, 64:], s2)
    assert not np.array_equal(s0, s2)
