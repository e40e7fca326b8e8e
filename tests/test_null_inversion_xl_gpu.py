"""SD-XL null-text inversion on the engine (sliders_conceptmod_amd/null_inversion_xl.py): the fused route and the autograd
route, with the pooled optimisation on and off, against the recorded CPU oracle run of the same recipe
(tests/null_inversion_xl_refs.py, tests/golden/null_inversion_xl_oracle.json: tiny_sdxl, 8 x 8 latents, 4 DDIM steps, 5
inner steps, early stop disabled, guidance 7.5, seeded embeddings), the per-step unconditional pooled embeddings in
slider_sweep_latents, and the `edit_image_xl` command end to end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctx_grad_refs as R
from tests import null_inversion_xl_refs as N

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", N.GOLDEN)))
KEY = {True: "losses_pooled_on", False: "losses_pooled_off"}


def make_inversion(fused, dtype=torch.float16):
    from sliders_conceptmod_amd.null_inversion_xl import NullInversionXL
    ocfg, _ou, pu = R.build_plain_pair(N.MODEL, dtype)
    inv = NullInversionXL(pu, N.ddim_scheduler(), num_ddim_steps=N.STEPS, guidance_scale=N.GUIDANCE, fused=fused,
                          image_size=N.IMAGE_SIZE)
    assert inv.time_ids.cpu().tolist() == [N.TIME_IDS]
    x0, uncond, cond, pooled_u, pooled_c = N.recipe(ocfg.cross_attention_dim, N.pooled_dim(ocfg))
    inv.context = torch.cat([uncond, cond]).cuda()
    inv.pooled = torch.cat([pooled_u, pooled_c]).cuda()
    return inv, x0.cuda()


_RUNS = {}


def run(fused, pooled, fresh=False):
    """(losses, embeddings, pooled embeddings, timesteps, the encoder's pooled) of one route on the recipe; computed once
    and left unchanged (fresh: a run of its own, not kept)"""
    if fresh or (fused, pooled) not in _RUNS:
        inv, x0 = make_inversion(fused)
        latents = inv.ddim_loop(x0)
        assert len(latents) == N.STEPS + 1
        embs, pooleds = inv.null_optimization(latents, N.INNER, N.NO_EARLY_STOP, optimize_pooled=pooled)
        got = (inv.losses, embs, pooleds, [int(t) for t in inv.scheduler.timesteps], inv.pooled[:1].clone())
        if fresh:
            return got
        _RUNS[(fused, pooled)] = got
    return _RUNS[(fused, pooled)]


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_losses_fall_where_the_reference_falls(fused, pooled):
    losses, embs, pooleds, ts, enc = run(fused, pooled)
    ref_all = GOLDEN[KEY[pooled]]
    assert ts == GOLDEN["timesteps"] and len(losses) == len(embs) == len(pooleds) == N.STEPS
    for t, got, ref in zip(ts, losses, ref_all):
        print(f"fused={fused} pooled={pooled} t={t}: engine {['%.5f' % v for v in got]}")
        print(f"fused={fused} pooled={pooled} t={t}: oracle {['%.5f' % v for v in ref]}")
        assert len(got) == N.INNER and all(np.isfinite(got))
        if (ref[0] - ref[-1]) / ref[0] > 0.01:
            assert got[-1] < got[0], f"t={t}: loss {got[0]:.5f} -> {got[-1]:.5f} does not fall (oracle {ref[0]:.5f} -> {ref[-1]:.5f})"
    assert (ref_all[0][0] - ref_all[0][-1]) / ref_all[0][0] > 0.01  # the first timestep is one of those
    P = enc.shape[1]
    for e, p in zip(embs, pooleds):
        assert e.shape == (1, 77, R.CFGS[N.MODEL]().cross_attention_dim) and e.dtype == torch.float32 and torch.isfinite(e).all()
        assert p.shape == (1, P) and torch.isfinite(p).all()
    assert not torch.equal(embs[0], embs[1])
    if pooled:
        assert not torch.equal(pooleds[0].float(), enc.float()) and not torch.equal(pooleds[0], pooleds[1])
    else:  # the encoder's, unchanged
        assert all(torch.equal(p, enc) for p in pooleds)


@pytest.mark.parametrize("fused", [True, False])
def test_the_pooled_optimisation_ends_lower_at_the_first_timestep(fused):
    """The oracle separates the two by 4.7 % there; both runs start from the same loss."""
    on, off = run(fused, True)[0][0], run(fused, False)[0][0]
    ref_on, ref_off = GOLDEN[KEY[True]][0], GOLDEN[KEY[False]][0]
    print(f"fused={fused}: last loss pooled on {on[-1]:.5f} off {off[-1]:.5f} ({100 * (off[-1] - on[-1]) / off[-1]:.2f} % lower); "
          f"oracle {ref_on[-1]:.5f} / {ref_off[-1]:.5f} ({100 * (ref_off[-1] - ref_on[-1]) / ref_off[-1]:.2f} %)")
    assert abs(on[0] - off[0]) <= 1e-5 * abs(off[0])
    assert on[-1] < off[-1]


def test_routes_agree_on_the_first_loss():
    """Same forward kernels on the same operands; only the fp32 sum of the loss differs."""
    a, b = run(True, True)[0][0][0], run(False, True)[0][0][0]
    print(f"first loss: fused {a:.8f} autograd {b:.8f} oracle {GOLDEN[KEY[True]][0][0]:.8f}")
    assert abs(a - b) <= 1e-5 * abs(b)


def test_two_fused_runs_give_equal_bits():
    a, b = run(True, True), run(True, True, fresh=True)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_fused_sequence_only_optimisation_returns_the_encoders_pooled():
    """optimize_pooled=False through the shared fused loop: the flat parameter is the sequence embedding alone"""
    _losses, embs, pooleds, _ts, enc = run(True, False)
    assert len(embs) == len(pooleds) == N.STEPS
    assert all(torch.isfinite(e).all() for e in embs)
    assert all(not torch.equal(a, b) for a, b in zip(embs, embs[1:]))
    assert all(torch.equal(p, enc) for p in pooleds)


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_early_stop_ends_the_inner_loop(fused, pooled):
    inv, x0 = make_inversion(fused)
    latents = inv.ddim_loop(x0)
    embs, pooleds = inv.null_optimization(latents, N.INNER, 1e9, optimize_pooled=pooled)  # above any loss: one inner step per timestep
    assert [len(l) for l in inv.losses] == [1] * N.STEPS
    assert len(embs) == len(pooleds) == N.STEPS


def test_refusals():
    from sliders_conceptmod_amd import model_util
    from sliders_conceptmod_amd._native import SmiError
    from sliders_conceptmod_amd.null_inversion_xl import NullInversionXL
    _ocfg, _ou, pu1 = R.build_plain_pair("tiny_sd1x", torch.float16)
    with pytest.raises(SmiError, match="use null_inversion.NullInversion"):
        NullInversionXL(pu1, N.ddim_scheduler())
    _ocfg, _ou, pu = R.build_plain_pair(N.MODEL, torch.float16)
    with pytest.raises(ValueError, match="DDIM"):
        NullInversionXL(pu, model_util.create_noise_scheduler("euler_a"))


def test_sweep_with_per_step_copies_of_the_encoders_pooled_is_the_plain_sweep():
    from sliders_conceptmod_amd import train_util as TU
    from tests.test_engine_gpu import build_pair
    ocfg, _ou, _onet, pu, pnet = build_pair(N.MODEL, torch.float16)
    g = torch.Generator().manual_seed(4)
    te = torch.randn(2, 77, ocfg.cross_attention_dim, generator=g).cuda().half()
    pooled = torch.randn(2, N.pooled_dim(ocfg), generator=g).cuda().half()
    tid = torch.tensor([N.TIME_IDS, N.TIME_IDS]).cuda()
    lat = torch.randn(1, 4, 8, 8, generator=g).cuda()
    sched = N.ddim_scheduler()
    unconds = [te[:1].float().clone() for _ in range(N.STEPS)]
    sweep = lambda **kw: TU.slider_sweep_latents(pu, pnet, sched, lat, te, 2.0, 500, 7.5, N.STEPS, added_cond=(pooled, tid),
                                                 uncond_per_step=unconds, **kw)
    plain = sweep()
    same = sweep(uncond_pooled_per_step=[pooled[:1].float().clone() for _ in range(N.STEPS)])
    assert torch.equal(plain, same)
    other = sweep(uncond_pooled_per_step=[pooled[:1].float() * (1 + 0.1 * k) for k in range(N.STEPS)])
    assert not torch.equal(plain, other)
    with pytest.raises(ValueError, match="unconditional pooled embeddings"):
        sweep(uncond_pooled_per_step=[pooled[:1]])


def test_edit_image_xl_cli(tmp_path):
    from PIL import Image
    from sliders_conceptmod_amd import edit_image_xl as E
    from tests.test_generate_gpu import save_lora
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(tmp_path / "photo.png")
    lora = save_lora(N.MODEL, tmp_path / "slider.pt", 1)
    out = tmp_path / "out"
    E.main(["--image", str(tmp_path / "photo.png"), "--prompt", "photo of a person", "--model_name", str(lora),
            "--save_path", str(out), "--pretrained_model", f"synthetic://{N.MODEL}", "--image_size", "64",
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
