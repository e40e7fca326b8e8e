"""train_lora_flux on a real MI355X: `synthetic://tiny_flux`, 4 optimiser steps, resolution 64 (an 8 x 8 latent), 3 zero rows for
the T5 block, batch_size 1 (8 iterations per optimiser step), fp16.

  * iteration 0's loss and LoRA gradient against the float64 restatement of the same iteration (same noise and prompt
    embeddings; the three frozen steps, the adapted step and the loss restated on flux_refs.forward) under
    bar = 3 e_q + 1e-4, e_q the storage twin's distance from float64 on the same quantity (flux_bwd_refs);
  * the native AdamW step against torch's under test_optim_train_gpu.py's yardstick: parameter distance after the 4 steps
    within that test's bar for the text trainer's AdamW pair, the bar below a quarter of the movement;
  * the accumulation count: one optimiser step per ceil(8 / batch_size) iterations, the parameters unchanged in between;
  * the written file: keys, strict load, a `generate_images --base flux` sweep; `--context_stream`; the refusals."""
import pytest
import torch

import flux_bwd_refs as B
import flux_refs as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T5_TOKENS, RES, ITER = 3, 64, 4
ADAMW_BAR = 4.9e-4  # test_optim_train_gpu.BARS[("tiny_sd1x", "adamw")]: the text trainer's fused / autograd AdamW pair
LR = 2e-3           # the learning rate that yardstick runs at
PROMPTS = ("person", "person, very old", "person, very young")
_runs = {}


def make(tmp_path, name="flux", batch_size=1):
    from sliders_conceptmod_amd import config_util, model_util, prompt_util
    cfg = config_util.load_config_from_yaml("data/config-flux.yaml")
    cfg.pretrained_model.name_or_path = "synthetic://tiny_flux"
    cfg.train.precision, cfg.save.precision = "float16", "float16"
    cfg.train.iterations, cfg.train.cfg = ITER, 3.5
    cfg.save.name, cfg.save.path, cfg.save.per_steps = name, str(tmp_path / "models"), 2
    settings = prompt_util.PromptSettings(target="person", positive="person, very old", negative="person, very young",
                                          unconditional="", neutral="person", action="enhance", guidance_scale=2.0,
                                          resolution=RES, batch_size=batch_size)
    models = model_util.load_models_flux("synthetic://tiny_flux", weight_dtype=torch.float16)
    return cfg, [settings], models


def run(tmp_path, fused, **kw):
    key = (fused, tuple(sorted(kw.items())))
    if key not in _runs:
        from sliders_conceptmod_amd import train_lora_flux as T
        cfg, prompts, models = make(tmp_path)
        torch.manual_seed(1)
        net = T.train(cfg, prompts, torch.device(DEV), models=models, fused_step=fused, t5_tokens=T5_TOKENS,
                      optimizer_kwargs={"lr": LR}, **kw)
        _runs[key] = (net, cfg, prompts, models)
    return _runs[key]


def restated_iteration(fwd, emb, first, eta, leaves):
    """Iteration 0 on `fwd(sample, ts, ctx, pooled, lora, mults)`: timesteps_to 0 of the 8-step schedule (no pre-roll step), the
    three frozen steps, the adapted one, the enhance loss on the stepped latents.  Returns (loss, its residual d)."""
    ts, sig = F.flux_sigmas(8)
    x = first["latents"].double()
    assert first["timesteps_to"] == 0 and float(ts[0]) == first["timestep"]

    def step(e, lora, m):
        v = fwd(x, [float(ts[0])], emb[e][0].double(), emb[e][1].double(), lora, [m])
        return x + (sig[1] - sig[0]) * v

    with torch.no_grad():
        pos, neu, neg = (step(e, leaves, 0.0) for e in ("person, very old", "person", "person, very young"))
    tgt = step("person", leaves, 1.0)
    d = tgt - (neu + eta * (pos - neg))
    return (d ** 2).mean(), d


def test_iteration_0_against_the_float64_restatement(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import train_util
    net, cfg, prompts, models = run(tmp_path, None)
    toks, encs, transformer, _sched = models
    first = net.first_step
    dt = torch.float16
    with torch.no_grad():
        emb = {}
        for p in PROMPTS:
            te, pooled = train_util.encode_prompts_flux(None, toks, encs, p, 1, T5_TOKENS, transformer.cfg.joint_attention_dim)
            emb[p] = (te.to(dt).cpu(), pooled.to(dt).cpu())  # what the trainer caches
    sd = {k: v.detach().cpu().double() for k, v in transformer.state_dict().items()}
    mcfg = transformer.cfg
    # the network as iteration 0 found it: lora_down as initialised, lora_up zero.  torch.manual_seed(1) again draws the same init
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    blank = M.FluxTransformer2DModel(mcfg)  # (built before the seed: its own default init draws from the same generator)
    torch.manual_seed(1)
    net0 = L.LoRANetwork(blank, rank=4, multiplier=1.0, delimiter="-", target_replace=["Attention"], train_method="full")
    names = [l.target_path for l in net0.unet_loras]
    assert len(names) == 14 and names == [l.target_path for l in net.unet_loras]
    lora = {l.target_path: (l.lora_down.weight.detach().double(), l.lora_up.weight.detach().double(), float(l.scale))
            for l in net0.unet_loras}

    def grads(dt_twin):
        leaves = B._leaves(lora)

        def fwd(sample, ts, ctx, pooled, lr, m):
            if dt_twin is None:
                return F.forward(sd, mcfg, sample, ts, None, ctx, pooled, lora=lr, mults=m)
            return B.twin_forward(sd, mcfg, sample, ts, None, ctx, pooled, lr, m, dt=dt_twin)

        loss, d = restated_iteration(fwd, emb, first, prompts[0].guidance_scale, leaves)
        ps = [t for n in names for t in leaves[n][:2]]
        gs = torch.autograd.grad(loss, ps, allow_unused=True)
        gs = [torch.zeros_like(p) if g is None else g for p, g in zip(ps, gs)]
        per = {n: (gs[2 * i], gs[2 * i + 1]) for i, n in enumerate(names)}
        return float(loss.detach()), per, d.detach()

    loss_a, ga, d_a = grads(None)
    loss_b, gb, d_b = grads(dt)
    acc = first["accumulation_steps"]
    assert acc == 8
    g0 = first["grad"].double() * acc  # the trainer differentiates loss / accumulation steps
    got = {l.target_path: (g0[l.off_down:l.off_down + 4 * l.in_dim], g0[net._n_down + l.off_up:net._n_down + l.off_up + l.out_dim * 4])
           for l in net.unet_loras}
    flat = lambda per: torch.cat([torch.cat([per[n][0].reshape(-1), per[n][1].reshape(-1)]) for n in names])
    e_q = B.rel(flat(gb), flat(ga))
    err = B.rel(flat(got), flat(ga))
    print(f"iteration 0: loss {first['loss']:.6e} (float64 {loss_a:.6e}, twin {loss_b:.6e}); "
          f"gradient rel {err:.3e}, e_q {e_q:.3e}, bar {B.bar(e_q):.3e}")
    assert float(flat(ga).norm()) > 0 and all(float(got[n][0].abs().max()) == 0 for n in names), "lora_up is zero: d(down) is"
    assert err <= B.bar(e_q)
    # the loss is mean(d^2): to first order its relative error is twice that of d, which the twin measures as a vector
    b_d = B.bar(B.rel(d_b, d_a))
    print(f"loss rel {abs(first['loss'] - loss_a) / abs(loss_a):.3e}, bound {2 * b_d + b_d ** 2:.3e}")
    assert abs(first["loss"] - loss_a) / abs(loss_a) <= 2 * b_d + b_d ** 2


def test_native_step_against_the_torch_classes(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    f, a = run(tmp_path, None)[0], run(tmp_path, False)[0]
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    blank = M.FluxTransformer2DModel(M.tiny_flux_config())
    torch.manual_seed(1)
    init = L.LoRANetwork(blank, rank=4, multiplier=1.0, delimiter="-", target_replace=["Attention"], train_method="full").flat.detach()
    pa, pf = a.flat.detach().cpu(), f.flat.detach().cpu()
    dist = float((pf - pa).norm() / pa.norm())
    moved = float((pf - init).norm() / pa.norm())
    print(f"native vs torch AdamW after {ITER} steps: distance {dist:.3e}, moved {moved:.3e}, bar {ADAMW_BAR:.1e}; "
          f"losses {f.training_losses[::8]} / {a.training_losses[::8]}")
    assert len(f.training_losses) == len(a.training_losses) == 8 * ITER
    assert f.training_losses[0] == pytest.approx(a.training_losses[0], rel=1e-5)  # nothing has been updated yet
    assert ADAMW_BAR < 0.25 * moved and dist <= ADAMW_BAR


def test_one_optimiser_step_per_eight_samples(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import train_lora_flux as T
    assert [T.accumulation_steps(b) for b in (1, 2, 3, 4, 7, 8, 16)] == [8, 4, 3, 2, 2, 1, 1]
    for fused in (None, False):
        net = run(tmp_path, fused)[0]
        sums = net.flat_sums
        assert net.optimizer_steps == ITER and len(sums) == 8 * ITER
        moved = [i for i in range(len(sums)) if sums[i] != (sums[i - 1] if i else sums[0])]
        # the optimiser steps at the end of iterations 7, 15, 23, 31 and the parameters stay as they are in between
        assert len(set(sums[:7])) == 1 and sums[7] != sums[6]
        assert moved == [7, 15, 23, 31], moved
    # batch_size 3: ceil(8 / 3) = 3 iterations per step
    cfg, prompts, models = make(tmp_path, "acc3", batch_size=3)
    cfg.train.iterations = 2
    torch.manual_seed(1)
    calls = []
    net = T.train(cfg, prompts, torch.device(DEV), calls.append, models=models, t5_tokens=T5_TOKENS, optimizer_kwargs={"lr": LR},
                  save_file=True)
    assert calls == [1, 2] and net.optimizer_steps == 2 and len(net.training_losses) == 6
    s = net.flat_sums
    assert s[0] == s[1] != s[2] and s[2] == s[3] == s[4] != s[5]


def test_written_file_loads_and_sweeps(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from pathlib import Path
    from safetensors.torch import load_file
    from sliders_conceptmod_amd import generate_images as G
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import model_util as MU
    net, cfg, _p, _m = run(tmp_path, None)
    folder = Path(cfg.save.path)  # (of the test that trained first)
    last, mid = folder / "flux_last.safetensors", folder / "flux_2steps.safetensors"
    assert last.exists() and mid.exists()
    state = load_file(str(last))
    _t, _e, model, _s = MU.load_models_flux("synthetic://tiny_flux")
    fresh = L.LoRANetwork(model, rank=4, delimiter="-", target_replace=["Attention"])
    assert len(fresh.unet_loras) == 14 and set(state) == set(fresh.state_dict())
    fresh.load_state_dict(state, strict=True)
    assert float(fresh.flat.detach()[fresh._n_down:].abs().max()) > 0, "lora_up has left zero"
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\n")
    G.main(["--model_name", str(last), "--save_path", str(tmp_path / "out"), "--scales=-1,1", "--prompts_path", str(prompts),
            "--pretrained_model", "synthetic://tiny_flux", "--base", "flux", "--image_size", "64", "--num_samples", "1",
            "--ddim_steps", "2", "--t5_tokens", str(T5_TOKENS), "--start_noise", "900"])
    assert (tmp_path / "out" / "flux_last" / "all" / "0_0.png").exists()


def test_context_stream_trains_the_added_modules(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import train_lora_flux as T
    cfg, prompts, models = make(tmp_path, "ctx", batch_size=4)
    cfg.train.iterations = 2
    torch.manual_seed(1)
    net = T.train(cfg, prompts, torch.device(DEV), models=models, t5_tokens=T5_TOKENS, context_stream=True, save_file=True,
                  optimizer_kwargs={"lr": LR})
    assert len(net.unet_loras) == 22  # 2 double blocks x 8 + 2 single blocks x 3
    ctx_up = torch.cat([l.lora_up.weight.detach().reshape(-1) for l in net.unet_loras if "add_" in l.target_path])
    assert float(ctx_up.abs().max()) > 0 and all(torch.isfinite(torch.tensor(net.training_losses)))


def test_train_lora_writes_no_file_into_data(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import os
    from sliders_conceptmod_amd import config_util
    from sliders_conceptmod_amd import train_lora_flux as T
    shipped = config_util.resolve_data_path("data/prompts-flux.yaml")
    before = open(shipped).read()
    _cfg, _prompts, models = make(tmp_path, "tl")
    where = tmp_path / "my-prompts.yaml"
    sd = T.train_lora("person", "person, old", "person, young", "", alpha=1.0, device=0, name="tl", batch_size=8, resolution=RES,
                      steps=1, models=models, prompts_file=str(where), t5_tokens=T5_TOKENS)
    assert where.exists() and open(shipped).read() == before and isinstance(sd, dict) and len(sd) > 0
    assert os.path.basename(str(where)) in os.listdir(tmp_path)


def test_refusals_raise_by_name(tmp_path):
    from sliders_conceptmod_amd import train_lora_flux as T
    cfg, prompts, models = make(tmp_path, "no")
    with pytest.raises(ValueError, match="dora"):
        T.train(cfg, prompts, torch.device(DEV), models=models, peft_type="dora")
    cfg.network.type = "c3lier"
    with pytest.raises(ValueError, match="c3lier"):
        T.train(cfg, prompts, torch.device(DEV), models=models)
