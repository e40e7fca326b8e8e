"""train_lora_sd3 on a real MI355X: `synthetic://tiny_sd3`, 4 iterations, resolution 64 (an 8 x 8 latent), 3 zero rows for the
T5 block (80 context tokens), 4 denoising steps, fp16.

  * iteration 0's loss and LoRA gradient against the float64 restatement of the same iteration (same noise, timesteps_to and
    prompt embeddings; the pre-roll, the three frozen steps, the adapted step and the loss restated on mmdit_refs.forward)
    under bar = 3 e_q + 1e-4, e_q the storage twin's distance from float64 on the same quantity (mmdit_bwd_refs);
  * the native clip + AdamW step against torch's under test_optim_train_gpu.py's yardstick: parameter distance after the 4
    iterations within that test's bar for the text trainer's AdamW pair, the bar below a quarter of the movement;
  * the written file: keys, strict load, a `generate_images --base sd3` sweep; `--context_stream`; the refusals."""
import pytest
import torch

import mmdit_bwd_refs as B
import mmdit_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T5_TOKENS, STEPS, RES, ITER = 3, 4, 64, 4
ADAMW_BAR = 4.9e-4  # test_optim_train_gpu.BARS[("tiny_sd1x", "adamw")]: the text trainer's fused / autograd AdamW pair
LR = 2e-3           # the learning rate that yardstick runs at
_runs = {}


def make(tmp_path, name="sd3"):
    from sliders_conceptmod_amd import config_util, model_util, prompt_util
    cfg = config_util.load_config_from_yaml("data/config-sd3.yaml")
    cfg.pretrained_model.name_or_path = "synthetic://tiny_sd3"
    cfg.train.precision, cfg.save.precision = "float16", "float16"
    cfg.train.iterations, cfg.train.max_denoising_steps, cfg.train.cfg = ITER, STEPS, 3.0
    cfg.save.name, cfg.save.path, cfg.save.per_steps = name, str(tmp_path / "models"), 2
    settings = prompt_util.PromptSettings(target="person", positive="person, very old", negative="person, very young",
                                          unconditional="", neutral="person", action="enhance", guidance_scale=2.0,
                                          resolution=RES, batch_size=1)
    models = model_util.load_models_sd3("synthetic://tiny_sd3", weight_dtype=torch.float16)
    return cfg, [settings], models


def run(tmp_path, fused, **kw):
    key = (fused, tuple(sorted(kw.items())))
    if key not in _runs:
        from sliders_conceptmod_amd import train_lora_sd3 as T
        cfg, prompts, models = make(tmp_path)
        torch.manual_seed(1)
        net = T.train(cfg, prompts, torch.device(DEV), models=models, fused_step=fused, t5_tokens=T5_TOKENS,
                      optimizer_kwargs={"lr": LR}, **kw)
        _runs[key] = (net, cfg, prompts, models)
    return _runs[key]


def restated_iteration(fwd, emb, first, cfg_scale, eta, leaves):
    """Iteration 0 on `fwd(sample, ts, ctx, pooled, lora, mults)`: the pre-roll under the adaptor, the three frozen CFG steps,
    the adapted one, the enhance loss on the stepped latents.  Returns (loss, the residual d whose mean square it is)."""
    ts, sig = R.flow_sigmas(STEPS)
    x = first["latents"].double()
    t_to = first["timesteps_to"]

    def cfg_step(x, i, e, lora, m):
        ctx = torch.cat([emb[""][0], emb[e][0]]).double()
        pooled = torch.cat([emb[""][1], emb[e][1]]).double()
        v = fwd(torch.cat([x, x]), [float(ts[i])] * 2, ctx, pooled, lora, [m, m])
        u, c = v.chunk(2)
        return x + (sig[i + 1] - sig[i]) * (u + cfg_scale * (c - u))

    with torch.no_grad():
        for i in range(t_to):
            x = cfg_step(x, i, "person", leaves, 1.0)
        pos, neu, neg = (cfg_step(x, t_to, e, leaves, 0.0) for e in ("person, very old", "person", "person, very young"))
    tgt = cfg_step(x, t_to, "person", leaves, 1.0)
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
        for p in ("", "person", "person, very old", "person, very young"):
            te, pooled = train_util.encode_prompts_sd3(None, toks, encs, p, 1, T5_TOKENS, transformer.cfg.joint_attention_dim)
            emb[p] = (te.to(dt).cpu(), pooled.to(dt).cpu())  # what the trainer caches
    sd = {k: v.detach().cpu().double() for k, v in transformer.state_dict().items()}
    mcfg = transformer.cfg
    # the network as iteration 0 found it: lora_down as initialised, lora_up zero.  torch.manual_seed(1) again draws the same init
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import mmdit as M
    blank = M.SD3Transformer2DModel(mcfg)  # (built before the seed: its own default init draws from the same generator)
    torch.manual_seed(1)
    net0 = L.LoRANetwork(blank, rank=4, multiplier=1.0, train_method="full")
    names = [l.target_path for l in net0.unet_loras]
    lora = {l.target_path: (l.lora_down.weight.detach().double(), l.lora_up.weight.detach().double(), float(l.scale))
            for l in net0.unet_loras}

    def grads(dt_twin):
        leaves = B._leaves(lora)

        def fwd(sample, ts, ctx, pooled, lr, m):
            if dt_twin is None:
                return R.forward(sd, mcfg, sample, ts, ctx, pooled, lora=lr, mults=m)
            return B.twin_forward(sd, mcfg, sample, ts, ctx, pooled, lr, m, dt=dt_twin)

        loss, d = restated_iteration(fwd, emb, first, cfg.train.cfg, prompts[0].guidance_scale, leaves)
        ps = [t for n in names for t in leaves[n][:2]]
        gs = torch.autograd.grad(loss, ps, allow_unused=True)
        gs = [torch.zeros_like(p) if g is None else g for p, g in zip(ps, gs)]
        per = {n: (gs[2 * i], gs[2 * i + 1]) for i, n in enumerate(names)}
        return float(loss.detach()), per, d.detach()

    loss_a, ga, d_a = grads(None)
    loss_b, gb, d_b = grads(dt)
    got = {l.target_path: (first["grad"][l.off_down:l.off_down + 4 * l.in_dim].double(),
                           first["grad"][net._n_down + l.off_up:net._n_down + l.off_up + l.out_dim * 4].double())
           for l in net.unet_loras}
    flat = lambda per: torch.cat([torch.cat([per[n][0].reshape(-1), per[n][1].reshape(-1)]) for n in names])
    e_q = B.rel(flat(gb), flat(ga))
    err = B.rel(flat(got), flat(ga))
    print(f"iteration 0: timesteps_to {first['timesteps_to']}, loss {first['loss']:.6e} (float64 {loss_a:.6e}, twin {loss_b:.6e}); "
          f"gradient rel {err:.3e}, e_q {e_q:.3e}, bar {B.bar(e_q):.3e}")
    assert float(flat(ga).norm()) > 0 and all(float(got[n][0].abs().max()) == 0 for n in names), "lora_up is zero: d(down) is"
    assert err <= B.bar(e_q)
    # the loss is mean(d^2): to first order its relative error is twice that of d, which the twin measures as a vector
    b_d = B.bar(B.rel(d_b, d_a))
    assert abs(first["loss"] - loss_a) / abs(loss_a) <= 2 * b_d + b_d ** 2


def test_native_step_against_the_torch_classes(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    f, a = run(tmp_path, None)[0], run(tmp_path, False)[0]
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import mmdit as M
    blank = M.SD3Transformer2DModel(M.tiny_sd3_config())
    torch.manual_seed(1)
    init = L.LoRANetwork(blank, rank=4, multiplier=1.0, train_method="full").flat.detach()
    pa, pf = a.flat.detach().cpu(), f.flat.detach().cpu()
    dist = float((pf - pa).norm() / pa.norm())
    moved = float((pf - init).norm() / pa.norm())
    print(f"native vs torch AdamW after {ITER} iterations: distance {dist:.3e}, moved {moved:.3e}, bar {ADAMW_BAR:.1e}; "
          f"losses {f.training_losses} / {a.training_losses}")
    assert len(f.training_losses) == len(a.training_losses) == ITER
    assert f.training_losses[0] == pytest.approx(a.training_losses[0], rel=1e-5)  # nothing has been updated yet
    assert ADAMW_BAR < 0.25 * moved and dist <= ADAMW_BAR


def test_written_file_loads_and_sweeps(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from safetensors.torch import load_file
    from sliders_conceptmod_amd import generate_images as G
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import model_util as MU
    from pathlib import Path
    net, cfg, _p, _m = run(tmp_path, None)
    folder = Path(cfg.save.path)  # (of the test that trained first)
    last, mid = folder / "sd3_last.safetensors", folder / "sd3_2steps.safetensors"
    assert last.exists() and mid.exists()
    state = load_file(str(last))
    _t, _e, model, _s = MU.load_models_sd3("synthetic://tiny_sd3")
    fresh = L.LoRANetwork(model, rank=4)
    assert len(fresh.unet_loras) == 8 and set(state) == set(fresh.state_dict())
    fresh.load_state_dict(state, strict=True)
    assert float(fresh.flat.detach()[fresh._n_down:].abs().max()) > 0, "lora_up has left zero"
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\n")
    G.main(["--model_name", str(last), "--save_path", str(tmp_path / "out"), "--scales=-1,1", "--prompts_path", str(prompts),
            "--pretrained_model", "synthetic://tiny_sd3", "--base", "sd3", "--image_size", "64", "--num_samples", "1",
            "--ddim_steps", "2", "--t5_tokens", str(T5_TOKENS), "--start_noise", "900"])
    assert (tmp_path / "out" / "sd3_last" / "all" / "0_0.png").exists()


def test_context_stream_trains_all_fifteen_modules(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import train_lora_sd3 as T
    cfg, prompts, models = make(tmp_path, "ctx")
    cfg.train.iterations = 2
    torch.manual_seed(1)
    net = T.train(cfg, prompts, torch.device(DEV), models=models, t5_tokens=T5_TOKENS, context_stream=True, save_file=True)
    assert len(net.unet_loras) == 15  # 191 on the 24-layer model
    ctx_up = torch.cat([l.lora_up.weight.detach().reshape(-1) for l in net.unet_loras if "add_" in l.target_path])
    assert float(ctx_up.abs().max()) > 0 and all(torch.isfinite(torch.tensor(net.training_losses)))


def test_refusals_raise_by_name(tmp_path):
    from sliders_conceptmod_amd import train_lora_sd3 as T
    cfg, prompts, models = make(tmp_path, "no")
    with pytest.raises(ValueError, match="dora"):
        T.train(cfg, prompts, torch.device(DEV), models=models, peft_type="dora")
    cfg.network.type = "c3lier"
    with pytest.raises(ValueError, match="c3lier"):
        T.train(cfg, prompts, torch.device(DEV), models=models)
    cfg.network.type = "lierla"
    cfg.pretrained_model.name_or_path = "stable-diffusion-3.5-medium"
    with pytest.raises(ValueError, match="SD3.5"):
        T.train(cfg, prompts, torch.device(DEV), models=models)
