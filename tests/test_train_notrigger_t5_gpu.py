"""The no-trigger trainer on a T5 tower, on the GPU: its loop on the small test tower against a float64 restatement of the
loop (tests/t5_bwd_refs.tower_forward under notrigger_refs.loss_ref, SGD and clip_grad_value_ written out), and `main()` on
`synthetic://tiny_flux --clip_index 1` and `synthetic://tiny_sd3 --clip_index 2` with a small --t5_tokens: the written files'
keys and prefixes, and their way through combine_loras --t5."""
import pytest
import torch

import notrigger_refs as N
import t5_bwd_refs as B
import t5_refs as R

pytestmark = pytest.mark.gpu

TOKENS, STEPS, LR, LAM, RANK, ALPHA = 24, 6, 0.5, 0.1, 4, 4.0


def loop_ref(cfg, sd, lora0, names, scale, ids3, which, dtype=None, steps=STEPS):
    """notrigger_refs.loop_ref on the T5 tower: the two-sided loop in float64 (dtype: every stored tensor rounded to it), SGD,
    clip_grad_value_(1.0), gradients never zeroed, targets from the un-adapted tower.  Returns [(reconstruction, curriculum)]."""
    neu_ids, pos_ids, neg_ids = ids3
    fwd = lambda ids, lora=None, m=None: B.tower_forward(cfg, sd, ids, lora, m, scale, dtype)[which]
    with torch.no_grad():
        neu, pos, neg = fwd(neu_ids), fwd(pos_ids), fwd(neg_ids)
    leaves = {n: (lora0[n][0].clone().requires_grad_(True), lora0[n][1].clone().requires_grad_(True)) for n in names}
    params = [t for n in names for t in leaves[n]]
    opt = torch.optim.SGD(params, lr=LR)
    out, norm_p, norm_n = [], None, None
    for i in range(steps):
        h = fwd(neu_ids.expand(2, -1), leaves, [1.0, -1.0])
        tp, tn = h[0:1], h[1:2]
        if i == 0:
            norm_p, norm_n = (pos - tp.detach()).norm(), (neg - tn.detach()).norm()
        total, recon, cur = N.loss_ref(tp, tn, pos, neg, neu, norm_p, norm_n, LAM)
        total.backward()
        torch.nn.utils.clip_grad_value_(params, 1.0)
        opt.step()
        out.append((float(recon.detach()), float(cur.detach())))
    return out


@pytest.mark.parametrize("chosen_layer", (-1, -2))
def test_loop_follows_the_f64_restatement(chosen_layer):
    """lambda 0.1, constant lr 0.5, 6 SGD steps, rank 4, the network's seeded init (lora_up zero: step 0 is the frozen tower).
    The first reconstruction MSE is held to 3 e_q + 1e-4, e_q the distance of the bf16-storage restatement's from the exact
    one; from then on the engine's reconstruction falls wherever the float64 loop's falls by more than 1 %."""
    from sliders_conceptmod_amd import lora, t5
    from sliders_conceptmod_amd.notrigger import TextEncoderStep
    from sliders_conceptmod_amd.train_notrigger import train_loop
    cfg = R.test_cfg()
    sd = R.rounded_state(B.halved_state(cfg), torch.bfloat16)
    model = t5.T5EncoderModel(t5.T5Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff,
                                          num_layers=cfg.num_layers, num_heads=cfg.num_heads), max_tokens=TOKENS)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.to("cuda", torch.bfloat16)
    torch.manual_seed(7)
    net = lora.LoRANetwork(model, rank=RANK, multiplier=1.0, alpha=ALPHA, target_replace=lora.T5_TARGET_REPLACE,
                           prefix="lora_te2", train_method="t5attn").to("cuda")
    lora0, names = N.lora_from_network(net)
    lora0 = {k: (d.cpu(), u.cpu()) for k, (d, u) in lora0.items()}  # the float64 loop runs on the CPU
    assert names == B.site_names(cfg.num_layers)
    g = torch.Generator().manual_seed(3)
    ids3 = [torch.cat([torch.randint(2, cfg.vocab_size, (1, k), generator=g), torch.ones(1, 1, dtype=torch.int64),
                       torch.zeros(1, TOKENS - k - 1, dtype=torch.int64)], dim=1) for k in (0, 3, 4)]  # words, EOS, pad
    which = "last_hidden" if chosen_layer == -1 else "penultimate"
    ref = loop_ref(cfg, sd, lora0, names, ALPHA / RANK, ids3, which)
    refq = loop_ref(cfg, sd, lora0, names, ALPHA / RANK, ids3, which, torch.bfloat16, steps=1)
    hist = train_loop(TextEncoderStep(model, net, chosen_layer), *(t.cuda() for t in ids3), LR, STEPS, LAM, lr_schedule="constant")
    rec = [h["reconstruction"] for h in hist]
    for i, (a, (b, c)) in enumerate(zip(rec, ref)):
        print(f"{which} step {i}: reconstruction {a:.6f} (f64 {b:.6f}, rel {abs(a - b) / b:.2e})  curriculum {hist[i]['curriculum']:.6f} (f64 {c:.6f})")
    e_q = abs(refq[0][0] - ref[0][0]) / ref[0][0]
    first = abs(rec[0] - ref[0][0]) / ref[0][0]
    print(f"{which}: first reconstruction MSE off by {first:.3e}, e_q {e_q:.3e}, bar {N.bar(e_q):.3e}")
    assert first <= N.bar(e_q)
    assert abs(hist[0]["curriculum"] - 1.0) < 1e-6  # by construction
    falls = [i for i in range(STEPS - 1) if ref[i + 1][0] < 0.99 * ref[i][0]]
    assert falls, "the float64 loop does not move: the test would show nothing"
    for i in falls:
        assert rec[i + 1] < rec[i], (i, rec[i], rec[i + 1])
    assert float(net.flat_up.detach().abs().max()) > 0  # lora_up left zero: it learns


@pytest.mark.parametrize("model,clip_index,name,prefix", (("FLUX.1", 1, "synthetic://tiny_flux", "lora_te2"),
                                                          ("SD3-Medium", 2, "synthetic://tiny_sd3", "lora_te3")))
def test_main_on_the_synthetic_t5_towers(tmp_path, model, clip_index, name, prefix):
    import yaml
    from safetensors.torch import load_file
    import sliders_conceptmod_amd.train_notrigger as T
    from sliders_conceptmod_amd import combine_loras as CL
    cfg = {"prompts_file": "data/prompts-flux.yaml", "pretrained_model": {"name_or_path": name},
           "network": {"type": "c3lier", "rank": 4, "alpha": 1.0, "training_method": "t5attn"},
           "train": {"precision": "bfloat16", "iterations": 4, "lr": 0.01, "lambda_similarity": 0.1},
           "save": {"name": "t", "path": str(tmp_path), "per_steps": 2, "precision": "bfloat16"}}
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    args = T.build_parser().parse_args(["--config_file", str(path), "--alpha", "1.0", "--rank", "4", "--name", "smile", "--positive",
                                        "smiling", "--negative", "frowning", "--model", model, "--clip_index", str(clip_index),
                                        "--t5_tokens", str(TOKENS)])
    hist = T.main(args)
    assert len(hist) == 4 and all(torch.isfinite(torch.tensor(h["reconstruction"])) for h in hist)
    out = tmp_path / "smile_alpha1.0_rank4_t5attn"
    file = out / f"smile_alpha1.0_rank4_t5attn_{clip_index}_last.safetensors"
    last = load_file(str(file))
    assert (out / f"smile_alpha1.0_rank4_t5attn_{clip_index}_2steps.safetensors").exists()
    want = {f"{prefix}_encoder_block_{i}_layer_0_SelfAttention_{p}.{t}" for i in range(2) for p in "qkvo"
            for t in ("alpha", "lora_down.weight", "lora_up.weight")}
    assert set(last) == want and all(v.dtype == torch.bfloat16 for k, v in last.items() if "lora" in k.split(".")[-2])
    assert any(float(v.float().abs().max()) > 0 for k, v in last.items() if k.endswith("lora_up.weight"))
    # through combine_loras --t5 either file ends under lora_te3_
    merged = CL.combine("-", "-", str(file), str(tmp_path / "m.safetensors"), t5=True)
    assert {k.replace("lora_te3_", "", 1) for k in merged} == {k.replace(prefix + "_", "", 1) for k in want}
    # float16 is refused by name for a T5 tower
    cfg["train"]["precision"] = "float16"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="T5 tower runs in bfloat16 only"):
        T.main(args)


def test_t5_lora_through_the_flux_and_sd3_sweeps(tmp_path):
    """A tiny Flux slider and a T5 tower's LoRA file, combined by `combine_loras --t5`, through `generate_images --base flux
    --t5_backend native`: scale 0 is bit-equal to the run without the T5 file, a non-zero scale changes the images, and
    switching scales serves no stale cached prompt (the file alone, as --te_model_name: scales 2, 1, 0 give three different
    images, the last one the frozen run's).  Then the same file under lora_te3_ through --base sd3."""
    import numpy as np
    from PIL import Image
    from safetensors.torch import save_file
    from sliders_conceptmod_amd import combine_loras as CL, config_util, generate_images as G, lora, model_util as MU, prompt_util
    from sliders_conceptmod_amd import train_lora_flux as TF
    # the T5 file: seeded, lora_up not zero (a file of four SGD steps would move no 8-bit pixel)
    tower = MU.load_models_flux("synthetic://tiny_flux", t5_backend="native")[1][1]
    torch.manual_seed(5)
    net = lora.LoRANetwork(tower.model, rank=4, alpha=4.0, target_replace=lora.T5_TARGET_REPLACE, prefix="lora_te2",
                           train_method="t5attn")
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0.0, 0.3)
    t5_file = str(tmp_path / "t5.safetensors")
    net.save_weights(t5_file, dtype=torch.bfloat16)
    del tower.model.__dict__["_lora_network"]
    # the slider: one iteration of train_lora_flux on the tiny model
    cfg = config_util.load_config_from_yaml("data/config-flux.yaml")
    cfg.pretrained_model.name_or_path = "synthetic://tiny_flux"
    cfg.train.iterations, cfg.train.cfg = 1, 3.5
    cfg.save.name, cfg.save.path, cfg.save.per_steps = "s", str(tmp_path / "models"), 100
    st = prompt_util.PromptSettings(target="person", positive="person, very old", negative="person, very young", unconditional="",
                                    neutral="person", action="enhance", guidance_scale=2.0, resolution=64, batch_size=1)
    torch.manual_seed(1)
    slider = TF.train(cfg, [st], torch.device("cuda:0"), save_file=False, t5_tokens=TOKENS, t5_backend="native")
    slider_file = str(tmp_path / "slider.safetensors")
    save_file({k: v.contiguous() for k, v in slider.items()}, slider_file)
    combined = str(tmp_path / "combined.safetensors")
    CL.main([slider_file, "-", t5_file, combined, "1.0", "1.0", "1.0", "--t5"])
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\n")

    def sweep(tag, scales, extra, base="flux", model="synthetic://tiny_flux"):
        """The per-scale images of one run, cut out of its `all` strip."""
        G.main([f"--scales={scales}", "--prompts_path", str(prompts), "--pretrained_model", model, "--base", base,
                "--image_size", "64", "--num_samples", "1", "--ddim_steps", "2", "--t5_tokens", str(TOKENS), "--start_noise", "1000",
                "--t5_backend", "native", "--save_path", str(tmp_path / tag)] + extra)
        name = [d for d in (tmp_path / tag).iterdir()][0]
        strip = np.asarray(Image.open(name / "all" / "0_0.png"))
        return [strip[:, 64 * i:64 * (i + 1)] for i in range(len(scales.split(",")))]

    frozen = sweep("frozen", "0", [])
    alone = sweep("slider", "0,2,1,0", ["--model_name", slider_file])
    both = sweep("both", "0,2,1,0", ["--model_name", combined])
    assert (both[0] == alone[0]).all() and (both[3] == alone[3]).all(), "scale 0: the bits of the run without the T5 file"
    assert (both[1] != alone[1]).any() and (both[2] != alone[2]).any(), "a non-zero scale changes the images"
    te = sweep("te", "2,1,0", ["--te_model_name", t5_file])
    assert (te[0] != te[1]).any() and (te[1] != te[2]).any() and (te[0] != te[2]).any(), "a stale cached prompt was served"
    assert (te[2] == frozen[0]).all()
    # SD3: the same adaptor under lora_te3_, on the prompt and on the negative prompt
    te3_file = str(tmp_path / "t5_te3.safetensors")
    CL.combine("-", "-", t5_file, te3_file, t5=True)
    sd3 = sweep("sd3", "0,2,0", ["--te_model_name", te3_file, "--guidance_scale", "3.0"], "sd3", "synthetic://tiny_sd3")
    assert (sd3[0] == sd3[2]).all() and (sd3[0] != sd3[1]).any()
    # refusals that need the files: a CLIP tower's keys, and the native backend
    clip_file = str(tmp_path / "clip.safetensors")
    save_file({"lora_te1_text_model_encoder_layers_0_self_attn_q_proj.alpha": torch.ones(())}, clip_file)
    with pytest.raises(ValueError, match="--te_model_name"):
        sweep("bad", "0", ["--te_model_name", clip_file])
    with pytest.raises(ValueError, match="--t5_backend native"):
        G.main(["--scales=0", "--prompts_path", str(prompts), "--pretrained_model", "synthetic://tiny_flux", "--base", "flux",
                "--save_path", str(tmp_path / "bad2"), "--model_name", combined])
    # the SD-XL sweep points a file with lora_te3_ keys to the bases that take it
    with pytest.raises(ValueError, match="--base flux . sd3 --t5_backend native"):
        G.main(["--scales=0", "--prompts_path", str(prompts), "--pretrained_model", "synthetic://tiny_sdxl", "--base", "xl",
                "--save_path", str(tmp_path / "bad3"), "--model_name", combined])
