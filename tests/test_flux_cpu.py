"""Flux without a GPU: the float64 restatement and its twin (tests/flux_refs.py), the mutations the model bar must see, the
fp32 emulation of qk_norm_rope under its per-element bound, the LoRA site walk, the scheduler's dynamic shift, the engine's
refusals through its host-only dry run, and the `generate_images --base flux` command line."""
import math

import pytest
import torch

import flux_refs as F

TS = [1000.0, 517.25, 31.0]
GS = [3.5, 1.0, 7.25]


def _setup(h, w, nc=13, guidance=True):
    from sliders_conceptmod_amd import flux as M
    cfg = M.tiny_flux_config(guidance_embeds=guidance)
    model = M.init_synthetic_(M.FluxTransformer2DModel(cfg), seed=3)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 16, h, w, generator=g)
    ctx = torch.randn(3, nc, cfg.joint_attention_dim, generator=g).half()
    pooled = torch.randn(3, cfg.pooled_projection_dim, generator=g).half()
    sd = {k: v.half() for k, v in model.state_dict().items()}
    return cfg, model, (sd, cfg, x, TS, GS if guidance else None, ctx, pooled)


# a non-square grid whose ids reach row 63 (128 x 6 latents: 64 x 3 tokens) and one whose ids reach column 63
GRIDS = {"rows_to_63": (128, 6), "cols_to_63": (6, 128)}
_bars = {}


def _bar(grid):
    if grid not in _bars:
        _cfg, _m, args = _setup(*GRIDS[grid])
        bar, ref = F.model_bar(*args, torch.float16)
        _bars[grid] = (args, bar, ref)
    return _bars[grid]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_twin_is_under_its_own_bar_and_bf16_is_coarser(grid):
    args, bar, ref = _bar(grid)
    twin = F.forward(*args, dt=torch.float16)
    assert 0 < F.rel_l2(twin, ref) <= bar < 5e-3
    assert F.model_bar(*args, torch.bfloat16, ref=ref)[0] > 4 * bar


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("mut", F.MUTATIONS)
def test_every_mutation_leaves_the_fp16_bar(mut, grid):
    """Each wrong network moves the float64 output by at least 2 x the fp16 bar: the engine test would see it."""
    args, bar, ref = _bar(grid)
    moved = F.rel_l2(F.forward(*args, mut=mut), ref)
    print(f"{mut} on {grid}: {moved / bar:.1f} x the fp16 bar")
    assert moved >= 2 * bar


def test_qk_norm_rope_emulation_under_its_bound_and_mutants_outside():
    """A self-check of the reference and its bound (no product code runs): what tests/test_flux_kernels_gpu.py holds the kernel
    to admits a correct fp32 kernel at 1.0 E and rejects three wrong ones beyond SLACK."""
    H, D, axes, n, T = 2, 64, (16, 24, 24), 2, 37
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 64, (T, 3), generator=g)
    ids[0, 1] = ids[0, 2] = 63
    cos, sin = F.rope_table(ids, axes, f32=True)
    mag = torch.tensor([1.0, 1e-3, 60.0])[torch.arange(T) % 3][None, :, None, None, None]
    for dt in (torch.float16, torch.bfloat16):
        x = (torch.randn(n, T, 3, H, D, generator=g, dtype=torch.float64) * mag).to(dt)
        wq, wk = (0.5 + torch.rand(D, generator=g, dtype=torch.float64)).to(dt), (0.5 + torch.rand(D, generator=g, dtype=torch.float64)).to(dt)
        ref, rmag = F.qk_norm_rope_ref(x, wq, wk, cos, sin)
        E = F.qk_norm_rope_bound(ref, rmag, dt)
        emu = F.qk_norm_rope_emulate(x, wq, wk, cos, sin, dt)
        assert F.worst(emu, ref, E) <= 1.0 and F.worst(ref.to(dt), ref, E) <= 1.0
        assert torch.equal(emu[:, :, 2], x[:, :, 2])
        # wrong kernels: half-split pairs, no eps (the 1e-3 rows), weights swapped
        half = F.rotate(F.rms(x[:, :, 0].double(), wq.double()), cos, sin, half_split=True)
        assert F.worst(half, ref[:, :, 0], E[:, :, 0]) > F.SLACK
        no_eps, _ = F.qk_norm_rope_ref(x, wq, wk, cos, sin, eps=0.0)
        assert F.worst(no_eps, ref, E) > F.SLACK
        swapped, _ = F.qk_norm_rope_ref(x, wk, wq, cos, sin)
        assert F.worst(swapped, ref, E) > F.SLACK


def test_rope_table_text_rows_and_first_axis_do_not_rotate():
    """A self-check of the REFERENCE's table (tests/flux_refs.py), not of the product: the engine's host-built table is held
    against this one through the engine tests, whose bar the rope mutations above leave."""
    cos, sin = F.rope_table(F.joint_ids(4, 3, 5), (16, 56, 56))
    assert torch.equal(cos[:5], torch.ones(5, 64, dtype=torch.float64)) and not sin[:5].any()
    assert torch.equal(cos[:, :8], torch.ones(17, 8, dtype=torch.float64)) and not sin[:, :8].any()
    # image token (row 2, col 1) = joint row 5 + 2 * 3 + 1; pair 8 is the row axis at j = 0 (angle = row), pair 36 the column axis
    r = 5 + 2 * 3 + 1
    assert math.isclose(float(cos[r, 8]), math.cos(2.0)) and math.isclose(float(sin[r, 36]), math.sin(1.0))
    assert math.isclose(float(sin[r, 9]), math.sin(2.0 / 10000 ** (2 / 56)))


def test_site_walk_matches_the_reference_trainer():
    """delimiter '-' and target_replace ['Attention']: 4 modules per double block (the add_ children skipped), 3 per single
    block -- 19 x 4 + 38 x 3 = 190 at full size -- with the reference's key names; context_stream=True keeps the add_ children."""
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    cfg = M.tiny_flux_config()
    model = M.FluxTransformer2DModel(cfg)
    net = L.LoRANetwork(model, rank=4, alpha=1.0, delimiter="-", target_replace=["Attention"], train_method="full")
    assert len(net.unet_loras) == cfg.num_layers * 4 + cfg.num_single_layers * 3 == 14
    assert 19 * 4 + 38 * 3 == 190
    names = [l.lora_name for l in net.unet_loras]
    assert names[0] == "lora_unet-transformer_blocks-0-attn-to_q"
    assert "lora_unet-transformer_blocks-1-attn-to_out-0" in names
    assert names[-1] == "lora_unet-single_transformer_blocks-1-attn-to_v"
    assert not any("add_" in k for k in names)
    full = L.LoRANetwork(model, rank=4, alpha=1.0, delimiter="-", target_replace=["Attention"], train_method="full",
                         context_stream=True)
    assert len(full.unet_loras) == cfg.num_layers * 8 + cfg.num_single_layers * 3
    # the engine accepts both sets (the add_q / add_k / add_v sites adjacent in its order) in a dry run
    for n_ in (net, full):
        assert M.workspace_bytes(cfg, torch.float16, n_.engine_sites(), 2, 8, 6, 5) > 0
    model.__dict__.pop("_lora_network")
    # the state dict carries diffusers' parameter names
    keys = set(model.state_dict())
    for k in ("x_embedder.weight", "time_text_embed.text_embedder.linear_2.bias", "transformer_blocks.0.attn.norm_added_k.weight",
              "transformer_blocks.1.ff_context.net.0.proj.weight", "single_transformer_blocks.0.attn.norm_q.weight",
              "single_transformer_blocks.1.proj_mlp.bias", "single_transformer_blocks.1.proj_out.weight", "norm_out.linear.weight"):
        assert k in keys, k
    assert "time_text_embed.guidance_embedder.linear_1.weight" not in keys
    assert "time_text_embed.guidance_embedder.linear_1.weight" in M.FluxTransformer2DModel(M.tiny_flux_config(True)).state_dict()
    full_size = M.flux_schnell_config()
    assert (full_size.inner_dim, full_size.num_layers, full_size.num_single_layers, full_size.guidance_embeds) == (3072, 19, 38, False)
    assert M.flux_dev_config().guidance_embeds


def test_scheduler_dynamic_shift_against_the_closed_form():
    from sliders_conceptmod_amd import model_util as MU
    s = MU.FlowMatchEulerDiscreteScheduler(1000, 3.0, use_dynamic_shifting=True)
    for seq, steps in ((256, 4), (4096, 28)):
        mu = s.calculate_shift(seq)
        assert math.isclose(mu, {256: 0.5, 4096: 1.15}[seq], abs_tol=1e-12) and math.isclose(mu, F.calculate_shift(seq))
        s.set_timesteps(sigmas=torch.linspace(1.0, 1.0 / steps, steps, dtype=torch.float64), mu=mu)
        ts, sig = F.flux_sigmas(steps, mu)
        assert torch.equal(s.sigmas, sig.float()) and torch.equal(s.timesteps, ts.float()) and s.sigmas[-1] == 0
        k = steps // 2
        base = 1.0 - k * (1.0 - 1.0 / steps) / (steps - 1)
        assert math.isclose(float(s.sigmas[k]), math.exp(mu) / (math.exp(mu) + 1 / base - 1), rel_tol=1e-6)
    with pytest.raises(ValueError, match="mu goes with use_dynamic_shifting"):
        s.set_timesteps(4)
    # schnell's kind: shift 1 is the identity on the pipeline's sigmas; mu is refused
    q = MU.FlowMatchEulerDiscreteScheduler(1000, 1.0)
    q.set_timesteps(sigmas=torch.linspace(1.0, 0.25, 4, dtype=torch.float64))
    assert torch.equal(q.sigmas, torch.tensor([1.0, 0.75, 0.5, 0.25, 0.0]))
    with pytest.raises(ValueError, match="shifts statically"):
        q.set_timesteps(4, mu=0.5)
    # SD3's schedule is what it was
    import mmdit_refs as R
    sd3 = MU.FlowMatchEulerDiscreteScheduler()
    sd3.set_timesteps(28)
    ts, sig = R.flow_sigmas(28)
    assert torch.equal(sd3.timesteps, ts.float()) and torch.equal(sd3.sigmas, sig.float())


REFUSALS = [
    (dict(axes_dims_rope=(16, 24, 32)), {}, "sum(axes_dims_rope)"),
    (dict(axes_dims_rope=(14, 25, 25)), {}, "is odd"),
    (dict(attention_head_dim=24, axes_dims_rope=(8, 8, 8)), {}, "multiple of 16"),
    (dict(attention_head_dim=176, axes_dims_rope=(16, 80, 80)), {}, "at most 160"),
    (dict(num_attention_heads=3, attention_head_dim=16, axes_dims_rope=(4, 6, 6)), {}, "multiple of 64"),
    (dict(in_channels=8), {}, "in_channels x patch_size^2"),
    ({}, dict(h=7), "must be even"),
    ({}, dict(w=5), "must be even"),
]


@pytest.mark.parametrize("cfg_kw,shape_kw,needle", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_engine_refusals_by_name(cfg_kw, shape_kw, needle):
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd import flux as M
    cfg = M.FluxConfig(**{**M.tiny_flux_config().__dict__, **cfg_kw})
    with pytest.raises(_native.SmiError) as e:
        M.workspace_bytes(cfg, torch.float16, [], 2, shape_kw.get("h", 8), shape_kw.get("w", 6), 5)
    assert needle in str(e.value), str(e.value)


def test_site_refusals_by_name():
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd import flux as M
    cfg = M.tiny_flux_config()
    site = dict(target="transformer_blocks.0.attn.to_out.0", off_down=0, off_up=0, rank=4, scale=1.0)
    assert M.workspace_bytes(cfg, torch.float16, [site], 2, 8, 6, 5) > 0
    for bad, needle in (({"off_dora": 0}, "DoRA site"), ({"rank": 17}, "outside [1, 16]"),
                        ({"target": "single_transformer_blocks.0.proj_mlp"}, "sites sit on"),
                        ({"target": "single_transformer_blocks.0.proj_out"}, "sites sit on"),
                        ({"target": "transformer_blocks.0.ff.net.2"}, "sites sit on"),
                        ({"target": "single_transformer_blocks.0.attn.to_out.0"}, "not an attention projection of this transformer"),
                        ({"target": "transformer_blocks.0.attn.to_q"}, "all or none")):
        with pytest.raises(_native.SmiError) as e:
            M.workspace_bytes(cfg, torch.float16, [{**site, **bad}], 2, 8, 6, 5)
        assert needle in str(e.value), str(e.value)


def test_generate_images_flux_command_line(tmp_path):
    from sliders_conceptmod_amd import generate_images as G
    d = G.fill_defaults(G.build_parser().parse_args(["--prompts_path", "p.csv", "--save_path", "o", "--base", "flux"]))
    # steps, tokens and guidance stay open until the scheduler's config is read
    assert (d.image_size, d.ddim_steps, d.t5_tokens, d.guidance_scale, d.no_t5) == (1024, None, None, None, False)
    assert "are ours" in G.__doc__ and "--base flux" in G.__doc__
    common = ["--prompts_path", str(tmp_path / "p.csv"), "--save_path", str(tmp_path), "--base", "flux",
              "--pretrained_model", "synthetic://tiny_flux"]
    with pytest.raises(ValueError, match="--te_model_name"):
        G.generate(G.build_parser().parse_args(common + ["--te_model_name", "x.pt"]))
    with pytest.raises(ValueError, match="flow-matching Euler"):
        G.generate(G.build_parser().parse_args(common + ["--scheduler", "ddim"]))
    dora = tmp_path / "dora.pt"
    torch.save({"lora_unet-transformer_blocks-0-attn-to_q.dora_scale": torch.ones(4)}, dora)
    with pytest.raises(ValueError, match="DoRA files"):
        G.generate(G.build_parser().parse_args(common + ["--model_name", str(dora)]))
    assert G.file_delimiter({"lora_unet-transformer_blocks-0-attn-to_q"}) == "-"
    assert G.file_delimiter({"lora_unet_transformer_blocks_0_attn_to_q"}) == "_"
    assert G.has_context_stream({"lora_unet-transformer_blocks-0-attn-add_q_proj"})
    assert not G.has_context_stream({"lora_unet-transformer_blocks-0-attn-to_q", "lora_unet-transformer_blocks-0-attn-norm_added_q"})


def test_load_models_flux_synthetic_and_prompt_encoding():
    from sliders_conceptmod_amd import model_util as MU
    from sliders_conceptmod_amd import train_util as TU
    toks, encs, model, sched = MU.load_models_flux("synthetic://tiny_flux")
    assert not sched.use_dynamic_shifting and sched.shift == 1.0 and not model.cfg.guidance_embeds
    e, p = TU.encode_prompts_flux(None, toks, encs, "a photo of a person", 2, 7, 64)
    assert tuple(e.shape) == (2, 7, 64) and tuple(p.shape) == (2, 32) and torch.equal(e[0], e[1])
    e2, _ = TU.encode_prompts_flux(None, toks, encs, "a photo of a person", 1, 7, 64)
    assert torch.equal(e2[0], e[0]) and len(encs[1]._prompt_cache) == 1  # cached: one T5 pass per distinct prompt
    calls = []
    encs[1].encode = lambda p_, n_: calls.append(p_) or torch.zeros(1, n_, 64)
    for i in range(encs[1].CACHE_MAX + 3):  # the cache is bounded, and the oldest entry goes first
        encs[1].encode_cached(f"prompt {i}", 7)
    encs[1].encode_cached(f"prompt {encs[1].CACHE_MAX + 2}", 7)
    assert len(calls) == encs[1].CACHE_MAX + 3 and len(encs[1]._prompt_cache) == encs[1].CACHE_MAX
    assert ("a photo of a person", 7) not in encs[1]._prompt_cache
    _t, encs0, _m, _s = MU.load_models_flux("synthetic://tiny_flux", no_t5=True)
    z, _ = TU.encode_prompts_flux(None, toks, encs0, "a photo of a person", 1, 7, 64)
    assert encs0[1] is None and not z.any()
    with pytest.raises(ValueError, match="flux_schnell"):
        MU.load_models_flux("synthetic://flux")
    lat = TU.get_initial_latents_flux(sched, 2, 64, 48, 1, generator=torch.manual_seed(1))
    assert tuple(lat.shape) == (2, 16, 8, 6)
