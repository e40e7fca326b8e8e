"""Slider composition, host side (no GPU): the stack plan, the CLI plumbing, what is refused, and -- on the oracle alone --
that the engine parity bar of tests/test_compose_engine_gpu.py can see a slider that is dropped."""
import pytest
import torch

from tests import compose_refs as CR

from sliders_conceptmod_amd import compose as CO
from sliders_conceptmod_amd import compose_images as CI
from sliders_conceptmod_amd import lora as LM

MODELS = list(CR.CFGS)


def _params(pu, states):
    return [CO.slider_params(pu, sd, name) for sd, name in zip(states, "ab")]


@pytest.fixture(scope="module")
def pairs():
    """{(model, pair name): (product UNet on the CPU, [state dict a, state dict b])} -- built once, weights never modified."""
    out = {}
    for model in MODELS:
        for name, pair in CR.PAIRS.items():
            ocfg, ou, _nets, states = CR.oracle_pair(model, pair)
            out[model, name] = (CR.product_unet(ocfg, ou), states)
    return out


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pair", list(CR.PAIRS))
def test_stack_plan(pairs, model, pair):
    pu, states = pairs[model, pair]
    sl = _params(pu, states)
    assert [(p.train_method, p.rank, p.alpha) for p in sl] == [tuple(x) for x in CR.PAIRS[pair]]
    plan = CO.plan_stack(pu, sl)
    names_a, names_b = sl[0].lora_names, sl[1].lora_names
    assert {s.lora_name for s in plan.sites} == names_a | names_b
    overlap = sum(1 for s in plan.sites if all(s.present))
    assert overlap == len(names_a & names_b)
    assert (overlap == 0) == (pair == "disjoint")
    # the union in LoRANetwork order: the walk of select_targets
    walk = [t[0] for t in LM.select_targets(pu, "full", LM.UNET_TARGET_REPLACE_MODULE_TRANSFORMER, LM.LORA_PREFIX_UNET, "_")]
    assert [s.lora_name for s in plan.sites] == [n for n in walk if n in names_a | names_b]
    down, up = CR.stack_reference(plan, sl, lambda s: CO.site_coefs(sl, s))
    od = ou = 0
    for s in plan.sites:
        assert s.rank == 12 and s.ranks == [4, 8] and s.c0 == [0, 4] and not s.is_conv
        assert (s.off_down, s.off_up) == (od, ou)  # back to back: the flat buffers have no holes
        d = down[od:od + 12 * s.row_len].view(12, s.row_len).double()
        u = up[ou:ou + s.n_out * 12].view(s.n_out, 12).double()
        want = torch.zeros(s.n_out, s.row_len, dtype=torch.float64)
        for k, p in enumerate(sl):
            blk_d, blk_u = d[s.c0[k]:s.c0[k] + s.ranks[k]], u[:, s.c0[k]:s.c0[k] + s.ranks[k]]
            if s.present[k]:
                c = torch.tensor(p.alpha / s.ranks[k], dtype=torch.float32).double()
                want += c * (p.state[f"{s.lora_name}.lora_up.weight"].double() @
                             p.state[f"{s.lora_name}.lora_down.weight"].double())
            else:
                assert not blk_d.any() and not blk_u.any(), "an absent slider's block must be zeros"
        torch.testing.assert_close(u @ d, want, rtol=1e-12, atol=1e-14)
        od += 12 * s.row_len
        ou += s.n_out * 12
    assert (plan.n_down, plan.n_up) == (od, ou)
    # the engine's demand on projections fused into one GEMM (to_q | to_k | to_v of a self-attention, to_k | to_v of a
    # cross-attention): all or none adapted, adjacent in both buffers, equal rank and scale
    by_path = {s.target_path: s for s in plan.sites}
    groups = 0
    for path, s in by_path.items():
        if not path.endswith(".to_k"):
            continue
        base = path[:-len(".to_k")]
        parts = ["to_q", "to_k", "to_v"] if ".attn1" in base else ["to_k", "to_v"]
        g = [by_path.get(f"{base}.{part}") for part in parts]
        assert all(x is not None for x in g), f"{base}: fused projections adapted in part"
        cs = g[0].n_out
        for i, x in enumerate(g):
            assert x.rank == g[0].rank and x.n_out == cs and x.row_len == g[0].row_len
            assert x.off_down == g[0].off_down + i * g[0].rank * g[0].row_len
            assert x.off_up == g[0].off_up + i * cs * g[0].rank
        groups += 1
    assert groups > 0
    sites = CO.SliderStack(pu, states).engine_sites()
    assert all(e["scale"] == 1.0 and e["rank"] == 12 for e in sites) and len(sites) == len(plan.sites)


def test_stack_plan_conv_rank_clamp():
    """c3lier: a conv site's rank is min(rank, Cin, Cout) per slider (lora.py:100-114) and alpha divides by the clamped one."""
    ocfg = CR.CFGS["tiny_sd1x"]()
    pu = CR.product_unet(ocfg, CR.OU.init_synthetic_(CR.OU.UNet2DConditionModel(ocfg), seed=0))
    every = LM.UNET_TARGET_REPLACE_MODULE_TRANSFORMER + LM.UNET_TARGET_REPLACE_MODULE_CONV
    g = torch.Generator().manual_seed(0)
    sl = []
    for name, rank in (("a", 96), ("b", 4)):
        sd = {}
        for lora_name, _path, child in LM.select_targets(pu, "noxattn", every, LM.LORA_PREFIX_UNET, "_"):
            r, dshape, ushape = LM.lora_shapes(child, rank)
            sd[f"{lora_name}.lora_down.weight"] = torch.randn(dshape, generator=g)
            sd[f"{lora_name}.lora_up.weight"] = torch.randn(ushape, generator=g)
        sl.append(CO.SliderParams(name, rank, 8.0, "noxattn", list(every), sd))
    plan = CO.plan_stack(pu, sl)
    assert plan.has_conv
    clamped = [s for s in plan.sites if s.is_conv and s.ranks[0] < 96]
    assert clamped, "the 64-channel convs must clamp rank 96"
    mods = dict(pu.named_modules())
    for s in plan.sites:
        if s.is_conv:
            conv = mods[s.target_path]
            assert s.ranks == [min(96, conv.in_channels, conv.out_channels), 4]
            assert s.row_len == conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1] and s.n_out == conv.out_channels
            assert CO.site_coefs(sl, s) == [float(torch.tensor(8.0 / s.ranks[0], dtype=torch.float32)), 2.0]
        else:
            assert s.ranks == [96, 4]
        assert s.c0 == [0, s.ranks[0]] and s.rank == s.ranks[0] + 4
    # folded scales: c_k = fp32(s_k) * fp32(alpha_k / r_k), one fp32 product
    s = clamped[0]
    assert CO.site_coefs(sl, s, [0.3, -2.0])[1] == float(torch.tensor(-2.0) * torch.tensor(2.0))


def test_cli_arguments_paths_and_multiplier_rows():
    args = CI.build_parser().parse_args(["--model_name", "out/age.pt", "--model_name", "out/smile.safetensors,x/curly.pt",
                                         "--scales=-1,0.5", "--scales=0,2", "--scales=1", "--prompts_path", "p.csv",
                                         "--save_path", "img"])
    names = CI.split_names(args.model_name)
    assert names == ["out/age.pt", "out/smile.safetensors", "x/curly.pt"]
    lists = CI.scale_lists(args.scales, 3)
    assert lists == [[-1, 0.5], [0, 2], [1]]
    cells = CI.grid_cells(lists)
    assert cells == [(-1, 0, 1), (-1, 2, 1), (0.5, 0, 1), (0.5, 2, 1)]
    per_cell, all_path = CI.output_paths("img", names, cells, 7, 2)
    assert per_cell == ["img/age+smile+curly/-1_0_1/7_2.png", "img/age+smile+curly/-1_2_1/7_2.png",
                        "img/age+smile+curly/half_0_1/7_2.png", "img/age+smile+curly/half_2_1/7_2.png"]
    assert all_path == "img/age+smile+curly/all/7_2.png"
    # one --scales applies to every slider; any other count is an error
    assert CI.scale_lists(["0,2"], 2) == [[0, 2], [0, 2]]
    with pytest.raises(ValueError, match="--scales"):
        CI.scale_lists(["0,2", "1", "3"], 2)
    # grid -> multiplier rows of one CFG pass: [uncond of every cell ; cond of every cell], both halves adapted
    rows = CO.grid_multiplier_rows([(0, 0), (0, 2), (2, 0)], num_samples=2)
    half = [[0, 0], [0, 0], [0, 2], [0, 2], [2, 0], [2, 0]]
    assert rows == half + half and len(rows) == 3 * 2 * 2
    assert all(isinstance(v, float) for r in rows for v in r)
    # defaults shared with generate_images
    assert args.scheduler is None and args.start_noise is None and args.vae_dtype is None and args.ddim_steps == 50


def test_grid_image_layout():
    from PIL import Image
    ims = [Image.new("RGB", (4, 3), (i * 40, 0, 0)) for i in range(6)]
    grid = CI.grid_image(ims, 3)  # 2 x 3: rows slider A, columns slider B
    assert grid.size == (12, 6)
    assert grid.getpixel((0, 0))[0] == 0 and grid.getpixel((8, 0))[0] == 80 and grid.getpixel((4, 3))[0] == 160
    assert CI.grid_image(ims, 6).size == (24, 3)


def test_refusals(pairs):
    pu, states = pairs["tiny_sd1x", "disjoint"]
    dora = dict(states[0])
    first = next(k for k in dora if k.endswith(".lora_down.weight"))[:-len(".lora_down.weight")]
    dora[f"{first}.dora_scale"] = torch.ones(1, 64)
    with pytest.raises(ValueError, match="DoRA"):
        CO.SliderStack(pu, [states[1], dora])
    # a file from another architecture: its layers match no train method of this UNet
    pu_xl, states_xl = pairs["tiny_sdxl", "disjoint"]
    with pytest.raises(ValueError, match="match no train method"):
        CO.SliderStack(pu, [states[0], states_xl[1]])
    # training through a stack is out of scope: tensors that require a gradient under enable_grad
    grad = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and v.ndim > 0 else v) for k, v in states[0].items()}
    with torch.enable_grad():
        with pytest.raises(ValueError, match="requires? a gradient"):
            CO.SliderStack(pu, [grad, states[1]])
        stack = CO.SliderStack(pu, states)
        assert not stack.flat.requires_grad
        x = torch.zeros(1, 4, 8, 8, requires_grad=True)
        with pytest.raises(ValueError, match="inference only"):
            stack.check_inference(x, torch.zeros(1, 77, 64))
    with torch.no_grad():
        stack.check_inference(x, torch.zeros(1, 77, 64))
    assert pu._lora_network is stack
    # scales: one per slider; a grid: one row of K per sample
    with pytest.raises(ValueError, match="scales for 2 sliders"):
        stack.set_scales([1.0])
    with pytest.raises(ValueError, match="scale grid"):
        stack.set_scale_grid([[1.0, 2.0, 3.0]])
    stack.set_scale_grid([[0, 1], [2, 3]])
    assert stack.engine_compose(2) is None  # off outside `with`
    with stack:
        assert stack.engine_compose(2) == ([4, 8], [[0.0, 1.0], [2.0, 3.0]])
        with pytest.raises(ValueError, match="2 rows but the UNet batch has 3"):
            stack.engine_compose(3)
    stack.set_scales([0.5, -1])
    with stack:
        assert stack.engine_compose(3) == ([4, 8], [[0.5, -1.0]] * 3)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pair", list(CR.PAIRS))
def test_parity_bar_sees_a_dropped_slider(model, pair):
    """On the oracle alone: with both sliders entered at (+2, -2), dropping either one moves eps by more than 3 x the fp16
    parity bar 1.5 e_q + 1e-4 of test_compose_engine_gpu.py -- so an engine that ignored a slider, or a block of the stack,
    cannot pass that bar.  Measured on the CPU (change from dropping a / b, fp16 e_q, smaller change in multiples of the
    bar): tiny_sd1x disjoint 2.5e-2 / 3.9e-2, 1.14e-3, 13.7; tiny_sd1x overlap 2.8e-2 / 7.9e-2, 1.16e-3, 15.2; tiny_sdxl
    disjoint 3.2e-2 / 2.6e-2, 8.4e-4, 19.3; tiny_sdxl overlap 3.2e-2 / 9.1e-2, 7.8e-4, 25.4.
    fp16 is the discriminating arm.  The bf16 bar (e_q ~ 8e-3) sees the same changes at only 1.8 to 3.4 multiples: the bf16
    engine test is a parity arm only and is not asserted to discriminate here."""
    ocfg, ou, nets, _states = CR.oracle_pair(model, CR.PAIRS[pair])
    x, ctx, add = CR.inputs(ocfg, 2, 16)
    t = 499.0
    both = CR.oracle_eps(ou, nets, CR.SCALES, x, t, ctx, add)
    drop_a = CR.oracle_eps(ou, nets, (None, CR.SCALES[1]), x, t, ctx, add)
    drop_b = CR.oracle_eps(ou, nets, (CR.SCALES[0], None), x, t, ctx, add)
    e_q = CR.rel(CR.oracle_eps(ou, nets, CR.SCALES, x, t, ctx, add, storage_dtype=torch.float16), both)
    bar = 1.5 * e_q + 1e-4
    ch_a, ch_b = CR.rel(drop_a, both), CR.rel(drop_b, both)
    print(f"{model} {pair}: drop a {ch_a:.2e}, drop b {ch_b:.2e}, fp16 e_q {e_q:.2e}, {min(ch_a, ch_b) / bar:.1f} x the bar")
    assert ch_a > 3 * bar and ch_b > 3 * bar
