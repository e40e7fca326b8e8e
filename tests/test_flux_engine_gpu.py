"""The Flux transformer engine (csrc/engine_flux.hip) on a real MI355X against the float64 restatement of tests/flux_refs.py.

Shapes: tiny_flux (d 128: 2 heads x 64, two double and two single blocks) at an 8 x 6 latent with 5 context tokens (joint
length 17: tails everywhere) and at 16 x 16 with 13 (77 keys: two key tiles); one double and one single block at the real
width (24 heads x 128, d 3072, joint 4096) on 8 x 8 latents with 5 tokens, without and with the guidance embedder: the
smallest shape at which the 3072-wide adaLN rows, head_dim 128 and the [rows, 5 d] operand can go wrong.  At each: n = 3 with
distinct timesteps under the model bar (2 x the storage-dtype twin's distance from float64, printed), again with rank-4 LoRA
at multipliers (0, 1, -2) for the reference's module set and for the set with the context stream, and the bitwise
properties."""
import pytest
import torch

import flux_refs as F

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
TS = [1000.0, 517.25, 31.0]
GS = [3.5, 1.0, 7.25]
MULTS = [0.0, 1.0, -2.0]
SHAPES = {"tiny_8x6_c5": ("tiny", 8, 6, 5), "tiny_16x16_c13": ("tiny", 16, 16, 13), "wide_8x8_c5": ("wide", 8, 8, 5),
          "wide_guidance_8x8_c5": ("wide_g", 8, 8, 5)}


def make_cfg(kind):
    from sliders_conceptmod_amd import flux as M
    if kind == "tiny":
        return M.tiny_flux_config()
    return M.FluxConfig(num_layers=1, num_single_layers=1, guidance_embeds=kind == "wide_g")  # d 3072, joint 4096, pooled 768


_cache = {}


def setup(name):
    """Per shape, made once and left unchanged: the model, two rank-4 networks with a non-zero lora_up (the reference's
    module set and the one with the context stream), the inputs; the float64 references are added per dtype by refs()."""
    if name in _cache:
        return _cache[name]
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    kind, h, w, nc = SHAPES[name]
    cfg = make_cfg(kind)
    # no default initialisation, and the seeded weights drawn on the GPU (0.5 billion parameters at d = 3072: seconds on the
    # CPU): the references below read the same tensors, so nothing depends on which generator drew them
    with torch.device("meta"):
        model = M.FluxTransformer2DModel(cfg)
    model = M.init_synthetic_(model.to_empty(device="cuda"), seed=3)
    g = torch.Generator().manual_seed(7)
    nets = {}
    for cs in (False, True):
        torch.manual_seed(5)
        net = L.LoRANetwork(model, rank=4, alpha=2.0, delimiter="-", train_method="full", context_stream=cs)
        with torch.no_grad():
            net.flat[net._n_down:].copy_(torch.randn(net._n_up, generator=g) * 0.5)
        model.__dict__.pop("_lora_network")
        nets[cs] = net
    x = torch.randn(3, cfg.in_channels, h, w, generator=g)
    ctx = torch.randn(3, nc, cfg.joint_attention_dim, generator=g)
    pooled = torch.randn(3, cfg.pooled_projection_dim, generator=g)
    out = dict(cfg=cfg, model=model, nets=nets, x=x, ctx=ctx, pooled=pooled, h=h, w=w, nc=nc, refs={},
               gs=GS if cfg.guidance_embeds else None)
    _cache[name] = out
    return out


def lora_of(net):
    return {l.target_path: (l.lora_down.weight.detach(), l.lora_up.weight.detach(), l.scale) for l in net.unet_loras}


def refs(s, dt):
    """(ref, bar, {context_stream: (ref_lora, bar_lora)}) for dt: inputs and weights first rounded to dt, as the engine gets them."""
    if dt in s["refs"]:
        return s["refs"][dt]
    sd = {k: v.to(dt).cpu().double() for k, v in s["model"].state_dict().items()}  # (converted once for the six forwards)
    args = (sd, s["cfg"], s["x"], TS, s["gs"], s["ctx"].to(dt), s["pooled"].to(dt))
    bar, ref = F.model_bar(*args, dt)
    with_lora = {cs: F.model_bar(*args, dt, lora=lora_of(net), mults=MULTS)[::-1] for cs, net in s["nets"].items()}
    s["refs"][dt] = (ref, bar, with_lora)
    return s["refs"][dt]


def engine(s, dt, sites, batch=3):
    from sliders_conceptmod_amd import flux as M
    if s.get("state_dt") != dt:  # the weights in the engine's dtype, cast once for the three engines of a case
        s["state"], s["state_dt"] = {k: v.detach().to("cuda", dt).contiguous() for k, v in s["model"].state_dict().items()}, dt
    state = s["state"]
    return M.FluxEngine(s["cfg"], dt, state, sites, batch, s["h"], s["w"], s["nc"], torch.device("cuda", 0))


def run(e, s, dt, net=None, idx=(0, 1, 2), mults=None):
    i = list(idx)
    down = up = None
    if net is not None:
        flat = net.flat.detach().cuda()
        down, up = flat[:net._n_down], flat[net._n_down:]
    gs = None if s["gs"] is None else [s["gs"][k] for k in i]
    out = e.forward(s["x"][i].cuda(), [TS[k] for k in i], gs, s["ctx"][i].to(dt).cuda(), s["pooled"][i].to(dt).cuda(),
                    down, up, mults)
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error, session stopped: {err}", returncode=3)
    return out


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_lora_against_fp64(name, dt):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import flux as M
    s = setup(name)
    ref, bar, with_lora = refs(s, dt)
    plain = None
    for cs, net in s["nets"].items():
        sites = net.engine_sites()
        e = engine(s, dt, sites)
        assert e.workspace_bytes == M.workspace_bytes(s["cfg"], dt, sites, 3, s["h"], s["w"], s["nc"])
        out = run(e, s, dt)
        if plain is None:
            plain = out
            err = F.rel_l2(plain.cpu(), ref)
            print(f"{name} {dt}: rel-L2 {err:.3e}, bar {bar:.3e}")
            assert torch.isfinite(plain).all() and err <= bar
        assert torch.equal(out, plain), "an engine with sites, adaptor off"
        ref_l, bar_l = with_lora[cs]
        adapted = run(e, s, dt, net, mults=MULTS)
        err_l = F.rel_l2(adapted.cpu(), ref_l)
        moved = F.rel_l2(ref_l, ref)
        print(f"{name} {dt} LoRA (0, 1, -2) on {len(sites)} sites: rel-L2 {err_l:.3e}, bar {bar_l:.3e}; the adaptor moves the "
              f"output by {moved:.3e}")
        assert torch.isfinite(adapted).all() and err_l <= bar_l
        assert moved > 10 * bar_l, "the adaptor must move the output far beyond the bar for this test to see it"
        # ---- bitwise properties
        assert torch.equal(adapted[0], plain[0]), "multiplier 0 inside an adapted batch"
        assert torch.equal(run(e, s, dt, net, mults=[0.0, 0.0, 0.0]), plain), "all multipliers 0"
        assert torch.equal(run(e, s, dt, None, mults=MULTS), plain), "NULL flat buffers"
        assert torch.equal(run(e, s, dt, net, mults=None), plain), "NULL multipliers"
        assert torch.equal(run(e, s, dt, net, mults=MULTS), adapted), "two runs"
        for i in range(3):  # n below the creation batch; a sample alone == the sample in the batch of 3
            assert torch.equal(run(e, s, dt, net, idx=(i,), mults=[MULTS[i]])[0], adapted[i]), f"sample {i} alone"
        e.close()
    e0 = engine(s, dt, [])  # an engine created without sites
    assert torch.equal(run(e0, s, dt), plain)
    assert torch.equal(run(e0, s, dt, s["nets"][False], mults=MULTS), plain), "flat buffers given to an engine without sites"
    e0.close()


def test_guidance_is_required_exactly_where_the_model_embeds_it():
    from sliders_conceptmod_amd import _native
    s = setup("tiny_8x6_c5")
    e = engine(s, torch.float16, [])
    with pytest.raises(_native.SmiError, match="guidance_embeds = 0"):
        e.forward(s["x"].cuda(), TS, GS, s["ctx"].half().cuda(), s["pooled"].half().cuda())
    e.close()
    sg = setup("wide_guidance_8x8_c5")
    eg = engine(sg, torch.float16, [])
    with pytest.raises(_native.SmiError, match="guidance_embeds = 1"):
        eg.forward(sg["x"].cuda(), TS, None, sg["ctx"].half().cuda(), sg["pooled"].half().cuda())
    eg.close()


def test_module_forward_follows_the_network():
    """FluxTransformer2DModel.forward: the attached network at its multiplier (0 outside `with network:`)."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    s = setup("tiny_8x6_c5")
    dt = torch.float16
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    model = M.FluxTransformer2DModel(s["cfg"])
    model.load_state_dict(s["model"].state_dict())
    model = model.to("cuda", dt)
    kw = dict(hidden_states=s["x"].cuda(), timestep=TS, guidance=None, pooled_projections=s["pooled"].to(dt).cuda(),
              encoder_hidden_states=s["ctx"].to(dt).cuda())
    frozen = model(**kw).sample
    net = L.LoRANetwork(model, rank=4, alpha=2.0, delimiter="-", train_method="full").to("cuda")
    net.load_state_dict(s["nets"][False].state_dict())
    net.__exit__(None, None, None)
    assert torch.equal(model(**kw).sample, frozen)
    net.set_lora_slider(-2.0)
    with net:
        on = model(**kw).sample
    e = engine(s, dt, s["nets"][False].engine_sites())
    want = run(e, s, dt, s["nets"][False], mults=[-2.0] * 3)
    e.close()
    assert torch.equal(on, want) and not torch.equal(on, frozen)
