"""The SD3 MMDiT engine (csrc/engine_mmdit.hip) on a real MI355X against the float64 restatement of tests/mmdit_refs.py.

Shapes: tiny_sd3 (d 128, a full block and the context_pre_only block) at an 8 x 6 latent with 5 context tokens (joint length
17: tails everywhere) and at 16 x 16 with 13 (77 keys: two key tiles); a 2-layer model at the real width (d 1536, 24 heads,
joint 4096) at 16 x 16 with 13 tokens, the smallest shape at which the 1536-wide kernels and the fused three-site LoRA
epilogue can go wrong.  At each: n = 3 with distinct timesteps under the model bar (2 x the storage-dtype twin's distance
from float64, printed), again with rank-4 LoRA at multipliers (0, 1, -2), and the bitwise properties."""
import pytest
import torch

import mmdit_refs as R

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
TS = [1000.0, 517.25, 31.0]
MULTS = [0.0, 1.0, -2.0]
SHAPES = {"tiny_8x6_c5": ("tiny", 8, 6, 5), "tiny_16x16_c13": ("tiny", 16, 16, 13), "wide_16x16_c13": ("wide", 16, 16, 13)}


def make_cfg(kind):
    from sliders_conceptmod_amd import mmdit as M
    if kind == "tiny":
        return M.tiny_sd3_config()
    return M.SD3Config(num_layers=2, pos_embed_max_size=12, sample_size=16)  # d 1536, 24 heads, joint 4096, pooled 2048


_cache = {}


def setup(name):
    """Per shape, made once and left unchanged: the model, a rank-4 network with a non-zero lora_up, the inputs, and the
    float64 references without and with the adaptor."""
    if name in _cache:
        return _cache[name]
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import mmdit as M
    kind, h, w, nc = SHAPES[name]
    cfg = make_cfg(kind)
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=3)
    torch.manual_seed(5)
    net = L.LoRANetwork(model, rank=4, alpha=2.0, train_method="full", context_stream=True)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        net.flat[net._n_down:].copy_(torch.randn(net._n_up, generator=g) * 0.3)
    model.__dict__.pop("_lora_network")
    x = torch.randn(3, cfg.in_channels, h, w, generator=g)
    ctx = torch.randn(3, nc, cfg.joint_attention_dim, generator=g)
    pooled = torch.randn(3, cfg.pooled_projection_dim, generator=g)
    lora = {l.target_path: (l.lora_down.weight.detach(), l.lora_up.weight.detach(), l.scale) for l in net.unet_loras}
    out = dict(cfg=cfg, model=model, net=net, x=x, ctx=ctx, pooled=pooled, lora=lora, h=h, w=w, nc=nc, refs={})
    _cache[name] = out
    return out


def refs(s, dt):
    """(ref, bar, ref_lora, bar_lora) for dt: the inputs and weights are first rounded to dt, as the engine receives them."""
    if dt in s["refs"]:
        return s["refs"][dt]
    sd = {k: v.to(dt) for k, v in s["model"].state_dict().items()}
    ctx, pooled = s["ctx"].to(dt), s["pooled"].to(dt)
    bar, ref = R.model_bar(sd, s["cfg"], s["x"], TS, ctx, pooled, dt)
    bar_l, ref_l = R.model_bar(sd, s["cfg"], s["x"], TS, ctx, pooled, dt, lora=s["lora"], mults=MULTS)
    s["refs"][dt] = (ref, bar, ref_l, bar_l)
    return s["refs"][dt]


def engine(s, dt, sites, batch=3):
    from sliders_conceptmod_amd import mmdit as M
    state = {k: v.detach().to("cuda", dt).contiguous() for k, v in s["model"].state_dict().items()}
    return M.MMDiTEngine(s["cfg"], dt, state, sites, batch, s["h"], s["w"], s["nc"], torch.device("cuda", 0))


def run(e, s, dt, idx=(0, 1, 2), lora=False, mults=None):
    i = list(idx)
    flat = s["net"].flat.detach().cuda()
    nd = s["net"]._n_down
    out = e.forward(s["x"][i].cuda(), [TS[k] for k in i], s["ctx"][i].to(dt).cuda(), s["pooled"][i].to(dt).cuda(),
                    flat[:nd] if lora else None, flat[nd:] if lora else None, mults)
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error, session stopped: {err}", returncode=3)
    return out


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_lora_against_fp64(name, dt):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    s = setup(name)
    ref, bar, ref_l, bar_l = refs(s, dt)
    e = engine(s, dt, s["net"].engine_sites())
    from sliders_conceptmod_amd import mmdit as M
    assert e.workspace_bytes == M.workspace_bytes(s["cfg"], dt, s["net"].engine_sites(), 3, s["h"], s["w"], s["nc"])
    plain = run(e, s, dt)
    err = R.rel_l2(plain.cpu(), ref)
    print(f"{name} {dt}: rel-L2 {err:.3e}, bar {bar:.3e}")
    assert torch.isfinite(plain).all() and err <= bar
    adapted = run(e, s, dt, lora=True, mults=MULTS)
    err_l = R.rel_l2(adapted.cpu(), ref_l)
    print(f"{name} {dt} LoRA (0, 1, -2): rel-L2 {err_l:.3e}, bar {bar_l:.3e}; adaptor moves the output by "
          f"{R.rel_l2(ref_l, ref):.3e}")
    assert torch.isfinite(adapted).all() and err_l <= bar_l
    assert R.rel_l2(ref_l, ref) > 4 * bar_l, "the adaptor must move the output far beyond the bar for this test to see it"
    # ---- bitwise properties
    assert torch.equal(adapted[0], plain[0]), "multiplier 0 inside an adapted batch"
    assert torch.equal(run(e, s, dt, lora=True, mults=[0.0, 0.0, 0.0]), plain), "all multipliers 0"
    assert torch.equal(run(e, s, dt, lora=False, mults=MULTS), plain), "NULL flat buffers"
    assert torch.equal(run(e, s, dt, lora=True, mults=MULTS), adapted), "two runs"
    for i in range(3):  # n below the creation batch; a sample alone == the sample in the batch
        assert torch.equal(run(e, s, dt, idx=(i,), lora=True, mults=[MULTS[i]])[0], adapted[i]), f"sample {i} alone"
    assert torch.equal(run(e, s, dt, idx=(2, 0), lora=True, mults=[MULTS[2], MULTS[0]]), adapted[[2, 0]]), "another order"
    e.close()
    e0 = engine(s, dt, [])  # an engine created without sites
    assert torch.equal(run(e0, s, dt), plain)
    assert torch.equal(run(e0, s, dt, lora=True, mults=MULTS), plain), "flat buffers given to an engine without sites"
    e0.close()


def test_module_forward_follows_the_network():
    """SD3Transformer2DModel.forward: the attached network at its multiplier (0 outside `with network:`)."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    s = setup("tiny_8x6_c5")
    dt = torch.float16
    from sliders_conceptmod_amd import lora as L
    from sliders_conceptmod_amd import mmdit as M
    model = M.SD3Transformer2DModel(s["cfg"])
    model.load_state_dict(s["model"].state_dict())
    model = model.to("cuda", dt)
    args = (s["x"].cuda(), TS, s["ctx"].to(dt).cuda(), s["pooled"].to(dt).cuda())
    frozen = model(*args).sample
    net = L.LoRANetwork(model, rank=4, alpha=2.0, train_method="full", context_stream=True).to("cuda")
    net.load_state_dict(s["net"].state_dict())
    net.__exit__(None, None, None)
    assert torch.equal(model(*args).sample, frozen)
    net.set_lora_slider(-2.0)
    with net:
        on = model(*args).sample
    e = engine(s, dt, s["net"].engine_sites())
    want = run(e, s, dt, lora=True, mults=[-2.0] * 3)
    e.close()
    assert torch.equal(on, want) and not torch.equal(on, frozen)
