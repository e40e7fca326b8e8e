"""The trainable Flux engine (smi_flux_train_create / _forward_save / _backward) on a real MI355X: the LoRA gradients against
float64 autograd through the forward restatement (form A of tests/flux_bwd_refs.py), whole vector and per site, each under
bar = 3 e_q + 1e-4 with e_q the storage twin's (form B) distance from A on the same part; and the contracts of the ABI
(bit-equal outputs, the pass kept across a no-grad forward, accumulation, -4 without a pass, nothing added at multiplier 0,
the forward-only workspace unchanged).

Shapes: tiny_flux (d 128, two double and two single blocks), rank 4, at an 8 x 6 latent with 5 context tokens, n = 3,
multipliers (0, 1, -2) (joint length 17: ragged tiles everywhere), and at 16 x 16 with 13 tokens, n = 2 (77 keys: two key
tiles); one double and one single block at d 3072 (24 x 128) at 8 x 8 with 5 tokens, n = 2, without and with the guidance
embedder.  Each in both dtypes and with both site sets (the attention projections of the image stream and the single blocks;
those plus the context stream's)."""
import pytest
import torch

import flux_bwd_refs as B

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
RANK, ALPHA = 4, 2.0
SHAPES = {"tiny_8x6_c5_n3": ("tiny", 8, 6, 5, [0.0, 1.0, -2.0]), "tiny_16x16_c13_n2": ("tiny", 16, 16, 13, [1.0, -2.0]),
          "wide_8x8_c5_n2": ("wide", 8, 8, 5, [1.0, -2.0]), "wide_guidance_8x8_c5_n2": ("wide_g", 8, 8, 5, [1.0, -2.0])}
FORMS = {"image": False, "context": True}
# smi_flux_workspace_bytes of the PARENT commit for the tiny config, n = 3, 8 x 6, 5 context tokens, rank 4 (by site set; None:
# no sites), from a run of a build of that commit
PARENT_BYTES = {False: 1335296, True: 1392640, None: 1245184}


def make_cfg(kind):
    from sliders_conceptmod_amd import flux as M
    if kind == "tiny":
        return M.tiny_flux_config()
    return M.FluxConfig(num_layers=1, num_single_layers=1, guidance_embeds=kind == "wide_g")  # d 3072 = 24 x 128


_cache = {}


def setup(name, form, dt):
    """Per (shape, form, dtype), made once and left unchanged: model, sites, LoRA values, inputs, form A and the bars."""
    key = (name, form, dt)
    if key in _cache:
        return _cache[key]
    from sliders_conceptmod_amd import flux as M
    kind, h, w, nc, mults = SHAPES[name]
    cfg = make_cfg(kind)
    model = M.init_synthetic_(M.FluxTransformer2DModel(cfg), seed=3)
    state = {k: v.to(dt) for k, v in model.state_dict().items()}  # what the engine receives
    sd = {k: v.double() for k, v in state.items()}
    names = B.site_names(cfg.num_layers, cfg.num_single_layers, FORMS[form])
    lora = B.make_lora(names, cfg.inner_dim, RANK, ALPHA, torch.Generator().manual_seed(11))
    x, ts, gd, ctx, pooled, d_out = B.tiny_inputs(cfg, len(mults), h, w, nc, seed=13)
    args = (sd, cfg, x, ts, gd, ctx, pooled, lora, names, mults, d_out)
    a = B.grads_a(*args)
    b = B.grads_twin(*args, dt=dt)
    bars = {k: B.bar(B.rel(v, parts(a, names)[k])) for k, v in parts(b, names).items()}
    sites, n_down, n_up = B.flat_layout(names, cfg.inner_dim, RANK, ALPHA)
    s = dict(cfg=cfg, state=state, names=names, lora=lora, x=x, ts=ts, gd=gd, ctx=ctx, pooled=pooled, d_out=d_out, mults=mults,
             a=parts(a, names), out_a=a[3], bars=bars, sites=sites, n_down=n_down, n_up=n_up, h=h, w=w, nc=nc)
    _cache[key] = s
    return s


def parts(res, names):
    """The whole gradient vector (down | up) and each site's (down, up) pair, from (flat down, flat up, per-site dict, ...)."""
    out = {"whole": torch.cat([res[0], res[1]])}
    for nm in names:
        out[nm] = torch.cat([res[2][nm][0].reshape(-1), res[2][nm][1].reshape(-1)])
    return out


def engine_parts(s, gd, gu):
    """The same parts from the engine's two flat buffers (the layout of B.flat_layout)."""
    gd, gu = gd.double().cpu(), gu.double().cpu()
    per = {}
    d, r = s["cfg"].inner_dim, RANK
    for site in s["sites"]:
        per[site["target"]] = (gd[site["off_down"]:site["off_down"] + r * d], gu[site["off_up"]:site["off_up"] + d * r])
    return parts((gd, gu, per), s["names"])


def engine(s, dt, trainable=True, batch=None):
    from sliders_conceptmod_amd import flux as M
    state = {k: v.detach().to("cuda").contiguous() for k, v in s["state"].items()}
    return M.FluxEngine(s["cfg"], dt, state, s["sites"], batch or len(s["mults"]), s["h"], s["w"], s["nc"],
                        torch.device("cuda", 0), trainable=trainable)


def sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error, session stopped: {err}", returncode=3)


def flats(s):
    down, up = B.flatten_lora(s["lora"], s["names"])
    return down.cuda(), up.cuda()


def fwd(e, s, dt, down, up, mults, idx=None, save=False):
    i = list(range(len(s["mults"]))) if idx is None else list(idx)
    fn = e.forward_save if save else e.forward
    gd = None if s["gd"] is None else [s["gd"][k] for k in i]
    out = fn(s["x"][i].cuda(), [s["ts"][k] for k in i], gd, s["ctx"][i].to(dt).cuda(), s["pooled"][i].to(dt).cuda(), down, up,
             mults)
    sync()
    return out


def bwd(e, s, idx=None, fill=0.0):
    i = list(range(len(s["mults"]))) if idx is None else list(idx)
    gd = torch.full((s["n_down"],), fill, dtype=torch.float32, device="cuda")
    gu = torch.full((s["n_up"],), fill, dtype=torch.float32, device="cuda")
    e.backward(s["d_out"][i].cuda(), gd, gu)
    sync()
    return gd, gu


def check_parts(s, got, what):
    for k, v in got.items():
        err = B.rel(v, s["a"][k])
        if k == "whole" or err > 0.5 * s["bars"][k]:
            print(f"{what} {k}: rel {err:.3e}, bar {s['bars'][k]:.3e}")
        assert torch.isfinite(v).all() and err <= s["bars"][k], f"{what} {k}: rel {err:.3e} > bar {s['bars'][k]:.3e}"


def run_case(name, form, dt):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    s = setup(name, form, dt)
    e = engine(s, dt)
    down, up = flats(s)
    out = fwd(e, s, dt, down, up, s["mults"], save=True)
    gd, gu = bwd(e, s)
    print(f"{name} {form} {dt}: output rel {B.rel(out, s['out_a']):.3e}, workspace {e.workspace_bytes} bytes")
    got = engine_parts(s, gd, gu)
    check_parts(s, got, f"{name} {form} {dt}")
    for k, v in got.items():
        if float(s["a"][k].abs().max()) > 0:
            assert float(v.abs().max()) > 0, f"{k} took no gradient"
    e.close()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["tiny_8x6_c5_n3", "tiny_16x16_c13_n2"])
def test_lora_gradients_against_fp64(name, form, dt):
    run_case(name, form, dt)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["wide_8x8_c5_n2", "wide_guidance_8x8_c5_n2"])
def test_wide_model_gradients_against_fp64(name, form, dt):
    run_case(name, form, dt)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_saved_pass_contracts(dt):
    """forward_save == forward in bits; a no-grad forward between save and backward changes no gradient bit; the backward
    adds to what the buffers hold; a second backward has no pass (-4); multipliers 0 and NULL flat buffers add nothing; the
    forward-only engine keeps the parent commit's workspace size and gives the trainable engine's forward bits."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import _native
    s = setup("tiny_8x6_c5_n3", "context", dt)
    e = engine(s, dt)
    down, up = flats(s)
    plain = fwd(e, s, dt, down, up, s["mults"])
    saved = fwd(e, s, dt, down, up, s["mults"], save=True)
    assert torch.equal(saved, plain)
    gd, gu = bwd(e, s)
    assert float(gd.abs().max()) > 0 and float(gu.abs().max()) > 0
    with pytest.raises(_native.SmiError, match=r"\(-4\)"):
        bwd(e, s)
    # a no-grad pass of other samples at other multipliers in between
    fwd(e, s, dt, down, up, s["mults"], save=True)
    other = fwd(e, s, dt, down, up, [1.0, 1.0], idx=(2, 0))
    assert torch.isfinite(other).all()
    gd2, gu2 = bwd(e, s)
    assert torch.equal(gd2, gd) and torch.equal(gu2, gu)
    # accumulation: pre-filled buffers get the gradient added (one fp32 addition per element)
    fwd(e, s, dt, down, up, s["mults"], save=True)
    fd, fu = bwd(e, s, fill=0.5)
    for f, g in ((fd, gd), (fu, gu)):
        assert float(((f - 0.5) - g).abs().max()) <= 2.0 ** -23 * float(0.5 + g.abs().max())
    # nothing to differentiate: every multiplier 0, or no flat buffers
    frozen = fwd(e, s, dt, down, up, [0.0, 0.0, 0.0], save=True)
    zd, zu = bwd(e, s, fill=0.25)
    assert bool((zd == 0.25).all()) and bool((zu == 0.25).all())
    assert torch.equal(fwd(e, s, dt, None, None, s["mults"], save=True), frozen)
    zd, zu = bwd(e, s, fill=0.25)
    assert bool((zd == 0.25).all()) and bool((zu == 0.25).all())
    # an engine from smi_flux_create: the parent's workspace, the same output bits as the trainable engine's forward
    e0 = engine(s, dt, trainable=False)
    assert e0.workspace_bytes == PARENT_BYTES[True]
    assert torch.equal(fwd(e0, s, dt, down, up, s["mults"]), plain)
    assert torch.equal(fwd(e0, s, dt, None, None, None), frozen)
    with pytest.raises(_native.SmiError, match="keeps no pass"):
        fwd(e0, s, dt, down, up, s["mults"], save=True)
    e0.close()
    e.close()


def test_forward_only_workspace_is_the_parents():
    from sliders_conceptmod_amd import flux as M
    cfg = M.tiny_flux_config()
    for cs in (False, True):
        sites = B.flat_layout(B.site_names(cfg.num_layers, cfg.num_single_layers, cs), cfg.inner_dim, RANK, ALPHA)[0]
        assert M.workspace_bytes(cfg, torch.float16, sites, 3, 8, 6, 5) == PARENT_BYTES[cs]
    assert M.workspace_bytes(cfg, torch.float16, [], 3, 8, 6, 5) == PARENT_BYTES[None]


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_one_pass_of_two_samples_against_two_passes_of_one(dt):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    s = setup("tiny_16x16_c13_n2", "context", dt)
    e = engine(s, dt)
    down, up = flats(s)
    both_out = fwd(e, s, dt, down, up, s["mults"], save=True)
    both = engine_parts(s, *bwd(e, s))
    gd = torch.zeros(s["n_down"], dtype=torch.float32, device="cuda")
    gu = torch.zeros(s["n_up"], dtype=torch.float32, device="cuda")
    for i in range(2):  # the second backward adds to the first one's buffers
        one = fwd(e, s, dt, down, up, [s["mults"][i]], idx=(i,), save=True)
        assert torch.equal(one[0], both_out[i]), "a sample has the same bits alone and in a batch"
        e.backward(s["d_out"][[i]].cuda(), gd, gu)
        sync()
    apart = engine_parts(s, gd, gu)
    for k in both:
        err = B.rel(apart[k], both[k])
        assert err <= s["bars"][k], f"{k}: {err:.3e} > {s['bars'][k]:.3e}"
    check_parts(s, apart, f"two passes of one sample {dt}")
    e.close()


def test_module_backward_reaches_the_network_parameter():
    """FluxTransformer2DModel.forward with grad enabled and a network attached: the output carries the gradient to the
    network's flat parameter, under the engine's bars."""
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import flux as M
    from sliders_conceptmod_amd import lora as L
    dt = torch.float16
    s = setup("tiny_8x6_c5_n3", "image", dt)
    model = M.FluxTransformer2DModel(s["cfg"])
    model.load_state_dict(s["state"])
    model = model.to("cuda", dt).requires_grad_(False)
    net = L.LoRANetwork(model, rank=RANK, alpha=ALPHA, delimiter="-", train_method="full").to("cuda")
    assert len(net.unet_loras) == len(s["names"]) == 14
    with torch.no_grad():
        for l in net.unet_loras:
            dn, up, _sc = s["lora"][l.target_path]
            l.lora_down.weight.copy_(dn)
            l.lora_up.weight.copy_(up)
    kw = dict(pooled_projections=s["pooled"].to(dt).cuda(), encoder_hidden_states=s["ctx"].to(dt).cuda(), multipliers=s["mults"])
    out = model(s["x"].cuda(), s["ts"], **kw).sample
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(model(s["x"].cuda(), s["ts"], **kw).sample, out)
    (out * s["d_out"].cuda()).sum().backward()
    sync()
    got = {l.target_path: (net.flat.grad[l.off_down:l.off_down + RANK * l.in_dim],
                           net.flat.grad[net._n_down + l.off_up:net._n_down + l.off_up + l.out_dim * RANK]) for l in net.unet_loras}
    res = (torch.cat([got[n][0] for n in s["names"]]).double().cpu(), torch.cat([got[n][1] for n in s["names"]]).double().cpu(),
           {n: (got[n][0].double().cpu(), got[n][1].double().cpu()) for n in s["names"]})
    check_parts(s, parts(res, s["names"]), "module backward")
    with pytest.raises(Exception, match="saved activations are gone"):
        out2 = model(s["x"].cuda(), s["ts"], **kw).sample
        model(s["x"].cuda(), s["ts"], **kw)  # a later grad-enabled forward takes the engine's one pass
        out2.sum().backward()
