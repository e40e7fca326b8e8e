"""The differentiable T5 tower (smi_t5_lora_*: LoRA on SelfAttention.{q,k,v} and SelfAttention.o, one multiplier per
sample, a saved pass and its backward) against torch autograd through the float64 tower of tests/t5_bwd_refs.py, on the
q / k-halved seeded state (see halved_state there), bf16.

Bar: relative L2 against the exact reference A at most notrigger_refs.bar(e_q) = 3 e_q + 1e-4, e_q being the distance from A
of the same reference with every stored tensor (values and gradients) rounded to bf16; over the whole gradient and per site
(down | up of the site).  tests/test_t5_bwd_refs_cpu.py shows which mutants miss it.  The ratio to the bar is printed."""
import functools

import pytest
import torch

import notrigger_refs as N
import t5_bwd_refs as B
import t5_refs as R

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
RANK = 4
WHICH = ("last_hidden", "penultimate")


def tiny64():
    from sliders_conceptmod_amd.t5 import tiny_t5_config
    c = tiny_t5_config(64)  # inner 128 != d_model 64
    return R.Cfg(vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, num_heads=c.num_heads, d_ff=c.d_ff,
                 num_layers=c.num_layers)


def wide():
    return R.Cfg(vocab_size=64, d_model=4096, d_kv=64, num_heads=64, d_ff=512, num_layers=1)


CFGS = {"test_cfg": R.test_cfg, "tiny64": tiny64, "wide": wide}


@functools.lru_cache(maxsize=None)
def state(cfg_name, halved=True):
    cfg = CFGS[cfg_name]()
    return cfg, (B.halved_state(cfg) if halved else R.seeded_state(cfg))


@functools.lru_cache(maxsize=None)
def case(cfg_name, L, mults, which, qkv_only=False, halved=True):
    """Inputs and both reference forms, formed once and shared (nothing below writes to them)."""
    cfg, sd = state(cfg_name, halved)
    names = B.site_names(cfg.num_layers, ("q", "k", "v") if qkv_only else B.SITE_PARTS)
    c = B.tower_case(cfg, sd, L, RANK, mults, which, DT, names)
    c["sites"], c["n_down"], c["n_up"] = B.flat_layout(cfg, names, RANK, RANK)
    c["down"], c["up"] = B.flatten_lora(c["lora"], names)
    return c


def engine(cfg_name, sites, max_tokens, batch=2, halved=True):
    from sliders_conceptmod_amd import _native
    cfg, sd = state(cfg_name, halved)
    st = {k: v.to(DT).cuda().contiguous() for k, v in sd.items()}
    return _native.T5LoraEngine(cfg, DT, st, sites, batch, max_tokens, torch.device("cuda"))


def run(eng, c, mults, which, between=None, dd=None, du=None):
    """One saved forward and its backward: (d_down, d_up) fp32 on the device, and the forward's outputs."""
    down, up = c["down"].cuda(), c["up"].cuda()  # (alive until the backward: it reads the saved pass's parameters again)
    out = eng.forward_lora(c["ids"], down, up, list(mults), save=True)
    if between is not None:
        between()
    dd = torch.zeros(c["n_down"], device="cuda") if dd is None else dd
    du = torch.zeros(c["n_up"], device="cuda") if du is None else du
    eng.backward(c["d_hidden"].float().contiguous().cuda(), dd, du, which=WHICH.index(which))
    torch.cuda.synchronize()
    return dd, du, out


def hold_to_bar(cfg, c, dd, du, which, tag):
    got = (dd.cpu(), du.cpu())
    assert torch.isfinite(torch.cat(got)).all()
    whole, _, _ = B.distance(cfg, c["names"], RANK, got, c["A"])
    print(f"{tag}: whole gradient e {whole:.3e}  e_q {c['e_q']:.3e}  e / bar {whole / N.bar(c['e_q']):.2f}")
    assert whole <= N.bar(c["e_q"]), (whole, c["e_q"])
    worst = 0.0
    last = f"encoder.block.{cfg.num_layers - 1}."
    for (nm, g), (_, a), (_, b) in zip(B.per_site(cfg, c["names"], RANK, *got), B.per_site(cfg, c["names"], RANK, *c["A"]),
                                       B.per_site(cfg, c["names"], RANK, *c["B"])):
        if float(a.abs().max()) == 0.0:  # penultimate: the last block's sites get exactly zero
            assert which == "penultimate" and nm.startswith(last) and float(g.abs().max()) == 0.0, nm
            continue
        e_s, eq_s = N.rel(g, a), N.rel(b, a)
        worst = max(worst, e_s / N.bar(eq_s))
        assert e_s <= N.bar(eq_s), (nm, e_s, eq_s)
    print(f"{tag}: worst per-site e / bar {worst:.2f}")


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("mults", ((1.0, -1.0), (0.0, 1.0)), ids=("pm1", "zero_one"))
@pytest.mark.parametrize("L", (5, 77, 130))
@pytest.mark.parametrize("cfg_name", ("test_cfg", "tiny64"))
def test_lora_gradients_against_f64_autograd(cfg_name, L, mults, which):
    cfg, _ = state(cfg_name)
    c = case(cfg_name, L, mults, which)
    eng = engine(cfg_name, c["sites"], 130)
    dd, du, out = run(eng, c, mults, which)
    hold_to_bar(cfg, c, dd, du, which, f"{cfg_name} L={L} {mults} {which}")
    if which == "last_hidden":  # the forward's outputs against the float64 tower under the same adaptor
        ref = B.tower_forward(cfg, c["sd"], c["ids"], c["lora"], mults, c["scale"])
        refq = B.tower_forward(cfg, c["sd"], c["ids"], c["lora"], mults, c["scale"], DT)
        for k in WHICH:
            assert N.rel(out[k], ref[k]) <= N.bar(N.rel(refq[k], ref[k])), k
    eng.close()


@pytest.mark.parametrize("which", WHICH)
def test_qkv_sites_only(which):
    cfg, _ = state("test_cfg")
    c = case("test_cfg", 77, (1.0, -1.0), which, True)
    eng = engine("test_cfg", c["sites"], 77)
    dd, du, _ = run(eng, c, (1.0, -1.0), which)
    hold_to_bar(cfg, c, dd, du, which, f"q|k|v only L=77 {which}")
    eng.close()


def test_wide_model():
    """d_model 4096, 64 heads: the workgroup-per-row norms and the fused attention backward on 64 heads."""
    cfg, _ = state("wide")
    c = case("wide", 70, (1.0, -1.0), "last_hidden")
    eng = engine("wide", c["sites"], 70)
    dd, du, _ = run(eng, c, (1.0, -1.0), "last_hidden")
    hold_to_bar(cfg, c, dd, du, "last_hidden", "wide L=70")
    eng.close()


def test_unhalved_state_to_its_own_bar():
    """The seeded state as it is (scores of standard deviation ~ 11, a saturated softmax): e_q is ten times larger, and so is
    the bar; the engine is held to it all the same."""
    cfg, _ = state("test_cfg", False)
    c = case("test_cfg", 77, (1.0, -1.0), "last_hidden", False, False)
    eng = engine("test_cfg", c["sites"], 77, halved=False)
    dd, du, _ = run(eng, c, (1.0, -1.0), "last_hidden")
    hold_to_bar(cfg, c, dd, du, "last_hidden", "unhalved L=77")
    eng.close()


def test_zero_multipliers_and_encode_give_the_frozen_bits():
    from sliders_conceptmod_amd import _native
    cfg, sd = state("test_cfg")
    c = case("test_cfg", 77, (1.0, -1.0), "last_hidden")
    eng = engine("test_cfg", c["sites"], 130)
    st = {k: v.to(DT).cuda().contiguous() for k, v in sd.items()}
    frozen = _native.T5Engine(cfg, DT, st, 2, 130, torch.device("cuda"))
    want = frozen.encode(c["ids"])
    got = eng.encode(c["ids"])  # smi_t5_encode on the LoRA engine
    zero = eng.forward_lora(c["ids"], c["down"].cuda(), c["up"].cuda(), [0.0, 0.0])
    on = eng.forward_lora(c["ids"], c["down"].cuda(), c["up"].cuda(), [1.0, -1.0])
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(want), bits(got)) and torch.equal(bits(want), bits(zero["last_hidden"]))
    assert not torch.equal(bits(on["last_hidden"]), bits(want))
    eng.close()
    frozen.close()


def test_saved_pass_contracts():
    """A no-grad call between forward and backward leaves the saved pass intact; the same call twice gives the same bits; a
    second backward is refused with -4; the backward accumulates."""
    from sliders_conceptmod_amd import _native
    c = case("test_cfg", 77, (1.0, -1.0), "last_hidden")
    eng = engine("test_cfg", c["sites"], 130)
    dd, du, _ = run(eng, c, (1.0, -1.0), "last_hidden")
    other = (c["down"] * 0.5).cuda()

    def between():  # a frozen encode, then an adapted no-grad pass with other parameters, multipliers and length
        eng.encode(c["ids"])
        eng.forward_lora(c["ids"][:, :40], other, c["up"].cuda(), [0.3, 2.0])

    dd2, du2, _ = run(eng, c, (1.0, -1.0), "last_hidden", between=between)
    assert torch.equal(dd, dd2) and torch.equal(du, du2)
    with pytest.raises(_native.SmiError, match=r"\(-4\).*no saved forward"):
        eng.backward(c["d_hidden"].float().cuda(), torch.zeros_like(dd), torch.zeros_like(du))
    # += : onto buffers that already hold a gradient, the sum (fp32 adds of the same addends: to rounding)
    dd3, du3, _ = run(eng, c, (1.0, -1.0), "last_hidden", dd=dd.clone(), du=du.clone())
    assert N.rel(dd3, 2 * dd) < 1e-6 and N.rel(du3, 2 * du) < 1e-6
    eng.close()


def test_refusals_leave_the_engine_working():
    from sliders_conceptmod_amd import _native
    cfg, _ = state("test_cfg")
    c = case("test_cfg", 77, (1.0, -1.0), "last_hidden")
    sites = c["sites"]
    with pytest.raises(_native.SmiError, match="DoRA site 'encoder.block.0.layer.0.SelfAttention.q'"):
        engine("test_cfg", [dict(s, off_dora=i * cfg.d_model) for i, s in enumerate(sites)], 77)
    with pytest.raises(_native.SmiError, match="rank 32 of"):
        engine("test_cfg", [dict(s, rank=32) for s in sites], 77)
    with pytest.raises(_native.SmiError, match="DenseReluDense.wo' -- sites sit on SelfAttention"):
        engine("test_cfg", sites + [dict(sites[-1], target="encoder.block.0.layer.1.DenseReluDense.wo")], 77)
    with pytest.raises(_native.SmiError, match="all or none"):
        engine("test_cfg", [s for s in sites if not s["target"].endswith("block.0.layer.0.SelfAttention.k")], 77)
    with pytest.raises(_native.SmiError, match="not a SelfAttention projection of this T5 encoder"):
        engine("test_cfg", sites + [dict(sites[-1], target="encoder.block.7.layer.0.SelfAttention.o")], 77)
    with pytest.raises(_native.SmiError, match="no LoRA sites"):
        engine("test_cfg", [], 77)
    eng = engine("test_cfg", sites, 77)
    down, up = c["down"].cuda(), c["up"].cuda()
    with pytest.raises(_native.SmiError, match="batch 3"):
        eng.forward_lora(R.seeded_ids(cfg, 3, 77), down, up, [1.0, 1.0, 1.0])
    with pytest.raises(_native.SmiError, match="L 78 outside"):
        eng.forward_lora(R.seeded_ids(cfg, 2, 78), down, up, [1.0, 1.0])
    with pytest.raises(_native.SmiError, match="which must be 0"):
        eng.backward(c["d_hidden"].float().cuda(), torch.zeros(c["n_down"], device="cuda"), torch.zeros(c["n_up"], device="cuda"), which=2)
    frozen = _native.T5Engine(cfg, DT, {k: v.to(DT).cuda().contiguous() for k, v in state("test_cfg")[1].items()}, 2, 77,
                              torch.device("cuda"))
    with pytest.raises(_native.SmiError, match="no LoRA sites"):
        _native.check(_native.lib().smi_t5_backward(frozen.handle, 0, _native.ptr(down), None, None), "smi_t5_backward")
    frozen.close()
    dd, du, _ = run(eng, c, (1.0, -1.0), "last_hidden")
    hold_to_bar(cfg, c, dd, du, "last_hidden", "after the refusals")
    eng.close()


def test_text_encoder_step_on_a_t5_tower():
    """notrigger.TextEncoderStep on t5.T5EncoderModel with a `t5attn` network: -1 is last_hidden (after the final norm), -2
    the penultimate state; the frozen targets are the plain encoder's bits; a backward fills network.flat.grad with what the
    engine gives directly; the model's own forward follows the attached network's multiplier."""
    from sliders_conceptmod_amd import lora, notrigger, t5
    dev = torch.device("cuda")
    model = t5.init_synthetic_(t5.T5EncoderModel(t5.tiny_t5_config(64), max_tokens=24), seed=5).to(dev, torch.bfloat16)
    ids = torch.randint(2, 1000, (2, 24), generator=torch.Generator().manual_seed(0))
    plain = model(ids)[0].clone()
    torch.manual_seed(0)
    net = lora.LoRANetwork(model, rank=4, alpha=4.0, target_replace=lora.T5_TARGET_REPLACE, prefix="lora_te2",
                           train_method="t5attn").to(dev)
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0.0, 0.05, generator=None)  # a non-zero up: the adaptor acts and down gets a gradient
    bits = lambda t: t.view(torch.int16)
    with net:  # (leaving the block sets the multiplier to 0, as after any sampled step)
        pass
    assert torch.equal(bits(model(ids)[0]), bits(plain))  # attached, multiplier 0 outside `with network:`
    for layer, which in ((-1, 0), (-2, 1)):
        step = notrigger.TextEncoderStep(model, net, layer)
        frozen = step.encode_frozen(ids)
        if layer == -1:
            assert torch.equal(frozen, plain.float())
        hidden = step.forward(ids, [1.0, -1.0])
        assert hidden.shape == (2, 24, 64) and not torch.equal(hidden.detach(), frozen)
        g = torch.randn(hidden.shape, generator=torch.Generator().manual_seed(1)).to(dev)
        net.flat.grad = None
        step.backward(g)
        got = net.flat.grad.clone()
        assert torch.isfinite(got).all() and float(got[:net._n_down].abs().max()) > 0 and float(got[net._n_down:].abs().max()) > 0
        eng = model.lora_engine(2)
        flat = net.flat.detach()
        eng.forward_lora(ids, flat[:net._n_down], flat[net._n_down:], [1.0, -1.0], save=True)
        dd, du = torch.zeros(net._n_down, device=dev), torch.zeros(net._n_up, device=dev)
        eng.backward(g.contiguous(), dd, du, which=which)
        assert torch.equal(got, torch.cat([dd, du]))
        with pytest.raises(Exception, match="one backward per forward"):
            step.backward(g)
    net.set_lora_slider(1.0)
    with net:
        assert not torch.equal(bits(model(ids)[0]), bits(plain))
