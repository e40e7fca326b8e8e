"""Slider composition end to end on the engine: a compose.SliderStack of two sliders against the CPU oracle with both
`LoRANetworkRef`s entered on one UNet (the reference's way of composing), and the properties the one-pass grid rests on.

Parity bars are those of tests/test_engine_gpu.py::test_forward_parity_lora_off_and_on: relative L2 error against the pure
fp32 oracle below 1.5 x the oracle's own storage-rounding error e_q (+ 1e-4) and below LOOSE[dtype].
tests/test_compose_cpu.py shows on the oracle alone that the fp16 bar sees a dropped slider at >= 13 multiples; bf16 is a parity
arm only (1.8 to 3.4 multiples)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import compose_refs as CR

from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import compose as CO

LOOSE = {torch.float16: 1.8e-3, torch.bfloat16: 1.4e-2}  # tests/test_engine_gpu.py
T = 499.0
CASES = [(m, p) for m in CR.CFGS for p in CR.PAIRS] + [("tiny_sdxl", "r4r4")]


def pair_of(name):
    return CR.PAIR_44 if name == "r4r4" else CR.PAIRS[name]


def cuda_add(add):
    return None if add is None else {k: v.cuda() for k, v in add.items()}


@pytest.fixture(scope="module")
def refs():
    """Per (model, pair): the oracle objects and the fp32 / rounded oracle outputs at scales (+2, -2) -- computed once on the
    CPU, shared by the tests, never modified."""
    out = {}
    for model, pair in CASES:
        ocfg, ou, nets, states = CR.oracle_pair(model, pair_of(pair))
        x, ctx, add = CR.inputs(ocfg, 2, 16)
        d = {"ocfg": ocfg, "ou": ou, "states": states, "x": x, "ctx": ctx, "add": add,
             "ref32": CR.oracle_eps(ou, nets, CR.SCALES, x, T, ctx, add)}
        for dt in (torch.float16, torch.bfloat16):
            d[dt] = CR.oracle_eps(ou, nets, CR.SCALES, x, T, ctx, add, storage_dtype=dt)
        out[model, pair] = d
    return out


def engine_args(r, dtype, n=None):
    """(sample, ctx, text_embeds, time_ids) as the engine takes them, the first n samples."""
    x, ctx, add = r["x"], r["ctx"], cuda_add(r["add"])
    sl = slice(0, n)
    te = ti = None
    if add is not None:
        te, ti = add["text_embeds"][sl].to(dtype).contiguous(), add["time_ids"][sl].float().contiguous()
    return x[sl].cuda().float().contiguous(), ctx[sl].cuda().to(dtype).contiguous(), te, ti


@pytest.mark.parametrize("model,pair", CASES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_stack_parity_against_chained_oracle_networks(refs, model, pair, dtype):
    r = refs[model, pair]
    pu = CR.product_unet(r["ocfg"], r["ou"], dtype, "cuda")
    stack = CO.SliderStack(pu, r["states"])
    ranks = [p[1] for p in pair_of(pair)]
    assert stack.ranks == ranks and not stack.fold
    # the stacked buffers are the plain-torch layout, bit for bit
    down, up = CR.stack_reference(stack.plan, stack.sliders, lambda s: CO.site_coefs(stack.sliders, s))
    assert torch.equal(stack.flat_down.cpu(), down) and torch.equal(stack.flat_up.cpu(), up)
    stack.set_scales(CR.SCALES)
    with torch.no_grad(), stack:
        got = pu(r["x"].cuda(), T, encoder_hidden_states=r["ctx"].cuda(), added_cond_kwargs=cuda_add(r["add"])).sample
    ref32, refq = r["ref32"], r[dtype]
    assert got.dtype == torch.float32 and got.shape == ref32.shape
    e_eng, e_q = CR.rel(got, ref32), CR.rel(refq, ref32)
    print(f"{model} {pair} {dtype}: engine-fp32 {e_eng:.2e}  rounded_oracle-fp32 {e_q:.2e}")
    assert e_eng < LOOSE[dtype], f"vs fp32 oracle {e_eng:.2e}"
    assert e_eng < 1.5 * e_q + 1e-4, f"engine noisier than its storage rounding explains: {e_eng:.2e} vs {e_q:.2e}"
    # leaving the block switches the adaptor off; the scales really act
    with torch.no_grad():
        off = pu(r["x"].cuda(), T, encoder_hidden_states=r["ctx"].cuda(), added_cond_kwargs=cuda_add(r["add"])).sample
    assert CR.rel(got, off) > 1e-3


@pytest.mark.parametrize("model,pair", CASES)
def test_grid_in_one_pass_equals_separate_passes_and_zero_is_off(refs, model, pair):
    """A 2 x 2 grid of scales as ONE forward_compose of 4 samples is torch.equal to four one-sample passes (per-sample
    arithmetic does not depend on the batch composition: the table only multiplies a sample's own xa columns), and a row of
    zero multipliers gives the eps of the adaptor-off pass bit for bit (0 * xa adds exact zeros in the epilogue's fmaf)."""
    dtype = torch.float16
    r = refs[model, pair]
    ocfg = r["ocfg"]
    x, ctx, add = CR.inputs(ocfg, 4, 16, seed=7)
    r4 = {"x": x, "ctx": ctx, "add": add}
    pu = CR.product_unet(ocfg, r["ou"], dtype, "cuda")
    stack = CO.SliderStack(pu, r["states"])
    flat, n_down, _ = stack.engine_params()
    down, up = flat[:n_down], flat[n_down:]
    eng = pu._ensure_engine(4, 16, 16, 77)
    xs, cs, te, ti = engine_args(r4, dtype)
    grid = [[0.0, 0.0], [0.0, 2.0], [2.0, 0.0], [2.0, -1.5]]
    one = eng.forward_compose(xs, T, cs, te, ti, down, up, stack.ranks, grid)
    parts = []
    for i in range(4):
        sl = slice(i, i + 1)
        parts.append(eng.forward_compose(xs[sl].contiguous(), T, cs[sl].contiguous(),
                                         None if te is None else te[sl].contiguous(),
                                         None if ti is None else ti[sl].contiguous(), down, up, stack.ranks, [grid[i]]))
    assert torch.equal(one, torch.cat(parts)), "the multiplier table changed a sample's arithmetic"
    # zero is off: against a pass without an adaptor
    off = eng.forward(xs, T, cs, te, ti, None, None, 0.0, False)
    assert torch.equal(one[0], off[0])
    zero = eng.forward_compose(xs, T, cs, te, ti, down, up, stack.ranks, [[0.0, 0.0]] * 4)
    assert torch.equal(zero, off)
    # the scales act: same sample, other row
    other = eng.forward_compose(xs, T, cs, te, ti, down, up, stack.ranks, [[2.0, 0.0]] + grid[1:])
    assert CR.rel(other[0], one[0]) > 1e-4 and torch.equal(other[1:], one[1:])
    # through the module: set_scale_grid routes to the same call
    stack.set_scale_grid(grid)
    with torch.no_grad(), stack:
        via = pu(x.cuda(), T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
    assert torch.equal(via, one)


def test_slider_grid_latents_equals_each_cell_alone(refs):
    """4 DDIM steps, 2 of them above start_noise (adaptor off, run once and broadcast), a 2 x 2 grid in one pass per step and
    in chunks: torch.equal to every cell on its own."""
    from sliders_conceptmod_amd import model_util, train_util
    dtype = torch.float16
    r = refs["tiny_sd1x", "overlap"]
    pu = CR.product_unet(r["ocfg"], r["ou"], dtype, "cuda")
    stack = CO.SliderStack(pu, r["states"])
    sched = model_util.create_noise_scheduler("ddim")
    sched.set_timesteps(4)
    ts = [int(t) for t in sched.timesteps]
    start_noise = (ts[1] + ts[2]) // 2
    assert sum(t > start_noise for t in ts) == 2
    g = torch.Generator().manual_seed(21)
    ns = 2
    lat = torch.randn(ns, 4, 16, 16, generator=g).cuda()
    unc, cond = torch.randn(1, 77, 64, generator=g), torch.randn(1, 77, 64, generator=g)
    te = train_util.concat_embeddings(unc, cond, ns).cuda().to(dtype)
    cells = [(0, 0), (0, 2), (2, 0), (2, -2)]
    kw = dict(guidance_scale=3.0, num_inference_steps=4)
    stack.set_scales([0.5, -1.0])
    grid = train_util.slider_grid_latents(pu, stack, sched, lat, te, cells, start_noise, **kw)
    assert stack.scale_state() == ([0.5, -1.0], None)  # the caller's scales are put back
    assert grid.shape == (4, ns, 4, 16, 16)
    chunked = train_util.slider_grid_latents(pu, stack, sched, lat, te, cells, start_noise, max_batch=2 * ns * 2, **kw)
    assert torch.equal(chunked, grid)
    for i, cell in enumerate(cells):
        alone = train_util.slider_grid_latents(pu, stack, sched, lat, te, [cell], start_noise, **kw)
        assert torch.equal(alone[0], grid[i]), f"cell {cell}"
    assert CR.rel(grid[3], grid[0]) > 1e-3 and CR.rel(grid[1], grid[2]) > 1e-3


def c3lier_pair():
    ocfg, ou, nets, states = CR.oracle_pair("tiny_sd1x", (("noxattn", 4, 1.0), ("noxattn", 8, 4.0)), c3lier=True)
    return ocfg, ou, nets, states


def test_c3lier_stack_folds_scales_and_refuses_unequal_rows():
    dtype = torch.float16
    ocfg, ou, nets, states = c3lier_pair()
    x, ctx, add = CR.inputs(ocfg, 2, 16)
    scales = (1.5, -1.0)
    ref32 = CR.oracle_eps(ou, nets, scales, x, T, ctx, add)
    refq = CR.oracle_eps(ou, nets, scales, x, T, ctx, add, storage_dtype=dtype)
    pu = CR.product_unet(ocfg, ou, dtype, "cuda")
    stack = CO.SliderStack(pu, states)
    assert stack.fold and stack.plan.has_conv
    stack.set_scales(scales)
    with torch.no_grad(), stack:
        got = pu(x.cuda(), T, encoder_hidden_states=ctx.cuda()).sample
    down, up = CR.stack_reference(stack.plan, stack.sliders, lambda s: CO.site_coefs(stack.sliders, s, scales))
    assert torch.equal(stack.flat_down.cpu(), down) and torch.equal(stack.flat_up.cpu(), up)
    e_eng, e_q = CR.rel(got, ref32), CR.rel(refq, ref32)
    print(f"c3lier stack fp16: engine-fp32 {e_eng:.2e}  rounded_oracle-fp32 {e_q:.2e}")
    assert e_eng < LOOSE[dtype] and e_eng < 1.5 * e_q + 1e-4
    # other scales: one re-stack, and the output follows
    stack.set_scales((0.0, 0.0))
    with torch.no_grad(), stack:
        zero = pu(x.cuda(), T, encoder_hidden_states=ctx.cuda()).sample
    with torch.no_grad():
        off = pu(x.cuda(), T, encoder_hidden_states=ctx.cuda()).sample
    assert CR.rel(zero, off) < 1e-6 and CR.rel(got, off) > 1e-3
    # a grid with unequal rows: refused by the stack; the engine entry point refuses conv sites altogether
    with pytest.raises(ValueError, match="conv"):
        stack.set_scale_grid([[1.0, 1.0], [1.0, 2.0]])
    stack.set_scale_grid([[1.0, 2.0], [1.0, 2.0]])  # equal rows are scales
    flat, n_down, _ = stack.engine_params()
    eng = pu._ensure_engine(2, 16, 16, 77)
    xs, cs = x.cuda().float().contiguous(), ctx.cuda().to(dtype).contiguous()
    with pytest.raises(_native.SmiError, match="conv or DoRA"):
        eng.forward_compose(xs, T, cs, None, None, flat[:n_down], flat[n_down:], [4, 8], [[1.0, 1.0], [1.0, 2.0]])
    with pytest.raises(_native.SmiError, match="conv or DoRA"):  # equal rows too: the conv sites would not see them
        eng.forward_compose(xs, T, cs, None, None, flat[:n_down], flat[n_down:], [4, 8], [[2.0, -2.0], [2.0, -2.0]])


def test_compose_errors(refs):
    dtype = torch.float16
    r = refs["tiny_sd1x", "disjoint"]
    pu = CR.product_unet(r["ocfg"], r["ou"], dtype, "cuda")
    stack = CO.SliderStack(pu, r["states"])
    flat, n_down, _ = stack.engine_params()
    down, up = flat[:n_down], flat[n_down:]
    eng = pu._ensure_engine(2, 16, 16, 77)
    xs, cs, te, ti = engine_args(r, dtype)
    with pytest.raises(_native.SmiError, match="ranks sum to 8"):
        eng.forward_compose(xs, T, cs, te, ti, down, up, [4, 4], [[1.0, 1.0]] * 2)
    with pytest.raises(_native.SmiError, match="adapted samples"):
        eng.forward_compose(xs, T, cs, te, ti, down, up, [4, 8], [], n_adapted=0)
    with pytest.raises(_native.SmiError, match="rows"):
        eng.forward_compose(xs, T, cs, te, ti, down, up, [4, 8], [[1.0, 1.0]])
    # inference only: a backward after a compose pass fails as after any pass that saved nothing
    eng.forward_compose(xs, T, cs, te, ti, down, up, [4, 8], [[1.0, 1.0]] * 2)
    g = torch.zeros_like(flat)
    with pytest.raises(_native.SmiError, match="no saved forward pass"):
        eng.backward(torch.zeros(2, 4, 16, 16, device="cuda"), g[:n_down], g[n_down:])
    # also when an earlier pass had saved one
    eng.forward(xs, T, cs, te, ti, down, up, 1.0, True)
    eng.forward_compose(xs, T, cs, te, ti, down, up, [4, 8], [[1.0, 1.0]] * 2)
    with pytest.raises(_native.SmiError, match="no saved forward pass"):
        eng.backward(torch.zeros(2, 4, 16, 16, device="cuda"), g[:n_down], g[n_down:])
    assert not g.any()
