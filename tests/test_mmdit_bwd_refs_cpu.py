"""The references of the SD3 MMDiT backward (tests/mmdit_bwd_refs.py) judged on the CPU, and the host-only parts of the
trainable engine: the dry run, its refusals, the new symbols.

Tiny model (d 128, two layers), 8 x 6 latent, 5 context tokens, n = 3, multipliers (0, 1, -2), rank 4, lora_up seeded non-zero,
all 15 sites (191-module form).  Seeds: model 3, LoRA 11, inputs 13.  The GPU test holds the engine's gradient to form A on the
whole vector AND on each site's (down, up) pair, each under its own bar = 3 e_q + 1e-4, e_q = rel(B, A) of that part; so a
mutant counts as caught where its worst part stands.  Measured here:
    form B fp16   whole e_q 1.14e-3  bar 3.5e-3   widest site e_q 1.5e-3
    form B bf16   whole e_q 9.08e-3  bar 2.7e-2   widest site e_q 1.1e-2
    mutants, distance from A in units of the bf16 bar (the wider one) of the part: whole vector / worst part
      drop_mean_g        2.7 x /   8.5 x (block 0 to_add_out)      drop_mean_gx    4.1 x /  8.9 x (block 0 add_q_proj)
      bwd_scale_no_one  12.5 x /  20.1 x (block 0 to_add_out)      bwd_drop_gate   157 x /  645 x (block 0 to_add_out)
      cut_ctx_split      1.3 x /  30.6 x (block 0 add_q_proj)      drop_add       36.5 x / 47.1 x (block 1 to_v)
      abs_mult          34.2 x /  42.8 x (block 1 to_out.0)
    (cut_ctx_split moves only what lies upstream of block 0's context output: the whole vector hides it, the per-site
    comparison does not.)  The last block's add_q_proj takes no gradient at all: its context output is dropped.
Erf-for-tanh in act' is held by the kernel bound (test_erf_gelu_grad_leaves_the_kernel_bound), as in the forward."""
import pytest
import torch

import mmdit_bwd_refs as B
import mmdit_refs as R
from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import mmdit as M

MULTS = [0.0, 1.0, -2.0]
RANK, ALPHA = 4, 2.0
# the last block drops its context output, so nothing downstream reads that block's context queries
DEAD = "transformer_blocks.1.attn.add_q_proj"


@pytest.fixture(scope="module")
def tiny():
    cfg = M.tiny_sd3_config()
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=3)
    sd = {k: v.double() for k, v in model.state_dict().items()}
    names = B.site_names(cfg.num_layers, context_stream=True)
    lora = B.make_lora(names, cfg.inner_dim, RANK, ALPHA, torch.Generator().manual_seed(11))
    x, ts, ctx, pooled, d_out = B.tiny_inputs(cfg, 3, 8, 6, 5, seed=13)
    args = (sd, cfg, x, ts, ctx, pooled, lora, names, MULTS, d_out)
    res = B.grads_a(*args)
    return dict(cfg=cfg, args=args, names=names, a=_vec(res), parts=_parts(res, names), out=res[3])


def _vec(res):
    return torch.cat([res[0], res[1]])


def _parts(res, names):
    """What the GPU test compares: the whole gradient vector, and each site's (down, up) pair."""
    out = {"whole": _vec(res)}
    for nm in names:
        out[nm] = torch.cat([res[2][nm][0].reshape(-1), res[2][nm][1].reshape(-1)])
    return out


def test_twin_without_roundings_is_form_a(tiny):
    res = B.grads_twin(*tiny["args"])
    assert B.rel(res[3], tiny["out"]) < 1e-12
    assert B.rel(_vec(res), tiny["a"]) < 1e-12
    assert float(tiny["a"].norm()) > 0


def test_twin_forward_rounds_where_the_forward_restatement_does(tiny):
    sd, cfg, x, ts, ctx, pooled, lora, names, mults, _ = tiny["args"]
    for dt in (torch.float16, torch.bfloat16):
        want = R.forward(sd, cfg, x, ts, ctx, pooled, dt=dt, lora=lora, mults=mults)
        got = B.twin_forward(sd, cfg, x, ts, ctx, pooled, lora, mults, dt=dt)
        assert torch.equal(got.detach(), want)


@pytest.fixture(scope="module")
def bars(tiny):
    """{dt: {part: (e_q, bar)}}: the whole vector and every site, as the GPU test holds the engine."""
    out = {}
    for dt in (torch.float16, torch.bfloat16):
        b = _parts(B.grads_twin(*tiny["args"], dt=dt), tiny["names"])
        out[dt] = {k: (B.rel(v, tiny["parts"][k]), B.bar(B.rel(v, tiny["parts"][k]))) for k, v in b.items()}
        worst = max(out[dt].values())
        print(f"form B {dt}: whole e_q {out[dt]['whole'][0]:.3e} bar {out[dt]['whole'][1]:.3e}; widest site e_q {worst[0]:.3e}")
    return out


def test_form_b_lies_inside_the_bar(tiny, bars):
    for dt, parts in bars.items():
        for k, (e_q, bar) in parts.items():
            if k == DEAD:  # no gradient reaches it: zero in every form
                assert float(tiny["parts"][k].abs().max()) == 0 and e_q == 0
                continue
            assert 0 < e_q <= bar, k
            assert bar < 0.1, f"{k}: a bar this wide would accept anything"


@pytest.mark.parametrize("mut", B.BWD_MUTATIONS)
def test_mutated_backward_lies_outside_the_bar(tiny, bars, mut):
    res = B.grads_twin(*tiny["args"], mut=mut)
    assert B.rel(res[3], tiny["out"]) < 1e-12, "a backward mutation leaves the forward alone"
    got = _parts(res, tiny["names"])
    # the GPU test asserts every part under its bar: a mutant is caught where its worst part stands, in units of the wider
    # (bf16) bar of that part
    ratio = {k: B.rel(v, tiny["parts"][k]) / bars[torch.bfloat16][k][1] for k, v in got.items()}
    k = max(ratio, key=ratio.get)
    print(f"{mut}: whole vector {ratio['whole']:.1f} x its bar; worst part {k} {ratio[k]:.1f} x")
    assert ratio[k] >= 2


def test_joint_path_carries_gradient_to_block_0(tiny, bars):
    """With the image stream's sites only (the 96-module form) block 0's to_q takes a gradient, and block 0's to_k / to_v take
    part of theirs through the context stream (block 0's context output reads the image keys and values and feeds block 1's
    context keys and values): cutting the context gradient at the split changes them.  (to_q itself is not read by the
    context rows of the attention output.)"""
    sd, cfg, x, ts, ctx, pooled, lora, _names, mults, d_out = tiny["args"]
    names = B.site_names(cfg.num_layers, context_stream=False)
    sub = {k: lora[k] for k in names}
    full = B.grads_twin(sd, cfg, x, ts, ctx, pooled, sub, names, mults, d_out)[2]
    cut = B.grads_twin(sd, cfg, x, ts, ctx, pooled, sub, names, mults, d_out, mut="cut_ctx_split")[2]
    assert float(full["transformer_blocks.0.attn.to_q"][0].norm()) > 0
    for part in ("to_k", "to_v"):
        k = f"transformer_blocks.0.attn.{part}"
        d = B.rel(cut[k][0], full[k][0])
        print(f"{part}: cutting the context gradient moves d(down) by {d:.3e}")
        assert d > 2 * bars[torch.float16][k][1], "the fp16 engine test must be able to see this path"


# ---- the kernel references ---------------------------------------------------------------------------------------------
def test_adaln_bwd_ref_is_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 64, generator=g, dtype=torch.float64, requires_grad=True)
    mod = torch.randn(3, 192, generator=g, dtype=torch.float64)
    dy = torch.randn(7, 64, generator=g, dtype=torch.float64)
    add = torch.randn(7, 64, generator=g, dtype=torch.float64)
    y = R.adaln_ref(x, mod, 3, 64, 128, 1e-6)["y"]
    (want,) = torch.autograd.grad((y * dy).sum(), x)
    ref = B.adaln_bwd_ref(x.detach(), dy, mod, 3, 64, 1e-6, add=add)
    assert torch.allclose(ref["dx"], want + add, rtol=1e-11, atol=1e-12)
    assert float(B.adaln_bwd_bound(ref, torch.float16).min()) > 0


def test_gelu_tanh_grad_is_autograd_and_safe_at_the_ends():
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(R.gelu_tanh(x).sum(), x)
    got = B.gelu_tanh_grad(x.detach())[0]
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-15)
    ends = B.gelu_tanh_grad(torch.tensor([-40.0, -12.0, 12.0, 40.0], dtype=torch.float64))[0]
    assert torch.isfinite(ends).all() and ends[0].abs() < 1e-300 and ends[3] == 1.0


def test_erf_gelu_grad_leaves_the_kernel_bound():
    x = torch.linspace(-4, 4, 801, dtype=torch.float64).half().double().requires_grad_(True)
    (erf_grad,) = torch.autograd.grad(R.gelu_erf(x).sum(), x)
    xd = x.detach()
    dy = torch.ones_like(xd)
    for dt in (torch.float16, torch.bfloat16):
        E = B.gelu_tanh_bwd_bound(xd, dy, dt)
        assert B.worst(erf_grad.to(dt), B.gelu_tanh_bwd_ref(xd, dy), E) > B.SLACK
        assert B.worst(B.gelu_tanh_bwd_ref(xd, dy).to(dt), B.gelu_tanh_bwd_ref(xd, dy), E) <= 1.0


# ---- host: the trainable engine's dry run and its refusals -------------------------------------------------------------
def _sites(cfg, context_stream=True):
    return B.flat_layout(B.site_names(cfg.num_layers, context_stream), cfg.inner_dim, RANK, ALPHA)[0]


def test_train_dry_run_sizes_a_workspace():
    cfg = M.tiny_sd3_config()
    sites = _sites(cfg)
    t = M.train_workspace_bytes(cfg, torch.float16, sites, 3, 8, 6, 5)
    assert t > M.workspace_bytes(cfg, torch.float16, sites, 3, 8, 6, 5) > 0
    assert M.train_workspace_bytes(cfg, torch.float16, sites, 6, 8, 6, 5) > t


def test_train_dry_run_takes_sd3_medium():
    cfg = M.sd3_medium_config()
    for cs in (False, True):
        sites = _sites(cfg, cs)
        assert len(sites) == (191 if cs else 96)
        t = M.train_workspace_bytes(cfg, torch.bfloat16, sites, 2, 64, 64, 333)
        assert t > M.workspace_bytes(cfg, torch.bfloat16, sites, 2, 64, 64, 333)


def test_train_refusals():
    cfg = M.tiny_sd3_config()
    sites = _sites(cfg)
    with pytest.raises(_native.SmiError, match="n_sites 0"):
        M.train_workspace_bytes(cfg, torch.float16, [], 2, 8, 6, 5)
    with pytest.raises(_native.SmiError, match="DoRA"):
        M.train_workspace_bytes(cfg, torch.float16, [dict(s, off_dora=0) for s in sites], 2, 8, 6, 5)
    for change, word in ((dict(dual_attention_layers=(0, 1)), "dual_attention_layers"), (dict(qk_norm="rms_norm"), "qk_norm")):
        bad = M.SD3Config(**{**cfg.__dict__, **change})
        with pytest.raises(_native.SmiError, match=word):
            M.train_workspace_bytes(bad, torch.float16, sites, 2, 8, 6, 5)


def test_new_symbols_are_in_the_library():
    import ctypes
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("smi_mmdit_train_workspace_bytes", "smi_mmdit_train_create", "smi_mmdit_forward_save", "smi_mmdit_backward",
                "smi_op_adaln_modulate_bwd", "smi_op_gate_residual_bwd"):
        assert hasattr(lib, sym), sym
        assert sym in _native.EXPORTED_SYMBOLS


# ---- the trainer's command line and its refusals -------------------------------------------------------------------------
def test_trainer_parser_takes_the_reference_command_line():
    from sliders_conceptmod_amd import train_lora_sd3 as T
    a = T.build_parser().parse_args(["--config_file", "data/config-sd3.yaml", "--alpha", "1.0", "--rank", "4", "--device", "0",
                                     "--name", "age", "--attributes", "male, female", "--peft_type", "lora"])
    assert (a.alpha, a.rank, a.name, a.peft_type, a.context_stream, a.fused_step) == (1.0, 4, "age", "lora", False, None)
    assert T.build_parser().parse_args(["--alpha", "1", "--context_stream", "--no_fused_step"]).context_stream
    with pytest.raises(SystemExit):
        T.build_parser().parse_args([])  # --alpha is required, as in the reference


def test_trainer_default_files_load():
    from sliders_conceptmod_amd import config_util, prompt_util
    cfg = config_util.load_config_from_yaml("data/config-sd3.yaml")
    assert cfg.pretrained_model.name_or_path == "synthetic://sd3" and cfg.network.type == "lierla"
    prompts = prompt_util.load_prompts_from_yaml(cfg.prompts_file, [])
    assert len(prompts) >= 1 and prompts[0].negative is not None
    e = prompt_util.PromptEmbedsSD3(torch.zeros(1, 5, 64), torch.zeros(1, 64))
    assert e.text_embeds.shape == (1, 5, 64) and e.pooled_embeds.shape == (1, 64)


def test_trainer_refusals_are_by_name():
    from sliders_conceptmod_amd import config_util
    from sliders_conceptmod_amd import train_lora_sd3 as T
    cfg = config_util.load_config_from_yaml("data/config-sd3.yaml")
    with pytest.raises(ValueError, match="dora"):
        T.check_supported(cfg, "dora")
    with pytest.raises(ValueError, match="dora"):
        T.train(cfg, [], torch.device("cpu"), peft_type="dora")
    c3 = config_util.load_config_from_yaml("data/config-sd3.yaml")
    c3.network.type = "c3lier"
    with pytest.raises(ValueError, match="c3lier"):
        T.check_supported(c3, "lora")
    s35 = config_util.load_config_from_yaml("data/config-sd3.yaml")
    s35.pretrained_model.name_or_path = "stabilityai/stable-diffusion-3.5-medium"
    with pytest.raises(ValueError, match="SD3.5"):
        T.check_supported(s35, "lora")
    T.check_supported(cfg, "lora")
