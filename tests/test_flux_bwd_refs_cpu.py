"""The references of the Flux backward (tests/flux_bwd_refs.py) judged on the CPU, and the host-only parts of the trainable
engine: the dry run, its refusals, the new symbols.

Tiny model (d 128, two double and two single blocks), 8 x 6 latent, 5 context tokens, n = 3, multipliers (0, 1, -2), rank 4,
lora_up seeded non-zero, all 22 sites (the context_stream form).  Seeds: model 3, LoRA 11, inputs 13.  The GPU test holds the
engine's gradient to form A on the whole vector AND on each site's (down, up) pair, each under its own bar = 3 e_q + 1e-4,
e_q = rel(B, A) of that part; so a mutant counts as caught where its worst part stands.  The measured distances and the
mutants' ratios are in DESIGN.md section 18."""
import pytest
import torch

import flux_bwd_refs as B
import flux_refs as F
import mmdit_refs as R
from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import flux as M

MULTS = [0.0, 1.0, -2.0]
RANK, ALPHA = 4, 2.0


@pytest.fixture(scope="module")
def tiny():
    cfg = M.tiny_flux_config()
    model = M.init_synthetic_(M.FluxTransformer2DModel(cfg), seed=3)
    sd = {k: v.float() for k, v in model.state_dict().items()}  # (fp32: both restatements round them to the storage type)
    names = B.site_names(cfg.num_layers, cfg.num_single_layers, context_stream=True)
    lora = B.make_lora(names, cfg.inner_dim, RANK, ALPHA, torch.Generator().manual_seed(11))
    x, ts, gd, ctx, pooled, d_out = B.tiny_inputs(cfg, 3, 8, 6, 5, seed=13)
    args = (sd, cfg, x, ts, gd, ctx, pooled, lora, names, MULTS, d_out)
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


def test_site_names_count():
    assert len(B.site_names(19, 38, False)) == 19 * 4 + 38 * 3
    assert len(B.site_names(19, 38, True)) == 19 * 8 + 38 * 3
    assert len(B.site_names(2, 2, True)) == 22


def test_twin_without_roundings_is_form_a(tiny):
    res = B.grads_twin(*tiny["args"])
    assert B.rel(res[3], tiny["out"]) < 1e-12
    assert B.rel(_vec(res), tiny["a"]) < 1e-12
    assert float(tiny["a"].norm()) > 0
    for k, v in tiny["parts"].items():
        assert float(v.norm()) > 0, f"{k} takes no gradient"


def test_twin_forward_rounds_where_the_forward_restatement_does(tiny):
    sd, cfg, x, ts, gd, ctx, pooled, lora, names, mults, _ = tiny["args"]
    for dt in (torch.float16, torch.bfloat16):
        want = F.forward(sd, cfg, x, ts, gd, ctx, pooled, dt=dt, lora=lora, mults=mults)
        got = B.twin_forward(sd, cfg, x, ts, gd, ctx, pooled, lora, mults, dt=dt)
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


# ---- the kernel references ---------------------------------------------------------------------------------------------
def test_qk_norm_rope_bwd_ref_is_autograd():
    g = torch.Generator().manual_seed(1)
    n, T, H, D = 2, 5, 2, 16
    x = torch.randn(n, T, 3, H, D, generator=g, dtype=torch.float64).half().double().requires_grad_(True)
    do = torch.randn(n, T, 3, H, D, generator=g, dtype=torch.float64).half().double()  # (v is a copy: no rounding allowed)
    wq, wk = (0.5 + torch.rand(D, generator=g, dtype=torch.float64) for _ in range(2))
    ids = torch.randint(0, 64, (T, 3), generator=g)
    cos, sin = F.rope_table(ids, (4, 6, 6))
    y, _ = F.qk_norm_rope_ref(x, wq, wk, cos, sin)
    (want,) = torch.autograd.grad((y * do).sum(), x)
    ref = B.qk_norm_rope_bwd_ref(x.detach(), do, wq, wk, cos, sin)
    assert torch.allclose(ref["dx"], want, rtol=1e-11, atol=1e-13)
    E = B.qk_norm_rope_bwd_bound(ref, torch.float16)
    assert float(E.min()) > 0
    # the result rounded to the storage type is inside 1 E; without the x r^2 mean(g x) term it is far outside
    assert B.worst(ref["dx"].half(), ref["dx"], E) <= 1.0
    bad = ref["dx"] + ref["r"] * ref["x"] * ref["k"]
    bad[:, :, 2] = ref["dx"][:, :, 2]
    assert B.worst(bad.half(), ref["dx"], E) > B.SLACK


def test_flux_unpack_bwd_ref_inverts_the_unpack():
    g = torch.Generator().manual_seed(2)
    n, C, gh, gw = 2, 16, 3, 5
    d_out = torch.randn(n, C, 2 * gh, 2 * gw, generator=g)
    rows = B.flux_unpack_bwd_ref(d_out, [1.0, 1.0])
    assert torch.equal(R.unpatchify(rows, n, C, gh, gw, 2, "cpp"), d_out.double())
    assert torch.equal(B.flux_unpack_bwd_ref(d_out, [4.0, 0.5])[:gh * gw], 4.0 * rows[:gh * gw])


def test_adaln_bwd_bound_takes_flux_width():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 3072, generator=g, dtype=torch.float64)
    dy = torch.randn(3, 3072, generator=g, dtype=torch.float64)
    mod = torch.randn(1, 3072, generator=g, dtype=torch.float64)
    ref = B.adaln_bwd_ref(x, dy, mod, 3, 0, 1e-6)
    E = B.adaln_bwd_bound(ref, torch.bfloat16)
    assert B.worst(ref["dx"].bfloat16(), ref["dx"], E) <= 1.0


# ---- host: the trainable engine's dry run and its refusals -------------------------------------------------------------
def _sites(cfg, context_stream=True):
    return B.flat_layout(B.site_names(cfg.num_layers, cfg.num_single_layers, context_stream), cfg.inner_dim, RANK, ALPHA)[0]


# smi_flux_workspace_bytes of the parent commit (tiny config, n = 3, 8 x 6 latent, 5 context tokens, rank 4), recorded from
# a build of that commit: the forward-only engine keeps its plan
PARENT_BYTES = {False: 1335296, True: 1392640, None: 1245184}


def test_forward_only_workspace_is_the_parents():
    cfg = M.tiny_flux_config()
    for dt in (torch.float16, torch.bfloat16):
        assert M.workspace_bytes(cfg, dt, _sites(cfg, False), 3, 8, 6, 5) == PARENT_BYTES[False]
        assert M.workspace_bytes(cfg, dt, _sites(cfg, True), 3, 8, 6, 5) == PARENT_BYTES[True]
    assert M.workspace_bytes(cfg, torch.float16, [], 3, 8, 6, 5) == PARENT_BYTES[None]


def test_train_dry_run_sizes_a_workspace():
    cfg = M.tiny_flux_config()
    sites = _sites(cfg)
    t = M.train_workspace_bytes(cfg, torch.float16, sites, 3, 8, 6, 5)
    assert t > M.workspace_bytes(cfg, torch.float16, sites, 3, 8, 6, 5) > 0
    assert M.train_workspace_bytes(cfg, torch.float16, sites, 6, 8, 6, 5) > t


def test_train_dry_run_takes_flux_schnell():
    cfg = M.flux_schnell_config()
    for cs in (False, True):
        sites = _sites(cfg, cs)
        assert len(sites) == 19 * (8 if cs else 4) + 38 * 3
        t = M.train_workspace_bytes(cfg, torch.bfloat16, sites, 1, 64, 64, 256)
        assert t > M.workspace_bytes(cfg, torch.bfloat16, sites, 1, 64, 64, 256)


def test_train_refusals():
    cfg = M.tiny_flux_config()
    sites = _sites(cfg)
    with pytest.raises(_native.SmiError, match="n_sites 0"):
        M.train_workspace_bytes(cfg, torch.float16, [], 2, 8, 6, 5)
    with pytest.raises(_native.SmiError, match="DoRA"):
        M.train_workspace_bytes(cfg, torch.float16, [dict(s, off_dora=0) for s in sites], 2, 8, 6, 5)
    bad = [dict(sites[0], target="single_transformer_blocks.0.proj_mlp")]
    with pytest.raises(_native.SmiError, match="proj_mlp"):
        M.train_workspace_bytes(cfg, torch.float16, bad, 2, 8, 6, 5)


def test_new_symbols_are_in_the_library():
    import ctypes
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("smi_flux_train_workspace_bytes", "smi_flux_train_create", "smi_flux_forward_save", "smi_flux_backward",
                "smi_op_qk_norm_rope_bwd", "smi_op_gelu_tanh_cols_bwd", "smi_op_flux_unpack_bwd"):
        assert hasattr(lib, sym), sym
        assert sym in _native.EXPORTED_SYMBOLS


# ---- the trainer's command line and its refusals -------------------------------------------------------------------------
def test_trainer_parser_takes_the_reference_command_line():
    from sliders_conceptmod_amd import train_lora_flux as T
    a = T.build_parser().parse_args(["--config_file", "data/config-flux.yaml", "--alpha", "1.0", "--rank", "4", "--device", "0",
                                     "--name", "age", "--attributes", "male, female", "--peft_type", "lora"])
    assert (a.alpha, a.rank, a.name, a.peft_type, a.context_stream, a.fused_step) == (1.0, 4, "age", "lora", False, None)
    assert T.build_parser().parse_args(["--alpha", "1", "--context_stream", "--no_fused_step"]).context_stream
    with pytest.raises(SystemExit):
        T.build_parser().parse_args([])  # --alpha is required, as in the reference


def test_trainer_default_files_load_and_constants():
    from sliders_conceptmod_amd import config_util, prompt_util
    from sliders_conceptmod_amd import train_lora_flux as T
    cfg = config_util.load_config_from_yaml("data/config-flux.yaml")
    assert cfg.pretrained_model.name_or_path == "synthetic://flux_schnell" and cfg.network.type == "lierla"
    prompts = prompt_util.load_prompts_from_yaml(cfg.prompts_file, [])
    assert len(prompts) >= 1 and prompts[0].negative is not None
    assert (T.TIMESTEPS_TO, T.NUM_INFERENCE_STEPS, T.CLIP_VALUE) == (0, 8, 1.0)
    assert [T.accumulation_steps(b) for b in (1, 2, 3, 5, 8, 9)] == [8, 4, 3, 2, 1, 1]


def test_trainer_refusals_are_by_name():
    from sliders_conceptmod_amd import config_util
    from sliders_conceptmod_amd import train_lora_flux as T
    cfg = config_util.load_config_from_yaml("data/config-flux.yaml")
    with pytest.raises(ValueError, match="dora"):
        T.check_supported(cfg, "dora")
    with pytest.raises(ValueError, match="dora"):
        T.train(cfg, [], torch.device("cpu"), peft_type="dora")
    cfg.network.type = "c3lier"
    with pytest.raises(ValueError, match="c3lier"):
        T.check_supported(cfg, "lora")
    cfg.network.type = "lierla"
    T.check_supported(cfg, "lora")
