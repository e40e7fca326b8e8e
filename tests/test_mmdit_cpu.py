"""The SD3 MMDiT without a GPU: the float64 restatement of tests/mmdit_refs.py rejects every mutation of the network on the
tiny configuration by at least 2 x the fp16 model bar (so a GPU run under the bar cannot hide one); LoRA selection and file
keys; the engine's refusals (config, sites) through the host-only dry run; the prompt encoding's shapes and zeros.

erf-GELU for tanh-GELU moves the tiny model's output by less than the model bar (the two functions differ by at most
4.8e-4 |x| near |x| = 2): that mutation is held against the KERNEL bound instead (here on the rounded float64 values, and on
the GPU in test_mmdit_kernels_gpu.py::test_gelu_tanh)."""
import pytest
import torch

import mmdit_refs as R
from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import generate_images as G
from sliders_conceptmod_amd import lora as L
from sliders_conceptmod_amd import mmdit as M
from sliders_conceptmod_amd import model_util as MU
from sliders_conceptmod_amd import train_util as TU

TS = [1000.0, 517.25, 31.0]


@pytest.fixture(scope="module")
def tiny():
    cfg = M.tiny_sd3_config()
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=3)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 16, 8, 6, generator=g)
    clip = torch.randn(3, 5, 64, generator=g)
    ctx = torch.cat([clip, torch.zeros(3, 4, 64)], dim=1)  # five "CLIP" rows and a block of four zero rows, as the T5 stand-in
    pooled = torch.randn(3, 64, generator=g)
    sd = model.state_dict()
    ref = R.forward(sd, cfg, x, TS, ctx, pooled)
    bar = 2.0 * R.rel_l2(R.forward(sd, cfg, x, TS, ctx, pooled, dt=torch.float16), ref)
    return dict(cfg=cfg, model=model, sd=sd, x=x, ctx=ctx, pooled=pooled, ref=ref, bar=bar)


def test_modulations_are_of_order_one(tiny):
    """What lets the parity tests see a dropped gate: modulation outputs and the position table of order 0.1 to 1."""
    sd = tiny["sd"]
    st = R.silu(torch.randn(64, 128, dtype=torch.float64) * 0.5)
    for k in ("transformer_blocks.0.norm1.linear", "transformer_blocks.1.norm1_context.linear", "norm_out.linear"):
        m = st @ sd[k + ".weight"].double().t() + sd[k + ".bias"].double()
        assert 0.1 <= float(m.std()) <= 1.0, k
    assert 0.1 <= float(sd["pos_embed.pos_embed"].std()) <= 1.0


@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS if m != "erf_gelu"])
def test_restatement_rejects_mutation(tiny, mut):
    d = R.rel_l2(R.forward(tiny["sd"], tiny["cfg"], tiny["x"], TS, tiny["ctx"], tiny["pooled"], mut=mut), tiny["ref"])
    print(f"{mut}: {d:.3e} against the fp16 bar {tiny['bar']:.3e}")
    assert d >= 2 * tiny["bar"]


def test_restatement_rejects_input_mutations(tiny):
    f = lambda ts, ctx: R.rel_l2(R.forward(tiny["sd"], tiny["cfg"], tiny["x"], ts, ctx, tiny["pooled"]), tiny["ref"])
    sigma = f([t / 1000.0 for t in TS], tiny["ctx"])      # the timestep fed as sigma instead of 1000 sigma
    no_zero = f(TS, tiny["ctx"][:, :5])                   # the zero-token block left out: its keys take softmax mass
    print(f"sigma for 1000 sigma: {sigma:.3e}; zero block left out: {no_zero:.3e}; bar {tiny['bar']:.3e}")
    assert sigma >= 2 * tiny["bar"] and no_zero >= 2 * tiny["bar"]


def test_erf_gelu_leaves_the_kernel_bound():
    x = torch.linspace(-6, 6, 4097, dtype=torch.float64).to(torch.float16)
    ref = R.gelu_tanh(x.double())
    E = R.gelu_tanh_bound(x, ref, torch.float16)
    assert R.worst(ref.to(torch.float16), ref, E) <= 1.0
    assert R.worst(R.gelu_erf(x.double()).to(torch.float16), ref, E) > R.SLACK


def test_twin_is_the_reference_without_roundings(tiny):
    a = R.forward(tiny["sd"], tiny["cfg"], tiny["x"], TS, tiny["ctx"], tiny["pooled"], dt=torch.float64)
    assert torch.equal(a, tiny["ref"])


def test_lora_restatement_is_the_merged_weight(tiny):
    """W + m (alpha / r) up down per sample == the delta form the restatement computes."""
    model = tiny["model"]
    torch.manual_seed(1)
    net = L.LoRANetwork(model, rank=4, alpha=2.0, train_method="full", context_stream=True)
    model.__dict__.pop("_lora_network")
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0, 0.3)
    lora = {l.target_path: (l.lora_down.weight.detach(), l.lora_up.weight.detach(), l.scale) for l in net.unet_loras}
    got = R.forward(tiny["sd"], tiny["cfg"], tiny["x"], TS, tiny["ctx"], tiny["pooled"], lora=lora, mults=[0.0, 1.0, -2.0])
    assert torch.equal(got[0], tiny["ref"][0])
    for i, m in ((1, 1.0), (2, -2.0)):
        sd = {k: v.double().clone() for k, v in tiny["sd"].items()}
        for path, (dn, up, sc) in lora.items():
            sd[path + ".weight"] += m * sc * (up.double() @ dn.double())
        one = R.forward(sd, tiny["cfg"], tiny["x"][i:i + 1], TS[i:i + 1], tiny["ctx"][i:i + 1], tiny["pooled"][i:i + 1])
        assert R.rel_l2(got[i:i + 1], one) < 1e-12


# ---- host: LoRA selection, file keys ------------------------------------------------------------------------------------
PROJ = ("to_q", "to_k", "to_v", "add_k_proj", "add_v_proj", "add_q_proj", "to_out_0", "to_add_out")


def test_lora_selection_and_keys(tiny):
    cfg, model = tiny["cfg"], tiny["model"]
    net = L.LoRANetwork(model, rank=4, alpha=1.0, train_method="full", context_stream=True)
    model.__dict__.pop("_lora_network")
    names = [l.lora_name for l in net.unet_loras]
    assert len(names) == 8 * cfg.num_layers - 1
    want = [f"lora_unet_transformer_blocks_{i}_attn_{p}" for i in range(cfg.num_layers) for p in PROJ
            if not (i == cfg.num_layers - 1 and p == "to_add_out")]
    assert names == want
    keys = set(net.state_dict())
    assert keys == {f"{n}.{s}" for n in names for s in ("alpha", "lora_down.weight", "lora_up.weight")}
    # the fused groups lie adjacent and in the engine's order in the flat buffers
    off = {s["target"]: s["off_down"] for s in net.engine_sites()}
    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}.attn."
        for trio in (("to_q", "to_k", "to_v"), ("add_q_proj", "add_k_proj", "add_v_proj")):
            o = [off[b + t] for t in trio]
            assert o[1] - o[0] == 4 * 128 and o[2] - o[1] == 4 * 128
    # the reference's own walk leaves out every 'add_' child: four per block
    ref_net = L.LoRANetwork(model, rank=4, alpha=1.0, train_method="full")
    model.__dict__.pop("_lora_network")
    assert len(ref_net.unet_loras) == 4 * cfg.num_layers
    assert all("add_" not in l.lora_name for l in ref_net.unet_loras)


def test_full_size_module_count():
    with torch.device("meta"):
        model = M.SD3Transformer2DModel(M.sd3_medium_config())
    assert len(L.select_targets(model, "full", ["Attention"], "lora_unet", "_", context_stream=True)) == 191
    assert len(L.select_targets(model, "full", ["Attention"], "lora_unet", "_")) == 96


@pytest.mark.parametrize("context_stream", [True, False])
def test_lora_file_params_recognises_an_sd3_file(tiny, context_stream):
    model = tiny["model"]
    net = L.LoRANetwork(model, rank=4, alpha=2.0, train_method="full", context_stream=context_stream)
    model.__dict__.pop("_lora_network")
    state = net.get_state_dict(torch.float16)
    rank, alpha, method, target = G.lora_file_params(state, model)
    assert (rank, alpha, target) == (4, 2.0, ["Attention"]) and method in G.TRAIN_METHODS
    again = G.lora_network_from_state(model, state, "cpu")
    model.__dict__.pop("_lora_network")
    assert [l.lora_name for l in again.unet_loras] == [l.lora_name for l in net.unet_loras]


# ---- host: the engine's refusals, through the dry run -----------------------------------------------------------------------
def _ws(cfg, sites=(), h=8, w=6, batch=2, ctx_len=5):
    return M.workspace_bytes(cfg, torch.float16, list(sites), batch, h, w, ctx_len)


def test_dry_run_sizes_a_workspace():
    cfg = M.tiny_sd3_config()
    assert _ws(cfg) > 0 and _ws(cfg, batch=4) > _ws(cfg, batch=2)


@pytest.mark.parametrize("change,word", [
    (dict(attention_head_dim=32, num_attention_heads=4), "attention_head_dim"),
    (dict(num_attention_heads=33), "2048"),
    (dict(in_channels=8), "multiple of 64"),
    (dict(dual_attention_layers=(0, 1)), "dual_attention_layers"),
    (dict(qk_norm="rms_norm"), "qk_norm"),
])
def test_config_refusals(change, word):
    cfg = M.SD3Config(**{**M.tiny_sd3_config().__dict__, **change})
    with pytest.raises(_native.SmiError, match=word):
        _ws(cfg)


def test_shape_refusals():
    cfg = M.tiny_sd3_config()
    with pytest.raises(_native.SmiError, match="multiple of patch_size"):
        _ws(cfg, h=7)
    with pytest.raises(_native.SmiError, match="pos_embed_max_size"):
        _ws(cfg, h=18, w=16)


def test_site_refusals():
    cfg = M.tiny_sd3_config()
    site = lambda t, **kw: {"target": t, "off_down": 0, "off_up": 0, "rank": 4, "scale": 1.0, **kw}
    with pytest.raises(_native.SmiError, match="DoRA"):
        _ws(cfg, [site("transformer_blocks.0.attn.to_out.0", off_dora=0)])
    with pytest.raises(_native.SmiError, match="ff.net.0.proj"):
        _ws(cfg, [site("transformer_blocks.0.ff.net.0.proj")])
    with pytest.raises(_native.SmiError, match="rank"):
        _ws(cfg, [site("transformer_blocks.0.attn.to_out.0", rank=32)])
    with pytest.raises(_native.SmiError, match="all or none"):
        _ws(cfg, [site("transformer_blocks.0.attn.to_q")])
    with pytest.raises(_native.SmiError, match="not an attention projection"):
        _ws(cfg, [site("transformer_blocks.1.attn.to_add_out")])  # the last block has none
    assert _ws(cfg, [site("transformer_blocks.0.attn.to_add_out")]) > _ws(cfg)


@pytest.mark.parametrize("plan", ["workspace_bytes", "train_workspace_bytes"])
@pytest.mark.parametrize("change,gist", [
    (dict(off_dora=0), r"DoRA site 'transformer_blocks\.0\.attn\.to_out\.0'"),
    (dict(rank=0), r"rank 0 of 'transformer_blocks\.0\.attn\.to_out\.0' outside \[1, 16\]"),
    (dict(rank=17), r"rank 17 of 'transformer_blocks\.0\.attn\.to_out\.0' outside \[1, 16\]"),
    (dict(target="transformer_blocks.0.ff.net.0.proj"),
     r"target 'transformer_blocks\.0\.ff\.net\.0\.proj'.*attention projections \(attn\.to_q/to_k/to_v/to_out\.0, "
     r"attn\.add_q_proj/add_k_proj/add_v_proj/to_add_out\)"),
], ids=["dora", "rank0", "rank17", "target"])
def test_site_refusal_codes_and_messages(plan, change, gist):
    """both dry runs return -1 with the model's prefix, the site and the reason in the message"""
    cfg = M.tiny_sd3_config()
    site = {"target": "transformer_blocks.0.attn.to_out.0", "off_down": 0, "off_up": 0, "rank": 4, "scale": 1.0}
    with pytest.raises(_native.SmiError, match=r"failed \(-1\): MMDiT: " + gist):
        getattr(M, plan)(cfg, torch.float16, [dict(site, **change)], 2, 8, 6, 5)
    assert getattr(M, plan)(cfg, torch.float16, [site], 2, 8, 6, 5) > 0


def test_generate_images_refuses_te_files_with_sd3(tmp_path):
    args = G.build_parser().parse_args(["--prompts_path", "p.csv", "--save_path", str(tmp_path), "--base", "sd3",
                                        "--model_name", "x.pt", "--te_model_name", "a.safetensors"])
    with pytest.raises(ValueError, match="te_model_name"):
        G.generate(args)
    d = G.fill_defaults(G.build_parser().parse_args(["--prompts_path", "p.csv", "--save_path", "o", "--base", "sd3"]))
    assert (d.ddim_steps, d.guidance_scale, d.image_size, d.t5_tokens) == (28, 7.0, 1024, 256)
    d = G.fill_defaults(G.build_parser().parse_args(["--prompts_path", "p.csv", "--save_path", "o"]))
    assert (d.ddim_steps, d.guidance_scale, d.image_size) == (50, 7.5, 512)


def test_module_without_gpu_fails_loudly(tiny):
    model = M.SD3Transformer2DModel(tiny["cfg"]).half()
    with pytest.raises(_native.SmiError):
        model(torch.zeros(1, 16, 8, 6), 10.0, torch.zeros(1, 5, 64), torch.zeros(1, 64))


# ---- host: the prompt encoding (the CLIP towers need the GPU: a stand-in pair with their call surface) ------------------------
class _Tower:
    def __init__(self, hidden, proj, seed):
        self.hidden, self.proj, self.seed, self.device = hidden, proj, seed, torch.device("cpu")

    def __call__(self, ids, output_hidden_states=False):
        g = torch.Generator().manual_seed(self.seed)

        class Out:
            hidden_states = [None, torch.randn(ids.shape[0], ids.shape[1], self.hidden, generator=g) + 3.0, None]

            def __getitem__(_s, i):
                return (torch.randn(ids.shape[0], self.proj, generator=g) + 3.0,)[i]
        return Out()


@pytest.mark.parametrize("t5_tokens", [256, 77])
def test_encode_prompts_sd3_shapes_and_zeros(t5_tokens):
    toks = [MU.SyntheticClipTokenizer(1000, 999), MU.SyntheticClipTokenizer(1000, 999)]
    encs = [_Tower(48, 24, 1), _Tower(80, 40, 2)]
    e, p = TU.encode_prompts_sd3(None, toks, encs, "a photo of a person", 1, t5_tokens, 160)
    assert tuple(e.shape) == (1, 77 + t5_tokens, 160) and tuple(p.shape) == (1, 64)
    assert float(e[:, :77, :128].abs().min()) > 0          # the two towers' features, side by side
    assert float(e[:, :77, 128:].abs().max()) == 0         # zero-padded to joint_attention_dim
    assert float(e[:, 77:].abs().max()) == 0               # the T5 block: zero rows
    e2, p2 = TU.encode_prompts_sd3(None, toks, encs, "a photo of a person", 3, t5_tokens, 160)
    assert tuple(e2.shape) == (3, 77 + t5_tokens, 160) and tuple(p2.shape) == (3, 64)
    with pytest.raises(ValueError):
        TU.encode_prompts_sd3(None, toks, encs, "x", 1, t5_tokens, 64)


def test_load_models_sd3_synthetic():
    toks, encs, model, sched = MU.load_models_sd3("synthetic://tiny_sd3")
    assert len(toks) == 2 and len(encs) == 2 and isinstance(sched, MU.FlowMatchEulerDiscreteScheduler)
    assert sum(e.config.projection_dim for e in encs) == model.cfg.pooled_projection_dim
    assert sum(e.config.hidden_size for e in encs) <= model.cfg.joint_attention_dim or model.cfg.joint_attention_dim == 64
    with pytest.raises(ValueError):
        MU.load_models_sd3("synthetic://sd1x")
    cfg = M.sd3_medium_config()
    assert (cfg.patch_size, cfg.in_channels, cfg.num_layers, cfg.num_attention_heads, cfg.attention_head_dim,
            cfg.joint_attention_dim, cfg.pooled_projection_dim, cfg.pos_embed_max_size, cfg.sample_size) == (
                2, 16, 24, 24, 64, 4096, 2048, 192, 128)
