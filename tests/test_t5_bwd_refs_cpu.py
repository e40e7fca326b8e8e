"""tests/t5_bwd_refs.py checked against itself on the CPU: every closed-form reference equals torch autograd through the
forward's float64 reference; the fp32 / storage-dtype emulation of each backward kernel holds its bound (<= 1 E) and every
listed mutant leaves it (> SLACK E) -- so the GPU test's bound can see a dropped projection term, a mirrored bias table or a
swapped half.  Also the host-side pieces of the new entries that need no GPU: the ctypes signatures and the refusals."""
import pytest
import torch

import attention_refs as A
import t5_bwd_refs as B
import t5_refs as R

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def close64(a, b, what):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < 1e-10, f"{what}: closed form and autograd differ by {err:.3g}"


# ---------------------------------------------------------------------------------------------------------------
# rmsnorm_rows_bwd
# ---------------------------------------------------------------------------------------------------------------
RMS_SMALL = [(M, C) for M, C in B.RMS_CASES if C <= 2056] + [(3, 4096), (3, 8192)]


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,C", RMS_SMALL, ids=[f"m{m}c{c}" for m, c in RMS_SMALL])
def test_rmsnorm_bwd_reference(dt, M, C):
    x, w, dy, add = B.rms_bwd_inputs(M, C, dt)
    close64(B.rms_bwd_ref(x, w, dy), B.rms_bwd_autograd(x, w, dy), "rmsnorm_bwd")
    for a in (None, add):
        ref = B.rms_bwd_ref(x, w, dy, a)
        E = B.rms_bwd_bound(x, w, dy, a, ref, C, dt)
        assert B.worst(B.rms_bwd_emulate(x, w, dy, a, dt), ref, E) <= 1.0
        assert B.worst(ref.to(dt), ref, E) <= 1.0
        if M >= 3:  # (a single row of magnitude 1 has r = 0.96: r and r^3 are then one rounding apart)
            for m in B.RMS_BWD_MUTANTS:
                assert B.worst(B.rms_bwd_ref(x, w, dy, a, fault=m).to(dt), ref, E) > B.SLACK, m


def test_rmsnorm_bwd_big_row():
    """The bf16 row of magnitude 3e4 is there and its gradient is finite in the fp32 emulation."""
    x, w, dy, add = B.rms_bwd_inputs(3, 4096, torch.bfloat16)
    assert float(x[-1].abs().max()) >= 2.9e4
    assert torch.isfinite(B.rms_bwd_emulate(x, w, dy, add, torch.bfloat16).float()).all()


# ---------------------------------------------------------------------------------------------------------------
# gated_gelu_tanh_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,F", B.GG_CASES, ids=[f"m{m}f{f}" for m, f in B.GG_CASES])
def test_gated_gelu_bwd_reference(dt, M, F):
    proj, dout = B.gg_bwd_inputs(M, F, dt)
    ref = B.gg_bwd_ref(proj, dout)
    close64(ref, B.gg_bwd_autograd(proj, dout), "gated_gelu_tanh_bwd")
    E = B.gg_bwd_bound(proj, dout, ref, dt)
    assert B.worst(B.gg_bwd_emulate(proj, dout, dt), ref, E) <= 1.0
    assert B.worst(ref.to(dt), ref, E) <= 1.0
    for m in B.GG_BWD_MUTANTS:
        assert B.worst(B.gg_bwd_ref(proj, dout, fault=m).to(dt), ref, E) > B.SLACK, m


# ---------------------------------------------------------------------------------------------------------------
# attention backward with the bias table
# ---------------------------------------------------------------------------------------------------------------
ATTN_CPU = (1, 3, 65, 130)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("L", ATTN_CPU)
def test_attention_bias_bwd_reference(dt, L):
    q, k, v, table, d_o = B.attn_bwd_inputs(B.ATTN_B, B.ATTN_H, L, dt)
    ref = B.attn_bias_bwd_ref(q, k, v, table, d_o, 1.0)
    auto = B.attn_bias_bwd_autograd(q, k, v, table, d_o, 1.0)
    for n in ("dQ", "dK", "dV"):
        err = float((ref[n] - auto[n]).abs().max())
        assert err < 1e-9 * max(1.0, float(auto[n].abs().max())), f"{n}: {err:.3g}"
    E = B.attn_bias_bwd_bounds(ref, q, k, v, d_o, 1.0, dt)
    emu = B.attn_bias_bwd_emulate(q, k, v, table, d_o, 1.0, dt)
    for n in ("dQ", "dK", "dV"):
        assert A.ratio(emu[n], ref[n], E[n]) <= 1.0, n
    if L == 1:  # one key: P = 1 whatever the bias, dS = 0
        return
    sees = {"bias_dropped": ("dQ", "dK", "dV"), "bias_mirrored": ("dQ", "dK", "dV"),
            "bias_after_lse_negated": ("dQ", "dK", "dV"), "no_delta": ("dQ", "dK")}
    for m in B.ATTN_BWD_MUTANTS:
        mut = B.attn_bias_bwd_ref(q, k, v, table, d_o, 1.0, fault=m)
        for n in sees[m]:
            assert A.ratio(mut[n].to(dt), ref[n], E[n]) > A.SLACK, (m, n)


def test_mirrored_table_differs_only_off_the_diagonal():
    """The mirrored index is key - query read as query - key: the same entry on the diagonal, so a test with one token, or
    with a symmetric table, could not see it.  The inputs' table is not symmetric."""
    _, _, _, table, _ = B.attn_bwd_inputs(B.ATTN_B, B.ATTN_H, 65, torch.bfloat16)
    bias = R.expand_table(table.double(), 65)
    assert torch.equal(torch.diagonal(bias, dim1=1, dim2=2), torch.diagonal(bias.transpose(1, 2), dim1=1, dim2=2))
    assert float((bias - bias.transpose(1, 2)).abs().max()) > 1.0


def test_expected_bias_path():
    assert B.expected_bias_path(130, 2, 3, "q+kv", -1) == [A.BWD_FUSED]
    assert B.expected_bias_path(3, 2, 3, "q+kv", 1) == [A.BWD_FUSED]  # short keys too: the single-pass kernels know no bias
    assert B.expected_bias_path(130, 2, 3, "q+kv", 0) == [A.DQ, A.DKV]
    assert B.expected_bias_path(130, 2, 3, "q", -1) == [A.DQ]
    assert B.expected_bias_path(130, 2, 3, "kv", -1) == [A.DELTA, A.DKV]
    assert B.expected_bias_path(512, 64, 64, "q+kv", -1) == [A.DQ, A.DKV]  # 4 x 64 x 64 query blocks > 1024


# ---------------------------------------------------------------------------------------------------------------
# the entries, host side
# ---------------------------------------------------------------------------------------------------------------
def test_entries_are_bound():
    from sliders_conceptmod_amd import _native
    lib = _native.lib()
    for name in ("smi_op_attention_bias_bwd", "smi_op_rmsnorm_bwd", "smi_op_gated_gelu_tanh_bwd"):
        assert getattr(lib, name).argtypes is not None, name


def test_refusals_without_a_gpu():
    """The shape checks run before any launch: they need no device."""
    import ctypes as C
    from sliders_conceptmod_amd import _native
    lib = _native.lib()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p)
    assert lib.smi_op_rmsnorm_bwd(1, ptr, ptr, ptr, None, ptr, 2, 12, 1e-6, None) != 0 and b"rmsnorm_bwd" in lib.smi_last_error()
    assert lib.smi_op_rmsnorm_bwd(1, ptr, ptr, ptr, None, ptr, 2, 8200, 1e-6, None) != 0 and b"rmsnorm_bwd" in lib.smi_last_error()
    assert lib.smi_op_gated_gelu_tanh_bwd(1, ptr, ptr, ptr, 2, 12, None) != 0 and b"gated_gelu_tanh_bwd" in lib.smi_last_error()
    a = _native.AttnArgsC()
    a.q = a.k = a.v = a.o = a.d_o = a.dq = a.dk = a.dv = ptr.value
    a.lse = a.delta = ptr.value
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = 64
    a.dtype, a.b, a.h, a.nq, a.nk, a.d, a.scale, a.causal, a.sel_xs, a.sel_fused = 1, 1, 1, 8, 8, 64, 1.0, 0, -1, -1
    ran = _native.AttnRanC()
    call = lambda ld, table=ptr: lib.smi_op_attention_bias_bwd(C.byref(a), table, ld, C.byref(ran))
    assert call(15, None) != 0 and b"table is NULL" in lib.smi_last_error()
    assert call(14) != 0 and b"2 L - 1" in lib.smi_last_error() and ran.n_launches == 0
    a.d = 32
    assert call(15) != 0 and b"head_dim 64" in lib.smi_last_error()
    a.d, a.nk = 64, 16
    assert call(31) != 0 and b"self-attention" in lib.smi_last_error()
    a.nk, a.causal = 8, 1
    assert call(15) != 0 and b"no causal mask" in lib.smi_last_error()
    a.causal, a.nq, a.nk = 0, 4096, 4096
    assert call(8191) != 0 and b"exceeds" in lib.smi_last_error()
    a.nq = a.nk = 8
    a.dq = a.dv = None  # dK without dV, no dQ: refused before the delta launch of that form is queued
    assert call(15) != 0 and b"dK and dV must both be given" in lib.smi_last_error() and ran.n_launches == 0


# ---------------------------------------------------------------------------------------------------------------
# the tower with LoRA sites: what the bar of tests/test_t5_backward_gpu.py can see
# ---------------------------------------------------------------------------------------------------------------
import notrigger_refs as N  # noqa: E402

TOWER_RANK, TOWER_MULTS = 4, (1.0, -1.0)


@pytest.mark.parametrize("which", ("last_hidden", "penultimate"))
@pytest.mark.parametrize("L", (5, 77))
def test_tower_forms_and_mutants(L, which):
    """A precondition on the references: form B is under 1 bar of form A, whole and per site; the hand-written attention
    backward is the derivative; every listed mutant is at least 2 bars from A on the whole vector or on some site."""
    cfg = R.test_cfg()
    c = B.tower_case(cfg, B.halved_state(cfg), L, TOWER_RANK, TOWER_MULTS, which, torch.bfloat16)
    args = (cfg, c["sd"], c["ids"], c["lora"], c["names"], TOWER_MULTS, c["scale"], c["d_hidden"], which)
    assert 0 < c["e_q"] < N.bar(c["e_q"]) and c["e_q_site"] < N.bar(c["e_q_site"])
    assert c["e_q"] < 4e-2, c["e_q"]  # the halved state keeps the bar sharp (the unhalved one: 0.14 .. 0.17)
    auto = B.tower_grads(*args, autograd_attention=True)
    assert B.distance(cfg, c["names"], TOWER_RANK, auto, c["A"])[0] < 1e-12
    last = f"encoder.block.{cfg.num_layers - 1}."
    for nm, a in B.per_site(cfg, c["names"], TOWER_RANK, *c["A"]):  # which 1: the last block's sites get exactly zero
        assert (float(a.abs().max()) == 0.0) == (which == "penultimate" and nm.startswith(last)), nm
    for m in B.TOWER_MUTANTS:
        if m == "final_norm_bwd_skipped" and which == "penultimate":
            continue  # hidden_states[-2] does not pass the final norm
        whole, site, at = B.distance(cfg, c["names"], TOWER_RANK, B.tower_grads(*args, mutate=m), c["A"])
        assert whole >= 2 * N.bar(c["e_q"]) or site >= 2 * N.bar(c["e_q_site"]), (m, whole, site, at)


def test_site_names_and_layout():
    cfg = R.test_cfg()
    names = B.site_names(cfg.num_layers)
    assert len(names) == 4 * cfg.num_layers and names[:4] == [f"encoder.block.0.layer.0.SelfAttention.{p}" for p in "qkvo"]
    sites, n_down, n_up = B.flat_layout(cfg, names, 4, 4.0)
    inner = cfg.num_heads * cfg.d_kv
    assert n_down == cfg.num_layers * 4 * (3 * cfg.d_model + inner) and n_up == cfg.num_layers * 4 * (3 * inner + cfg.d_model)
    assert sites[1]["off_down"] == 4 * cfg.d_model and sites[1]["off_up"] == inner * 4  # q, k, v adjacent, in that order


# ---------------------------------------------------------------------------------------------------------------
# the trainable engine, host side: the dry run and the refusals that need no GPU
# ---------------------------------------------------------------------------------------------------------------
def test_trainable_engine_dry_run_and_refusals():
    from sliders_conceptmod_amd import _native
    cfg = R.test_cfg()
    sites, _, _ = B.flat_layout(cfg, B.site_names(cfg.num_layers), 4, 4.0)
    frozen = _native.t5_workspace_bytes(cfg, torch.bfloat16, 2, 130)
    a = _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites, 2, 130)
    b = _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites, 2, 65)
    assert a > frozen and a > b > 0  # the saved pass and the transposed copies; shorter sequences need less
    with pytest.raises(_native.SmiError, match="DoRA site"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, [dict(s, off_dora=0) for s in sites], 2, 130)
    with pytest.raises(_native.SmiError, match=r"rank 17 of 'encoder.block.0.layer.0.SelfAttention.q' outside \[1, 16\]"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, [dict(s, rank=17) for s in sites], 2, 130)
    with pytest.raises(_native.SmiError, match="wi_0' -- sites sit on SelfAttention"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, [dict(sites[0], target="encoder.block.0.layer.1.DenseReluDense.wi_0")], 2, 130)
    with pytest.raises(_native.SmiError, match="all or none"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites[:2] + sites[3:], 2, 130)
    with pytest.raises(_native.SmiError, match="adjacent in the flat buffers"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, [dict(sites[1], target=sites[0]["target"]), dict(sites[0], target=sites[1]["target"])] + sites[2:], 2, 130)
    with pytest.raises(_native.SmiError, match="not a SelfAttention projection of this T5 encoder"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites + [dict(sites[3], target="encoder.block.9.layer.0.SelfAttention.o")], 2, 130)
    with pytest.raises(_native.SmiError, match="no LoRA sites"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, [], 2, 130)
    with pytest.raises(_native.SmiError, match="f16 is refused"):
        _native.t5_lora_workspace_bytes(cfg, torch.float16, sites, 2, 130)
    with pytest.raises(_native.SmiError, match="exceeds the"):
        _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites, 1025, 130)


def test_xxl_workspace_plan():
    """T5-XXL, n = 2, L = 512, rank 4, all 96 sites: the plan DESIGN.md states (host-only dry run)."""
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd.t5 import t5_xxl_config
    cfg = t5_xxl_config()
    names = B.site_names(cfg.num_layers)
    assert len(names) == 96
    sites, _, _ = B.flat_layout(cfg, names, 4, 4.0)
    total = _native.t5_lora_workspace_bytes(cfg, torch.bfloat16, sites, 2, 512)
    frozen = _native.t5_workspace_bytes(cfg, torch.bfloat16, 2, 512)
    print(f"T5-XXL n=2 L=512 rank 4, 96 sites: {total} bytes ({total / 2**30:.2f} GiB); frozen engine {frozen / 2**30:.2f} GiB")
    weights = 2 * sum(p for p in [cfg.num_layers * (4 * cfg.d_model * cfg.num_heads * cfg.d_kv + 3 * cfg.d_model * cfg.d_ff)])
    assert total > 2 * weights  # every Linear twice (its transposed copy serves dX), the fused copies included
    assert total < 64 * 2**30


# ---------------------------------------------------------------------------------------------------------------
# the site walk on the native T5 container
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ("lora_te2", "lora_te3"))
def test_t5_site_walk(prefix):
    """`t5attn` on t5.T5EncoderModel: 4 sites per block, q, k, v, o in the engine's order, the bias Embedding not among them."""
    from sliders_conceptmod_amd import lora, t5
    model = t5.T5EncoderModel(t5.tiny_t5_config(64))
    net = lora.LoRANetwork(model, rank=4, alpha=1.0, target_replace=lora.T5_TARGET_REPLACE, prefix=prefix, train_method="t5attn")
    n = model.config.num_layers
    names = [l.lora_name for l in net.unet_loras]
    assert names == [f"{prefix}_encoder_block_{i}_layer_0_SelfAttention_{p}" for i in range(n) for p in "qkvo"]
    assert [l.target_path for l in net.unet_loras] == B.site_names(n)
    sites = net.engine_sites()
    d, inner = model.config.d_model, model.config.num_heads * model.config.d_kv
    assert [s["off_down"] for s in sites[:4]] == [0, 4 * d, 8 * d, 12 * d]        # q, k, v adjacent in the flat buffers
    assert [s["off_up"] for s in sites[:4]] == [0, 4 * inner, 8 * inner, 12 * inner]
    assert model.__dict__["_lora_network"] is net
    assert not any("relative_attention_bias" in k for k in net.state_dict())
    # `full` reaches the same modules (the class filter does the work); a UNet method finds nothing on a T5 stack
    assert len(lora.select_targets(model, "full", lora.T5_TARGET_REPLACE, prefix, "_")) == 4 * n
    assert lora.select_targets(model, "xattn", lora.T5_TARGET_REPLACE, prefix, "_") == []
    # the host-side dry run takes the walk's sites as they are
    from sliders_conceptmod_amd import _native
    assert _native.t5_lora_workspace_bytes(model.config, torch.bfloat16, sites, 2, 64) > 0


# ---------------------------------------------------------------------------------------------------------------
# the trainer's and combine_loras' command lines
# ---------------------------------------------------------------------------------------------------------------
def test_check_args_accepts_exactly_the_two_t5_towers():
    import sliders_conceptmod_amd.train_notrigger as T
    T.check_args("FLUX.1", 1, "lora")
    T.check_args("SD3-Medium", 2, "lora")
    assert T.T5_TOWERS == {("FLUX.1", 1): "lora_te2", ("SD3-Medium", 2): "lora_te3"}
    for model, ci, word in (("FLUX.1", 0, "FLUX"), ("FLUX.1", 2, "FLUX"), ("SD3-Medium", 0, "SD3"), ("SD3-Medium", 1, "SD3"),
                            ("SD3", 2, "SD3"), ("SDXL", 2, "T5"), ("SD1", 2, "T5"), ("SD1", 1, "one CLIP tower"),
                            ("PonyXL", 3, "two CLIP towers"), ("Cascade", 0, "Cascade")):
        with pytest.raises(ValueError, match=word):
            T.check_args(model, ci, "lora")
    for model, ci in (("FLUX.1", 1), ("SD3-Medium", 2)):
        with pytest.raises(ValueError, match="dora"):
            T.check_args(model, ci, "dora")
        with pytest.raises(ValueError, match="expected lora"):
            T.check_args(model, ci, "loha")
    T.check_args("SDXL", 1, "lora")


def test_trainer_command_line_and_t5_refusals():
    import types
    import sliders_conceptmod_amd.train_notrigger as T
    from sliders_conceptmod_amd import config_util
    a = T.build_parser().parse_args(["--config_file", "data/config-notrigger-flux.yaml", "--alpha", "1.0", "--name", "smile",
                                     "--positive", "smiling", "--negative", "frowning", "--model", "FLUX.1", "--clip_index", "1"])
    assert (a.model, a.clip_index, a.t5_tokens, a.rank) == ("FLUX.1", 1, 512, 4)
    assert T.build_parser().parse_args(["--config_file", "x", "--alpha", "1", "--clip_index", "2", "--t5_tokens", "24"]).t5_tokens == 24
    cfg = config_util.load_config_from_yaml("data/config-notrigger-flux.yaml")
    assert cfg.network.training_method == "t5attn" and cfg.train.precision == "bfloat16"
    assert cfg.pretrained_model.name_or_path.startswith("synthetic://flux")
    dev = torch.device("cpu")
    cfg.train.precision = "float16"
    with pytest.raises(ValueError, match="float16: the T5 tower runs in bfloat16 only"):
        T.train(cfg, dev, positive=["a"], clip_index=1, model="FLUX.1", towers=(None, None))
    cfg.train.precision = "bfloat16"
    with pytest.raises(ValueError, match="--t5_tokens 0"):
        T.train(cfg, dev, positive=["a"], clip_index=1, model="FLUX.1", towers=(None, None), t5_tokens=0)
    with pytest.raises(ValueError, match="give --positive"):
        T.train(cfg, dev, clip_index=2, model="SD3-Medium", towers=(None, None))
    # a UNet training method finds no site on a T5 stack: refused by name, not an empty file
    from sliders_conceptmod_amd import t5
    model = t5.T5EncoderModel(t5.tiny_t5_config(64))
    cfg.network.training_method = "xattn"
    with pytest.raises(ValueError, match="xattn: no LoRA site on this tower"):
        T.train(cfg, dev, positive=["a"], clip_index=1, model="FLUX.1", towers=(t5.SyntheticT5Tokenizer(1024), model))
    ids = T.tokenize_t5(t5.SyntheticT5Tokenizer(1024), "", 24)
    assert ids.shape == (1, 24) and ids[0, 0] == 1 and int(ids[0, 1:].abs().sum()) == 0  # EOS, then the pad token: no mask


def test_combine_loras_t5(tmp_path):
    from safetensors.torch import load_file, save_file
    from sliders_conceptmod_amd import combine_loras as CL
    mk = lambda prefix, stem: {f"{prefix}{stem}.{part}": torch.full((2, 2), v) for part, v in
                              (("alpha", 1.0), ("lora_down.weight", 2.0), ("lora_up.weight", 3.0))}
    f = lambda name, d: (save_file(d, str(tmp_path / name)), str(tmp_path / name))[1]
    unet = f("u.safetensors", mk("lora_unet_", "transformer_blocks_0_attn_to_q"))
    te1 = f("c.safetensors", mk("lora_te1_", "text_model_encoder_layers_0_self_attn_q_proj"))
    t5_te2 = f("t.safetensors", mk("lora_te2_", "encoder_block_0_layer_0_SelfAttention_q"))
    t5_te3 = f("t3.safetensors", mk("lora_te3_", "encoder_block_0_layer_0_SelfAttention_q"))
    out = str(tmp_path / "o.safetensors")
    CL.main([unet, te1, t5_te2, out, "0.5", "1.0", "0.25", "--t5"])
    got = load_file(out)
    assert not any(k.startswith("lora_te2_") for k in got)
    k = "lora_te3_encoder_block_0_layer_0_SelfAttention_q"
    assert float(got[k + ".lora_down.weight"][0, 0]) == 0.5 and float(got[k + ".lora_up.weight"][0, 0]) == 3.0
    parts = CL.split_by_prefix(got)
    assert [len(parts[p]) for p in CL.PREFIXES] == [3, 3, 0, 3] and set(parts["lora_te3_"]) == {k + s for s in (".alpha", ".lora_down.weight", ".lora_up.weight")}
    assert set(CL.combine("-", "-", t5_te3, out, t5=True)) == set(parts["lora_te3_"])  # an SD3 trainer's file passes as it is
    # without the flag nothing changes: the T5 file stays lora_te2_, and a lora_te3_ file is refused as a second encoder's
    assert all(k.startswith("lora_te2_") for k in CL.combine("-", "-", t5_te2, out))
    with pytest.raises(ValueError, match="does not start with 'lora_te2_'"):
        CL.combine("-", "-", t5_te3, out)
    with pytest.raises(ValueError, match="does not start with 'lora_te3_'"):
        CL.combine("-", "-", te1, out, t5=True)
    with pytest.raises(ValueError, match="starts with none of"):
        CL.split_by_prefix({"lora_te4_x.alpha": torch.zeros(1)})


def test_sweep_command_line_and_refusals(tmp_path):
    """generate_images --base flux|sd3 with a T5 tower's LoRA file: what is refused before any model is loaded."""
    from safetensors.torch import save_file
    from sliders_conceptmod_amd import generate_images as G
    t5_keys = {f"lora_te2_encoder_block_0_layer_0_SelfAttention_q.{p}": torch.ones(2, 2) for p in ("lora_down.weight", "lora_up.weight")}
    clip_keys = {f"lora_te2_text_model_encoder_layers_0_self_attn_q_proj.{p}": torch.ones(2, 2) for p in ("lora_down.weight", "lora_up.weight")}
    t5_file, clip_file, te3_file, both = (str(tmp_path / n) for n in ("t5.safetensors", "clip.safetensors", "te3.safetensors", "both.safetensors"))
    save_file(t5_keys, t5_file)
    save_file(clip_keys, clip_file)
    save_file({k.replace("lora_te2_", "lora_te3_"): v for k, v in t5_keys.items()}, te3_file)
    save_file({**{k.replace("lora_te2_", "lora_te3_"): v for k, v in t5_keys.items()},
               "lora_unet_transformer_blocks_0_attn_to_q.lora_down.weight": torch.ones(2, 2)}, both)
    P = G.build_parser()
    for base in ("flux", "sd3"):
        args = lambda *extra: G.fill_defaults(P.parse_args(["--prompts_path", "p.csv", "--save_path", str(tmp_path), "--base", base,
                                                            "--pretrained_model", f"synthetic://tiny_{base}"] + list(extra)))
        # without the native backend: the ValueError that names --te_model_name, before the file is read
        for backend in ([], ["--t5_backend", "torch"]) if base == "flux" else ([],):
            with pytest.raises(ValueError, match="--te_model_name only with --t5_backend native"):
                G.t5_sweep_states(args("--te_model_name", "missing.safetensors", *backend), base)
        with pytest.raises(ValueError, match="--synthetic_towers"):
            G.t5_sweep_states(args("--synthetic_towers", "--t5_backend", "native"), base)
        # a CLIP tower's keys keep a ValueError that names --te_model_name
        with pytest.raises(ValueError, match="--te_model_name .*clip.safetensors: not a T5 tower's LoRA file"):
            G.t5_sweep_states(args("--te_model_name", clip_file, "--t5_backend", "native"), base)
        with pytest.raises(ValueError, match="one --te_model_name file"):
            G.t5_sweep_states(args("--te_model_name", f"{t5_file},{te3_file}", "--t5_backend", "native"), base)
        # accepted: either prefix as --te_model_name, or the T5 part of a combine_loras file as --model_name
        for f, prefix in ((t5_file, "lora_te2"), (te3_file, "lora_te3")):
            slider, state, got = G.t5_sweep_states(args("--te_model_name", f, "--t5_backend", "native"), base)
            assert slider is None and got == prefix and len(state) == 2
        slider, state, got = G.t5_sweep_states(args("--model_name", both, "--t5_backend", "native"), base)
        assert list(slider) == ["lora_unet_transformer_blocks_0_attn_to_q.lora_down.weight"] and got == "lora_te3" and len(state) == 2
        with pytest.raises(ValueError, match="--t5_backend native"):
            G.t5_sweep_states(args("--model_name", both), base)
        with pytest.raises(ValueError, match="already holds a T5 tower's LoRA"):
            G.t5_sweep_states(args("--model_name", both, "--te_model_name", t5_file, "--t5_backend", "native"), base)
        # no T5 file: the slider's state as it is
        assert G.t5_sweep_states(args(), base) == (None, None, None)


def test_native_tower_cache_is_bypassed_under_an_adaptor():
    """NativeT5Tower.encode_cached: the cache serves the frozen tower only; with an attached network at a non-zero
    multiplier every call runs the encoder."""
    from sliders_conceptmod_amd import lora, model_util as MU
    tower = MU._synthetic_native_t5(64)
    calls = []
    tower.encode = lambda p, n: (calls.append((p, n)), torch.zeros(1))[1]
    tower.encode_cached("a", 4), tower.encode_cached("a", 4)
    assert calls == [("a", 4)]
    net = lora.LoRANetwork(tower.model, rank=4, alpha=1.0, target_replace=lora.T5_TARGET_REPLACE, prefix="lora_te2", train_method="t5attn")
    net.set_lora_slider(2.0)
    with net:
        tower.encode_cached("a", 4), tower.encode_cached("a", 4)
    assert calls == [("a", 4)] * 3
    tower.encode_cached("a", 4)  # outside the block the multiplier is 0: the frozen rows, from the cache
    net.set_lora_slider(0.0)
    with net:
        tower.encode_cached("a", 4)
    assert calls == [("a", 4)] * 3
