"""The float64 references of tests/notrigger_refs.py checked on the CPU: the tower against the oracle, and the bars of the
GPU tests against mutated references -- a bar that a wrong kernel or a wrong engine passes checks nothing."""
import pytest
import torch

import notrigger_refs as R
from oracle import clip_ref

DT = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("act,proj", [("quick_gelu", None), ("gelu", 64)])
def test_f64_tower_equals_the_oracle(act, proj):
    cfg = R.tiny_config(act, proj)
    sd = R.tiny_state(cfg)
    ids = R.tiny_ids(cfg, 3)
    want = clip_ref.clip_text_forward(sd, ids, cfg.num_attention_heads, cfg.hidden_act, cfg.eos_token_id)
    got = R.tower_forward({k: v.double() for k, v in sd.items()}, ids, cfg.num_attention_heads, cfg.hidden_act)
    assert R.rel(got["last_hidden_state"], want["last_hidden_state"]) < 2e-6
    assert R.rel(got["penultimate"], want["penultimate"]) < 2e-6


@pytest.fixture(scope="module", params=DT, ids=["fp16", "bf16"])
def attn_case(request):
    return request.param, R.causal_attn_case(77, request.param)


def _errs(got, want):
    return [R.rel(g, w) for g, w in zip(got, want)]


def test_kernel_bar_accepts_the_rounded_reference(attn_case):
    dtype, c = attn_case
    e_q = _errs(c["B"][2:], c["A"][2:])
    print(f"{dtype}: e_q dq {e_q[0]:.2e} dk {e_q[1]:.2e} dv {e_q[2]:.2e}")
    assert all(0 < e < (2e-3 if dtype == torch.float16 else 1.6e-2) for e in e_q)  # a few unit roundoffs (2^-11, 2^-8)


@pytest.mark.parametrize("mutation", R.ATTN_MUTATIONS)
def test_kernel_bar_rejects_a_wrong_backward(attn_case, mutation):
    """Each mutation, in the ROUNDED form (what a wrong kernel would compute), misses the bar on at least one output --
    by at least twice the bar (the single extra cell is the smallest miss: 5 % against bars of 0.1 % / 0.8 %)."""
    dtype, c = attn_case
    oB, lse = c["B"][0], c["B"][1]
    bad = R.causal_attn_bwd(c["q"], c["k"], c["v"], oB, lse, c["do"], c["scale"], dtype, mutate=mutation)
    e_q = _errs(c["B"][2:], c["A"][2:])
    e = _errs(bad, c["A"][2:])
    worst = max(err / R.bar(q) for err, q in zip(e, e_q))
    print(f"{dtype} {mutation}: errors {e}, worst / bar {worst:.1f}")
    assert worst > 2


def test_act_bar_rejects_the_other_activation():
    g = torch.Generator().manual_seed(5)
    for dtype in DT:
        x, dy = R.representable((4096,), g, dtype, 2.0), R.representable((4096,), g, dtype)
        for kind in (0, 1):
            A, B = R.act_bwd(x, dy, kind), R.act_bwd(x, dy, kind, dtype)
            e_q = R.rel(B, A)
            wrong = R.rel(R.act_bwd(x, dy, 1 - kind, dtype), A)
            print(f"{dtype} kind {kind}: e_q {e_q:.2e}, the other activation {wrong:.2e}")
            assert wrong > 2 * R.bar(e_q)


@pytest.fixture(scope="module")
def tower_case():
    cfg = R.tiny_config()
    sd = {k: v.double() for k, v in R.tiny_state(cfg).items()}
    ids = R.tiny_ids(cfg, 2)
    names = R.site_names(cfg.num_hidden_layers)
    g = torch.Generator().manual_seed(11)
    lora = R.make_lora(names, cfg.hidden_size, 4, 1.0, g)
    d_hidden = torch.randn((2, 77, cfg.hidden_size), generator=g, dtype=torch.float64).float().double()
    return cfg, sd, ids, names, lora, d_hidden


@pytest.mark.parametrize("which", ["last_layer_out", "penultimate"])
@pytest.mark.parametrize("dtype", DT, ids=["fp16", "bf16"])
def test_engine_bar_rejects_a_wrong_tower(tower_case, which, dtype):
    cfg, sd, ids, names, lora, dh = tower_case
    args = (sd, ids, cfg.num_attention_heads, cfg.hidden_act, lora, names, [1.0, -1.0], 0.25, dh, which)
    A = torch.cat(R.tower_grads(*args))
    B = torch.cat(R.tower_grads(*args, dtype=dtype))
    e_q = R.rel(B, A)
    print(f"{which} {dtype}: e_q {e_q:.2e}")
    assert 0 < e_q < (5e-3 if dtype == torch.float16 else 4e-2)
    for mutation in ("drop_site", "flip_sign", "drop_layer"):
        if which == "penultimate" and mutation == "drop_layer":
            continue  # hidden_states[-2] does not depend on the last layer: nothing to drop
        bad = torch.cat(R.tower_grads(*args, dtype=dtype, mutate=mutation))
        print(f"  {mutation}: {R.rel(bad, A):.2e} against a bar of {R.bar(e_q):.2e}")
        assert R.rel(bad, A) > 2 * R.bar(e_q), (mutation, R.rel(bad, A), e_q)
    if which == "penultimate":  # the last layer's sites get a zero gradient
        d_down, _ = R.tower_grads(*args)
        per = 4 * 4 * cfg.hidden_size
        assert float(d_down[per:].abs().max()) == 0.0 and float(d_down[:per].abs().max()) > 0.0


def test_new_abi_symbols_exist():
    from sliders_conceptmod_amd import _native
    lib = _native.lib()
    for name in ("smi_op_attention_causal_fwd", "smi_op_attention_causal_bwd", "smi_op_act", "smi_clip_lora_workspace_bytes",
                 "smi_clip_lora_create", "smi_clip_forward_lora", "smi_clip_backward"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_lora_plan_refuses_what_the_backward_cannot_take():
    """smi_clip_lora_workspace_bytes is a host-only dry run: it sizes the tiny tower and refuses DoRA sites, a rank above 16,
    sites off the attention projections and a head_dim the causal backward does not take."""
    import sliders_conceptmod_amd.clip as PC
    from sliders_conceptmod_amd import _native
    cfg = R.tiny_config()
    names = R.site_names(cfg.num_hidden_layers)
    sites, nd, nu = R.flat_layout(names, cfg.hidden_size, 4, 1.0)
    small = _native.clip_lora_workspace_bytes(cfg, torch.float16, sites, 1)
    assert 0 < small < _native.clip_lora_workspace_bytes(cfg, torch.float16, sites, 4)
    with pytest.raises(_native.SmiError, match="DoRA"):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, [dict(s, off_dora=0) for s in sites], 2)
    with pytest.raises(_native.SmiError, match="rank"):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, R.flat_layout(names, cfg.hidden_size, 32, 1.0)[0], 2)
    with pytest.raises(_native.SmiError, match="self_attn"):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, [dict(sites[0], target="text_model.encoder.layers.0.mlp.fc1")], 2)
    with pytest.raises(_native.SmiError, match="all or none"):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, sites[:2], 2)
    wide = PC.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                             num_attention_heads=4, eos_token_id=999)
    with pytest.raises(_native.SmiError, match="head_dim"):
        _native.clip_lora_workspace_bytes(wide, torch.float16, sites, 2)
