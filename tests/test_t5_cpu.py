"""What the native T5 encoder's tests stand on, checked without a GPU: the float64 restatement of tests/t5_refs.py against
transformers, the host bucket function against transformers' at every offset, what the engine's twin bar can and cannot see
(mutated restatements), the kernel bounds against fp32 emulations and mutated references, and the host logic: state-dict
names, refusals by name, the tower's dtype rule, encode_prompts_sd3 with two towers, the new flag and its defaults.

Measured (relative L2; test model of t5_refs.test_cfg, batch 2, L = 3 / 77 / 130 / 256):
  restatement, T5LayerNorm's variance in fp32 as transformers keeps it, vs transformers .double():  6e-16 .. 2.4e-15
  restatement, all float64, vs transformers .double():   8.1e-8 / 5.2e-7 / 7.5e-7 / 7.1e-7
  transformers float32 vs transformers .double():        6.7e-7 / 2.5e-6 / 2.5e-6 / 2.9e-6
  so the all-float64 restatement is 8.3 / 4.8 / 3.4 / 4.0 times closer than the float32 run: its whole distance is the double
  model's own fp32 variance (with that one site restated the two agree to rounding), amplified by scores of standard
  deviation ~11 -- the factor of 4 holds for the restatement of what the double model computes, by nine orders of magnitude.
  twin (transformers bf16) distance from float64: 0.0096 / 0.026 / 0.026 / 0.030, the bar twice that
  mutations (L = 3 / 77 / 130 / 256): bias dropped 0.20 / 0.49 / 0.46 / 0.36, mirrored 0.21 / 0.57 / 0.51 / 0.43, scores / 8
  0.63 / 0.87 / 0.84 / 0.85, halves swapped 0.54 / 0.72 / 0.69 / 0.72, final weight ignored 0.18 / 0.19 / 0.19 / 0.19,
  max_distance 64 0 / 0.51 / 0.50 / 0.38, mean subtracted 0.18 / 0.52 / 0.52 / 0.51, block 1 on a zero table 0.078 / 0.20 /
  0.18 / 0.14; erf-GELU 1.7e-4 .. 2.3e-4: inside the bar, the kernel test is what catches it."""
import argparse
import warnings

import pytest
import torch

import attention_refs as A
import t5_refs as R

BF = torch.bfloat16


@pytest.fixture(scope="module")
def model():
    cfg = R.test_cfg()
    return cfg, R.rounded_state(R.seeded_state(cfg), BF)


@pytest.fixture(scope="module")
def refs(model):
    """Per length: ids, the float64 reference and the twin bar; computed once, never modified."""
    cfg, sd = model
    out = {}
    for L in R.LENGTHS:
        ids = R.seeded_ids(cfg, R.BATCH, L)
        ref = R.forward64(cfg, sd, ids)
        out[L] = (ids, ref, R.twin_bar(cfg, sd, ids, ref))
    return out


# ---- the restatement against transformers ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.LENGTHS)
def test_restatement_against_transformers(model, refs, L):
    cfg, sd = model
    ids, ref, _ = refs[L]
    with torch.no_grad():
        m64 = R.hf_model(cfg, sd, torch.float64)(ids)[0]
        m32 = R.hf_model(cfg, sd, torch.float32)(ids)[0]
    own = R.rel_l2(m32, m64)
    as_hf = R.rel_l2(R.forward64(cfg, sd, ids, hf_variance=True), m64)
    pure = R.rel_l2(ref, m64)
    print(f"L={L}: float32 run {own:.3g}; restatement with transformers' fp32 variance {as_hf:.3g}, all float64 {pure:.3g} "
          f"({own / pure:.1f} x closer)")
    # transformers' double model keeps one fp32 site (T5LayerNorm's variance): restated with it, 4 x closer than the float32 run
    assert 4.0 * as_hf <= own
    # all in float64 the restatement can only differ from the double model by that site: closer than the float32 run, which
    # has it and every other one
    assert pure < own


# ---- the bucket function ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,md", [(32, 128), (32, 64), (16, 128), (64, 256)])
def test_relative_buckets_against_transformers(nb, md):
    from transformers.models.t5.modeling_t5 import T5Attention
    from sliders_conceptmod_amd import _native
    L = 1101
    rel = torch.arange(-(L - 1), L)
    want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=nb, max_distance=md).tolist()
    assert _native.t5_relative_buckets(nb, md, L) == want
    assert R.buckets(nb, md, L) == want
    # a shorter table is the middle of a longer one: what lets one engine serve every L up to max_tokens
    assert _native.t5_relative_buckets(nb, md, 77) == want[L - 77:L + 76]


def test_relative_buckets_refusals():
    from sliders_conceptmod_amd import _native
    for args in ((32, 128, 0), (31, 128, 8), (2, 128, 8), (32, 8, 8)):
        with pytest.raises(_native.SmiError, match="smi_t5_relative_buckets"):
            _native.t5_relative_buckets(*args)


# ---- what the engine bar can see ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.LENGTHS)
def test_mutations_leave_the_twin_bar(model, refs, L):
    cfg, sd = model
    ids, ref, bar = refs[L]
    print(f"L={L}: bar {bar:.4f}")
    assert bar <= 0.12  # (the bar is no blank cheque: the twin is 1 .. 3 % from float64)
    for mut in R.ENGINE_MUTATIONS:
        dist = R.rel_l2(R.forward64(cfg, sd, ids, mut), ref)
        print(f"  {mut}: {dist:.4f}")
        if mut == "max_distance_64" and L == 3:
            assert dist == 0.0  # identical by construction: every offset is below max_exact
            continue
        assert dist > bar, f"{mut} at L={L}: {dist:.4f} inside the bar {bar:.4f}"
    erf = R.rel_l2(R.forward64(cfg, sd, ids, "erf_gelu"), ref)
    print(f"  erf_gelu: {erf:.3g}")
    assert 0.0 < erf < bar  # the whole-network bar cannot see it; test_gated_gelu_bounds / the GPU kernel test do


# ---- kernel bounds: an fp32 emulation stays under E, mutated references leave 2 E --------------------------------------
DT = [torch.float16, BF]
IDS = ["f16", "bf16"]


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,C", [(3, 64), (130, 2056), (3, 4096), (1, 8192)])
def test_rmsnorm_bounds(dt, M, C):
    x, w = R.rms_inputs(M, C, dt)
    if dt == BF:
        assert float(x.abs().max()) >= 2.9e4
    ref = R.rms_ref(x, w, 1e-6)
    E = R.rms_bound(ref, C, dt)
    r = R.worst(R.rms_emulate(x, w, 1e-6, dt), ref, E)
    print(f"rmsnorm emulation M={M} C={C}: {r:.3f} E")
    assert r <= 1.0
    for fault in R.RMS_MUTANTS:
        rm = R.worst(R.rms_ref(x, w, 1e-6, fault), ref, E)
        print(f"  {fault}: {rm:.3g} E")
        if fault == "eps_outside" and M < 2:
            continue  # shows on rows whose mean of squares is near eps: row 1 of every three
        assert rm > 2.0 * R.SLACK, fault


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,F", R.GG_CASES)
def test_gated_gelu_bounds(dt, M, F):
    proj = R.gg_inputs(M, F, dt)
    ref = R.gg_ref(proj)
    E = R.gg_bound(ref, dt)
    r = R.worst(R.gg_emulate(proj, dt), ref, E)
    print(f"gated_gelu emulation M={M} F={F}: {r:.3f} E")
    assert r <= 1.0
    for fault in R.GG_MUTANTS:
        rm = R.worst(R.gg_ref(proj, fault), ref, E)
        print(f"  {fault}: {rm:.3g} E")
        assert rm > 2.0 * R.SLACK, fault


@pytest.mark.parametrize("H,L", [(3, 3), (64, 130)])
def test_bias_table_mutants(H, L):
    w = (1.5 * torch.randn(32, H, generator=torch.Generator().manual_seed(H))).to(BF)
    ref = R.bias_table(w, 32, 128, L)
    assert tuple(ref.shape) == (H, 2 * L - 1)
    assert torch.equal(ref[:, L - 1], w[0].double())  # offset 0 is bucket 0
    for fault in R.TABLE_MUTANTS:
        assert not torch.equal(R.bias_table(w, 32, 128, L, fault), ref), fault


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("L", (3, 77, 130))
def test_attention_bias_bounds(dt, L):
    B, H = R.ATTN_B, R.ATTN_H
    q, k, v, table = R.attn_inputs(B, H, L, dt)
    ref = R.attn_bias_ref(q, k, v, table, 1.0)
    E = R.attn_bias_bound(ref, q, k, v, 1.0, dt)
    r = A.ratio(R.attn_bias_emulate(q, k, v, table, 1.0, dt), ref["O"], E)
    print(f"attention_bias emulation L={L}: {r:.3f} E")
    assert r <= 1.0
    for fault in R.ATTN_MUTANTS:
        rm = A.ratio(R.attn_bias_ref(q, k, v, table, 1.0, fault, dt)["O"], ref["O"], E)
        print(f"  {fault}: {rm:.3g} E")
        assert rm > 2.0 * A.SLACK, fault


# ---- host logic --------------------------------------------------------------------------------------------------------
def test_state_dict_names_round_trip():
    from sliders_conceptmod_amd import t5 as PT
    cfg = R.test_cfg()
    hf = R.hf_model(cfg, R.seeded_state(cfg), torch.float32)
    mine = PT.T5EncoderModel(PT.T5Config(**cfg.__dict__))
    assert set(mine.state_dict()) == set(hf.state_dict())
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    mine.load_state_dict(hf.state_dict())
    back = R.hf_model(cfg, R.seeded_state(cfg, seed=9), torch.float32)
    back.load_state_dict(mine.state_dict())
    assert all(torch.equal(v, hf.state_dict()[k]) for k, v in back.state_dict().items())
    # the tied embedding stored once, under either name
    for keep, drop in (PT.T5EncoderModel.TIED, PT.T5EncoderModel.TIED[::-1]):
        sd = {k: v for k, v in hf.state_dict().items() if k != drop}
        other = PT.T5EncoderModel(PT.T5Config(**cfg.__dict__))
        other.load_state_dict(sd)
        assert torch.equal(other.shared.weight, hf.state_dict()[keep]) and other.encoder.embed_tokens is other.shared
    with pytest.raises(RuntimeError):
        mine.load_state_dict({k: v for k, v in hf.state_dict().items() if "final_layer_norm" not in k})


def test_refusals_by_name():
    from sliders_conceptmod_amd import _native, t5 as PT
    cfg = PT.T5Config(**R.test_cfg().__dict__)
    with_ = lambda **kw: PT.T5Config(**{**cfg.__dict__, **kw})
    assert _native.t5_workspace_bytes(cfg, BF, 2, 256) > 0
    for bad, dt, mt, match in ((cfg, torch.float16, 64, "f16 is refused"), (with_(d_kv=32), BF, 64, "d_kv 32"),
                               (with_(d_model=96), BF, 64, "d_model 96"), (with_(d_ff=200), BF, 64, "d_ff 200"),
                               (cfg, BF, 0, "max_tokens 0"), (cfg, BF, 4096, "max_tokens 4096"),
                               (with_(feed_forward_proj="relu"), BF, 64, "gated"), (cfg, torch.float32, 64, "bfloat16")):
        with pytest.raises(_native.SmiError, match=match):
            _native.t5_workspace_bytes(bad, dt, 1, mt)
    with pytest.raises(_native.SmiError, match="gated"):
        PT.T5EncoderModel(with_(feed_forward_proj="gated-silu"))
    m = PT.T5EncoderModel(cfg)
    with pytest.raises(_native.SmiError, match="cuda device"):  # no CPU fallback
        m(torch.zeros(1, 4, dtype=torch.int64))
    with pytest.raises(_native.SmiError, match="attention mask"):
        m(torch.zeros(1, 4, dtype=torch.int64), attention_mask=torch.ones(1, 4))


def test_native_tower_dtype_rule_and_tokenizer():
    from sliders_conceptmod_amd import model_util as MU, t5 as PT
    tower = MU._synthetic_native_t5(64)
    assert tower.dim == 64 and tower.model.config.num_heads * tower.model.config.d_kv == 128
    with pytest.warns(UserWarning, match="float16 requested"):
        tower.to(dtype=torch.float16)
    assert tower.dtype == BF and tower.device.type == "cpu"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tower.to(dtype=BF)
    tok = PT.SyntheticT5Tokenizer(1024)
    a = tok("A photo of a cat", padding="max_length", max_length=16).input_ids
    b = tok("a photo of a dog", padding="max_length", max_length=16).input_ids
    assert tuple(a.shape) == (1, 16) and a[0, 5] == 1 and int(a[0, 6:].sum()) == 0 and int(a[0, :5].min()) >= 2 and int(a.max()) < 1024
    assert torch.equal(a[0, :4], b[0, :4]) and a[0, 4] != b[0, 4]
    assert tuple(tok("one two three four", padding="max_length", max_length=3).input_ids[0][-1:]) == (1,)


def test_encode_prompts_sd3_with_two_towers_is_unchanged():
    from sliders_conceptmod_amd import model_util as MU, train_util as TU
    toks, encs = MU.synthetic_sd3_towers(True)
    got, pooled = TU.encode_prompts_sd3(None, toks, encs, "a photo of a cat", 2, 5, 64)
    # what the function did before it knew a third tower: the CLIP block, then t5_tokens zero rows
    embeds, pl = [], []
    for tok, enc in zip(toks, encs):
        ids = tok("a photo of a cat", padding="max_length", max_length=tok.model_max_length, truncation=True,
                  return_tensors="pt").input_ids
        out = enc(ids.to(enc.device), output_hidden_states=True)
        pl.append(out[0])
        embeds.append(out.hidden_states[-2])
    clip = torch.cat(embeds, dim=-1)
    want = torch.cat([clip, torch.zeros(1, 5, 64)], dim=1).repeat_interleave(2, dim=0)
    assert torch.equal(got, want) and torch.equal(pooled, torch.cat(pl, dim=-1).repeat_interleave(2, dim=0))
    assert torch.equal(TU.encode_prompts_sd3(None, toks, encs + [None], "a photo of a cat", 2, 5, 64)[0], want)

    class Tower:  # a third tower writes its rows where the zero rows are
        def encode_cached(self, prompt, n):
            return torch.full((1, n, 64), 3.0)
    third = TU.encode_prompts_sd3(None, toks + [None], encs + [Tower()], "a photo of a cat", 2, 5, 64)[0]
    assert torch.equal(third[:, :-5], want[:, :-5]) and bool((third[:, -5:] == 3.0).all())


def test_flag_and_defaults():
    import inspect
    from sliders_conceptmod_amd import generate_images as GI, model_util as MU, train_lora_flux as TF, train_lora_sd3 as TS
    assert inspect.signature(MU.load_models_flux).parameters["t5_backend"].default == "torch"
    assert inspect.signature(MU.load_models_sd3).parameters["t5_backend"].default is None
    assert inspect.signature(TF.train).parameters["t5_backend"].default == "torch"
    assert inspect.signature(TS.train).parameters["t5_backend"].default is None
    assert TF.build_parser().parse_args(["--alpha", "1"]).t5_backend == "torch"
    assert TF.build_parser().parse_args(["--alpha", "1", "--t5_backend", "native"]).t5_backend == "native"
    assert TS.build_parser().parse_args(["--alpha", "1"]).t5_backend is None
    assert TS.build_parser().parse_args(["--alpha", "1", "--t5_backend", "native"]).t5_backend == "native"
    parser = next(v for v in vars(GI).values() if callable(v) and getattr(v, "__name__", "") in ("build_parser", "make_parser"))
    ns = parser().parse_args(["--prompts_path", "p.csv", "--save_path", "out"])
    assert ns.t5_backend is None
    assert isinstance(ns, argparse.Namespace)
    with pytest.raises(SystemExit):
        TF.build_parser().parse_args(["--alpha", "1", "--t5_backend", "triton"])
    # the default towers are what they were: the hashed stand-in for synthetic Flux, two towers for SD3
    _, encs, _, _ = MU.load_models_flux("synthetic://tiny_flux")
    assert isinstance(encs[1], MU.SyntheticT5Tower)
    _, encs, _, _ = MU.load_models_flux("synthetic://tiny_flux", t5_backend="native")
    assert isinstance(encs[1], MU.NativeT5Tower) and encs[1].dim == 64
    toks, encs, _, _ = MU.load_models_sd3("synthetic://tiny_sd3")
    assert len(encs) == 2 and len(toks) == 2
    toks, encs, _, _ = MU.load_models_sd3("synthetic://tiny_sd3", t5_backend="native")
    assert len(encs) == 3 and isinstance(encs[2], MU.NativeT5Tower)
    for bad in ("torch", "triton"):
        with pytest.raises(ValueError, match="t5_backend"):
            MU.load_models_sd3("synthetic://tiny_sd3", t5_backend=bad)
    with pytest.raises(ValueError, match="t5_backend"):
        MU.load_models_flux("synthetic://tiny_flux", t5_backend="triton")
