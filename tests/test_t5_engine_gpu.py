"""The native T5 encoder (csrc/engine_t5.hip through sliders_conceptmod_amd.t5.T5EncoderModel) on a real MI355X against the
float64 restatement of tests/t5_refs.py, under the project's twin bar: the engine's relative L2 distance from float64 may be
at most twice that of transformers' own bf16 run on the same bf16-rounded weights.  Then the bitwise properties (the same
call twice, one engine across lengths, a prompt alone and in a batch) and every refusal."""
import ctypes as C

import pytest
import torch

import t5_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def native():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    _native.lib()
    return _native


def build(cfg, sd, max_tokens=512):
    from sliders_conceptmod_amd import t5 as PT
    m = PT.T5EncoderModel(PT.T5Config(**cfg.__dict__), max_tokens)
    m.load_state_dict(sd)
    return m.to("cuda", BF).requires_grad_(False).eval()


@pytest.fixture(scope="module")
def test_model():
    cfg = R.test_cfg()
    sd = R.rounded_state(R.seeded_state(cfg), BF)
    return cfg, sd, build(cfg, sd)


def check_bar(cfg, sd, model, ids, what):
    ref = R.forward64(cfg, sd, ids)
    bar = R.twin_bar(cfg, sd, ids, ref)
    got = model(ids.cuda())[0]
    torch.cuda.synchronize()
    assert got.dtype == BF and tuple(got.shape) == (ids.shape[0], ids.shape[1], cfg.d_model)
    dist = R.rel_l2(got.cpu(), ref)
    print(f"{what}: engine {dist:.4f}, bar (2 x twin) {bar:.4f}")
    assert torch.isfinite(got).all() and dist <= bar, f"{what}: {dist:.4f} > {bar:.4f}"
    return got


@pytest.mark.parametrize("L", R.LENGTHS)
def test_model_under_twin_bar(native, test_model, L):
    cfg, sd, model = test_model
    check_bar(cfg, sd, model, R.seeded_ids(cfg, R.BATCH, L), f"test model L={L}")


@pytest.mark.parametrize("L", (5, 130))
def test_inner_wider_than_model(native, L):
    """tiny_t5_config(64): 2 heads of 64, inner 128 != d_model 64."""
    from sliders_conceptmod_amd import t5 as PT
    cfg = PT.tiny_t5_config(64)
    assert cfg.num_heads * cfg.d_kv != cfg.d_model
    sd = R.rounded_state(R.seeded_state(cfg, seed=5), BF)
    check_bar(cfg, sd, build(cfg, sd), R.seeded_ids(cfg, R.BATCH, L), f"tiny_t5_config(64) L={L}")


def test_xxl_width(native):
    """One block at T5-XXL's width: d_model 4096 (the four-wave RMSNorm), 64 heads, inner 4096."""
    cfg = R.Cfg(vocab_size=64, d_model=4096, num_heads=64, d_ff=512, num_layers=1)
    sd = R.rounded_state(R.seeded_state(cfg, seed=6), BF)
    check_bar(cfg, sd, build(cfg, sd), R.seeded_ids(cfg, 1, 70), "width 4096 L=70")


def test_bitwise_properties(native, test_model):
    cfg, sd, model = test_model
    ids256, ids3 = R.seeded_ids(cfg, R.BATCH, 256).cuda(), R.seeded_ids(cfg, R.BATCH, 3).cuda()
    a = model(ids256)[0].clone()
    assert torch.equal(model(ids256)[0], a), "the same call twice"
    engine = model._engine(R.BATCH)
    model(ids3)
    assert torch.equal(model(ids256)[0], a), "L = 256, then 3, then 256"
    assert model._engine(R.BATCH) is engine, "one engine served both lengths"
    # A prompt alone and in a batch of 2: bitwise, as test_flux_engine_gpu.py holds it for its engine.  Every GEMM tile gives
    # the same bits and the engine lends no split-K scratch, so the row count of a launch changes no sum's order; the norm,
    # the gate and the attention work row by row or per (sample, head).
    for L in (3, 130):
        ids = R.seeded_ids(cfg, R.BATCH, L).cuda()
        both = model(ids)[0].clone()
        for i in range(R.BATCH):
            assert torch.equal(model(ids[i:i + 1])[0][0], both[i]), f"sample {i} alone, L={L}"


def test_out_of_range_ids_are_clamped(native, test_model):
    cfg, sd, model = test_model
    ids = R.seeded_ids(cfg, 1, 9).cuda()
    bad = ids.clone()
    bad[0, 2], bad[0, 5] = -7, cfg.vocab_size + 3
    ids[0, 2], ids[0, 5] = 0, cfg.vocab_size - 1
    assert torch.equal(model(bad)[0], model(ids)[0])


def test_refusals(native, test_model):
    from sliders_conceptmod_amd import t5 as PT
    cfg, sd, model = test_model
    pcfg = PT.T5Config(**cfg.__dict__)
    dev = torch.device("cuda")
    state = {k: v.detach() for k, v in model.state_dict().items()}

    def refused(match, fn):
        with pytest.raises(native.SmiError, match=match):
            fn()

    # by the config: no workspace is sized, nothing is launched
    refused("f16 is refused", lambda: native.t5_workspace_bytes(pcfg, torch.float16, 1, 64))
    for field, value, match in (("d_kv", 32, "d_kv 32"), ("d_model", 96, "d_model 96"), ("d_ff", 200, "d_ff 200")):
        bad = PT.T5Config(**{**cfg.__dict__, field: value})
        refused(match, lambda: native.t5_workspace_bytes(bad, BF, 1, 64))
    refused("max_tokens", lambda: native.t5_workspace_bytes(pcfg, BF, 1, 4096))
    refused("gated", lambda: native.t5_config_c(PT.T5Config(**{**cfg.__dict__, "feed_forward_proj": "relu"}), BF, 64))
    # by the weights
    wi0 = "encoder.block.1.layer.1.DenseReluDense.wi_0.weight"
    missing = {k: v for k, v in state.items() if k != "encoder.block.1.layer.0.SelfAttention.o.weight"}
    refused("missing weight 'encoder.block.1.layer.0.SelfAttention.o.weight'", lambda: native.T5Engine(pcfg, BF, missing, 1, 64, dev))
    shaped = dict(state)
    shaped[wi0] = state[wi0][:-8].contiguous()
    refused("wi_0.weight': expected", lambda: native.T5Engine(pcfg, BF, shaped, 1, 64, dev))
    plain = {k: v for k, v in state.items() if ".wi_" not in k}
    plain.update({f"encoder.block.{i}.layer.1.DenseReluDense.wi.weight": state[wi0] for i in range(cfg.num_layers)})
    refused("non-gated feed-forward", lambda: native.T5Engine(pcfg, BF, plain, 1, 64, dev))
    # by the call: the output stays as it was
    e = native.T5Engine(pcfg, BF, state, 1, 64, dev)
    out = torch.full((1, 70, cfg.d_model), float("nan"), dtype=BF, device=dev)
    ids = torch.zeros(2, 70, dtype=torch.int32, device=dev)
    lib = native.lib()
    for n, L, match in ((1, 65, b"L 65 outside [1, 64]"), (1, 0, b"L 0 outside"), (2, 8, b"batch 2 outside")):
        assert lib.smi_t5_encode(e.handle, n, L, C.c_void_p(ids.data_ptr()), C.c_void_p(out.data_ptr())) != 0
        assert match in lib.smi_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # not a T5 engine
    assert lib.smi_t5_encode(None, 1, 8, C.c_void_p(ids.data_ptr()), C.c_void_p(out.data_ptr())) != 0
    e.close()
