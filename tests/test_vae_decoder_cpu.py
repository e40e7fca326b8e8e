"""AutoencoderKL decoder and the slider image command, host side: the parameter container against the CPU restatement
(tests/vae_decoder_ref.py), state-dict loading, the library's dry-run planner and batch rule (no GPU needed), and the
command line's host logic (CSV, folder names, what a LoRA file says about its network)."""
import ctypes as C
import os

import pytest
import torch

import vae_decoder_ref as R
from sliders_conceptmod_amd import _native
from sliders_conceptmod_amd import generate_images as G
from sliders_conceptmod_amd import vae as PV
from sliders_conceptmod_amd import vae_decoder as PD


def product(cfg):
    return PD.AutoencoderKLDecoder(PV.VAEConfig(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}))


@pytest.mark.parametrize("cfg", [R.VAEConfig(), R.tiny_vae_config()], ids=["sd", "tiny"])
def test_container_keys_and_shapes_match_restatement(cfg):
    with torch.device("meta"):
        a = product(cfg).state_dict()
        b = R.AutoencoderKLDecoderRef(cfg).state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape for k in a)


def test_sd_decoder_parameter_count():
    with torch.device("meta"):
        d = PD.AutoencoderKLDecoder(PV.sd_vae_config())
    n_dec = sum(p.numel() for k, p in d.named_parameters() if k.startswith("decoder."))
    n_pq = sum(p.numel() for k, p in d.named_parameters() if k.startswith("post_quant_conv."))
    assert (n_dec, n_pq) == (49490179, 20)  # the public SD VAE decoder + post_quant_conv


def _full_state(cfg, seed=0):
    """A full AutoencoderKL state dict: encoder + quant_conv (the encoder container) and decoder + post_quant_conv."""
    from oracle import vae_ref as OV
    enc = OV.init_synthetic_(OV.AutoencoderKLRef(cfg), seed=seed).state_dict()
    dec = R.init_synthetic_(R.AutoencoderKLDecoderRef(cfg), seed=seed + 1).state_dict()
    return {**enc, **dec}, dec


def test_full_state_dict_loads_strictly():
    cfg = R.tiny_vae_config()
    full, dec = _full_state(cfg)
    d = product(cfg)
    d.load_state_dict(full, strict=True)
    for k, v in d.state_dict().items():
        assert torch.equal(v, dec[k]), k


def test_deprecated_attention_names_load():
    cfg = R.tiny_vae_config()
    full, dec = _full_state(cfg)
    old = {}
    for k, v in full.items():
        for new, dep in ((".to_q.", ".query."), (".to_k.", ".key."), (".to_v.", ".value."), (".to_out.0.", ".proj_attn.")):
            if k.startswith("decoder.mid_block.attentions.0") and new in k:
                k = k.replace(new, dep)
                if v.ndim == 2:  # some SD-1.x checkpoints store them as 1 x 1 conv kernels
                    v = v[:, :, None, None]
                break
        old[k] = v
    assert any(".proj_attn." in k for k in old)
    d = product(cfg)
    d.load_state_dict(old, strict=True)
    for k, v in d.state_dict().items():
        assert torch.equal(v, dec[k]), k


def test_decode_off_gpu_raises():
    d = product(R.tiny_vae_config())
    with pytest.raises(_native.SmiError):
        d.decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(_native.SmiError):
        d.decode_to_uint8(torch.zeros(1, 4, 8, 8))


def _cfg_c():
    c = _native.VaeConfigC()
    c.dtype, c.in_channels, c.latent_channels, c.n_levels = 0, 3, 4, 4
    for i, v in enumerate((128, 256, 512, 512)):
        c.block_out_channels[i] = v
    c.layers_per_block, c.norm_num_groups = 2, 32
    return c


def test_decoder_workspace_plan_dry_run():
    c = _cfg_c()
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 2, 1024, 1024, C.byref(out)), "plan")
    assert 1e9 < out.value < 40e9  # ~17 GB: two 1024^2 images, fp32 16384^2 scores of the mid-block attention included
    assert _native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 1, 1020, 1024, C.byref(out)) != 0  # not % 8
    assert _native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 8, 1024, 1024, C.byref(out)) != 0  # > 4 GiB operand
    assert b"largest batch that fits is 7" in _native.lib().smi_last_error()
    assert _native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 7, 1024, 1024, C.byref(out)) == 0
    assert _native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 31, 512, 512, C.byref(out)) == 0
    assert _native.lib().smi_vae_decoder_workspace_bytes(C.byref(c), 32, 512, 512, C.byref(out)) != 0
    assert PD.max_decode_batch(PV.sd_vae_config(), 1024, 1024) == 7
    assert PD.max_decode_batch(PV.sd_vae_config(), 512, 512) == 31


# ---- command line host logic ---------------------------------------------------------------------------------------------
def test_prompts_csv_parsing(tmp_path):
    p = tmp_path / "prompts.csv"
    p.write_text('prompt,evaluation_seed,case_number,extra\n"a photo of a person, smiling",42,0,x\nold man,7.0,3,y\n')
    rows = G.read_prompts(str(p))
    assert rows == [{"prompt": "a photo of a person, smiling", "evaluation_seed": 42, "case_number": 0},
                    {"prompt": "old man", "evaluation_seed": 7, "case_number": 3}]


def test_scale_str_and_output_paths():
    assert [G.scale_str(s) for s in G.parse_scales("-2,-1,-0.5,0,0.5,1,2")] == ["-2", "-1", "-half", "0", "half", "1", "2"]
    per, strip = G.output_paths("out", "age", G.parse_scales("-1,0,1.5"), 3, 1)
    assert per == [os.path.join("out", "age", d, "3_1.png") for d in ("-1", "0", "1.5")]
    assert strip == os.path.join("out", "age", "all", "3_1.png")


@pytest.mark.parametrize("model", ["tiny_sd1x", "tiny_sdxl"])
@pytest.mark.parametrize("method", G.TRAIN_METHODS)
@pytest.mark.parametrize("ext", [".pt", ".safetensors"])
def test_lora_file_params_recovered(tmp_path, model, method, ext):
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    _, _, unet, _ = MU.load_models(f"synthetic://{model}", xl=model.endswith("xl"))
    rank, alpha = (8, 2.0) if method.startswith("x") else (4, 1.0)
    net = L.LoRANetwork(unet, rank=rank, multiplier=1.0, alpha=alpha, train_method=method)
    f = tmp_path / f"slider{ext}"
    net.save_weights(str(f), dtype=torch.float16)
    if not net.unet_loras:  # e.g. noxattn-hspace-last without conv targets: an empty file is no slider
        with pytest.raises(ValueError):
            G.lora_file_params(G.load_lora_state(str(f)), unet)
        return
    got_rank, got_alpha, got_method, _ = G.lora_file_params(G.load_lora_state(str(f)), unet)
    assert (got_rank, got_alpha) == (rank, alpha)
    # methods with equal key sets build the same network: the recovered one must select the same layers
    want = {t[0] for t in L.select_targets(unet, method, L.DEFAULT_TARGET_REPLACE, L.LORA_PREFIX_UNET, "_")}
    have = {t[0] for t in L.select_targets(unet, got_method, L.DEFAULT_TARGET_REPLACE, L.LORA_PREFIX_UNET, "_")}
    assert want == have
    if method in ("xattn", "full", "xattn-strict"):  # the only methods with their own key set on these UNets
        assert got_method == method


def test_lora_file_params_c3lier(tmp_path):
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.model_util as MU
    _, _, unet, _ = MU.load_models("synthetic://tiny_sd1x")
    net = L.LoRANetwork(unet, rank=4, alpha=1.0, train_method="noxattn",
                        target_replace=L.DEFAULT_TARGET_REPLACE + L.UNET_TARGET_REPLACE_MODULE_CONV)
    f = tmp_path / "c3.pt"
    net.save_weights(str(f))
    rank, alpha, method, tr = G.lora_file_params(G.load_lora_state(str(f)), unet)
    assert (rank, alpha, method) == (4, 1.0, "noxattn") and "ResnetBlock2D" in tr
