"""AutoencoderKL decoder on the HIP engine (`vae.decode(latents / scaling_factor).sample`, E/generate_images_sd1.py:195-200)
against the CPU restatement (tests/vae_decoder_ref.py, parity-unpinned like the encoder's oracle) on the same seeded
weights and latents; the fused tail (csrc/vae_decode.hip) against the unfused composition (SMI_VAE_DEC_TAIL=0); the
uint8 output against torch's post-processing of the engine's own sample; batch composition and chunking."""
import ctypes as C

import pytest
import torch

import vae_decoder_ref as R
from sliders_conceptmod_amd import _native

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def pair(cfg, dtype, seed=7):
    from sliders_conceptmod_amd import vae as PV
    from sliders_conceptmod_amd import vae_decoder as PD
    ref = R.init_synthetic_(R.AutoencoderKLDecoderRef(cfg), seed=seed).eval()
    d = PD.AutoencoderKLDecoder(PV.VAEConfig(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}))
    d.load_state_dict(ref.state_dict())
    return ref, d.to("cuda", dtype).requires_grad_(False).eval()


def latents(n, h, w, seed=3):
    return torch.randn(n, 4, h // 8, w // 8, generator=torch.Generator().manual_seed(seed))


# bars = 1.5 x measured (tiny: fp16 1.61e-3, bf16 1.32e-2; SD 256^2: fp16 1.24e-3, bf16 9.94e-3) -- the encoder's are
# 2.3e-3 / 1.85e-2
TINY_BARS = {torch.float16: 2.4e-3, torch.bfloat16: 2.0e-2}
REAL_BARS = {torch.float16: 1.9e-3, torch.bfloat16: 1.5e-2}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("size", [(64, 64), (96, 64)])
def test_tiny_decoder_matches_restatement(dtype, size):
    ref, d = pair(R.tiny_vae_config(), dtype)
    z = latents(2, *size)
    with torch.no_grad():
        want = ref.decode(z)
    got = d.decode(z.cuda()).sample
    assert got.shape == want.shape == (2, 3, *size) and got.dtype == torch.float32
    e = rel(got, want)
    print(f"tiny VAE decoder {dtype} {size}: sample rel err {e:.2e}")
    assert e < TINY_BARS[dtype], e
    # batch composition must not matter: sample 1 alone == sample 1 in the batch of 2, bitwise
    alone = d.decode(z[1:].cuda()).sample
    assert torch.equal(alone, got[1:])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_real_sd_decoder_256px_matches_restatement(dtype):
    """The real SD / SD-XL decoder architecture (49.5 M parameters, 512-wide single-head attention over 32 x 32 latent
    pixels, 256 x 256 x 128 last map) at 256 x 256 against the restatement; sample 1 alone vs in a batch of 2."""
    torch.set_num_threads(16)
    ref, d = pair(R.VAEConfig(), dtype)
    z = latents(2, 256, 256, seed=5)
    with torch.no_grad():
        want = ref.decode(z[:1])
    got = d.decode(z.cuda()).sample
    e = rel(got[:1], want)
    print(f"SD VAE decoder 256px {dtype}: sample rel err {e:.2e}")
    assert e < REAL_BARS[dtype], e
    alone = d.decode(z[1:].cuda()).sample
    eb = rel(alone, got[1:])
    print(f"SD VAE decoder 256px {dtype}: alone vs batch of 2 rel diff {eb:.2e} (bitwise: {torch.equal(alone, got[1:])})")
    # the decoder lends no split-K scratch to its GEMMs: a sample's arithmetic does not depend on its batch mates
    assert torch.equal(alone, got[1:])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_rgb8_is_torch_postprocess_of_sample_exactly(dtype):
    _, d = pair(R.tiny_vae_config(), dtype)
    z = latents(3, 64, 96, seed=9) * 3.0  # wide range: many pixels clamp at both ends
    s = d.decode(z.cuda()).sample
    u8 = d.decode_to_uint8(z.cuda())
    want = R.to_uint8(s)
    assert u8.dtype == torch.uint8 and u8.shape == (3, 64, 96, 3)
    assert (want == 0).any() and (want == 255).any()
    assert torch.equal(u8, want)


@pytest.mark.parametrize("cfg,size,tol", [(R.tiny_vae_config(), (64, 96), 2e-3), (R.VAEConfig(), (256, 256), 2e-3)],
                         ids=["tiny", "sd256"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fused_tail_matches_unfused(monkeypatch, cfg, size, tol, dtype):
    """Only the fp32 summation order of conv_out differs (both round the activation to the storage type)."""
    _, d = pair(cfg, dtype)
    z = latents(2, *size, seed=11)
    fused = d.decode(z.cuda()).sample
    fused8 = d.decode_to_uint8(z.cuda())
    monkeypatch.setenv("SMI_VAE_DEC_TAIL", "0")
    _, d0 = pair(cfg, dtype)
    plain = d0.decode(z.cuda()).sample
    plain8 = d0.decode_to_uint8(z.cuda())
    e = rel(fused, plain)
    print(f"fused vs unfused tail {dtype} {size}: rel diff {e:.2e}, max abs {float((fused - plain).abs().max()):.2e}")
    assert e < tol, e
    assert torch.equal(plain8, R.to_uint8(plain))
    assert int((fused8.int() - plain8.int()).abs().max()) <= 1


def test_chunked_decode_equals_per_chunk_decodes():
    _, d = pair(R.tiny_vae_config(), torch.float16)
    z = latents(5, 64, 64, seed=13).cuda()
    whole = d.decode(z, max_batch=2).sample
    parts = torch.cat([d.decode(z[i:i + 2], max_batch=2).sample for i in range(0, 5, 2)])
    assert torch.equal(whole, parts)
    u8 = d.decode_to_uint8(z, max_batch=2)
    assert torch.equal(u8, R.to_uint8(whole))


def test_engine_kinds_do_not_mix():
    from sliders_conceptmod_amd import vae as PV
    _, d = pair(R.tiny_vae_config(), torch.float16)
    z = latents(1, 64, 64).cuda()
    d.decode(z)
    dec = next(iter(d._engines.values()))
    enc_model = PV.init_synthetic_(PV.AutoencoderKL(PV.VAEConfig(block_out_channels=(64, 128, 128, 128),
                                                                  norm_num_groups=16))).to("cuda", torch.float16)
    x = torch.zeros(1, 3, 64, 64, device="cuda")
    enc_model.encode(x)
    enc = next(iter(enc_model._engines.values()))
    L = _native.lib()
    img = torch.empty(1, 3, 64, 64, device="cuda")
    mom = torch.empty(1, 8, 8, 8, device="cuda")
    assert L.smi_vae_encode(dec.handle, 1, _native.ptr(x), _native.ptr(mom)) != 0
    assert b"decoder" in L.smi_last_error()
    assert L.smi_vae_decode(enc.handle, 1, _native.ptr(z), _native.ptr(img), None) != 0
    assert b"not a VAE decoder" in L.smi_last_error()
    ctx = torch.zeros(2, 77, 64, device="cuda", dtype=torch.float16)
    eps = torch.empty(2, 4, 8, 8, device="cuda")
    s = torch.zeros(2, 4, 8, 8, device="cuda")
    assert L.smi_unet_forward(dec.handle, 2, _native.ptr(s), 1.0, _native.ptr(ctx), None, None, None, None, 0.0, 0,
                              _native.ptr(eps)) != 0
    mults = (C.c_float * 2)(1.0, -1.0)
    assert L.smi_unet_forward_multi(dec.handle, 2, 2, _native.ptr(s), 1.0, _native.ptr(ctx), None, None, None, None,
                                    mults, 0, _native.ptr(eps)) != 0
    assert L.smi_unet_backward(dec.handle, _native.ptr(eps), _native.ptr(eps), _native.ptr(eps)) != 0
    assert L.smi_replan(dec.handle, 1, 1, 8, 8, 77, None, 0) != 0
    # the engines still work after the refused calls
    assert torch.equal(d.decode(z).sample, d.decode(z).sample)
