"""`AutoencoderKL` decoder half -- what the reference's eval scripts do with a slider's final latents,
`vae.decode(latents / scaling_factor).sample` and the uint8 post-processing (eval-scripts/generate_images_sd1.py:195-200,
generate_images_xl.py:367-377) -- as a parameter container with diffusers' module names (`decoder.conv_in`,
`decoder.mid_block.{resnets,attentions}`, `decoder.up_blocks.{i}.resnets.{j}`, `decoder.up_blocks.{i}.upsamplers.0.conv`,
`decoder.conv_norm_out`, `decoder.conv_out`, `post_quant_conv`) whose arithmetic runs in the HIP engine
(csrc/engine.hip `forward_vae_dec`, csrc/vae_decode.hip).  A full diffusers VAE state dict loads by key; encoder
entries are ignored.  No PyTorch forward: without the HIP library, or on a CPU device, decode() raises SmiError.

SD-XL: its VAE is known to overflow fp16 in the decoder (diffusers upcasts it to fp32); the engine has no fp32 path, so
SD-XL decodes in bf16 by default (generate_images.py `--vae_dtype`).  Synthetic weights cannot show that overflow."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin
from .vae import VAEConfig, _Mid, _Resnet, half_state_dict

_GEMM_OPERAND_LIMIT = 0xFFFFFFF0  # the GEMM addresses an operand with a 32-bit byte offset (csrc/gemm.hip)


class _Up(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, 1, 1)


class _UpBlock(nn.Module):
    def __init__(self, cin, cout, layers, groups, up):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if i == 0 else cout, cout, groups) for i in range(layers)])
        self.upsamplers = nn.ModuleList([_Up(cout)]) if up else None


class _Decoder(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        boc = list(reversed(cfg.block_out_channels))
        self.conv_in = nn.Conv2d(cfg.latent_channels, boc[0], 3, 1, 1)
        self.mid_block = _Mid(boc[0], cfg.norm_num_groups)
        self.up_blocks = nn.ModuleList()
        ch = boc[0]
        for i, out in enumerate(boc):
            self.up_blocks.append(_UpBlock(ch, out, cfg.layers_per_block + 1, cfg.norm_num_groups, i != len(boc) - 1))
            ch = out
        self.conv_norm_out = nn.GroupNorm(cfg.norm_num_groups, ch, eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(ch, cfg.in_channels, 3, padding=1)


def image_operand_bytes(cfg: VAEConfig, h: int, w: int) -> int:
    """Bytes of the largest 16-bit conv / GEMM operand of one decoded h x w image (csrc/engine.hip, same walk)."""
    boc = cfg.block_out_channels
    f = 2 ** (len(boc) - 1)
    hw = (h // f) * (w // f)
    ch = boc[-1]
    m = max(hw * 64, hw * ch)
    for i, out in enumerate(reversed(boc)):
        m = max(m, hw * max(ch, out))
        ch = out
        if i != len(boc) - 1:
            hw *= 4
            m = max(m, hw * ch)
    return 2 * m


def max_decode_batch(cfg: VAEConfig, h: int, w: int) -> int:
    """Largest batch one engine decodes at h x w (SD config: 7 at 1024^2, 31 at 512^2)."""
    return (_GEMM_OPERAND_LIMIT - 1) // image_operand_bytes(cfg, h, w)


class DecoderOutput:
    def __init__(self, sample: torch.Tensor):
        self.sample = sample


class AutoencoderKLDecoder(EngineCacheMixin, nn.Module):
    _component, _handle = "VAE decoder", "vae"

    def __init__(self, cfg: VAEConfig):
        super().__init__()
        self.config = cfg
        self.decoder = _Decoder(cfg)
        if cfg.use_post_quant_conv:
            self.post_quant_conv = nn.Conv2d(cfg.latent_channels, cfg.latent_channels, 1)
        self._engines = {}

    @property
    def dtype(self):
        return self.decoder.conv_in.weight.dtype

    @property
    def device(self):
        return self.decoder.conv_in.weight.device

    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts a full diffusers AutoencoderKL state dict: the encoder / quant_conv entries are not used."""
        return super().load_state_dict(half_state_dict(state_dict, ("decoder.", "post_quant_conv.")), strict=strict)

    def _new_engine(self, state, n, h, w):
        return _native.VaeDecoderEngine(self.config, self.dtype, state, n, h, w, self.device)

    def _run(self, z: torch.Tensor, want_rgb8: bool, max_batch: Optional[int] = None):
        if z.ndim != 4 or z.shape[1] != self.config.latent_channels:
            raise ValueError(f"latents must be [n, {self.config.latent_channels}, h, w], got {tuple(z.shape)}")
        if self.device.type != "cuda":
            self._engine(1, 0, 0)  # raises: no CPU fallback
        f = 2 ** (len(self.config.block_out_channels) - 1)
        n, h, w = z.shape[0], z.shape[2] * f, z.shape[3] * f
        chunk = min(n, max_decode_batch(self.config, h, w))
        if max_batch is not None:
            chunk = min(chunk, max_batch)
        z = z.to(self.device, torch.float32).contiguous()
        e = self._engine(max(chunk, 1), h, w)
        samples, rgbs = [], []
        for i in range(0, n, chunk):
            s, r = e.decode(z[i:i + chunk], want_rgb8)
            samples.append(s)
            rgbs.append(r)
        sample = samples[0] if len(samples) == 1 else torch.cat(samples)
        rgb = None
        if want_rgb8:
            rgb = rgbs[0] if len(rgbs) == 1 else torch.cat(rgbs)
        return sample, rgb

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True, max_batch: Optional[int] = None):
        """z: [n, latent, h/f, w/f], ALREADY divided by scaling_factor -> `.sample` f32 [n, 3, h, w] (unclamped).
        Batches above the engine's limit (4 GiB operand rule) or above `max_batch` are decoded in chunks."""
        sample, _ = self._run(z, False, max_batch)
        return DecoderOutput(sample) if return_dict else (sample,)

    @torch.no_grad()
    def decode_to_uint8(self, z: torch.Tensor, max_batch: Optional[int] = None) -> torch.Tensor:
        """The eval scripts' images: uint8 [n, h, w, 3] = round(clamp(sample / 2 + 0.5, 0, 1) * 255), on the device."""
        return self._run(z, True, max_batch)[1]


@torch.no_grad()
def init_synthetic_(vae: nn.Module, seed: int = 0):
    """Seeded weights in the same style as vae.init_synthetic_ (fan-in scaled, snapped to bf16-representable values)."""
    from .vae import init_synthetic_ as _init
    return _init(vae, seed)
