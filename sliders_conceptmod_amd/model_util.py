"""Noise schedulers with the interface the reference's helpers call (conceptmod/textsliders/model_util.py:388-436
builds them; train_util.py:103,287,324,705 and train_lora.py:157-213 use them), plus the model factory.

The scheduler classes of the reference live in diffusers (absent here); these are native restatements of the four it
can construct -- DDIM (eta = 0), Euler-ancestral, DDPM and LMS (order 4) -- with the same constants
(beta 0.00085 -> 0.012 scaled-linear, 1000 train steps, clip_sample False) and both prediction types
(`epsilon`, and `v_prediction` for `pretrained_model.v_pred`, model_util.py:134).  Every update is affine in
(sample, model output, noise): the coefficients are computed on the host and the latent update runs on the GPU
through `smi_sched_step` when the latents are on a cuda device."""
from __future__ import annotations

import os
from typing import Literal, Optional

import numpy as np
import torch

from . import _native

AVAILABLE_SCHEDULERS = Literal["ddim", "ddpm", "lms", "euler_a"]


class _StepOutput:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


def _affine(x: torch.Tensor, eps: torch.Tensor, noise, cx: float, ce: float, cn: float) -> torch.Tensor:
    if x.is_cuda and x.dtype == torch.float32 and eps.dtype == torch.float32:
        out = x.contiguous().clone()
        e = eps.contiguous()
        nz = None if noise is None else noise.to(x.device, torch.float32).contiguous()
        _native.check(_native.lib().smi_sched_step(_native.ptr(out), _native.ptr(e), _native.ptr(nz), cx, ce, cn,
                                                   out.numel(), _native.stream_ptr()), "smi_sched_step")
        return out
    out = cx * x + ce * eps
    return out if noise is None else out + cn * noise.to(x.device, x.dtype)


def _alphas_cumprod(n=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _check_prediction_type(p):
    if p not in ("epsilon", "v_prediction"):
        raise ValueError(f"prediction_type must be epsilon or v_prediction, got {p}")
    return p


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, prediction_type="epsilon"):
        self.prediction_type = _check_prediction_type(prediction_type)
        self.num_train_timesteps = num_train_timesteps
        self.alphas_cumprod = _alphas_cumprod(num_train_timesteps)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.init_noise_sigma = torch.tensor(1.0)
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        self.timesteps = torch.from_numpy((np.arange(0, num_inference_steps) * ratio).round()[::-1].copy()
                                          .astype(np.int64))  # kept on the host: indexing it never syncs the GPU

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, eta: float = 0.0, generator=None):
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        if self.prediction_type == "epsilon":
            # prev = sqrt(a_prev) * (x - sqrt(1-a_t) eps) / sqrt(a_t) + sqrt(1 - a_prev) eps
            cx = (a_prev / a_t) ** 0.5
            ce = (1 - a_prev) ** 0.5 - (a_prev * (1 - a_t) / a_t) ** 0.5
        else:
            # x0 = sqrt(a_t) x - sqrt(1-a_t) v ; eps = sqrt(a_t) v + sqrt(1-a_t) x ; prev = sqrt(a_prev) x0 + sqrt(1-a_prev) eps
            cx = (a_prev * a_t) ** 0.5 + ((1 - a_prev) * (1 - a_t)) ** 0.5
            ce = ((1 - a_prev) * a_t) ** 0.5 - (a_prev * (1 - a_t)) ** 0.5
        return _StepOutput(_affine(sample, model_output, None, cx, ce, 0.0))

    def add_noise(self, original, noise, timesteps):
        t = torch.as_tensor(timesteps).reshape(-1).long().cpu()
        sa = (self.alphas_cumprod[t] ** 0.5).to(original.device, original.dtype)
        sb = ((1 - self.alphas_cumprod[t]) ** 0.5).to(original.device, original.dtype)
        while sa.ndim < original.ndim:
            sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
        return sa * original + sb * noise


class DDPMScheduler(DDIMScheduler):
    """Ancestral sampling with the "fixed_small" posterior variance (diffusers' default), leading timestep spacing."""

    def step(self, model_output, timestep, sample, generator=None):
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else 1.0
        b_t, b_prev = 1 - a_t, 1 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1 - cur_a
        c0 = a_prev ** 0.5 * cur_b / b_t  # weight of the predicted x0
        c1 = cur_a ** 0.5 * b_prev / b_t  # weight of the current sample
        if self.prediction_type == "epsilon":  # x0 = (x - sqrt(b_t) eps) / sqrt(a_t)
            cx, ce = c1 + c0 / a_t ** 0.5, -c0 * (b_t / a_t) ** 0.5
        else:                                  # x0 = sqrt(a_t) x - sqrt(b_t) v
            cx, ce = c1 + c0 * a_t ** 0.5, -c0 * b_t ** 0.5
        noise, cn = None, 0.0
        if t > 0:
            rank, world = getattr(self, "dp_shard", (0, 1))
            from .parallel import shard_noise
            noise = shard_noise(lambda shp: torch.randn(shp, dtype=torch.float32, generator=generator),
                                tuple(model_output.shape), rank, world)
            cn = max(b_prev / b_t * cur_b, 1e-20) ** 0.5
        return _StepOutput(_affine(sample, model_output, noise, cx, ce, cn))


class EulerAncestralDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, prediction_type="epsilon"):
        self.prediction_type = _check_prediction_type(prediction_type)
        self.num_train_timesteps = num_train_timesteps
        ac = _alphas_cumprod(num_train_timesteps)
        self._train_sigmas = (((1 - ac) / ac) ** 0.5).numpy().astype(np.float64)
        self.sigmas = torch.from_numpy(np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(
            np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.num_inference_steps = None

    @property
    def init_noise_sigma(self):
        return self.sigmas.max()

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts = np.linspace(0, self.num_train_timesteps - 1, num_inference_steps, dtype=np.float32)[::-1].copy()
        sig = np.interp(ts, np.arange(0, len(self._train_sigmas)), self._train_sigmas)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)

    def _index(self, timestep) -> int:
        return int((self.timesteps == float(timestep)).nonzero()[0].item())

    def scale_model_input(self, sample, timestep):
        sigma = float(self.sigmas[self._index(timestep)])
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def step(self, model_output, timestep, sample, generator=None):
        i = self._index(timestep)
        sigma, sigma_to = float(self.sigmas[i]), float(self.sigmas[i + 1])
        sigma_up = (sigma_to ** 2 * (sigma ** 2 - sigma_to ** 2) / sigma ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        # host torch RNG (global generator) keeps the draw order of the reference run: SURVEY.md section 7 "RNG parity"
        # under data parallelism (`dp_shard = (rank, world)`, set by the trainers) the GLOBAL batch's noise is drawn and
        # this rank's rows are taken, so W ranks consume the control RNG like one rank at the global batch
        rank, world = getattr(self, "dp_shard", (0, 1))
        from .parallel import shard_noise
        # `noise_on_device` (or a device generator) draws on the sample's device instead, as diffusers' randn_tensor does
        # when it is handed no CPU generator: no host draw and no 1 MB host-to-device copy per denoising step
        on_dev = model_output.is_cuda and (getattr(self, "noise_on_device", False)
                                           or (generator is not None and generator.device.type != "cpu"))
        dev = model_output.device if on_dev else None
        noise = shard_noise(lambda shp: torch.randn(shp, dtype=torch.float32, generator=generator, device=dev),
                            tuple(model_output.shape), rank, world)
        dt = sigma_down - sigma
        if self.prediction_type == "epsilon":
            # prev = x + eps * dt + noise * sigma_up       (derivative = eps for epsilon prediction)
            cx, ce = 1.0, dt
        else:
            # x0 = -sigma v / sqrt(sigma^2+1) + x / (sigma^2+1); derivative = (x - x0) / sigma
            cx, ce = 1.0 + dt * sigma / (sigma ** 2 + 1), dt / (sigma ** 2 + 1) ** 0.5
        return _StepOutput(_affine(sample, model_output, noise, cx, ce, sigma_up))

    def add_noise(self, original, noise, timesteps):
        i = self._index(torch.as_tensor(timesteps).reshape(-1)[0])
        return original + noise * float(self.sigmas[i])


class LMSDiscreteScheduler(EulerAncestralDiscreteScheduler):
    """Linear multistep (order 4, Katherine Crowson's k-diffusion `sample_lms`) on the same sigma ladder as Euler-a:
    prev = x + sum_j c_j d_{i-j}, d = (x - x0) / sigma, c_j = integral over [sigma_i, sigma_{i+1}] of the j-th Lagrange
    basis polynomial through the last `order` sigmas.  Stateful: the derivative history restarts at set_timesteps."""
    order = 4

    def set_timesteps(self, num_inference_steps: int, device=None):
        super().set_timesteps(num_inference_steps, device)
        self.derivatives = []

    def get_lms_coefficient(self, order, t, current_order):
        from scipy import integrate
        sig = self.sigmas.double().numpy()

        def basis(tau):
            prod = 1.0
            for k in range(order):
                if current_order == k:
                    continue
                prod *= (tau - sig[t - k]) / (sig[t - current_order] - sig[t - k])
            return prod

        return integrate.quad(basis, sig[t], sig[t + 1], epsrel=1e-4)[0]

    def step(self, model_output, timestep, sample, order: int = 4, generator=None):
        i = self._index(timestep)
        sigma = float(self.sigmas[i])
        # derivative d = (x - x0) / sigma as an affine map of (x, model output)
        if self.prediction_type == "epsilon":
            dx, de = 0.0, 1.0
        else:
            dx, de = sigma / (sigma ** 2 + 1), 1.0 / (sigma ** 2 + 1) ** 0.5
        d = dx * sample.float() + de * model_output.float()
        hist = getattr(self, "derivatives", [])
        hist.append(d)
        if len(hist) > order:
            hist.pop(0)
        self.derivatives = hist
        order = min(i + 1, order, len(hist))
        coeffs = [self.get_lms_coefficient(order, i, j) for j in range(order)]
        prev = sample.float()
        for c, dj in zip(coeffs, reversed(hist)):
            prev = prev + float(c) * dj
        return _StepOutput(prev)


def create_noise_scheduler(scheduler_name: AVAILABLE_SCHEDULERS = "ddpm", prediction_type="epsilon"):
    """model_util.py:388-436: the four schedulers with the reference's constants; unknown names raise ValueError."""
    name = scheduler_name.lower().replace(" ", "_")
    if name == "ddim":
        return DDIMScheduler(prediction_type=prediction_type)
    if name == "ddpm":
        return DDPMScheduler(prediction_type=prediction_type)
    if name == "lms":
        return LMSDiscreteScheduler(prediction_type=prediction_type)
    if name == "euler_a":
        s = EulerAncestralDiscreteScheduler(prediction_type=prediction_type)
        s.noise_on_device = os.environ.get("SMI_DEVICE_NOISE", "0") == "1"
        return s
    raise ValueError(f"Unknown scheduler name: {name}")


class FlowMatchEulerDiscreteScheduler:
    """The flow-matching Euler scheduler SD3 samples with (the published diffusers class, restated from its documented
    behaviour; `diffusers` is not a dependency here, so the restatement is unpinned -- DESIGN.md section 17).
    Base sigmas linspace(1, N, N)[::-1] / N, shifted by s' = shift s / (1 + (shift - 1) s).  `set_timesteps(n)`:
    t = linspace(N s'_max, N s'_min, n), sigma = t / N SHIFTED ONCE MORE, timesteps = N sigma, a final sigma 0 appended.
    `step`: x + (sigma_{i+1} - sigma_i) v in fp32.  init_noise_sigma 1, scale_model_input the identity.  The model is fed
    the timestep N sigma."""

    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 3.0, use_dynamic_shifting: bool = False,
                 base_shift: float = 0.5, max_shift: float = 1.15, base_image_seq_len: int = 256,
                 max_image_seq_len: int = 4096):
        """use_dynamic_shifting (FLUX.1-dev's scheduler config): the shift is chosen per call from the image sequence length
        -- `set_timesteps(..., mu=calculate_shift(seq_len))` -- and sigma' = e^mu / (e^mu + 1 / sigma - 1) replaces the static
        shift; the training sigmas then stay un-shifted (sigma_max 1, sigma_min 1 / N), as in the published class."""
        self.num_train_timesteps, self.shift = num_train_timesteps, float(shift)
        self.use_dynamic_shifting = bool(use_dynamic_shifting)
        self.base_shift, self.max_shift = float(base_shift), float(max_shift)
        self.base_image_seq_len, self.max_image_seq_len = int(base_image_seq_len), int(max_image_seq_len)
        base = torch.linspace(1, num_train_timesteps, num_train_timesteps, dtype=torch.float64).flip(0) / num_train_timesteps
        self._train_sigmas = base if self.use_dynamic_shifting else self.shift_sigma(base)
        self.sigma_max, self.sigma_min = float(self._train_sigmas[0]), float(self._train_sigmas[-1])
        self.set_timesteps(num_train_timesteps, mu=0.0 if self.use_dynamic_shifting else None)

    def shift_sigma(self, s):
        return self.shift * s / (1 + (self.shift - 1) * s)

    def calculate_shift(self, image_seq_len: int) -> float:
        """mu of the Flux pipeline: linear in the image sequence length, base_shift at base_image_seq_len and max_shift at
        max_image_seq_len."""
        m = (self.max_shift - self.base_shift) / (self.max_image_seq_len - self.base_image_seq_len)
        return image_seq_len * m + (self.base_shift - m * self.base_image_seq_len)

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, sigmas=None, mu: Optional[float] = None):
        """sigmas: the un-shifted schedule to use instead of the linspace over the training range (the Flux pipeline passes
        linspace(1, 1 / n, n)); mu: required with use_dynamic_shifting, refused without."""
        import math
        n = self.num_train_timesteps
        if self.use_dynamic_shifting != (mu is not None):
            raise ValueError("set_timesteps: mu goes with use_dynamic_shifting (pass mu=scheduler.calculate_shift(seq_len))"
                             if self.use_dynamic_shifting else "set_timesteps: mu given but the scheduler shifts statically")
        if sigmas is not None:
            base = torch.as_tensor(sigmas, dtype=torch.float64)
            num_inference_steps = base.numel()
        else:
            base = torch.linspace(self.sigma_max * n, self.sigma_min * n, num_inference_steps, dtype=torch.float64) / n
        sig = math.exp(mu) / (math.exp(mu) + (1 / base - 1)) if mu is not None else self.shift_sigma(base)
        self.num_inference_steps = num_inference_steps
        self.timesteps = (sig * n).to(torch.float32)
        self.sigmas = torch.cat([sig, torch.zeros(1, dtype=torch.float64)]).to(torch.float32)
        self._step_index = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def index_for_timestep(self, timestep) -> int:
        t = float(timestep)
        hits = (self.timesteps == torch.tensor(t, dtype=torch.float32)).nonzero()
        if hits.numel() == 0:
            raise ValueError(f"timestep {t} is not one of this schedule's (call set_timesteps and pass scheduler.timesteps[i])")
        return int(hits[0])

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        i = self.index_for_timestep(timestep)
        dt = float(self.sigmas[i + 1]) - float(self.sigmas[i])
        prev = (sample.float() + dt * model_output.float()).to(sample.dtype)
        return _StepOutput(prev) if return_dict else (prev,)


# ----------------------------------------------------------------------------------------------------------------
# model factory (reference: conceptmod/textsliders/model_util.py:27-137, 170-385 -- hub / checkpoint loaders)
# ----------------------------------------------------------------------------------------------------------------
class SyntheticTextEncoder:
    """Offline stand-in for tokenizer + CLIP text encoder(s): a prompt maps to seeded normal embeddings
    ([1, 77, D] and, for SD-XL, a pooled [1, P]) keyed by a hash of the text, so equal prompts share embeddings
    exactly as the reference's PromptEmbedsCache assumes (train_lora.py:106-146).  The real front end (CLIP-L /
    OpenCLIP-bigG) is a 'next' row of the scope table."""

    def __init__(self, dim: int, pooled_dim: int = 0, seq_len: int = 77):
        self.dim, self.pooled_dim, self.seq_len = dim, pooled_dim, seq_len

    def encode(self, prompt: str):
        import hashlib
        seed = int.from_bytes(hashlib.sha256(prompt.encode()).digest()[:8], "little") % (2 ** 31)
        g = torch.Generator().manual_seed(seed)
        te = torch.randn(1, self.seq_len, self.dim, generator=g)
        if self.pooled_dim:
            return te, torch.randn(1, self.pooled_dim, generator=g)
        return te


def _unet_from_dir(path: str, dtype):
    """diffusers directory layout: <path>/unet/config.json + diffusion_pytorch_model.safetensors (safe loader only)."""
    import json
    import os
    from safetensors.torch import load_file
    from . import unet as PU
    cfgj = json.load(open(os.path.join(path, "unet", "config.json")))
    ahd = cfgj.get("attention_head_dim", 8)
    n = len(cfgj["block_out_channels"])
    tl = cfgj.get("transformer_layers_per_block", 1)
    cfg = PU.UNetConfig(
        in_channels=cfgj.get("in_channels", 4), out_channels=cfgj.get("out_channels", 4),
        block_out_channels=tuple(cfgj["block_out_channels"]), down_block_types=tuple(cfgj["down_block_types"]),
        up_block_types=tuple(cfgj["up_block_types"]), layers_per_block=cfgj.get("layers_per_block", 2),
        transformer_layers_per_block=tuple(tl) if isinstance(tl, (list, tuple)) else (tl,) * n,
        num_attention_heads=tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * n,
        cross_attention_dim=cfgj["cross_attention_dim"], norm_num_groups=cfgj.get("norm_num_groups", 32),
        use_linear_projection=cfgj.get("use_linear_projection", False),
        addition_embed_type=cfgj.get("addition_embed_type"),
        addition_time_embed_dim=cfgj.get("addition_time_embed_dim") or 256,
        projection_class_embeddings_input_dim=cfgj.get("projection_class_embeddings_input_dim") or 2816)
    unet = PU.UNet2DConditionModel(cfg)
    sd = load_file(os.path.join(path, "unet", "diffusion_pytorch_model.safetensors"))
    unet.load_state_dict(sd)
    return unet


def _clip_from_dir(path: str, sub: str):
    """<path>/<sub>/config.json + model.safetensors (transformers layout, safe loader only) -> native CLIP text encoder;
    `architectures` tells CLIPTextModel from CLIPTextModelWithProjection."""
    import json
    from safetensors.torch import load_file
    from . import clip as PC
    cj = json.load(open(os.path.join(path, sub, "config.json")))
    proj = "CLIPTextModelWithProjection" in (cj.get("architectures") or [])
    cfg = PC.CLIPTextConfig(vocab_size=cj["vocab_size"], hidden_size=cj["hidden_size"],
                            intermediate_size=cj["intermediate_size"], num_hidden_layers=cj["num_hidden_layers"],
                            num_attention_heads=cj["num_attention_heads"],
                            max_position_embeddings=cj.get("max_position_embeddings", 77),
                            hidden_act=cj.get("hidden_act", "quick_gelu"),
                            projection_dim=cj.get("projection_dim") if proj else None,
                            eos_token_id=cj.get("eos_token_id", 2))
    enc = (PC.CLIPTextModelWithProjection if proj else PC.CLIPTextModel)(cfg)
    enc.load_state_dict(load_file(os.path.join(path, sub, "model.safetensors")))
    return enc


def load_vae(pretrained_model_name_or_path: str, xl: bool = False):
    """The AutoencoderKL the image-slider scripts get next to the UNet (I/model_util.py:75,179): `synthetic://...`
    builds the SD / SD-XL VAE encoder architecture with seeded weights; a local diffusers directory is read from its
    `vae/` sub-folder with the safetensors loader."""
    import json
    import os
    from . import vae as PV
    name = pretrained_model_name_or_path
    if name.startswith("synthetic://"):
        if "tiny" in name:
            cfg = PV.VAEConfig(block_out_channels=(64, 128, 128, 128), norm_num_groups=16,
                               scaling_factor=0.13025 if xl else 0.18215)
        else:
            cfg = PV.sdxl_vae_config() if xl else PV.sd_vae_config()
        return PV.init_synthetic_(PV.AutoencoderKL(cfg), seed=7)
    if os.path.isdir(name):
        from safetensors.torch import load_file
        cj = json.load(open(os.path.join(name, "vae", "config.json")))
        cfg = PV.VAEConfig(in_channels=cj.get("in_channels", 3), latent_channels=cj.get("latent_channels", 4),
                           block_out_channels=tuple(cj["block_out_channels"]),
                           layers_per_block=cj.get("layers_per_block", 2),
                           norm_num_groups=cj.get("norm_num_groups", 32),
                           scaling_factor=cj.get("scaling_factor", 0.18215))
        vae = PV.AutoencoderKL(cfg)
        vae.load_state_dict(load_file(os.path.join(name, "vae", "diffusion_pytorch_model.safetensors")))
        return vae
    raise ValueError(f"cannot load a VAE from '{name}': pass a local diffusers directory or synthetic://sd1x | sdxl")


def load_vae_decoder(pretrained_model_name_or_path: str, xl: bool = False):
    """The AutoencoderKL decoder the eval scripts decode with (E/generate_images_sd1.py:195): `synthetic://(tiny_)sd1x |
    sdxl` builds it with seeded weights (the tiny config `load_vae` uses); a local diffusers directory is read from its
    `vae/` sub-folder with the safetensors loader."""
    import json
    import os
    from . import vae as PV
    from . import vae_decoder as PD
    name = pretrained_model_name_or_path
    if name.startswith("synthetic://"):
        xl = xl or "sdxl" in name
        if "tiny" in name:
            cfg = PV.VAEConfig(block_out_channels=(64, 128, 128, 128), norm_num_groups=16,
                               scaling_factor=0.13025 if xl else 0.18215)
        else:
            cfg = PV.sdxl_vae_config() if xl else PV.sd_vae_config()
        return PD.init_synthetic_(PD.AutoencoderKLDecoder(cfg), seed=11)
    if os.path.isdir(name):
        from safetensors.torch import load_file
        cj = json.load(open(os.path.join(name, "vae", "config.json")))
        cfg = PV.VAEConfig(in_channels=cj.get("out_channels", cj.get("in_channels", 3)),
                           latent_channels=cj.get("latent_channels", 4),
                           block_out_channels=tuple(cj["block_out_channels"]),
                           layers_per_block=cj.get("layers_per_block", 2),
                           norm_num_groups=cj.get("norm_num_groups", 32),
                           scaling_factor=cj.get("scaling_factor", 0.18215))
        vae = PD.AutoencoderKLDecoder(cfg)
        vae.load_state_dict(load_file(os.path.join(name, "vae", "diffusion_pytorch_model.safetensors")))
        return vae
    raise ValueError(f"cannot load a VAE decoder from '{name}': pass a local diffusers directory or "
                     f"synthetic://sd1x | sdxl | tiny_sd1x | tiny_sdxl")


def load_models(pretrained_model_name_or_path: str, scheduler_name: str = "ddim", v2: bool = False,
                v_pred: bool = False, weight_dtype=torch.float32, xl: bool = False):
    """Returns (tokenizer(s), text_encoder(s), unet, noise_scheduler) like the reference (model_util.py:112-137,
    :359-385).  `synthetic://sd1x|sdxl|tiny_sd1x|tiny_sdxl` builds the architecture with seeded random weights (no
    network here).  A local diffusers directory is loaded with safetensors; its text encoders through `transformers`."""
    from . import unet as PU
    if v2 and not os.path.isdir(pretrained_model_name_or_path):
        raise ValueError("SD-2.x needs a local diffusers directory (its UNet config is read from it)")
    # model_util.py:134: prediction_type = "v_prediction" if v_pred else "epsilon"
    scheduler = create_noise_scheduler(scheduler_name, prediction_type="v_prediction" if v_pred else "epsilon")
    name = pretrained_model_name_or_path
    if name.startswith("synthetic://"):
        kind = name[len("synthetic://"):]
        tiny = {"tiny_sd1x": PU.UNetConfig(block_out_channels=(64, 128, 256, 256), num_attention_heads=(4, 4, 4, 4),
                                           cross_attention_dim=64, norm_num_groups=16),
                "tiny_sdxl": PU.UNetConfig(
                    block_out_channels=(64, 128, 256),
                    down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                    up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                    transformer_layers_per_block=(1, 2, 3), num_attention_heads=(2, 4, 8), cross_attention_dim=64,
                    norm_num_groups=16, use_linear_projection=True, addition_embed_type="text_time",
                    addition_time_embed_dim=32, projection_class_embeddings_input_dim=256)}
        cfg = {"sd1x": PU.sd1x_config, "sdxl": PU.sdxl_config}.get(kind, lambda: tiny[kind])()
        unet = PU.init_synthetic_(PU.UNet2DConditionModel(cfg), seed=0)
        pooled = 0
        if cfg.addition_embed_type == "text_time":
            pooled = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
        enc = SyntheticTextEncoder(cfg.cross_attention_dim, pooled)
        return None, enc, unet, scheduler
    if os.path.isdir(name):
        unet = _unet_from_dir(name, weight_dtype)
        # tokenisation is host text processing (transformers.CLIPTokenizer reads the directory's vocab files); the text
        # encoders are the native ones (clip.py: transformers parameter names, arithmetic on the HIP engine)
        from transformers import CLIPTokenizer
        toks = [CLIPTokenizer.from_pretrained(name, subfolder="tokenizer")]
        encs = [_clip_from_dir(name, "text_encoder")]
        if os.path.isdir(os.path.join(name, "text_encoder_2")):
            toks.append(CLIPTokenizer.from_pretrained(name, subfolder="tokenizer_2"))
            encs.append(_clip_from_dir(name, "text_encoder_2"))
        return toks, encs, unet, scheduler
    raise ValueError(f"cannot load '{name}': no network in this environment; pass a local diffusers directory or "
                     f"synthetic://sd1x | synthetic://sdxl")


# ----------------------------------------------------------------------------------------------------------------
# CLIP image-text model for scoring a sweep (reference: eval-scripts/clip_score.py loads a hub name)
# ----------------------------------------------------------------------------------------------------------------
class SyntheticClipTokenizer:
    """Deterministic stand-in for `CLIPTokenizer` where no vocabulary files exist (the `synthetic://` CLIP models): BOS,
    one id per lower-cased word (a hash of the word into [1, bos)), EOS; no padding -- `CLIPModel` pads.  In the spirit
    of `SyntheticTextEncoder`: equal prompts give equal ids, and that is all a seeded model can use."""

    def __init__(self, vocab_size: int, eos_token_id: int, model_max_length: int = 77):
        self.vocab_size, self.eos_token_id, self.bos_token_id = vocab_size, eos_token_id, eos_token_id - 1
        self.model_max_length = model_max_length

    def encode(self, prompt: str):
        import hashlib
        words = prompt.lower().split()[: self.model_max_length - 2]
        ids = [1 + int.from_bytes(hashlib.sha256(w.encode()).digest()[:8], "little") % (self.bos_token_id - 1)
               for w in words]
        return [self.bos_token_id] + ids + [self.eos_token_id]

    def __call__(self, prompts, padding=None, max_length=None, **_):
        rows = [self.encode(p) for p in ([prompts] if isinstance(prompts, str) else prompts)]
        width = max(len(r) for r in rows)
        if padding == "max_length":  # as CLIPTokenizer: every row to max_length (EOS fills: the stand-in's pad token)
            width = max_length or self.model_max_length
            rows = [r[:width - 1] + [self.eos_token_id] if len(r) > width else r for r in rows]
        ids = torch.tensor([r + [self.eos_token_id] * (width - len(r)) for r in rows], dtype=torch.int64)

        class _Encoding:
            input_ids = ids
        return _Encoding()


def init_synthetic_clip_(model, seed: int):
    """Seeded weights for a `clip.CLIPModel`: embeddings 0.02 N, matrices 0.8 N / sqrt(fan_in) (the patch filter by its
    3 P^2 fan-in), norm scales 1 + 0.1 N, biases 0.02 N; logit_scale = ln 100 (what the trained models saturate at)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "logit_scale":
                p.fill_(float(np.log(100.0)))
            elif p.ndim >= 2 and "embedding" in name and p.ndim == 2:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            elif p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (0.8 / (p[0].numel()) ** 0.5))
            elif name.endswith("class_embedding"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return model


def load_clip(name: str):
    """(model, tokenizer, image_size) for `clip_score`: a local transformers directory (config.json, model.safetensors,
    preprocessor_config.json for mean / std / size; tokenizer through `CLIPTokenizer.from_pretrained(dir)`), or
    `synthetic://tiny_clip | vit_b32 | vit_l14` with seeded weights and the stand-in tokenizer."""
    import json
    from . import clip as PC
    if name.startswith("synthetic://"):
        kind = name[len("synthetic://"):]
        if kind == "tiny_clip":
            tc = PC.CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=256, num_hidden_layers=3,
                                   num_attention_heads=4, projection_dim=32, eos_token_id=999)
            vc = PC.CLIPVisionConfig(hidden_size=64, intermediate_size=256, num_hidden_layers=3, num_attention_heads=4,
                                     image_size=32, patch_size=8, projection_dim=32)
        elif kind == "vit_b32":
            tc, vc = PC.vit_b32_text_config(), PC.vit_b32_vision_config()
        elif kind == "vit_l14":
            tc, vc = PC.vit_l14_text_config(), PC.vit_l14_vision_config()
        else:
            raise ValueError(f"unknown synthetic CLIP '{name}': synthetic://tiny_clip | vit_b32 | vit_l14")
        model = init_synthetic_clip_(PC.CLIPModel(tc, vc), seed=13)
        return model, SyntheticClipTokenizer(tc.vocab_size, tc.eos_token_id, tc.max_position_embeddings), vc.image_size
    if os.path.isdir(name):
        from safetensors.torch import load_file
        cj = json.load(open(os.path.join(name, "config.json")))
        pj = json.load(open(os.path.join(name, "preprocessor_config.json")))
        t, v = cj["text_config"], cj["vision_config"]
        proj = cj.get("projection_dim", 512)
        tc = PC.CLIPTextConfig(vocab_size=t.get("vocab_size", 49408), hidden_size=t.get("hidden_size", 512),
                               intermediate_size=t.get("intermediate_size", 2048),
                               num_hidden_layers=t.get("num_hidden_layers", 12),
                               num_attention_heads=t.get("num_attention_heads", 8),
                               max_position_embeddings=t.get("max_position_embeddings", 77),
                               hidden_act=t.get("hidden_act", "quick_gelu"), projection_dim=proj,
                               eos_token_id=t.get("eos_token_id", 2))
        size = pj.get("crop_size", pj.get("size", 224))
        if isinstance(size, dict):
            size = size.get("height", size.get("shortest_edge"))
        vc = PC.CLIPVisionConfig(hidden_size=v.get("hidden_size", 768), intermediate_size=v.get("intermediate_size", 3072),
                                 num_hidden_layers=v.get("num_hidden_layers", 12),
                                 num_attention_heads=v.get("num_attention_heads", 12),
                                 image_size=v.get("image_size", 224), patch_size=v.get("patch_size", 32),
                                 hidden_act=v.get("hidden_act", "quick_gelu"), projection_dim=proj,
                                 image_mean=tuple(pj.get("image_mean", PC.OPENAI_CLIP_MEAN)),
                                 image_std=tuple(pj.get("image_std", PC.OPENAI_CLIP_STD)))
        if int(size) != vc.image_size:
            raise ValueError(f"{name}: the processor crops to {size} but the vision tower takes {vc.image_size}")
        model = PC.CLIPModel(tc, vc, cj.get("logit_scale_init_value", 2.6592))
        model.load_state_dict(load_file(os.path.join(name, "model.safetensors")))
        from transformers import CLIPTokenizer
        return model, CLIPTokenizer.from_pretrained(name), vc.image_size
    raise ValueError(f"cannot load '{name}': no network in this environment; pass a local transformers directory or "
                     f"synthetic://tiny_clip | synthetic://vit_b32 | synthetic://vit_l14")


def _sd3_from_dir(path: str):
    """<path>/transformer/config.json + diffusion_pytorch_model.safetensors (safe loader only) -> SD3Transformer2DModel."""
    import json
    from safetensors.torch import load_file
    from . import mmdit as PM
    cj = json.load(open(os.path.join(path, "transformer", "config.json")))
    cfg = PM.SD3Config(patch_size=cj.get("patch_size", 2), in_channels=cj.get("in_channels", 16),
                       out_channels=cj.get("out_channels") or cj.get("in_channels", 16), num_layers=cj.get("num_layers", 24),
                       num_attention_heads=cj.get("num_attention_heads", 24),
                       attention_head_dim=cj.get("attention_head_dim", 64),
                       joint_attention_dim=cj.get("joint_attention_dim", 4096),
                       pooled_projection_dim=cj.get("pooled_projection_dim", 2048),
                       pos_embed_max_size=cj.get("pos_embed_max_size", 192), sample_size=cj.get("sample_size", 128),
                       dual_attention_layers=tuple(cj.get("dual_attention_layers") or ()), qk_norm=cj.get("qk_norm"))
    if cfg.dual_attention_layers or cfg.qk_norm:
        raise ValueError(f"{path}: dual_attention_layers / qk_norm (SD3.5) are not built")
    model = PM.SD3Transformer2DModel(cfg)
    model.load_state_dict(load_file(os.path.join(path, "transformer", "diffusion_pytorch_model.safetensors")))
    return model


class SyntheticClipTower:
    """Offline stand-in for one CLIPTextModelWithProjection of `synthetic://tiny_sd3`, in the spirit of SyntheticTextEncoder:
    token ids map to seeded normal features keyed by a hash of the ids (equal prompts share embeddings).  The native CLIP
    engine needs a hidden size that is a multiple of 64, and two such towers would not fit tiny_sd3's 64-wide context."""

    class _Config:
        def __init__(self, hidden_size, projection_dim):
            self.hidden_size, self.projection_dim = hidden_size, projection_dim

    def __init__(self, hidden_size: int, projection_dim: int, salt: int):
        self.config, self.salt = self._Config(hidden_size, projection_dim), salt
        self.device, self.dtype = torch.device("cpu"), torch.float32

    def to(self, device=None, dtype=None):
        self.device = torch.device(device) if device is not None else self.device
        self.dtype = dtype or self.dtype
        return self

    def __call__(self, input_ids, output_hidden_states: bool = False, **_):
        import hashlib
        hs, pooled = [], []
        for row in input_ids.cpu().tolist():
            seed = int.from_bytes(hashlib.sha256(repr((self.salt, row)).encode()).digest()[:8], "little") % (2 ** 31)
            g = torch.Generator().manual_seed(seed)
            hs.append(torch.randn(len(row), self.config.hidden_size, generator=g))
            pooled.append(torch.randn(self.config.projection_dim, generator=g))
        pen = torch.stack(hs).to(self.device, self.dtype)
        pool = torch.stack(pooled).to(self.device, self.dtype)

        class _Out:
            hidden_states = (None, pen, None)
            pooler_output = pool  # (a Flux model reads the un-projected pooled row; the stand-in has one pooled vector)

            def __getitem__(_self, i):
                return (pool,)[i]
        return _Out()


def synthetic_sd3_towers(tiny: bool):
    """(tokenizers, text encoders) of SD3's two CLIP towers: CLIP-L and OpenCLIP-bigG (both WithProjection) with seeded
    weights on the native engine, or for tiny_sd3 two hashed stand-ins (hidden 32, projection 32 each)."""
    from . import clip as PC
    if tiny:
        encs = [SyntheticClipTower(32, 32, 1), SyntheticClipTower(32, 32, 2)]
        return [SyntheticClipTokenizer(1000, 999), SyntheticClipTokenizer(1000, 999)], encs
    c1 = PC.CLIPTextConfig(**{**PC.clip_l_config().__dict__, "projection_dim": 768})
    c2 = PC.open_clip_bigg_config()
    encs = [init_synthetic_clip_(PC.CLIPTextModelWithProjection(c1), seed=1),
            init_synthetic_clip_(PC.CLIPTextModelWithProjection(c2), seed=2)]
    toks = [SyntheticClipTokenizer(e.config.vocab_size, e.config.eos_token_id) for e in encs]
    return toks, encs


def load_models_sd3(pretrained_model_name_or_path: str, weight_dtype=torch.float16, t5_backend=None):
    """(tokenizers, text_encoders, transformer, scheduler) of an SD3 pipeline loaded with text_encoder_3=None, as the
    reference loads it (conceptmod/textsliders/train_lora_sd3.py).  `synthetic://sd3 | tiny_sd3`: the architecture with
    seeded weights.  A local diffusers directory is read with the safetensors loader from transformer/, text_encoder/ and
    text_encoder_2/; text_encoder_3 (T5) is not loaded unless t5_backend is "native": then a NativeT5Tower is the third tower
    (the directory's text_encoder_3 / tokenizer_3, or for `synthetic://` a seeded tiny_t5_config(joint_attention_dim)
    encoder), and train_util.encode_prompts_sd3 writes its rows where the zero rows are."""
    from . import mmdit as PM
    if t5_backend not in (None, "native"):
        raise ValueError(f"t5_backend '{t5_backend}' is not built for SD3: None (zero rows stand in for T5) | native")
    name = pretrained_model_name_or_path
    scheduler = FlowMatchEulerDiscreteScheduler(num_train_timesteps=1000, shift=3.0)
    if name.startswith("synthetic://"):
        kind = name[len("synthetic://"):]
        if kind not in ("sd3", "tiny_sd3"):
            raise ValueError(f"unknown synthetic model '{name}': synthetic://sd3 | synthetic://tiny_sd3")
        tiny = kind == "tiny_sd3"
        model = PM.init_synthetic_(PM.SD3Transformer2DModel(PM.tiny_sd3_config() if tiny else PM.sd3_medium_config()), seed=0)
        toks, encs = synthetic_sd3_towers(tiny)
        if t5_backend == "native":
            encs.append(_synthetic_native_t5(model.config.joint_attention_dim))
            toks.append(encs[-1].tokenizer)
        return toks, encs, model, scheduler
    if os.path.isdir(name):
        import json
        sj = os.path.join(name, "scheduler", "scheduler_config.json")
        if os.path.exists(sj):
            cj = json.load(open(sj))
            scheduler = FlowMatchEulerDiscreteScheduler(cj.get("num_train_timesteps", 1000), cj.get("shift", 3.0))
        from transformers import CLIPTokenizer
        toks = [CLIPTokenizer.from_pretrained(name, subfolder="tokenizer"),
                CLIPTokenizer.from_pretrained(name, subfolder="tokenizer_2")]
        encs = [_clip_from_dir(name, "text_encoder"), _clip_from_dir(name, "text_encoder_2")]
        if t5_backend == "native":
            encs.append(_native_t5_from_dir(name, "text_encoder_3", "tokenizer_3"))
            toks.append(encs[-1].tokenizer)
        return toks, encs, _sd3_from_dir(name), scheduler
    raise ValueError(f"cannot load '{name}': pass a local diffusers directory or synthetic://sd3 | synthetic://tiny_sd3")


class _PromptCachedTower:
    """What the two T5 towers share: `encode_cached(prompt, max_length)` runs `encode` once per distinct (prompt, length) and
    keeps the result -- the tower is frozen, so a prompt's rows never change.  At most CACHE_MAX entries; the oldest goes."""

    CACHE_MAX = 64

    def encode_cached(self, prompt: str, max_length: int):
        cache = self.__dict__.setdefault("_prompt_cache", {})
        key = (prompt, max_length)
        if key not in cache:
            if len(cache) >= self.CACHE_MAX:
                cache.pop(next(iter(cache)))
            cache[key] = self.encode(prompt, max_length)
        return cache[key]


class SyntheticT5Tower(_PromptCachedTower):
    """Offline stand-in for the T5 encoder of a `synthetic://` Flux model, as SyntheticClipTower is for CLIP: a prompt maps
    to seeded normal rows [1, max_length, dim] keyed by a hash of the text."""

    def __init__(self, dim: int):
        self.dim = dim
        self.device, self.dtype = torch.device("cpu"), torch.float32

    def to(self, device=None, dtype=None):
        self.device = torch.device(device) if device is not None else self.device
        self.dtype = dtype or self.dtype
        return self

    def encode(self, prompt: str, max_length: int):
        import hashlib
        seed = int.from_bytes(hashlib.sha256(("t5:" + prompt).encode()).digest()[:8], "little") % (2 ** 31)
        return torch.randn(1, max_length, self.dim, generator=torch.Generator().manual_seed(seed)).to(self.device, self.dtype)


class T5Tower(_PromptCachedTower):
    """Flux's text_encoder_2, a frozen `transformers.T5EncoderModel` with its tokenizer: the one torch forward of the product
    (NativeT5Tower is the same tower on the HIP engine, t5_backend="native").  bf16 or fp32, never fp16 (T5's activations overflow it)."""

    def __init__(self, model, tokenizer):
        self.model, self.tokenizer = model.requires_grad_(False).eval(), tokenizer
        self.dim = model.config.d_model

    @property
    def device(self):
        return next(self.model.parameters()).device

    def to(self, device=None, dtype=None):
        """A request for fp16 is served in bf16, with a warning: the rest of a pipeline may be moved to fp16 in one loop."""
        if dtype == torch.float16:
            import warnings
            warnings.warn("T5Tower: float16 requested; the T5 encoder runs in bfloat16 instead (its activations overflow fp16)")
            dtype = torch.bfloat16
        self.model.to(device=device, dtype=dtype)
        return self

    @torch.no_grad()
    def encode(self, prompt: str, max_length: int):
        ids = self.tokenizer(prompt, padding="max_length", max_length=max_length, truncation=True,
                             return_tensors="pt").input_ids
        return self.model(ids.to(self.device))[0]


class NativeT5Tower(_PromptCachedTower):
    """The T5 encoder on the HIP engine (t5.T5EncoderModel with its tokenizer) behind T5Tower's interface: Flux's
    text_encoder_2, SD3's text_encoder_3.  bf16 only (T5's activations overflow fp16), on a cuda device only."""

    def __init__(self, model, tokenizer):
        self.model, self.tokenizer = model.requires_grad_(False).eval(), tokenizer
        self.dim = model.config.d_model

    @property
    def device(self):
        return self.model.device

    @property
    def dtype(self):
        return self.model.dtype

    def to(self, device=None, dtype=None):
        """A request for fp16 is served in bf16, with T5Tower's warning; fp32 has no engine and is served in bf16 too."""
        if dtype == torch.float16:
            import warnings
            warnings.warn("T5Tower: float16 requested; the T5 encoder runs in bfloat16 instead (its activations overflow fp16)")
        self.model.to(device=device, dtype=torch.bfloat16)
        self.__dict__.pop("_prompt_cache", None)  # rows of another device or engine
        return self

    @torch.no_grad()
    def encode(self, prompt: str, max_length: int):
        ids = self.tokenizer(prompt, padding="max_length", max_length=max_length, truncation=True,
                             return_tensors="pt").input_ids
        return self.model(ids.to(self.device))[0]

    def encode_cached(self, prompt: str, max_length: int):
        """The cache holds the FROZEN tower's rows only.  With a LoRANetwork attached to the model and its multiplier not 0
        (inside `with network:`, generate_images' T5 sweep) the call bypasses it: the rows then depend on the adaptor's
        parameters and multiplier, which may change between two calls.  At multiplier 0 the adapted engine gives the frozen
        bits, so those rows are the cached ones."""
        net = self.model.__dict__.get("_lora_network")
        if net is not None and net.unet_loras and net.engine_params()[2] != 0.0:
            return self.encode(prompt, max_length)
        return super().encode_cached(prompt, max_length)


T5_BACKENDS = ("torch", "native")


def _synthetic_native_t5(dim: int) -> NativeT5Tower:
    """The seeded tiny T5 of the `synthetic://` models on the native engine, `dim` wide, with the hashing tokenizer."""
    from . import t5 as PT
    cfg = PT.tiny_t5_config(dim)
    model = PT.init_synthetic_(PT.T5EncoderModel(cfg), seed=3).to(torch.bfloat16)
    return NativeT5Tower(model, PT.SyntheticT5Tokenizer(cfg.vocab_size))


def _native_t5_from_dir(name: str, sub: str, tok_sub: str) -> NativeT5Tower:
    from transformers import T5TokenizerFast
    from . import t5 as PT
    return NativeT5Tower(PT.t5_from_dir(name, sub), T5TokenizerFast.from_pretrained(name, subfolder=tok_sub))


def _flux_from_dir(path: str):
    """<path>/transformer/config.json + diffusion_pytorch_model.safetensors (safe loader only) -> FluxTransformer2DModel.
    diffusers' config counts the PACKED width (in_channels 64, patch_size 1); FluxConfig the latent channels and the pack."""
    import json
    from safetensors.torch import load_file
    from . import flux as PF
    cj = json.load(open(os.path.join(path, "transformer", "config.json")))
    packed = cj.get("in_channels", 64)
    if cj.get("patch_size", 1) != 1 or packed % 4:
        raise ValueError(f"{path}: a Flux transformer config with patch_size 1 and a packed width that is a multiple of 4")
    cfg = PF.FluxConfig(in_channels=packed // 4, num_layers=cj.get("num_layers", 19),
                        num_single_layers=cj.get("num_single_layers", 38),
                        num_attention_heads=cj.get("num_attention_heads", 24),
                        attention_head_dim=cj.get("attention_head_dim", 128),
                        joint_attention_dim=cj.get("joint_attention_dim", 4096),
                        pooled_projection_dim=cj.get("pooled_projection_dim", 768),
                        guidance_embeds=bool(cj.get("guidance_embeds", False)),
                        axes_dims_rope=tuple(cj.get("axes_dims_rope", (16, 56, 56))))
    model = PF.FluxTransformer2DModel(cfg)
    sd = {}
    files = [f for f in sorted(os.listdir(os.path.join(path, "transformer"))) if f.endswith(".safetensors")]
    for f in files:  # (the published checkpoints are sharded)
        sd.update(load_file(os.path.join(path, "transformer", f)))
    model.load_state_dict(sd)
    return model


def load_models_flux(pretrained_model_name_or_path: str, weight_dtype=torch.float16, no_t5: bool = False,
                     t5_backend: str = "torch"):
    """(tokenizers, text_encoders, transformer, scheduler) of a Flux pipeline (conceptmod/textsliders/model_util.py
    load_models_flux).  text_encoders = [CLIP-L on the native engine (its un-projected pooled row conditions the network),
    the T5 tower or None]: a directory's text_encoder_2 is loaded as a transformers.T5EncoderModel unless `no_t5`; without it
    zero rows stand in for the sequence embedding (train_util.encode_prompts_flux).  The T5 tower runs in bf16 (fp32 with
    weight_dtype=torch.float32), never fp16: `T5Tower.to(dtype=torch.float16)` moves it to bf16 and warns.  `synthetic://flux_schnell | flux_dev |
    tiny_flux`: the architecture with seeded weights and hashed stand-in towers.  t5_backend "native": the T5 tower is a
    NativeT5Tower -- the directory's text_encoder_2 on the HIP engine (t5.T5EncoderModel), or for `synthetic://` a seeded
    tiny_t5_config(joint_attention_dim) encoder with a SyntheticT5Tokenizer; "torch" (the default) is as before."""
    from . import flux as PF
    if t5_backend not in T5_BACKENDS:
        raise ValueError(f"t5_backend '{t5_backend}': torch | native")
    name = pretrained_model_name_or_path
    if name.startswith("synthetic://"):
        kind = name[len("synthetic://"):]
        cfgs = {"flux_schnell": PF.flux_schnell_config, "flux_dev": PF.flux_dev_config, "tiny_flux": PF.tiny_flux_config}
        if kind not in cfgs:
            raise ValueError(f"unknown synthetic model '{name}': synthetic://flux_schnell | flux_dev | tiny_flux")
        cfg = cfgs[kind]()
        model = PF.init_synthetic_(PF.FluxTransformer2DModel(cfg), seed=0)
        scheduler = FlowMatchEulerDiscreteScheduler(1000, 3.0 if kind == "flux_dev" else 1.0,
                                                    use_dynamic_shifting=kind == "flux_dev")
        clip = SyntheticClipTower(cfg.pooled_projection_dim, cfg.pooled_projection_dim, 1)
        t5 = None if no_t5 else (_synthetic_native_t5(cfg.joint_attention_dim) if t5_backend == "native"
                                 else SyntheticT5Tower(cfg.joint_attention_dim))
        return [SyntheticClipTokenizer(1000, 999), None], [clip, t5], model, scheduler
    if os.path.isdir(name):
        import json
        scheduler = FlowMatchEulerDiscreteScheduler(1000, 1.0)
        sj = os.path.join(name, "scheduler", "scheduler_config.json")
        if os.path.exists(sj):
            cj = json.load(open(sj))
            scheduler = FlowMatchEulerDiscreteScheduler(
                cj.get("num_train_timesteps", 1000), cj.get("shift", 1.0), cj.get("use_dynamic_shifting", False),
                cj.get("base_shift", 0.5), cj.get("max_shift", 1.15), cj.get("base_image_seq_len", 256),
                cj.get("max_image_seq_len", 4096))
        from transformers import CLIPTokenizer
        toks, encs = [CLIPTokenizer.from_pretrained(name, subfolder="tokenizer"), None], [_clip_from_dir(name, "text_encoder"), None]
        if not no_t5 and t5_backend == "native" and os.path.isdir(os.path.join(name, "text_encoder_2")):
            encs[1] = _native_t5_from_dir(name, "text_encoder_2", "tokenizer_2")
            toks[1] = encs[1].tokenizer
        elif not no_t5 and os.path.isdir(os.path.join(name, "text_encoder_2")):
            from transformers import T5EncoderModel, T5TokenizerFast
            tok2 = T5TokenizerFast.from_pretrained(name, subfolder="tokenizer_2")
            t5 = T5EncoderModel.from_pretrained(name, subfolder="text_encoder_2",
                                                torch_dtype=torch.float32 if weight_dtype == torch.float32 else torch.bfloat16)
            toks[1], encs[1] = tok2, T5Tower(t5, tok2)
        return toks, encs, _flux_from_dir(name), scheduler
    raise ValueError(f"cannot load '{name}': pass a local diffusers directory or synthetic://flux_schnell | flux_dev | tiny_flux")


def load_vae_decoder_sd3(pretrained_model_name_or_path: str):
    """The 16-channel AutoencoderKL decoder of SD3 (no post_quant_conv; scaling 1.5305, shift 0.0609): seeded for
    `synthetic://(tiny_)sd3`, else read from the directory's `vae/` with the safetensors loader."""
    import json
    from . import vae as PV
    from . import vae_decoder as PD
    name = pretrained_model_name_or_path
    if name.startswith("synthetic://"):
        cfg = PV.sd3_vae_config()
        if "flux" in name:  # FLUX.1's vae/config.json: the same decoder, other latent statistics
            cfg = PV.VAEConfig(**{**cfg.__dict__, "scaling_factor": 0.3611, "shift_factor": 0.1159})
        if "tiny" in name:
            cfg = PV.VAEConfig(**{**cfg.__dict__, "block_out_channels": (64, 128, 128, 128), "norm_num_groups": 16})
        return PD.init_synthetic_(PD.AutoencoderKLDecoder(cfg), seed=11)
    if os.path.isdir(name):
        from safetensors.torch import load_file
        cj = json.load(open(os.path.join(name, "vae", "config.json")))
        cfg = PV.VAEConfig(in_channels=cj.get("out_channels", cj.get("in_channels", 3)),
                           latent_channels=cj.get("latent_channels", 16), block_out_channels=tuple(cj["block_out_channels"]),
                           layers_per_block=cj.get("layers_per_block", 2), norm_num_groups=cj.get("norm_num_groups", 32),
                           scaling_factor=cj.get("scaling_factor", 1.5305), shift_factor=cj.get("shift_factor") or 0.0,
                           use_post_quant_conv=cj.get("use_post_quant_conv", True))
        vae = PD.AutoencoderKLDecoder(cfg)
        vae.load_state_dict(load_file(os.path.join(name, "vae", "diffusion_pytorch_model.safetensors")))
        return vae
    raise ValueError(f"cannot load a VAE decoder from '{name}': a local diffusers directory or synthetic://sd3 | tiny_sd3")


# ----------------------------------------------------------------------------------------------------------------
# LPIPS (AlexNet) for scoring a sweep (reference: eval-scripts/lpip_score.py builds lpips.LPIPS(net='alex') from the hub)
# ----------------------------------------------------------------------------------------------------------------
TINY_ALEX_CHANNELS = (16, 24, 32, 24, 16)  # multiples of 8 (the kernels' limit), all different from their neighbours


def _read_state_file(path: str):
    """A state dict from `.safetensors`, or from `.pth` with the safe unpickler only (weights_only=True)."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    if path.endswith(".pth"):
        return torch.load(path, map_location="cpu", weights_only=True)
    raise ValueError(f"'{path}': state dicts are read from .safetensors or .pth files")


def load_lpips(name: str):
    """The `lpips.LPIPS(net='alex')` container for `lpips_score`: `synthetic://alex | tiny_alex` with seeded weights, or
    the released weights from local files -- a directory, or two files joined by a comma -- that together hold an AlexNet
    state dict (torchvision's `features.*` names or the package's `net.slice*` names) and the `lin` weights
    (`lin{0..4}.model.1.weight`).  Files are merged in sorted order; every parameter must be found."""
    from . import lpips as PL
    if name.startswith("synthetic://"):
        kind = name[len("synthetic://"):]
        if kind not in ("alex", "tiny_alex"):
            raise ValueError(f"unknown synthetic LPIPS '{name}': synthetic://alex | tiny_alex")
        return PL.init_synthetic_(PL.LPIPS(PL.ALEX_CHANNELS if kind == "alex" else TINY_ALEX_CHANNELS), seed=17)
    if os.path.isdir(name):
        files = sorted(os.path.join(name, f) for f in os.listdir(name) if f.endswith((".safetensors", ".pth")))
    else:
        files = [f for f in name.split(",") if f]
    if not files or not all(os.path.isfile(f) for f in files):
        raise ValueError(f"cannot load LPIPS from '{name}': no network in this environment; pass a local directory, two "
                         f"files joined by a comma, or synthetic://alex | synthetic://tiny_alex")
    merged = {}
    for f in files:
        merged.update(PL.canonical_state_dict(_read_state_file(f)))
    want = [f"{c}.weight" for c in PL.conv_names()]
    missing = [k for k in want if k not in merged]
    if missing:
        raise ValueError(f"cannot load LPIPS from '{name}': no AlexNet convolution {missing[0]} (or its torchvision name) "
                         f"in {files}")
    model = PL.LPIPS(tuple(int(merged[k].shape[0]) for k in want))
    model.load_state_dict(merged, strict=False)
    have = set(merged)
    lost = [k for k, _ in model.named_parameters() if k not in have]
    if lost:
        raise ValueError(f"cannot load LPIPS from '{name}': {lost} not found in {files}")
    return model
