"""Null-text inversion of a real image (demo_image_editing.ipynb, class NullInversion), step for step, on the HIP engine:

    load_512            crop by the offsets, centre-crop to a square, resize (host, PIL)
    image2latent        vae.encode(image).latent_dist.mean x scaling_factor
    ddim_loop           DDIM inversion with the CONDITIONAL embedding only (`next_step`)
    null_optimization   per timestep: a fresh Adam (lr = 1e-2 (1 - i / 100)) on the unconditional embedding, the conditional
                        prediction once without gradient, up to num_inner_steps steps on
                        mse(prev_step(eps_u + g (eps_c - eps_u)), the DDIM latent of the step before), early stop at
                        loss < epsilon + i 2e-5, then one guided `prev_step` with the optimised embedding
    invert              ((image, reconstruction), x_T, [unconditional embedding per step])

`fused=True` (default) runs an inner step as five native calls and one scalar read, on buffers allocated once: the cast of
the fp32 embedding to the UNet's dtype, the UNet forward on the one unconditional sample (smi_unet_forward, saving), the fused
loss and d(loss)/d(eps_u) (smi_nulltext_loss), the backward to the embedding (smi_unet_backward_ctx) and Adam
(_native.adam_step: the step's AdamW call with weight_decay 0 and no clipping).  `fused=False` is the notebook's own code against the product UNet:
torch autograd through `unet(latent, t, encoder_hidden_states=uncond)`, `nnf.mse_loss`, `torch.optim.Adam`.

Differences from the notebook: the UNet computes in fp16 / bf16 storage (the embedding and Adam's state stay fp32 and the
embedding is rounded for each UNet call); `next_step` / `prev_step` are two coefficients computed on the host and one
affine kernel (smi_sched_step's arithmetic) instead of five tensor ops; prompts are encoded by a callable the caller passes
(`encode_prompt`), not by a pipeline object; prompt-to-prompt attention control is not part of this package.
SD-XL is refused here: its added conditioning (`text_embeds`, `time_ids`) goes through the loop of
null_inversion_xl.NullInversionXL.  That class is a subclass of this one: every loop below is written once and carries an
optional pooled embedding (`self.pooled`, None here: no `added_cond_kwargs`, no pooled parameter, no pooled gradient)."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _native, model_util


def load_512(image_path, left=0, right=0, top=0, bottom=0, size: int = 512) -> np.ndarray:
    """The notebook's load_512 (its offset clamps included, `top = min(top, h - left - 1)` as written there): uint8
    [size, size, 3]."""
    from PIL import Image
    if isinstance(image_path, str):
        image = np.array(Image.open(image_path))
        if image.ndim == 2:
            image = np.stack([image] * 3, axis=-1)
        image = image[:, :, :3]
    else:
        image = np.asarray(image_path)
    h, w, _c = image.shape
    left = min(left, w - 1)
    right = min(right, w - left - 1)
    top = min(top, h - left - 1)
    bottom = min(bottom, h - top - 1)
    image = image[top:h - bottom, left:w - right]
    h, w, _c = image.shape
    if h < w:
        offset = (w - h) // 2
        image = image[:, offset:offset + h]
    elif w < h:
        offset = (h - w) // 2
        image = image[offset:offset + w]
    return np.array(Image.fromarray(np.ascontiguousarray(image)).resize((size, size)))


def step_coefficients(scheduler, timestep: int, forward: bool):
    """(c_x, c_eps) with next_step / prev_step(eps, t, x) = c_x x + c_eps eps, from the scheduler's alphas_cumprod."""
    t = int(timestep)
    ratio = scheduler.num_train_timesteps // scheduler.num_inference_steps
    alphas, final = scheduler.alphas_cumprod, float(scheduler.final_alpha_cumprod)
    if forward:  # next_step: from t - ratio up to t
        cur = min(t - ratio, 999)
        a_from = float(alphas[cur]) if cur >= 0 else final
        a_to = float(alphas[t])
    else:  # prev_step: from t down to t - ratio
        a_from = float(alphas[t])
        a_to = float(alphas[t - ratio]) if t - ratio >= 0 else final
    return (a_to / a_from) ** 0.5, (1 - a_to) ** 0.5 - (a_to * (1 - a_from) / a_from) ** 0.5


class NullInversion:
    """unet: the product UNet2DConditionModel on a cuda device; scheduler: a DDIM scheduler of this package; vae /
    vae_decoder: the AutoencoderKL encoder and decoder (only `invert`, `image2latent`, `latent2image` need them);
    encode_prompt(str) -> [1, L, D] embedding (only `invert` needs it)."""

    ADDED_COND = False  # the UNet takes text_embeds / time_ids (SD-XL): True in null_inversion_xl.NullInversionXL

    def __init__(self, unet, scheduler, vae=None, vae_decoder=None, encode_prompt: Optional[Callable] = None,
                 num_ddim_steps: int = 50, guidance_scale: float = 7.5, fused: bool = True, image_size: int = 512):
        if unet.device.type != "cuda":
            raise _native.SmiError("null-text inversion runs only on an MI355X through the HIP engine; move the UNet to a "
                                   "cuda device with unet.to(device, dtype) (there is no CPU fallback)")
        if (unet.cfg.addition_embed_type == "text_time") != self.ADDED_COND:
            raise _native.SmiError("NullInversionXL needs a UNet with text_time added conditioning (SD-XL); for an SD-1.x "
                                   "UNet use null_inversion.NullInversion" if self.ADDED_COND else
                                   "NullInversion is the SD-1.x class; an SD-XL UNet needs its added conditioning "
                                   "(text_embeds, time_ids) passed through the loop: use "
                                   "null_inversion_xl.NullInversionXL")
        if not isinstance(scheduler, model_util.DDIMScheduler) or type(scheduler) is not model_util.DDIMScheduler:
            raise ValueError("null-text inversion needs the deterministic DDIM scheduler (scheduler_name='ddim')")
        self.unet, self.scheduler, self.vae, self.vae_decoder = unet, scheduler, vae, vae_decoder
        self.encode_prompt = encode_prompt
        self.num_ddim_steps, self.guidance_scale, self.fused = int(num_ddim_steps), float(guidance_scale), bool(fused)
        self.image_size = image_size
        self.scheduler.set_timesteps(self.num_ddim_steps)
        self.context = None  # cat([uncond, cond]) sequence embeddings
        self.pooled = None   # cat([uncond, cond]) pooled embeddings: SD-XL only
        self.time_ids = None  # [1, 6]: SD-XL only
        self.prompt = None
        self.losses: List[List[float]] = []  # per timestep, the loss of every inner step taken (last run)

    # ---- the notebook's small pieces ---------------------------------------------------------------------------------
    def _affine(self, x, eps, t, forward):
        cx, ce = step_coefficients(self.scheduler, t, forward)
        return model_util._affine(x, eps, None, cx, ce, 0.0)

    def prev_step(self, model_output, timestep, sample):
        return self._affine(sample, model_output, timestep, False)

    def next_step(self, model_output, timestep, sample):
        return self._affine(sample, model_output, timestep, True)

    def _eps(self, latents, t, context, pooled):
        """One UNet call; pooled None: no added conditioning"""
        added = None if pooled is None else {"text_embeds": pooled, "time_ids": self.time_ids.expand(pooled.shape[0], -1)}
        return self.unet(latents, t, encoder_hidden_states=context, added_cond_kwargs=added).sample

    def _halves(self):
        """(uncond, cond), (pooled_uncond, pooled_cond) of the prompt; the pooled pair is (None, None) for SD-1.x"""
        return self.context.chunk(2), (None, None) if self.pooled is None else self.pooled.chunk(2)

    def get_noise_pred_single(self, latents, t, context):
        return self._eps(latents, t, context, None)

    @torch.no_grad()
    def _guided_step(self, latents, t, is_forward, context, pooled):
        context = self.context if context is None else context
        pooled = self.pooled if pooled is None else pooled
        guidance_scale = 1.0 if is_forward else self.guidance_scale
        u, c = self._eps(torch.cat([latents] * 2), t, context, pooled).chunk(2)
        noise_pred = u + guidance_scale * (c - u)
        return self.next_step(noise_pred, t, latents) if is_forward else self.prev_step(noise_pred, t, latents)

    def get_noise_pred(self, latents, t, is_forward=True, context=None):
        return self._guided_step(latents, t, is_forward, context, None)

    @torch.no_grad()
    def latent2image(self, latents) -> np.ndarray:
        rgb = self.vae_decoder.decode_to_uint8(latents.detach().float() / self.vae_decoder.config.scaling_factor)
        return rgb[0].cpu().numpy()

    @torch.no_grad()
    def image2latent(self, image) -> torch.Tensor:
        if isinstance(image, torch.Tensor) and image.dim() == 4:
            return image
        image = torch.from_numpy(np.asarray(image)).float() / 127.5 - 1
        image = image.permute(2, 0, 1).unsqueeze(0).to(self.vae.device)
        return (self.vae.encode(image).latent_dist.mode() * self.vae.config.scaling_factor).float()

    @torch.no_grad()
    def init_prompt(self, prompt: str):
        uncond, cond = self.encode_prompt(""), self.encode_prompt(prompt)
        self.context = torch.cat([uncond, cond]).to(self.unet.device)
        self.prompt = prompt

    @torch.no_grad()
    def ddim_loop(self, latent) -> List[torch.Tensor]:
        (_uncond, cond), (_pooled_u, pooled_c) = self._halves()
        all_latent = [latent]
        latent = latent.clone().detach().float()
        for i in range(self.num_ddim_steps):
            t = int(self.scheduler.timesteps[len(self.scheduler.timesteps) - i - 1])
            noise_pred = self._eps(latent, t, cond, pooled_c)
            latent = self.next_step(noise_pred, t, latent)
            all_latent.append(latent)
        return all_latent

    @torch.no_grad()
    def ddim_inversion(self, image):
        latent = self.image2latent(image)
        image_rec = self.latent2image(latent)
        return image_rec, self.ddim_loop(latent)

    # ---- the optimisation ---------------------------------------------------------------------------------------------
    def null_optimization(self, latents: Sequence[torch.Tensor], num_inner_steps: int = 10, epsilon: float = 1e-5):
        return self._null_optimization(latents, num_inner_steps, epsilon, False)[0]

    def _null_optimization(self, latents, num_inner_steps, epsilon, optimize_pooled):
        """(uncond_embeddings_list, uncond_pooled_list): one [1, L, D] per DDIM step and, for SD-XL, one [1, P]"""
        run = self._null_optimization_fused if self.fused else self._null_optimization_autograd
        return run(latents, num_inner_steps, epsilon, optimize_pooled)

    def _null_optimization_autograd(self, latents, num_inner_steps, epsilon, optimize_pooled):
        """The notebook's loop, unchanged but for the scheduler arithmetic: autograd through the product UNet; for SD-XL
        with the pooled embedding carried along, as a second parameter when optimize_pooled."""
        import torch.nn.functional as nnf
        g = self.guidance_scale
        (uncond, cond), (pooled_u, pooled_c) = self._halves()
        has_pooled = pooled_u is not None
        out, out_pooled, self.losses = [], [], []
        latent_cur = latents[-1]
        uncond, pooled = uncond.float(), pooled_u.float() if has_pooled else None
        for i in range(self.num_ddim_steps):
            uncond = uncond.clone().detach().requires_grad_(True)
            if has_pooled:
                pooled = pooled.clone().detach().requires_grad_(optimize_pooled)
            optimizer = torch.optim.Adam([uncond, pooled] if optimize_pooled else [uncond], lr=1e-2 * (1. - i / 100.))
            latent_prev = latents[len(latents) - i - 2]
            t = int(self.scheduler.timesteps[i])
            cx, ce = step_coefficients(self.scheduler, t, False)
            with torch.no_grad():
                noise_pred_cond = self._eps(latent_cur, t, cond, pooled_c)
            self.losses.append([])
            for _j in range(num_inner_steps):
                noise_pred_uncond = self._eps(latent_cur, t, uncond, pooled)
                noise_pred = noise_pred_uncond + g * (noise_pred_cond - noise_pred_uncond)
                latents_prev_rec = cx * latent_cur + ce * noise_pred
                loss = nnf.mse_loss(latents_prev_rec, latent_prev)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                loss_item = loss.item()
                self.losses[-1].append(loss_item)
                if loss_item < epsilon + i * 2e-5:
                    break
            out.append(uncond[:1].detach())
            if has_pooled:  # with the optimisation off: the encoder's, unchanged
                out_pooled.append(pooled[:1].detach() if optimize_pooled else pooled_u[:1].clone())
            with torch.no_grad():
                context = torch.cat([uncond.detach().to(cond.dtype), cond])
                pooled2 = torch.cat([pooled.detach().to(pooled_c.dtype), pooled_c]) if has_pooled else None
                latent_cur = self._guided_step(latent_cur, t, False, context, pooled2)
        return out, out_pooled

    @torch.no_grad()
    def _null_optimization_fused(self, latents, num_inner_steps, epsilon, optimize_pooled):
        unet, g = self.unet, self.guidance_scale
        dev, dt = unet.device, unet.dtype
        (uncond, cond), (pooled_u, pooled_c) = self._halves()
        has_pooled = pooled_u is not None
        latent_cur = latents[-1].float().contiguous()
        _n, _c, h, w = latent_cur.shape
        L, D = uncond.shape[1], uncond.shape[2]
        n_seq = L * D
        # every buffer of the inner loop, once: the flat fp32 master copy [L D (+ P)], its gradient and Adam's state
        param = torch.cat([uncond[:1].detach().float().reshape(-1)] +
                          ([pooled_u[:1].detach().float().reshape(-1)] if optimize_pooled else [])).contiguous()
        grad, m, v = (torch.zeros_like(param) for _ in range(3))
        seq, seq_g = param[:n_seq].view(1, L, D), grad[:n_seq].view(1, L, D)
        seq_t = torch.empty((1, L, D), dtype=dt, device=dev)
        pooled_t = time_ids = None
        if has_pooled:
            pooled_t = pooled_u[:1].detach().to(dt).contiguous().clone()  # stays the encoder's with the pooled optimisation off
            time_ids = self.time_ids[:1].float().contiguous()
        if optimize_pooled:
            P = pooled_u.shape[1]
            pool, pool_g = param[n_seq:].view(1, P), grad[n_seq:].view(1, P)
        eps_u = torch.empty_like(latent_cur)
        d_eps_u = torch.empty_like(latent_cur)
        loss_dev = torch.zeros(1, device=dev)
        scratch = torch.empty(1025, device=dev)
        out, out_pooled, self.losses = [], [], []
        for i in range(self.num_ddim_steps):
            lr = 1e-2 * (1. - i / 100.)
            m.zero_(), v.zero_()  # a fresh Adam per timestep
            latent_prev = latents[len(latents) - i - 2].float().contiguous()
            t = int(self.scheduler.timesteps[i])
            cx, ce = step_coefficients(self.scheduler, t, False)
            eps_c = self._eps(latent_cur, t, cond, pooled_c).contiguous()
            # capacity two (the guided step below), so that no call of this loop re-plans the engine
            eng = unet._ensure_engine(2, h, w, L)
            eng.set_ctx_grad(True)
            if has_pooled:
                eng.set_pooled_grad(optimize_pooled)
            self.losses.append([])
            for j in range(num_inner_steps):
                _native.cast_f32(seq, seq_t)
                if optimize_pooled:
                    _native.cast_f32(pool, pooled_t)
                eng.forward(latent_cur, float(t), seq_t, pooled_t, time_ids, None, None, 0.0, True, out=eps_u)
                _native.nulltext_loss(eps_u, eps_c, latent_cur, latent_prev, g, cx, ce, loss_dev, d_eps_u, scratch)
                if optimize_pooled:
                    eng.backward_cond(d_eps_u, None, None, seq_g, pool_g)
                else:
                    eng.backward_ctx(d_eps_u, None, None, seq_g)
                _native.adam_step(param, grad, m, v, lr, j + 1, scratch)
                loss_item = loss_dev.item()  # the one read the early stop needs
                self.losses[-1].append(loss_item)
                if loss_item < epsilon + i * 2e-5:
                    break
            if has_pooled:
                eng.set_pooled_grad(False)
            eng.set_ctx_grad(False)
            out.append(seq.clone())
            context = torch.cat([seq.to(cond.dtype), cond])
            pooled2 = None
            if has_pooled:
                out_pooled.append(pool.clone() if optimize_pooled else pooled_u[:1].clone())
                pooled2 = torch.cat([out_pooled[-1].to(pooled_c.dtype), pooled_c])
            latent_cur = self._guided_step(latent_cur, t, False, context, pooled2).contiguous()
        return out, out_pooled

    def _ddim_invert(self, image_path, prompt, offsets, verbose):
        """The first half of `invert`: ((image, reconstruction), the DDIM latents)"""
        if self.vae is None or self.vae_decoder is None or self.encode_prompt is None:
            raise ValueError("invert needs the VAE encoder, the VAE decoder and encode_prompt")
        self.init_prompt(prompt)
        image_gt = load_512(image_path, *offsets, size=self.image_size)
        if verbose:
            print("DDIM inversion...")
        image_rec, ddim_latents = self.ddim_inversion(image_gt)
        if verbose:
            print("Null-text optimization...")
        return (image_gt, image_rec), ddim_latents

    def invert(self, image_path, prompt: str, offsets=(0, 0, 0, 0), num_inner_steps: int = 10,
               early_stop_epsilon: float = 1e-5, verbose: bool = False):
        images, ddim_latents = self._ddim_invert(image_path, prompt, offsets, verbose)
        uncond_embeddings = self.null_optimization(ddim_latents, num_inner_steps, early_stop_epsilon)
        return images, ddim_latents[-1], uncond_embeddings


