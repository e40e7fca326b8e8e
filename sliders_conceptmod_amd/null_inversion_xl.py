"""Null-text inversion of a real image on an SD-XL UNet: the methods of `null_inversion.NullInversion`
(demo_image_editing.ipynb, class NullInversion) by name, with SD-XL's added conditioning carried through every UNet call.

SD-XL's unconditional conditioning has two parts: the sequence embedding [1, 77, D] and the pooled embedding `text_embeds`
[1, P], which enters every resnet through the time embedding.  `null_optimization(..., optimize_pooled=True)` optimises
both (one Adam over the two tensors); with `optimize_pooled=False` only the sequence embedding, as the notebook does for
SD-1.4, and the pooled entries returned are the encoder's, unchanged.  `time_ids` are
`train_util.get_add_time_ids(image_size, image_size)` and take no gradient.  The notebook is SD-1.4 only: this route and the
pooled optimisation are this package's additions.

`fused=True` (default): one flat fp32 parameter [77 D + P] ([77 D] with the pooled optimisation off); an inner step is the
casts of its parts to the UNet's dtype (smi_op_cast_f32), one saving smi_unet_forward on the one unconditional sample,
smi_nulltext_loss, smi_unet_backward_cond (smi_unet_backward_ctx with the pooled optimisation off) writing into the flat
gradient, one smi_clip_adamw over the flat buffer with weight_decay 0 and no clipping (Adam is element-wise: this equals one
torch.optim.Adam over the two tensors) and one scalar read for the early stop; every buffer is allocated before the loop.
`fused=False` is the notebook's loop with torch autograd through the product UNet's seam."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _native, model_util, train_util
from .null_inversion import load_512, step_coefficients


class NullInversionXL:
    """unet: the product SD-XL UNet2DConditionModel on a cuda device; scheduler: a DDIM scheduler of this package; vae /
    vae_decoder: the AutoencoderKL encoder and decoder (only `invert`, `image2latent`, `latent2image` need them);
    encode_prompt(str) -> (embeds [1, L, D], pooled [1, P]) (only `invert` / `init_prompt` need it)."""

    def __init__(self, unet, scheduler, vae=None, vae_decoder=None, encode_prompt: Optional[Callable] = None,
                 num_ddim_steps: int = 50, guidance_scale: float = 7.5, fused: bool = True, image_size: int = 1024):
        if unet.device.type != "cuda":
            raise _native.SmiError("null-text inversion runs only on an MI355X through the HIP engine; move the UNet to a "
                                   "cuda device with unet.to(device, dtype) (there is no CPU fallback)")
        if unet.cfg.addition_embed_type != "text_time":
            raise _native.SmiError("NullInversionXL needs a UNet with text_time added conditioning (SD-XL); for an SD-1.x "
                                   "UNet use null_inversion.NullInversion")
        if not isinstance(scheduler, model_util.DDIMScheduler) or type(scheduler) is not model_util.DDIMScheduler:
            raise ValueError("null-text inversion needs the deterministic DDIM scheduler (scheduler_name='ddim')")
        self.unet, self.scheduler, self.vae, self.vae_decoder = unet, scheduler, vae, vae_decoder
        self.encode_prompt = encode_prompt
        self.num_ddim_steps, self.guidance_scale, self.fused = int(num_ddim_steps), float(guidance_scale), bool(fused)
        self.image_size = image_size
        self.scheduler.set_timesteps(self.num_ddim_steps)
        self.time_ids = train_util.get_add_time_ids(image_size, image_size, dtype=torch.float32).to(unet.device)  # [1, 6]
        self.context = None  # cat([uncond, cond]) sequence embeddings
        self.pooled = None   # cat([uncond, cond]) pooled embeddings
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

    def _added(self, pooled):
        return {"text_embeds": pooled, "time_ids": self.time_ids.expand(pooled.shape[0], -1)}

    def get_noise_pred_single(self, latents, t, context, pooled):
        return self.unet(latents, t, encoder_hidden_states=context, added_cond_kwargs=self._added(pooled)).sample

    @torch.no_grad()
    def get_noise_pred(self, latents, t, is_forward=True, context=None, pooled=None):
        context = self.context if context is None else context
        pooled = self.pooled if pooled is None else pooled
        guidance_scale = 1.0 if is_forward else self.guidance_scale
        noise_pred = self.unet(torch.cat([latents] * 2), t, encoder_hidden_states=context,
                               added_cond_kwargs=self._added(pooled)).sample
        u, c = noise_pred.chunk(2)
        noise_pred = u + guidance_scale * (c - u)
        return self.next_step(noise_pred, t, latents) if is_forward else self.prev_step(noise_pred, t, latents)

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
        (uncond, pooled_u), (cond, pooled_c) = self.encode_prompt(""), self.encode_prompt(prompt)
        self.context = torch.cat([uncond, cond]).to(self.unet.device)
        self.pooled = torch.cat([pooled_u, pooled_c]).to(self.unet.device)
        self.prompt = prompt

    @torch.no_grad()
    def ddim_loop(self, latent) -> List[torch.Tensor]:
        cond, pooled_c = self.context.chunk(2)[1], self.pooled.chunk(2)[1]
        all_latent = [latent]
        latent = latent.clone().detach().float()
        for i in range(self.num_ddim_steps):
            t = int(self.scheduler.timesteps[len(self.scheduler.timesteps) - i - 1])
            noise_pred = self.get_noise_pred_single(latent, t, cond, pooled_c)
            latent = self.next_step(noise_pred, t, latent)
            all_latent.append(latent)
        return all_latent

    @torch.no_grad()
    def ddim_inversion(self, image):
        latent = self.image2latent(image)
        image_rec = self.latent2image(latent)
        return image_rec, self.ddim_loop(latent)

    # ---- the optimisation ---------------------------------------------------------------------------------------------
    def null_optimization(self, latents: Sequence[torch.Tensor], num_inner_steps: int = 10, epsilon: float = 1e-5,
                          optimize_pooled: bool = True):
        """(uncond_embeddings_list, uncond_pooled_list): one [1, L, D] and one [1, P] per DDIM step."""
        run = self._null_optimization_fused if self.fused else self._null_optimization_autograd
        return run(latents, num_inner_steps, epsilon, bool(optimize_pooled))

    def _null_optimization_autograd(self, latents, num_inner_steps, epsilon, optimize_pooled):
        """The notebook's loop with the pooled embedding as a second parameter: autograd through the product UNet."""
        import torch.nn.functional as nnf
        g = self.guidance_scale
        (uncond, cond), (pooled_u, pooled_c) = self.context.chunk(2), self.pooled.chunk(2)
        out, out_pooled, self.losses = [], [], []
        latent_cur = latents[-1]
        uncond, pooled = uncond.float(), pooled_u.float()
        for i in range(self.num_ddim_steps):
            uncond = uncond.clone().detach().requires_grad_(True)
            pooled = pooled.clone().detach().requires_grad_(optimize_pooled)
            optimizer = torch.optim.Adam([uncond, pooled] if optimize_pooled else [uncond], lr=1e-2 * (1. - i / 100.))
            latent_prev = latents[len(latents) - i - 2]
            t = int(self.scheduler.timesteps[i])
            cx, ce = step_coefficients(self.scheduler, t, False)
            with torch.no_grad():
                noise_pred_cond = self.get_noise_pred_single(latent_cur, t, cond, pooled_c)
            self.losses.append([])
            for _j in range(num_inner_steps):
                noise_pred_uncond = self.get_noise_pred_single(latent_cur, t, uncond, pooled)
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
            out_pooled.append(pooled[:1].detach())
            with torch.no_grad():
                context = torch.cat([uncond.detach().to(cond.dtype), cond])
                pooled2 = torch.cat([pooled.detach().to(pooled_c.dtype), pooled_c])
                latent_cur = self.get_noise_pred(latent_cur, t, False, context, pooled2)
        if not optimize_pooled:
            out_pooled = [pooled_u[:1].clone() for _ in out]  # the encoder's, unchanged
        return out, out_pooled

    @torch.no_grad()
    def _null_optimization_fused(self, latents, num_inner_steps, epsilon, optimize_pooled):
        unet, g = self.unet, self.guidance_scale
        dev, dt = unet.device, unet.dtype
        (uncond, cond), (pooled_u, pooled_c) = self.context.chunk(2), self.pooled.chunk(2)
        latent_cur = latents[-1].float().contiguous()
        _n, _c, h, w = latent_cur.shape
        L, D, P = uncond.shape[1], uncond.shape[2], pooled_u.shape[1]
        n_seq = L * D
        # every buffer of the inner loop, once: the flat fp32 master copy [L D (+ P)], its gradient and Adam's state
        param = torch.cat([uncond[:1].detach().float().reshape(-1)] +
                          ([pooled_u[:1].detach().float().reshape(-1)] if optimize_pooled else [])).contiguous()
        grad, m, v = (torch.zeros_like(param) for _ in range(3))
        seq, seq_g = param[:n_seq].view(1, L, D), grad[:n_seq].view(1, L, D)
        seq_t = torch.empty((1, L, D), dtype=dt, device=dev)
        pooled_t = pooled_u[:1].detach().to(dt).contiguous().clone()  # stays the encoder's with the pooled optimisation off
        if optimize_pooled:
            pool, pool_g = param[n_seq:].view(1, P), grad[n_seq:].view(1, P)
        time_ids = self.time_ids[:1].float().contiguous()
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
            eps_c = self.get_noise_pred_single(latent_cur, t, cond, pooled_c).contiguous()
            # capacity two (the guided step below), so that no call of this loop re-plans the engine
            eng = unet._ensure_engine(2, h, w, L)
            eng.set_ctx_grad(True)
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
            eng.set_pooled_grad(False)
            eng.set_ctx_grad(False)
            out.append(seq.clone())
            out_pooled.append(pool.clone() if optimize_pooled else pooled_u[:1].clone())
            context = torch.cat([seq.to(cond.dtype), cond])
            pooled2 = torch.cat([(pool if optimize_pooled else pooled_u[:1]).to(pooled_c.dtype), pooled_c])
            latent_cur = self.get_noise_pred(latent_cur, t, False, context, pooled2).contiguous()
        return out, out_pooled

    def invert(self, image_path, prompt: str, offsets=(0, 0, 0, 0), num_inner_steps: int = 10,
               early_stop_epsilon: float = 1e-5, verbose: bool = False, optimize_pooled: bool = True):
        """((image, reconstruction), x_T, [unconditional embedding per step], [unconditional pooled embedding per step])"""
        if self.vae is None or self.vae_decoder is None or self.encode_prompt is None:
            raise ValueError("invert needs the VAE encoder, the VAE decoder and encode_prompt")
        self.init_prompt(prompt)
        image_gt = load_512(image_path, *offsets, size=self.image_size)
        if verbose:
            print("DDIM inversion...")
        image_rec, ddim_latents = self.ddim_inversion(image_gt)
        if verbose:
            print("Null-text optimization...")
        unconds, pooleds = self.null_optimization(ddim_latents, num_inner_steps, early_stop_epsilon, optimize_pooled)
        return (image_gt, image_rec), ddim_latents[-1], unconds, pooleds
