"""The slider train step as one device-side sequence: 3 frozen UNet passes + 1 adapted pass + guidance loss +
backward + (all-reduce) + global-norm clip + AdamW, without a host sync and without autograd graph construction.

It is the same arithmetic, in the same order, as the reference loop body (conceptmod/textsliders/train_lora.py:
216-300 for SD-1.x; train_lora_xl.py:240-351 for SD-XL) -- the drop-in helpers in train_util.py + torch autograd give
identical results and stay available; this class only removes Python/autograd overhead from the hot loop:

    positive / neutral / negative|unconditional : predict_noise(_xl) with the adaptor off     (train_lora.py:216-252)
    target                                      : predict_noise(_xl) inside `with network`     (train_lora.py:261-273)
    loss = PromptEmbedsPair.loss(...)                                                          (prompt_util.py:134-174)
    loss.backward(); [clip_grad_norm_(0.2)]; optimizer.step()                    (train_lora_xl.py:348-350)

Data parallelism (no reference counterpart): each rank runs the step on its shard of the batch; the flat fp32
LoRA gradient is all-reduced (RCCL, sum / world) after backward and BEFORE the clip, so the clip sees the
global-batch gradient exactly as a single-GPU run of the global batch would."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import _native, parallel
from .optim import OptimSpec


def tail_backward_ok(guidance_scale: float, allowed: bool = True) -> bool:
    """The adapted pass runs the CFG-doubled batch [unconditional x B ; conditional x B] and the prediction is
    u + g (t - u), so d_eps = [(1 - g) d ; g d].  At g == 1 -- the reference trainers' value for this pass
    (T/train_lora.py:226-272, `train.cfg` = 1.0 in T/config_util.py:41) -- the first half is exactly zero and the backward
    runs on the conditional samples alone (smi_unet_backward_tail); the forward is untouched.  SMI_FULL_BACKWARD=1 keeps
    the full backward on [zeros ; d] (A/B switch)."""
    return bool(allowed) and 1.0 - float(guidance_scale) == 0.0 and os.environ.get("SMI_FULL_BACKWARD") != "1"


def _doubled(first, second, batch_size: int, dev, dt) -> torch.Tensor:
    """The reference's concat_embeddings (train_util.py:267-272), [first x B ; second x B], on the engine's device."""
    return torch.cat([first, second]).repeat_interleave(batch_size, dim=0).to(dev, dt).contiguous()


def _doubled_cond(unet, batch_size: int, first, second, first_pooled=None, pooled=None, time_ids=None) -> dict:
    """CFG-doubled conditioning of one prompt: `second` paired with `first` (the unconditional one)."""
    dt, dev = unet.dtype, unet.device
    c = {"ctx": _doubled(first, second, batch_size, dev, dt)}
    if pooled is not None:
        c["text_embeds"] = _doubled(first_pooled, pooled, batch_size, dev, dt)
        c["time_ids"] = _doubled(time_ids, time_ids, batch_size, dev, torch.float32)
    return c


class _FusedStep:
    """What the two steps share: the step's ONE message, [flat fp32 LoRA gradient | n_loss loss
    scalars] -- the losses ride on the gradient's all-reduce -- the optimiser state, the adaptor snapshot, the backward
    through the CFG mix and the all-reduce / clip / optimiser tail (AdamW, Lion or Prodigy: one native call each)."""

    def __init__(self, unet, network, scheduler, n_loss: int, lr, betas, eps, weight_decay, max_grad_norm,
                 process_group, optimizer: Optional[OptimSpec] = None):
        """`optimizer`: an optim.OptimSpec ("adamw", "lion" or "prodigy" with its hyper-parameters); None = AdamW with
        `betas`, `eps` and `weight_decay`.  The step owns the state vectors of that optimiser only."""
        self.unet, self.network, self.scheduler = unet, network, scheduler
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.pg = process_group
        flat = network.flat
        self.msg = torch.zeros(flat.numel() + n_loss, dtype=flat.dtype, device=flat.device)
        self.grad = self.msg[:flat.numel()]
        self.optimizer = OptimSpec.adamw(betas, eps, weight_decay) if optimizer is None else optimizer
        if self.optimizer.name not in ("adamw", "lion", "prodigy"):
            raise ValueError(f"the fused step has no native {self.optimizer.name} (adamw, lion, prodigy)")
        self.exp_avg = torch.zeros_like(flat)
        if self.optimizer.name in ("adamw", "prodigy"):
            self.exp_avg_sq = torch.zeros_like(flat)
        if self.optimizer.name == "prodigy":
            self.p0, self.s = torch.empty_like(flat), torch.empty_like(flat)
            self.prodigy_state = torch.zeros(_native.PRODIGY_STATE_DOUBLES, dtype=torch.float64, device=flat.device)
            self._prodigy_hyper = _native.prodigy_hyper(lr=lr, **self.optimizer.hyper)
        self.scratch = torch.empty(4096, dtype=torch.float32, device=flat.device)
        self.step_count = 0

    def _adaptor_params(self):
        """(lora_down, lora_up, multiplier) as the engine takes them, read with the adaptor switched on."""
        net = self.network
        net.__enter__()
        flat, n_down, mult = net.engine_params()
        net.__exit__(None, None, None)
        return flat[:n_down], flat[n_down:], mult

    def _backward_cfg(self, engine, d_pred: torch.Tensor, guidance_scale: float, tail_ok: bool):
        """Backward of the saved CFG-doubled pass from d_pred = d(loss)/d(u + g (t - u)); accumulates into self.grad."""
        n_down = self.network._n_down
        if tail_ok:  # g == 1: d_eps = [0 ; d_pred], the zero half is not built and not run
            engine.backward_tail(d_pred, self.grad[:n_down], self.grad[n_down:])
        else:  # d(u + g (t - u)) = (1 - g) du + g dt
            d_eps = torch.cat([d_pred * (1.0 - guidance_scale), d_pred * guidance_scale])
            engine.backward(d_eps, self.grad[:n_down], self.grad[n_down:])

    def _optimizer_tail(self, lr: Optional[float]):
        parallel.allreduce_mean_(self.msg, self.pg)  # gradient + losses in one collective; no-op on a single rank
        self.step_count += 1
        lr = self.lr if lr is None else lr
        flat, opt = self.network.flat, self.optimizer
        if opt.name == "adamw":
            _native.clip_adamw(flat, self.grad, self.exp_avg, self.exp_avg_sq, lr, self.step_count, self.scratch,
                               opt.hyper["betas"], opt.hyper["eps"], opt.hyper["weight_decay"], self.max_grad_norm)
        elif opt.name == "lion":
            _native.clip_lion(flat, self.grad, self.exp_avg, lr, self.scratch, opt.hyper["betas"],
                              opt.hyper["weight_decay"], self.max_grad_norm)
        else:  # prodigy: p0 is the parameter vector as the first step finds it; d and k live on the device
            if self.step_count == 1:
                _native.prodigy_init(flat, self.p0, self.exp_avg, self.exp_avg_sq, self.s, self.prodigy_state,
                                     opt.hyper["d0"])
            self._prodigy_hyper.lr = float(lr)
            _native.clip_prodigy(flat, self.grad, self.p0, self.exp_avg, self.exp_avg_sq, self.s, self.prodigy_state,
                                 self.scratch, self._prodigy_hyper, self.max_grad_norm)

    def prodigy_d(self) -> float:
        """Prodigy's current step-size estimate d, for logging: ONE device read (a synchronisation) -- call it where the
        trainer already waits for the loss."""
        if self.optimizer.name != "prodigy":
            raise ValueError(f"prodigy_d(): the step's optimiser is {self.optimizer.name}")
        if self.step_count == 0:
            return float(self.optimizer.hyper["d0"])
        return float(self.prodigy_state[0].item())


class SliderStep(_FusedStep):
    def __init__(self, unet, network, scheduler, *, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float = 0.0, cfg_scale: float = 1.0,
                 skip_dead_cfg_half: bool = False, process_group=None, batch_passes: bool = True,
                 dedup_uncond: bool = False, preroll_skip_dead_half: bool = True, tail_backward: bool = True,
                 optimizer: Optional[OptimSpec] = None):
        super().__init__(unet, network, scheduler, 1, lr, betas, eps, weight_decay, max_grad_norm, process_group,
                         optimizer)
        self.loss = self.msg[self.grad.numel():]
        self.cfg_scale = cfg_scale
        # With CFG scale 1 the unconditional half of the doubled batch is algebraically dead (u + 1*(t-u) == t).
        # Off by default: the reference computes it, so the headline number does too.
        self.skip_dead = bool(skip_dead_cfg_half and cfg_scale == 1.0)
        # Run the four guidance passes as ONE UNet pass (frozen samples first, adapted target samples last;
        # smi_unet_forward_batched): same per-sample arithmetic, 4x larger GEMM M, ~60 % fewer launches.
        self.batch_passes = batch_passes
        # The three frozen passes each carry the same unconditional half (same latents, timestep and "" prompt), and
        # the `unconditional` pass is that sample twice: 6B frozen samples, of which only 3B (4B with a real negative
        # prompt) are distinct.  With dedup_uncond the distinct ones run once and are shared -- bit-identical results
        # (per-sample arithmetic does not depend on batch composition: tests/test_engine_gpu.py), 8B -> 5B samples
        # per step.  Off by default: the reference runs all of them, so the headline number does too.
        self.dedup = bool(dedup_uncond and batch_passes and not self.skip_dead)
        # Pre-roll at guidance scale exactly 1 (the SD-XL trainer's default, `train.cfg` = 1.0, T/config_util.py:41,
        # T/train_lora_xl.py:66,209-231): predict_noise_xl forms u + 1 * (t - u) from the doubled batch, i.e. t up to one fp32
        # rounding (<= 6e-8 relative) -- the unconditional half only feeds that rounding.  The pre-roll then runs the
        # conditional half alone (UNet batch B instead of 2B).  Off: the doubled batch at every scale.
        self.preroll_skip_dead_half = bool(preroll_skip_dead_half) and os.environ.get("SMI_PREROLL_FULL") != "1"  # (A/B switch)
        # guidance scale exactly 1: the unconditional half of d_eps is zero, the backward skips those samples
        self.tail_backward = tail_backward_ok(cfg_scale, tail_backward) and not self.skip_dead

    # ---- conditioning for one prompt pair, laid out as the reference's concat_embeddings does (train_util.py:267-272)
    def make_conditioning(self, emb: Dict[str, torch.Tensor], batch_size: int, pooled: Optional[dict] = None,
                          time_ids: Optional[torch.Tensor] = None) -> dict:
        dt, dev = self.unet.dtype, self.unet.device
        sub = "negative" if "negative" in emb else "unconditional"
        out = {"B": batch_size, "keys": {"positive": "positive", "neutral": "neutral", "negative": sub,
                                         "target": "target"}}

        def rows(src, key):
            return src[key].repeat_interleave(batch_size, dim=0)

        def doubled(key):
            if pooled is None:
                return _doubled_cond(self.unet, batch_size, emb["unconditional"], emb[key])
            return _doubled_cond(self.unet, batch_size, emb["unconditional"], emb[key], pooled["unconditional"],
                                 pooled[key], time_ids)

        for role, key in out["keys"].items():
            if not self.skip_dead:
                out[role] = doubled(key)
                continue
            c = {"ctx": rows(emb, key).to(dev, dt).contiguous()}
            if pooled is not None:
                c["text_embeds"] = rows(pooled, key).to(dev, dt).contiguous()
                c["time_ids"] = time_ids.repeat_interleave(batch_size, dim=0).to(dev, torch.float32).contiguous()
            out[role] = c
        # the pre-roll always runs the doubled [unconditional, target] batch (guidance 3 / train.cfg there)
        out["target_full"] = doubled("target")
        order = ("positive", "neutral", "negative", "target")  # adapted (target) samples LAST
        out["all"] = {k: torch.cat([out[r][k] for r in order]).contiguous() for k in out["target"]}
        if self.dedup:
            # distinct frozen prompts, unconditional first; then the adapted pair [unconditional, target]
            uniq = ["unconditional"]
            for role in ("positive", "neutral", "negative"):
                if out["keys"][role] not in uniq:
                    uniq.append(out["keys"][role])
            out["uniq"] = uniq
            seq = uniq + ["unconditional", "target"]
            d = {"ctx": torch.cat([rows(emb, k) for k in seq]).to(dev, dt).contiguous()}
            if pooled is not None:
                d["text_embeds"] = torch.cat([rows(pooled, k) for k in seq]).to(dev, dt).contiguous()
                d["time_ids"] = torch.cat([time_ids.repeat_interleave(batch_size, dim=0)] * len(seq)).to(
                    dev, torch.float32).contiguous()
            out["dedup"] = d
        return out

    def _pass(self, engine, x, t, c, lora: bool, save: bool):
        flat, n_down, mult = self.network.engine_params()
        down = up = None
        if lora:
            down, up = flat[:n_down], flat[n_down:]
        eps = engine.forward(x, t, c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up,
                             mult if lora else 0.0, save)
        return eps if self.skip_dead else _native.cfg_combine(eps, self.cfg_scale)

    @torch.no_grad()
    def preroll(self, latents: torch.Tensor, cond: dict, total_timesteps: int, guidance_scale: float,
                start_timesteps: int = 0) -> torch.Tensor:
        """The no-grad pre-roll `diffusion(_xl)` (train_util.py:306-327, 677-708): for each of the first
        `total_timesteps` scheduler timesteps, predict_noise(_xl) with the adaptor ON at `guidance_scale` on the target
        prompt pair, then scheduler.step(...).prev_sample.  Same arithmetic as train_util.diffusion(_xl) on this
        engine, without autograd bookkeeping; returns the denoised latents (fp32)."""
        lat = latents.float()
        c = cond["target_full"]
        B = lat.shape[0]
        down, up, mult = self._adaptor_params()
        live_only = self.preroll_skip_dead_half and float(guidance_scale) == 1.0  # the conditional half alone
        if live_only:
            c = {k: v[B:].contiguous() for k, v in c.items()}  # rows [B, 2B) of concat_embeddings: the conditional ones
        for timestep in self.scheduler.timesteps[start_timesteps:total_timesteps]:
            x = self.scheduler.scale_model_input(lat if live_only else torch.cat([lat] * 2), timestep).contiguous()
            n, _, h, w = x.shape
            engine = self.unet._ensure_engine(n, h, w, c["ctx"].shape[1])
            pred = engine.forward(x, float(timestep), c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up, mult,
                                  False)
            if not live_only:
                pred = _native.cfg_combine(pred, guidance_scale)
            lat = self.scheduler.step(pred, timestep, lat).prev_sample
        return lat

    def train_step(self, denoised_latents: torch.Tensor, timestep, cond: dict, action: str, eta: float,
                   lr: Optional[float] = None) -> torch.Tensor:
        """One optimisation step; returns the loss as a 1-element device tensor (no host sync)."""
        lat = denoised_latents.float()
        if self.dedup:
            return self._train_step_dedup(lat, timestep, cond, action, eta, lr)
        x = lat if self.skip_dead else torch.cat([lat] * 2)
        x = self.scheduler.scale_model_input(x, timestep).contiguous()
        t = float(timestep)
        if self.batch_passes:
            return self._train_step_batched(x, t, cond, action, eta, lr)
        n, _, h, w = x.shape
        engine = self.unet._ensure_engine(n, h, w, cond["target"]["ctx"].shape[1])
        net = self.network
        net.__exit__(None, None, None)
        positive = self._pass(engine, x, t, cond["positive"], False, False)
        neutral = self._pass(engine, x, t, cond["neutral"], False, False)
        negative = self._pass(engine, x, t, cond["negative"], False, False)
        net.__enter__()
        target = self._pass(engine, x, t, cond["target"], True, True)
        net.__exit__(None, None, None)
        return self._finish(engine, target, positive, neutral, negative, action, eta, lr)

    def _train_step_dedup(self, lat, timestep, cond, action, eta, lr):
        uniq, c = cond["uniq"], cond["dedup"]
        B = lat.shape[0]
        nu = len(uniq)
        x = self.scheduler.scale_model_input(torch.cat([lat] * (nu + 2)), timestep).contiguous()
        _, _, h, w = x.shape
        engine = self.unet._ensure_engine((nu + 2) * B, h, w, c["ctx"].shape[1], n_adapted=2 * B)
        down, up, mult = self._adaptor_params()
        eps = engine.forward(x, float(timestep), c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up, mult, True,
                             n_adapted=2 * B)
        e = {k: eps[i * B:(i + 1) * B] for i, k in enumerate(uniq)}
        outs = [_native.cfg_combine(torch.cat([e["unconditional"], e[cond["keys"][r]]]), self.cfg_scale)
                for r in ("positive", "neutral", "negative")]
        target = _native.cfg_combine(eps[nu * B:].contiguous(), self.cfg_scale)
        return self._finish(engine, target, outs[0], outs[1], outs[2], action, eta, lr)

    def _train_step_batched(self, x, t, cond, action, eta, lr):
        n, _, h, w = x.shape
        engine = self.unet._ensure_engine(4 * n, h, w, cond["target"]["ctx"].shape[1], n_adapted=n)
        down, up, mult = self._adaptor_params()
        c = cond["all"]
        x4 = torch.cat([x] * 4)
        eps = engine.forward(x4, t, c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up, mult, True, n_adapted=n)
        outs = [eps[i * n:(i + 1) * n] for i in range(4)]
        if not self.skip_dead:
            outs = [_native.cfg_combine(e, self.cfg_scale) for e in outs]
        positive, neutral, negative, target = outs
        return self._finish(engine, target, positive, neutral, negative, action, eta, lr)

    def _finish(self, engine, target, positive, neutral, negative, action, eta, lr):
        sign_eta = eta if action == "enhance" else -eta
        if action not in ("enhance", "erase"):
            raise ValueError("action must be erase or enhance")
        dtarget = torch.empty_like(target)
        _native.slider_loss(target, positive, neutral, negative, sign_eta, self.loss, dtarget, self.scratch)
        self.grad.zero_()
        if self.skip_dead:
            n_down = self.network._n_down
            engine.backward(dtarget, self.grad[:n_down], self.grad[n_down:])
        else:
            self._backward_cfg(engine, dtarget, self.cfg_scale, self.tail_backward)
        self._optimizer_tail(lr)
        return self.loss


class ImageSliderStep(_FusedStep):
    """The image-slider step (trainscripts/imagesliders/train_lora-scale-xl.py:317-381; SD-1.x twin train_lora-scale.py:
    283-345) as one device-side sequence, without an autograd graph:

        slider +s : eps = predict_noise(_xl)(high_noised, positive prompt) -> MSE(eps, high_noise) -> backward
        slider -s : eps = predict_noise(_xl)(low_noised,  neutral prompt)  -> MSE(eps, low_noise)  -> backward
        (gradients accumulate in the flat fp32 buffer) -> all-reduce -> AdamW

    Same arithmetic and order as `train_lora_scale_xl.image_slider_step` + torch.optim.AdamW (tested against it).  The two
    sides differ in their adaptor multiplier (+s / -s); with Linear-only adaptors they still share ONE UNet pass and one
    backward through per-sample multipliers (`smi_unet_forward_multi`: twice the GEMM rows, half the launches); conv
    (c3lier) or DoRA adaptors fall back to one pass per side."""

    def __init__(self, unet, network, scheduler, *, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float = 0.0, process_group=None, one_pass: bool = True,
                 tail_backward: bool = True, optimizer: Optional[OptimSpec] = None):
        super().__init__(unet, network, scheduler, 2, lr, betas, eps, weight_decay, max_grad_norm, process_group,
                         optimizer)
        self.losses = self.msg[self.grad.numel():]  # (high side, low side); mean over ranks after the step's all-reduce
        self.one_pass = one_pass  # both sides in one UNet pass where the adaptor set allows it (see _one_pass_ok)
        self._one_pass_cached = None
        self.tail_backward = tail_backward  # at guidance scale 1 the backward skips the unconditional samples

    def make_conditioning(self, text_embeds: torch.Tensor, batch_size: int, pooled: Optional[torch.Tensor] = None,
                          time_ids: Optional[torch.Tensor] = None, uncond: Optional[torch.Tensor] = None,
                          uncond_pooled: Optional[torch.Tensor] = None) -> dict:
        """CFG-doubled conditioning of one side: the prompt paired with the unconditional one (`uncond`,
        `uncond_pooled`), as the reference does (I/train_lora-scale-xl.py:321-337, I/train_lora-scale.py:283-318); without
        them the prompt is paired with itself (the same prediction at guidance 1)."""
        return _doubled_cond(self.unet, batch_size, text_embeds if uncond is None else uncond, text_embeds,
                             pooled if uncond_pooled is None else uncond_pooled, pooled, time_ids)

    def _mse(self, idx, eps_pair, noise, guidance_scale):
        """Side `idx`: its loss slot = MSE(u + g (t - u), noise) in fp32 (I/train_lora-scale-xl.py:338); returns
        d(loss)/d(prediction)."""
        diff = _native.cfg_combine(eps_pair, guidance_scale) - noise.float()
        self.losses[idx] = (diff * diff).mean()
        return diff * (2.0 / diff.numel())

    def _side(self, idx, sign_scale, noised, noise, timestep, c, guidance_scale):
        x = self.scheduler.scale_model_input(torch.cat([noised.float()] * 2), timestep).contiguous()
        n, _, h, w = x.shape
        engine = self.unet._ensure_engine(n, h, w, c["ctx"].shape[1])
        self.network.set_lora_slider(scale=sign_scale)
        down, up, mult = self._adaptor_params()
        eps = engine.forward(x, float(timestep), c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up, mult, True)
        dpred = self._mse(idx, eps, noise, guidance_scale)
        self._backward_cfg(engine, dpred.contiguous(), guidance_scale,
                           tail_backward_ok(guidance_scale, self.tail_backward))  # accumulates

    def _one_pass_ok(self) -> bool:
        """Both sides can share ONE UNet pass (per-sample adaptor multipliers +s / -s, smi_unet_forward_multi) when every
        adaptor sits on a Linear layer: plain LoRA, no conv (c3lier) sites."""
        if self._one_pass_cached is None:
            net = self.network
            self._one_pass_cached = type(net).__name__ == "LoRANetwork" and all(
                not getattr(l, "is_conv", False) and len(l.lora_down._shape) == 2 for l in net.unet_loras)
        return self._one_pass_cached

    def _both_sides(self, scale, noised_high, noised_low, noise_high, noise_low, timestep, cond_pos, cond_neu,
                    guidance_scale):
        B = noised_high.shape[0]
        # [u_hi, u_lo, t_hi, t_lo]: both unconditional halves first, so that the samples with a non-zero output gradient
        # at guidance 1 are the tail of the batch (per-sample arithmetic does not depend on the batch position)
        x = torch.cat([noised_high.float(), noised_low.float()] * 2)
        x = self.scheduler.scale_model_input(x, timestep).contiguous()
        n, _, h, w = x.shape
        c = {k: torch.cat([cond_pos[k][:B], cond_neu[k][:B], cond_pos[k][B:], cond_neu[k][B:]]).contiguous()
             for k in cond_pos}
        engine = self.unet._ensure_engine(n, h, w, c["ctx"].shape[1])
        self.network.set_lora_slider(scale=1)
        down, up, mult = self._adaptor_params()
        mults = ([mult * scale] * B + [-mult * scale] * B) * 2
        eps = engine.forward(x, float(timestep), c["ctx"], c.get("text_embeds"), c.get("time_ids"), down, up, mults, True)
        dpreds = [self._mse(idx, torch.cat([eps[idx * B:(idx + 1) * B], eps[(2 + idx) * B:(3 + idx) * B]]), noise,
                            guidance_scale)  # this side's CFG pair
                  for idx, noise in enumerate((noise_high, noise_low))]
        self._backward_cfg(engine, torch.cat(dpreds).contiguous(), guidance_scale,
                           tail_backward_ok(guidance_scale, self.tail_backward))

    def train_step(self, noised_low, noised_high, noise_low, noise_high, timestep, cond_pos: dict, cond_neu: dict,
                   scale: float, guidance_scale: float = 1.0, lr: Optional[float] = None) -> torch.Tensor:
        """One optimisation step; returns the two side losses (high, low) as a device tensor (no host sync)."""
        self.grad.zero_()
        if self.one_pass and self._one_pass_ok():
            self._both_sides(scale, noised_high, noised_low, noise_high, noise_low, timestep, cond_pos, cond_neu,
                             guidance_scale)
        else:
            self._side(0, +scale, noised_high, noise_high, timestep, cond_pos, guidance_scale)
            self._side(1, -scale, noised_low, noise_low, timestep, cond_neu, guidance_scale)
        self.network.set_lora_slider(scale=1)
        self._optimizer_tail(lr)
        return self.losses
