"""Flux transformer (diffusers `FluxTransformer2DModel`: FLUX.1-schnell / dev) as a parameter container on the HIP engine.

The module tree carries diffusers' state-dict names (`x_embedder`, `context_embedder`, `time_text_embed.{timestep_embedder,
guidance_embedder,text_embedder}`, `transformer_blocks.<i>.{norm1,norm1_context}.linear`, `.attn.{to_q,to_k,to_v,to_out.0,
add_q_proj,add_k_proj,add_v_proj,to_add_out,norm_q,norm_k,norm_added_q,norm_added_k}`, `.ff`, `.ff_context`,
`single_transformer_blocks.<i>.{norm.linear,attn.{to_q,to_k,to_v,norm_q,norm_k},proj_mlp,proj_out}`, `norm_out.linear`,
`proj_out`); the attention class is called `Attention`, so `lora.select_targets` finds it as the reference's
`target_replace=["Attention"]` does (conceptmod/textsliders/train_lora_flux.py).  No arithmetic happens here: `forward` runs
csrc/engine_flux.hip.  With grad enabled and an attached network whose flat parameter requires grad, the call goes through
`_FluxFn`: the trainable engine saves the pass and its backward gives the gradient to that parameter (train_lora_flux);
nothing else is differentiated.

`forward` takes UN-packed NCHW latents: the engine packs ([n, 16, h, w] -> [n, (h/2)(w/2), 64], columns (c, py, px), which
is the pipeline's `_pack_latents`), builds the rotary table from (h, w, context length) itself, and un-packs its output;
`txt_ids` / `img_ids` are accepted and ignored."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin
from .mmdit import TransformerOutput, _AdaNorm, _FeedForward, _TwoLinear


@dataclass
class FluxConfig:
    patch_size: int = 2  # (diffusers' config says 1 and leaves the 2 x 2 pack to the pipeline; here the pack is the model's)
    in_channels: int = 16  # latent channels: the packed width is in_channels x patch_size^2 = 64
    num_layers: int = 19
    num_single_layers: int = 38
    num_attention_heads: int = 24
    attention_head_dim: int = 128
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 768
    guidance_embeds: bool = False
    axes_dims_rope: tuple = (16, 56, 56)
    rope_theta: float = 10000.0

    @property
    def inner_dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    @property
    def out_channels(self) -> int:
        return self.in_channels


def flux_schnell_config() -> FluxConfig:  # black-forest-labs/FLUX.1-schnell transformer/config.json
    return FluxConfig()


def flux_dev_config() -> FluxConfig:  # black-forest-labs/FLUX.1-dev: the same network with a guidance embedder
    return FluxConfig(guidance_embeds=True)


def tiny_flux_config(guidance_embeds: bool = False) -> FluxConfig:
    """d 128 (2 heads x 64, rotary axes (16, 24, 24)), two double and two single blocks, joint 64, pooled 32."""
    return FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, attention_head_dim=64,
                      joint_attention_dim=64, pooled_projection_dim=32, axes_dims_rope=(16, 24, 24),
                      guidance_embeds=guidance_embeds)


class _RMSNorm(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))


class Attention(nn.Module):
    """diffusers' Attention as Flux builds it: parameters only, in diffusers' declaration order.  A double block's has the
    added (context) projections and both output projections; a single block's (`pre_only`) has q, k, v and their norms."""

    def __init__(self, d: int, head_dim: int, single: bool):
        super().__init__()
        self.norm_q, self.norm_k = _RMSNorm(head_dim), _RMSNorm(head_dim)
        self.to_q, self.to_k, self.to_v = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        if not single:
            self.add_k_proj, self.add_v_proj, self.add_q_proj = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
            self.to_out = nn.ModuleList([nn.Linear(d, d), nn.Dropout(0.0)])
            self.to_add_out = nn.Linear(d, d)
            self.norm_added_q, self.norm_added_k = _RMSNorm(head_dim), _RMSNorm(head_dim)


class FluxTransformerBlock(nn.Module):
    def __init__(self, d: int, head_dim: int):
        super().__init__()
        self.norm1 = _AdaNorm(d, 6)
        self.norm1_context = _AdaNorm(d, 6)
        self.attn = Attention(d, head_dim, single=False)
        self.ff = _FeedForward(d)
        self.ff_context = _FeedForward(d)


class FluxSingleTransformerBlock(nn.Module):
    def __init__(self, d: int, head_dim: int):
        super().__init__()
        self.norm = _AdaNorm(d, 3)
        self.proj_mlp = nn.Linear(d, 4 * d)
        self.proj_out = nn.Linear(5 * d, d)
        self.attn = Attention(d, head_dim, single=True)


class _TimeTextEmbed(nn.Module):
    def __init__(self, cfg: FluxConfig):
        super().__init__()
        self.timestep_embedder = _TwoLinear(256, cfg.inner_dim)
        if cfg.guidance_embeds:
            self.guidance_embedder = _TwoLinear(256, cfg.inner_dim)
        self.text_embedder = _TwoLinear(cfg.pooled_projection_dim, cfg.inner_dim)


def engine_config_c(cfg: FluxConfig, dtype: torch.dtype, context_len: int) -> _native.FluxConfigC:
    c = _native.FluxConfigC()
    c.dtype = _native.DTYPE_CODE[dtype]
    c.in_channels, c.patch_size = cfg.in_channels, cfg.patch_size
    c.num_layers, c.num_single_layers = cfg.num_layers, cfg.num_single_layers
    c.num_heads, c.attention_head_dim = cfg.num_attention_heads, cfg.attention_head_dim
    c.joint_attention_dim, c.pooled_projection_dim = cfg.joint_attention_dim, cfg.pooled_projection_dim
    c.guidance_embeds = int(bool(cfg.guidance_embeds))
    axes = tuple(cfg.axes_dims_rope)
    if len(axes) != 3:
        raise _native.SmiError(f"axes_dims_rope {axes}: three axes (a constant one, rows, columns)")
    for i in range(3):
        c.axes_dims_rope[i] = int(axes[i])
    c.context_len, c.rope_theta = context_len, float(cfg.rope_theta)
    return c


def workspace_bytes(cfg: FluxConfig, dtype: torch.dtype, sites: Sequence[dict], batch: int, h: int, w: int,
                    context_len: int) -> int:
    """smi_flux_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused config, site or shape."""
    arr, _keep = _native.make_sites(sites)
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_flux_workspace_bytes(C.byref(engine_config_c(cfg, dtype, context_len)), arr,
                                                         len(sites), batch, h, w, C.byref(out)),
                  "smi_flux_workspace_bytes")
    return out.value


def train_workspace_bytes(cfg: FluxConfig, dtype: torch.dtype, sites: Sequence[dict], batch: int, h: int, w: int,
                          context_len: int) -> int:
    """smi_flux_train_workspace_bytes: the host-only dry forward + saved forward + backward of a trainable engine."""
    arr, _keep = _native.make_sites(sites)
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_flux_train_workspace_bytes(C.byref(engine_config_c(cfg, dtype, context_len)), arr,
                                                               len(sites), batch, h, w, C.byref(out)),
                  "smi_flux_train_workspace_bytes")
    return out.value


class FluxEngine(_native._EngineBase):
    """Flux transformer on the HIP engine for one latent size and context length (smi_flux_*): the forward with Linear LoRA
    sites at one multiplier per sample; `trainable=True` (smi_flux_train_*): also `forward_save` and `backward`, the gradient
    of the output to the LoRA parameters."""

    def __init__(self, cfg: FluxConfig, dtype: torch.dtype, state: dict, sites: Sequence[dict], batch: int, h: int,
                 w: int, context_len: int, device, trainable: bool = False):
        self.cfg, self.dtype, self.batch, self.h, self.w, self.context_len = cfg, dtype, batch, h, w, context_len
        self.trainable = trainable
        self.cfg_c = engine_config_c(cfg, dtype, context_len)
        arr, self._site_keep = _native.make_sites(sites)
        out = C.c_size_t(0)
        lib = _native.lib()
        size_fn, create_fn, name = ((lib.smi_flux_train_workspace_bytes, lib.smi_flux_train_create, "smi_flux_train")
                                    if trainable else (lib.smi_flux_workspace_bytes, lib.smi_flux_create, "smi_flux"))
        _native.check(size_fn(C.byref(self.cfg_c), arr, len(sites), batch, h, w, C.byref(out)), name + "_workspace_bytes")
        self.workspace_bytes = out.value
        self.workspace = torch.empty(out.value, dtype=torch.uint8, device=device)
        warr, self._keep = _native._weight_table(state, dtype, self.workspace.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.workspace.device):
            _native.check(create_fn(C.byref(self.cfg_c), warr, len(state), arr, len(sites), batch, h, w,
                                    _native.ptr(self.workspace), out.value, _native.stream_ptr(), C.byref(handle)),
                          name + "_create")
        self.handle = handle
        self._borrowed = None  # the operands of the saved pass: the engine reads the LoRA parameters again in its backward

    def forward_save(self, sample, timesteps, guidance, ctx, pooled, lora_down, lora_up, multipliers, out=None) -> torch.Tensor:
        """`forward`, with the pass kept for one `backward` (smi_flux_forward_save): the same bits in the output."""
        return self.forward(sample, timesteps, guidance, ctx, pooled, lora_down, lora_up, multipliers, out, save=True)

    def backward(self, d_out: torch.Tensor, d_down: Optional[torch.Tensor], d_up: Optional[torch.Tensor]) -> None:
        """smi_flux_backward: d_out f32 [n, 16, h, w]; the LoRA gradients are ADDED to d_down / d_up (f32, flat layout).
        Consumes the saved pass (SmiError without one)."""
        d_out = d_out.to(self.workspace.device, torch.float32).contiguous()
        with torch.cuda.device(self.workspace.device):
            rc = _native.lib().smi_flux_backward(self.handle, _native.ptr(d_out), _native.ptr(d_down), _native.ptr(d_up))
        self._borrowed = None
        _native.check(rc, "smi_flux_backward")

    def forward(self, sample: torch.Tensor, timesteps, guidance, ctx: torch.Tensor, pooled: torch.Tensor,
                lora_down: Optional[torch.Tensor] = None, lora_up: Optional[torch.Tensor] = None,
                multipliers: Optional[Sequence[float]] = None, out: Optional[torch.Tensor] = None,
                save: bool = False) -> torch.Tensor:
        """sample [n, 16, h, w] -> f32 [n, 16, h, w].  timesteps: n floats (the scheduler's 1000 sigma), on the host;
        guidance: n floats for a guidance_embeds model, None for one without."""
        n = sample.shape[0]
        cfg, dev = self.cfg, self.workspace.device
        if tuple(sample.shape[1:]) != (cfg.in_channels, self.h, self.w):
            raise _native.SmiError(f"sample {tuple(sample.shape)} does not match the engine's {self.h}x{self.w} latent")
        if tuple(ctx.shape) != (n, self.context_len, cfg.joint_attention_dim):
            raise _native.SmiError(f"encoder_hidden_states {tuple(ctx.shape)}: expected "
                                   f"{(n, self.context_len, cfg.joint_attention_dim)}")
        if tuple(pooled.shape) != (n, cfg.pooled_projection_dim):
            raise _native.SmiError(f"pooled_projections {tuple(pooled.shape)}: expected {(n, cfg.pooled_projection_dim)}")
        ts = [float(t) for t in timesteps]
        if len(ts) != n:
            raise _native.SmiError(f"{len(ts)} timesteps for {n} samples")
        garr = None
        if guidance is not None:
            gs = [float(g) for g in guidance]
            if len(gs) != n:
                raise _native.SmiError(f"{len(gs)} guidance values for {n} samples")
            garr = (C.c_float * n)(*gs)
        if multipliers is not None and len(multipliers) != n:
            raise _native.SmiError(f"{len(multipliers)} multipliers for {n} samples")
        sample = sample.to(dev, torch.float32).contiguous()
        ctx, pooled = ctx.to(dev, self.dtype).contiguous(), pooled.to(dev, self.dtype).contiguous()
        if out is None:
            out = torch.empty((n, cfg.in_channels, self.h, self.w), dtype=torch.float32, device=dev)
        tarr = (C.c_float * n)(*ts)
        marr = None if multipliers is None else (C.c_float * n)(*[float(m) for m in multipliers])
        fn, name = ((_native.lib().smi_flux_forward_save, "smi_flux_forward_save") if save
                    else (_native.lib().smi_flux_forward, "smi_flux_forward"))
        with torch.cuda.device(dev):
            _native.check(fn(self.handle, n, _native.ptr(sample), tarr, garr, _native.ptr(ctx), _native.ptr(pooled),
                             _native.ptr(lora_down), _native.ptr(lora_up), marr, _native.ptr(out)), name)
        if save:
            self._borrowed = (lora_down, lora_up)
        return out


class _FluxFn(torch.autograd.Function):
    """Autograd bookkeeping only: forward and backward are single calls into the trainable engine.  The one differentiable
    input is the network's flat parameter."""

    @staticmethod
    def forward(ctx, engine, flat, n_down, sample, ts, gs, ehs, pooled, multipliers):
        flat_d = flat.detach()
        out = engine.forward_save(sample, ts, gs, ehs, pooled, flat_d[:n_down], flat_d[n_down:], multipliers)
        ctx.engine, ctx.n_down, ctx.flat = engine, n_down, flat_d
        engine._saved_by = ctx
        return out

    @staticmethod
    def backward(ctx, d_out):
        if getattr(ctx.engine, "_saved_by", None) is not ctx:
            raise _native.SmiError(
                "backward through a Flux transformer output whose saved activations are gone: the engine keeps the pass of "
                "the LAST grad-enabled forward only (a later grad-enabled forward or a previous backward released it)")
        ctx.engine._saved_by = None
        g = torch.zeros_like(ctx.flat)
        ctx.engine.backward(d_out, g[:ctx.n_down], g[ctx.n_down:])
        return None, g, None, None, None, None, None, None, None


def _per_sample(v, n):
    if torch.is_tensor(v):
        v = v.detach().float().cpu().reshape(-1).tolist()
    v = list(v) if isinstance(v, (list, tuple)) else [float(v)]
    return v * n if len(v) == 1 else v


class FluxTransformer2DModel(EngineCacheMixin, nn.Module):
    _component, _handle = "Flux transformer", "transformer"

    def __init__(self, cfg: FluxConfig):
        super().__init__()
        self.config = self.cfg = cfg
        d, hd = cfg.inner_dim, cfg.attention_head_dim
        self.time_text_embed = _TimeTextEmbed(cfg)
        self.context_embedder = nn.Linear(cfg.joint_attention_dim, d)
        self.x_embedder = nn.Linear(cfg.in_channels * cfg.patch_size ** 2, d)
        self.transformer_blocks = nn.ModuleList([FluxTransformerBlock(d, hd) for _ in range(cfg.num_layers)])
        self.single_transformer_blocks = nn.ModuleList(
            [FluxSingleTransformerBlock(d, hd) for _ in range(cfg.num_single_layers)])
        self.norm_out = _AdaNorm(d, 2)
        self.proj_out = nn.Linear(d, cfg.patch_size ** 2 * cfg.out_channels)
        self._engines = {}

    @property
    def dtype(self):
        return self.proj_out.weight.dtype

    @property
    def device(self):
        return self.proj_out.weight.device

    def _sites(self):
        net = self.__dict__.get("_lora_network")
        return net.engine_sites() if net is not None and net.unet_loras else []

    def _new_engine(self, state, n, h, w, context_len, trainable, _net_id):
        return FluxEngine(self.cfg, self.dtype, state, self._sites(), max(n, 1), h, w, context_len, self.device,
                          trainable=trainable)

    def engine(self, n: int, h: int, w: int, context_len: int, trainable: bool = False) -> FluxEngine:
        """The engine for this latent size and context length, with the attached network's sites (fixed at creation: an engine
        built for another network is closed first).  trainable: the engine that saves a pass and differentiates it."""
        net = self.__dict__.get("_lora_network")
        for key, e in list(self._engines.items()):
            if key[-1] != id(net):
                e.close()
                del self._engines[key]
        return self._engine(n, h, w, context_len, trainable, id(net))

    def forward(self, hidden_states, timestep, guidance=None, pooled_projections=None, encoder_hidden_states=None,
                txt_ids=None, img_ids=None, multipliers=None, return_dict: bool = True, **_):
        """diffusers' call on un-packed latents [n, 16, h, w].  `timestep`: a number or n of them, the scheduler's 1000 sigma
        (the reference passes timestep / 1000 to a model that multiplies by 1000); `guidance`: the embedded guidance scale
        of a guidance_embeds model (a number or n), ignored by a model without the embedder.  An attached LoRANetwork runs at
        its current multiplier (0 outside `with network:`) on every sample, or at `multipliers` (one per sample).  With grad
        enabled and a network whose parameter requires grad, the pass is saved and the output carries the gradient to that
        parameter."""
        n, _c, h, w = hidden_states.shape
        ts = _per_sample(timestep, n)
        gs = None
        if self.cfg.guidance_embeds:
            if guidance is None:
                raise _native.SmiError("this Flux transformer has guidance_embeds: pass guidance (FLUX.1-dev's default is 3.5)")
            gs = _per_sample(guidance, n)
        net = self.__dict__.get("_lora_network")
        down = up = None
        hidden_states, encoder_hidden_states = hidden_states.detach(), encoder_hidden_states.detach()
        pooled_projections = pooled_projections.detach()
        if net is not None and net.unet_loras:
            flat, n_down, mult = net.engine_params()
            if multipliers is None:
                multipliers = [mult] * n
            if torch.is_grad_enabled() and flat.requires_grad:
                e = self.engine(n, h, w, encoder_hidden_states.shape[1], trainable=True)
                out = _FluxFn.apply(e, flat, n_down, hidden_states, ts, gs, encoder_hidden_states, pooled_projections,
                                    [float(m) for m in multipliers])
                return TransformerOutput(out) if return_dict else (out,)
            flat = flat.detach()
            down, up = flat[:n_down], flat[n_down:]
        else:
            multipliers = None
        e = self.engine(n, h, w, encoder_hidden_states.shape[1])
        with torch.no_grad():
            out = e.forward(hidden_states, ts, gs, encoder_hidden_states, pooled_projections, down, up, multipliers)
        return TransformerOutput(out) if return_dict else (out,)


def init_synthetic_(model: FluxTransformer2DModel, seed: int = 0) -> FluxTransformer2DModel:
    """Seeded weights under which every term of the forward counts: matrices N / sqrt(fan_in) (x 0.8), so activations keep
    unit scale; the modulation Linears (norm1, norm1_context, the single blocks' norm, norm_out) N x 0.5 / sqrt(d) with
    biases 0.3 N, so that scales, shifts and gates come out of order 0.1 to 1 (a zero init would hide a dropped gate); the
    RMSNorm weights uniform in 0.5 .. 1.5 (ones would hide a dropped or swapped one); other biases 0.1 N.  The generator is
    the parameters' device's: the same seed gives other values on the CPU than on a GPU."""
    dev = model.proj_out.weight.device  # drawn where the parameters live: a model on the GPU is filled there, in milliseconds
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            mod = (".norm1.linear" in name or ".norm1_context.linear" in name or ".norm.linear" in name
                   or name.startswith("norm_out.linear"))
            if ".attn.norm_" in name:
                p.copy_(0.5 + torch.rand(p.shape, generator=g, device=dev))
            elif p.ndim >= 2:  # (drawn in place: the full-width blocks hold half a billion parameters)
                p.normal_(0.0, (0.5 if mod else 0.8) / p[0].numel() ** 0.5, generator=g)
            else:
                p.normal_(0.0, 0.3 if mod else 0.1, generator=g)
    return model
