"""SD3 MMDiT (diffusers `SD3Transformer2DModel`, SD3-medium's family) as a parameter container on the HIP engine.

The module tree carries diffusers' state-dict names (`pos_embed.proj`, `pos_embed.pos_embed`, `context_embedder`,
`time_text_embed.*`, `transformer_blocks.<i>.{norm1,norm1_context}.linear`, `.attn.{to_q,to_k,to_v,to_out.0,add_q_proj,
add_k_proj,add_v_proj,to_add_out}`, `.ff`, `.ff_context`, `norm_out.linear`, `proj_out`); the attention class is called
`Attention`, so `lora.select_targets` finds it as the reference's `target_replace=["Attention"]` does
(conceptmod/textsliders/train_lora_sd3.py).  No arithmetic happens here: `forward` runs csrc/engine_mmdit.hip.

With grad enabled and a LoRANetwork attached, `forward` goes through a trainable engine (smi_mmdit_train_create) and an
autograd Function whose backward is the engine's: gradients reach the network's flat parameter and nothing else.
SD3.5's qk-norm and dual attention are not built (the engine refuses them by name)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin


@dataclass
class SD3Config:
    patch_size: int = 2
    in_channels: int = 16
    out_channels: int = 16
    num_layers: int = 24
    num_attention_heads: int = 24
    attention_head_dim: int = 64
    joint_attention_dim: int = 4096
    pooled_projection_dim: int = 2048
    pos_embed_max_size: int = 192
    sample_size: int = 128
    dual_attention_layers: tuple = ()
    qk_norm: Optional[str] = None

    @property
    def inner_dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim


def sd3_medium_config() -> SD3Config:  # stabilityai/stable-diffusion-3-medium-diffusers transformer/config.json
    return SD3Config()


def tiny_sd3_config() -> SD3Config:
    """d 128, two layers (a full block and the context_pre_only block), joint 64, pooled 64, an 8 x 8 position table."""
    return SD3Config(num_layers=2, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=64,
                     pos_embed_max_size=8, sample_size=16)


class Attention(nn.Module):
    """The joint attention's projections (diffusers Attention with added_kv_proj_dim): parameters only.  Declaration order
    is diffusers' (to_q, to_k, to_v, add_k_proj, add_v_proj, add_q_proj, to_out, to_add_out)."""

    def __init__(self, d: int, context_pre_only: bool):
        super().__init__()
        self.to_q, self.to_k, self.to_v = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.add_k_proj, self.add_v_proj, self.add_q_proj = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.to_out = nn.ModuleList([nn.Linear(d, d), nn.Dropout(0.0)])
        if not context_pre_only:
            self.to_add_out = nn.Linear(d, d)


class _AdaNorm(nn.Module):
    def __init__(self, d: int, chunks: int):
        super().__init__()
        self.linear = nn.Linear(d, chunks * d)


class _Proj(nn.Module):
    def __init__(self, d_in: int, d_out: int):
        super().__init__()
        self.proj = nn.Linear(d_in, d_out)


class _FeedForward(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.net = nn.ModuleList([_Proj(d, 4 * d), nn.Dropout(0.0), nn.Linear(4 * d, d)])


class JointTransformerBlock(nn.Module):
    def __init__(self, d: int, context_pre_only: bool):
        super().__init__()
        self.norm1 = _AdaNorm(d, 6)
        self.norm1_context = _AdaNorm(d, 2 if context_pre_only else 6)
        self.attn = Attention(d, context_pre_only)
        self.ff = _FeedForward(d)
        if not context_pre_only:
            self.ff_context = _FeedForward(d)


class _PatchEmbed(nn.Module):
    def __init__(self, cfg: SD3Config):
        super().__init__()
        self.proj = nn.Conv2d(cfg.in_channels, cfg.inner_dim, cfg.patch_size, cfg.patch_size)
        # a persistent buffer in diffusers: it arrives with the weights
        self.register_buffer("pos_embed", torch.zeros(1, cfg.pos_embed_max_size ** 2, cfg.inner_dim))


class _TwoLinear(nn.Module):
    def __init__(self, d_in: int, d: int):
        super().__init__()
        self.linear_1, self.linear_2 = nn.Linear(d_in, d), nn.Linear(d, d)


class _TimeTextEmbed(nn.Module):
    def __init__(self, cfg: SD3Config):
        super().__init__()
        self.timestep_embedder = _TwoLinear(256, cfg.inner_dim)
        self.text_embedder = _TwoLinear(cfg.pooled_projection_dim, cfg.inner_dim)


class TransformerOutput:
    def __init__(self, sample):
        self.sample = sample

    def __getitem__(self, i):
        return (self.sample,)[i]


def engine_config_c(cfg: SD3Config, dtype: torch.dtype, context_len: int) -> _native.MMDiTConfigC:
    c = _native.MMDiTConfigC()
    c.dtype = _native.DTYPE_CODE[dtype]
    c.patch_size, c.in_channels, c.out_channels = cfg.patch_size, cfg.in_channels, cfg.out_channels
    c.num_layers, c.num_heads, c.attention_head_dim = cfg.num_layers, cfg.num_attention_heads, cfg.attention_head_dim
    c.joint_attention_dim, c.pooled_projection_dim = cfg.joint_attention_dim, cfg.pooled_projection_dim
    c.pos_embed_max_size, c.context_len = cfg.pos_embed_max_size, context_len
    c.dual_attention_layers = len(cfg.dual_attention_layers or ())
    c.qk_norm = 0 if cfg.qk_norm in (None, "", "none") else 1
    return c


def workspace_bytes(cfg: SD3Config, dtype: torch.dtype, sites: Sequence[dict], batch: int, h: int, w: int,
                    context_len: int) -> int:
    """smi_mmdit_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused config, site or shape."""
    arr, _keep = _native.make_sites(sites)
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_mmdit_workspace_bytes(C.byref(engine_config_c(cfg, dtype, context_len)), arr,
                                                          len(sites), batch, h, w, C.byref(out)),
                  "smi_mmdit_workspace_bytes")
    return out.value


def train_workspace_bytes(cfg: SD3Config, dtype: torch.dtype, sites: Sequence[dict], batch: int, h: int, w: int,
                          context_len: int) -> int:
    """smi_mmdit_train_workspace_bytes: the host-only dry forward + backward of a trainable engine."""
    arr, _keep = _native.make_sites(sites)
    out = C.c_size_t(0)
    _native.check(_native.lib().smi_mmdit_train_workspace_bytes(C.byref(engine_config_c(cfg, dtype, context_len)), arr,
                                                                len(sites), batch, h, w, C.byref(out)),
                  "smi_mmdit_train_workspace_bytes")
    return out.value


class MMDiTEngine(_native._EngineBase):
    """SD3 MMDiT on the HIP engine for one latent size and context length (smi_mmdit_*): the forward with Linear LoRA
    sites at one multiplier per sample; `trainable=True` (smi_mmdit_train_*): also `forward_save` and `backward`, the
    gradient of the output to the LoRA parameters."""

    def __init__(self, cfg: SD3Config, dtype: torch.dtype, state: dict, sites: Sequence[dict], batch: int, h: int,
                 w: int, context_len: int, device, trainable: bool = False):
        self.cfg, self.dtype, self.batch, self.h, self.w, self.context_len = cfg, dtype, batch, h, w, context_len
        self.trainable = trainable
        self.cfg_c = engine_config_c(cfg, dtype, context_len)
        arr, self._site_keep = _native.make_sites(sites)
        out = C.c_size_t(0)
        lib = _native.lib()
        size_fn, create_fn, name = ((lib.smi_mmdit_train_workspace_bytes, lib.smi_mmdit_train_create, "smi_mmdit_train")
                                    if trainable else (lib.smi_mmdit_workspace_bytes, lib.smi_mmdit_create, "smi_mmdit"))
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

    def forward_save(self, sample, timesteps, ctx, pooled, lora_down, lora_up, multipliers, out=None) -> torch.Tensor:
        """`forward`, with the pass kept for one `backward` (smi_mmdit_forward_save): the same bits in the output."""
        return self.forward(sample, timesteps, ctx, pooled, lora_down, lora_up, multipliers, out, save=True)

    def backward(self, d_out: torch.Tensor, d_down: Optional[torch.Tensor], d_up: Optional[torch.Tensor]) -> None:
        """smi_mmdit_backward: d_out f32 [n, Cout, h, w]; the LoRA gradients are ADDED to d_down / d_up (f32, flat layout).
        Consumes the saved pass (SmiError without one)."""
        d_out = d_out.to(self.workspace.device, torch.float32).contiguous()
        with torch.cuda.device(self.workspace.device):
            rc = _native.lib().smi_mmdit_backward(self.handle, _native.ptr(d_out), _native.ptr(d_down), _native.ptr(d_up))
        self._borrowed = None
        _native.check(rc, "smi_mmdit_backward")

    def forward(self, sample: torch.Tensor, timesteps, ctx: torch.Tensor, pooled: torch.Tensor,
                lora_down: Optional[torch.Tensor] = None, lora_up: Optional[torch.Tensor] = None,
                multipliers: Optional[Sequence[float]] = None, out: Optional[torch.Tensor] = None,
                save: bool = False) -> torch.Tensor:
        """sample [n, Cin, h, w] -> f32 [n, Cout, h, w].  timesteps: n floats (the scheduler's 1000 sigma), on the host."""
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
        if multipliers is not None and len(multipliers) != n:
            raise _native.SmiError(f"{len(multipliers)} multipliers for {n} samples")
        sample = sample.to(dev, torch.float32).contiguous()
        ctx, pooled = ctx.to(dev, self.dtype).contiguous(), pooled.to(dev, self.dtype).contiguous()
        if out is None:
            out = torch.empty((n, cfg.out_channels, self.h, self.w), dtype=torch.float32, device=dev)
        tarr = (C.c_float * n)(*ts)
        marr = None if multipliers is None else (C.c_float * n)(*[float(m) for m in multipliers])
        fn, name = ((_native.lib().smi_mmdit_forward_save, "smi_mmdit_forward_save") if save
                    else (_native.lib().smi_mmdit_forward, "smi_mmdit_forward"))
        with torch.cuda.device(dev):
            _native.check(fn(self.handle, n, _native.ptr(sample), tarr, _native.ptr(ctx), _native.ptr(pooled),
                             _native.ptr(lora_down), _native.ptr(lora_up), marr, _native.ptr(out)), name)
        if save:
            self._borrowed = (lora_down, lora_up)
        return out


class _MMDiTFn(torch.autograd.Function):
    """Autograd bookkeeping only: forward and backward are single calls into the trainable engine.  The one differentiable
    input is the network's flat parameter."""

    @staticmethod
    def forward(ctx, engine, flat, n_down, sample, ts, ehs, pooled, multipliers):
        flat_d = flat.detach()
        out = engine.forward_save(sample, ts, ehs, pooled, flat_d[:n_down], flat_d[n_down:], multipliers)
        ctx.engine, ctx.n_down, ctx.flat = engine, n_down, flat_d
        engine._saved_by = ctx
        return out

    @staticmethod
    def backward(ctx, d_out):
        if getattr(ctx.engine, "_saved_by", None) is not ctx:
            raise _native.SmiError(
                "backward through an SD3 transformer output whose saved activations are gone: the engine keeps the pass of "
                "the LAST grad-enabled forward only (a later grad-enabled forward or a previous backward released it)")
        ctx.engine._saved_by = None
        g = torch.zeros_like(ctx.flat)
        ctx.engine.backward(d_out, g[:ctx.n_down], g[ctx.n_down:])
        return None, g, None, None, None, None, None, None


class SD3Transformer2DModel(EngineCacheMixin, nn.Module):
    _component, _handle = "SD3 transformer", "transformer"

    def __init__(self, cfg: SD3Config):
        super().__init__()
        self.config = self.cfg = cfg
        d = cfg.inner_dim
        self.pos_embed = _PatchEmbed(cfg)
        self.time_text_embed = _TimeTextEmbed(cfg)
        self.context_embedder = nn.Linear(cfg.joint_attention_dim, d)
        self.transformer_blocks = nn.ModuleList(
            [JointTransformerBlock(d, context_pre_only=i == cfg.num_layers - 1) for i in range(cfg.num_layers)])
        self.norm_out = _AdaNorm(d, 2)
        self.proj_out = nn.Linear(d, cfg.patch_size * cfg.patch_size * cfg.out_channels)
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
        return MMDiTEngine(self.cfg, self.dtype, state, self._sites(), max(n, 1), h, w, context_len, self.device,
                           trainable=trainable)

    def engine(self, n: int, h: int, w: int, context_len: int, trainable: bool = False) -> MMDiTEngine:
        """The engine for this latent size and context length, with the attached network's sites (fixed at creation: an engine
        built for another network is closed first).  trainable: the engine that saves a pass and differentiates it."""
        net = self.__dict__.get("_lora_network")
        for key, e in list(self._engines.items()):
            if key[-1] != id(net):
                e.close()
                del self._engines[key]
        return self._engine(n, h, w, context_len, trainable, id(net))

    def forward(self, hidden_states, timestep, encoder_hidden_states, pooled_projections, multipliers=None,
                return_dict: bool = True, **_):
        """diffusers' call.  `timestep`: a number or n of them.  An attached LoRANetwork runs at its current multiplier
        (0 outside `with network:`) on every sample, or at `multipliers` (one per sample).  With grad enabled and a network
        whose parameter requires grad, the pass is saved and the output carries the gradient to that parameter."""
        n, _c, h, w = hidden_states.shape
        if torch.is_tensor(timestep):
            timestep = timestep.detach().float().cpu().reshape(-1).tolist()
        ts = list(timestep) if isinstance(timestep, (list, tuple)) else [float(timestep)]
        ts = ts * n if len(ts) == 1 else ts
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
                out = _MMDiTFn.apply(e, flat, n_down, hidden_states, ts, encoder_hidden_states, pooled_projections,
                                     [float(m) for m in multipliers])
                return TransformerOutput(out) if return_dict else (out,)
            flat = flat.detach()
            down, up = flat[:n_down], flat[n_down:]
        else:
            multipliers = None
        e = self.engine(n, h, w, encoder_hidden_states.shape[1])
        with torch.no_grad():
            out = e.forward(hidden_states, ts, encoder_hidden_states, pooled_projections, down, up, multipliers)
        return TransformerOutput(out) if return_dict else (out,)


def init_synthetic_(model: SD3Transformer2DModel, seed: int = 0) -> SD3Transformer2DModel:
    """Seeded weights under which every term of the forward counts: matrices N / sqrt(fan_in) (x 0.8), so activations keep
    unit scale; the modulation Linears (norm1, norm1_context, norm_out) N x 0.5 / sqrt(d) with biases 0.3 N, so that with
    |silu(temb)| of order 0.5 the scales, shifts and gates come out of order 0.1 to 1 (adaLN-ZERO's zero init would hide a
    dropped gate); the position table 0.5 N; other biases 0.1 N."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            mod = ".norm1.linear" in name or ".norm1_context.linear" in name or name.startswith("norm_out.linear")
            if p.ndim >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * ((0.5 if mod else 0.8) / fan_in ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 if mod else 0.1))
        model.pos_embed.pos_embed.copy_(0.5 * torch.randn(model.pos_embed.pos_embed.shape, generator=g))
    return model
