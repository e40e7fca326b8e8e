"""CLIP text encoders for the prompt front end -- drop-ins for `transformers.CLIPTextModel` (SD-1.x; SD-XL encoder 1)
and `CLIPTextModelWithProjection` (SD-XL encoder 2) as the reference calls them:
    text_encoder(tokens)[0]                                             (conceptmod/textsliders/train_util.py:119-120)
    out = text_encoder(tokens, output_hidden_states=True); out[0]; out.hidden_states[-2]          (train_util.py:139-144)
They are parameter containers with the transformers parameter names (a transformers state dict loads by key); the
arithmetic runs in the HIP engine (csrc/engine.hip `forward_clip`: fused causal attention, LayerNorm, GEMM kernels).  No
PyTorch forward: without the HIP library, or on a CPU device, a call raises.  Tokenisation stays host text processing
(`transformers.CLIPTokenizer`).  A `lora.LoRANetwork` built on a text encoder (the no-trigger trainer,
conceptmod/notrigger/train_notrigger.py:204-213) attaches itself: the forward then runs under the adaptor at the network's
multiplier, and `notrigger.TextEncoderStep` differentiates it (csrc/engine_clip.hip `smi_clip_forward_lora` / `smi_clip_backward`).

The image tower and the joint model -- `CLIPVisionModelWithProjection` and `CLIPModel`, what eval-scripts/clip_score.py
scores a slider sweep with -- are containers of the same kind (csrc/engine.hip `forward_clip_vision`, csrc/clip_vision.hip).
The image front end stays on the host up to the uint8 crop (`clip_image_preprocess`: PIL's antialiased bicubic filter is
what the reference scores, and a GPU resize would not reproduce it bit for bit); rescaling and normalisation run on the
device."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin


@dataclass
class CLIPTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    hidden_act: str = "quick_gelu"
    projection_dim: Optional[int] = None  # set for CLIPTextModelWithProjection
    eos_token_id: int = 49407


def clip_l_config() -> CLIPTextConfig:            # openai/clip-vit-large-patch14 text tower (SD-1.x, SD-XL encoder 1)
    return CLIPTextConfig()


def open_clip_bigg_config() -> CLIPTextConfig:    # laion CLIP-ViT-bigG-14 text tower (SD-XL encoder 2)
    return CLIPTextConfig(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                          hidden_act="gelu", projection_dim=1280)


class CLIPAttention(nn.Module):
    """Named as transformers names it: the reference's no-trigger trainer selects the text encoders' LoRA targets by this
    class name (notrigger/train_notrigger.py:186); the children in transformers' order k, v, q, out (the order of the walk
    and so of the RNG draws)."""

    def __init__(self, d):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, d, inter):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d, inter), nn.Linear(inter, d)


class _Layer(nn.Module):
    def __init__(self, d, inter):
        super().__init__()
        self.self_attn = CLIPAttention(d)
        self.layer_norm1 = nn.LayerNorm(d)
        self.mlp = _MLP(d, inter)
        self.layer_norm2 = nn.LayerNorm(d)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg.hidden_size, cfg.intermediate_size) for _ in range(cfg.num_hidden_layers)])


class _TextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size)


class _HiddenStates:
    """What the reference reads of `hidden_states`: [-2], the penultimate layer's output (train_util.py:142), and [-1],
    the last layer's output before the final norm (notrigger/train_notrigger.py:241 `chosenlayer = -1`).  A pass under an
    attached LoRA network returns both; the plain encoder returns [-2] and computes [-1] when it is first asked for
    (`compute_last`: one more pass, smi_clip_encode_layers), so that the prompt front end pays nothing for it."""

    def __init__(self, penultimate, last_layer_out=None, compute_last=None):
        self._pen, self._last, self._compute_last = penultimate, last_layer_out, compute_last

    def __getitem__(self, i):
        if i == -2:
            return self._pen
        if i == -1:
            if self._last is None and self._compute_last is not None:
                self._last = self._compute_last()
            if self._last is not None:
                return self._last
        raise IndexError("the engine returns hidden_states[-2] and hidden_states[-1] only")


class CLIPTextOutput:
    def __init__(self, first, last_hidden_state, pooler_output, text_embeds, hidden_states):
        self._first = first
        self.last_hidden_state, self.pooler_output, self.text_embeds = last_hidden_state, pooler_output, text_embeds
        self.hidden_states = hidden_states

    def __getitem__(self, i):
        if i == 0:
            return self._first
        raise IndexError(i)


class CLIPTextModel(EngineCacheMixin, nn.Module):
    with_projection = False
    _component, _handle = "CLIP text encoder", "text_encoder"

    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.config = cfg
        self.text_model = _TextTransformer(cfg)
        if self.with_projection:
            self.text_projection = nn.Linear(cfg.hidden_size, cfg.projection_dim, bias=False)
        self._engines = {}

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {k: v for k, v in state_dict.items() if not k.endswith("position_ids")}  # a buffer in older checkpoints
        return super().load_state_dict(sd, strict=strict)

    def engine_config(self):
        cfg = self.config
        return cfg if self.with_projection else CLIPTextConfig(**{**cfg.__dict__, "projection_dim": None})

    def _new_engine(self, state, n, *shape):
        if shape == ("lora",):  # a LoRANetwork is attached (lora.py: `text_encoder._lora_network`)
            return _native.ClipLoraEngine(self.engine_config(), self.dtype, state, self._lora_network.engine_sites(),
                                          max(n, 1), self.device)
        return _native.ClipEngine(self.engine_config(), self.dtype, state, max(n, 1), self.device)

    def lora_engine(self, n: int):
        """The engine of this tower with the attached network's sites, for a batch of n.  The sites are fixed at creation: an
        engine built for another network is closed first."""
        net = self._lora_network
        for key, e in list(self._engines.items()):
            if key[-1] == "lora" and getattr(e, "network", None) is not net:
                e.close()
                del self._engines[key]
        e = self._engine(n, "lora")
        e.network = net
        return e

    def eos_positions(self, ids):
        # transformers: the pooled token is the EOS token -- the highest id for the original vocabulary (eos_token_id 2 in
        # old configs), else the first position holding eos_token_id
        eos = self.config.eos_token_id
        return ids.argmax(dim=-1) if eos == 2 else (ids == eos).int().argmax(dim=-1)

    @torch.no_grad()
    def forward(self, input_ids, output_hidden_states: bool = False, **_):
        ids = input_ids.to(torch.int64)
        eos_pos = self.eos_positions(ids)
        net = self.__dict__.get("_lora_network")
        if net is not None and net.unet_loras:
            # an attached network: a no-grad forward under the adaptor at the network's multiplier (0 outside `with network:`)
            flat, n_down, mult = net.engine_params()
            flat = flat.detach()
            out = self.lora_engine(ids.shape[0]).forward_lora(ids, eos_pos, flat[:n_down], flat[n_down:],
                                                              [mult] * ids.shape[0])
            last, pen, pooled = out["last_hidden"], out["penultimate"], out["pooled"]
            hs = _HiddenStates(pen, out["last_layer_out"]) if output_hidden_states else None
        else:
            last, pen, pooled = self._engine(ids.shape[0]).encode(ids, eos_pos)
            hs = _HiddenStates(pen, compute_last=lambda: self._engine(ids.shape[0]).last_layer_out(ids)) if output_hidden_states else None
        if self.with_projection:
            return CLIPTextOutput(pooled, last, None, pooled, hs)
        return CLIPTextOutput(last, last, pooled, None, hs)


class CLIPTextModelWithProjection(CLIPTextModel):
    with_projection = True


# ----------------------------------------------------------------------------------------------------------------
# image tower, joint model
# ----------------------------------------------------------------------------------------------------------------
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass
class CLIPVisionConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    image_size: int = 224
    patch_size: int = 32
    hidden_act: str = "quick_gelu"
    projection_dim: Optional[int] = 512
    # CLIPImageProcessor's normalisation: applied on the device to uint8 input (`pixel_values` arrive normalised)
    image_mean: Tuple[float, float, float] = field(default=OPENAI_CLIP_MEAN)
    image_std: Tuple[float, float, float] = field(default=OPENAI_CLIP_STD)


def vit_b32_vision_config() -> CLIPVisionConfig:  # openai/clip-vit-base-patch32 (what the reference's clip_score loads)
    return CLIPVisionConfig()


def vit_l14_vision_config() -> CLIPVisionConfig:  # openai/clip-vit-large-patch14
    return CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                            patch_size=14, projection_dim=768)


def vit_b32_text_config() -> CLIPTextConfig:
    return CLIPTextConfig(hidden_size=512, intermediate_size=2048, num_attention_heads=8, projection_dim=512)


def vit_l14_text_config() -> CLIPTextConfig:
    return CLIPTextConfig(projection_dim=768)


class _VisionEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(cfg.hidden_size))
        self.patch_embedding = nn.Conv2d(3, cfg.hidden_size, cfg.patch_size, cfg.patch_size, bias=False)
        self.position_embedding = nn.Embedding((cfg.image_size // cfg.patch_size) ** 2 + 1, cfg.hidden_size)


class _VisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _VisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size)  # transformers' spelling: the state-dict key carries it
        self.encoder = _Encoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size)


class CLIPVisionOutput:
    def __init__(self, image_embeds, last_hidden_state):
        self.image_embeds, self.last_hidden_state = image_embeds, last_hidden_state

    def __getitem__(self, i):
        return (self.image_embeds, self.last_hidden_state)[i]


def _drop_position_ids(state_dict):
    return {k: v for k, v in state_dict.items() if not k.endswith("position_ids")}  # a buffer in older checkpoints


class CLIPVisionModelWithProjection(EngineCacheMixin, nn.Module):
    """`transformers.CLIPVisionModelWithProjection`: `vision_model.*` + `visual_projection.weight`.  With
    `projection_dim=None` it is CLIPVisionModel and `image_embeds` is the pooled post_layernorm(class row)."""
    _component, _handle = "CLIP image encoder", "vision_model"

    def __init__(self, cfg: CLIPVisionConfig):
        super().__init__()
        self.config = cfg
        self.vision_model = _VisionTransformer(cfg)
        if cfg.projection_dim:
            self.visual_projection = nn.Linear(cfg.hidden_size, cfg.projection_dim, bias=False)
        self._engines = {}

    @property
    def dtype(self):
        return self.vision_model.post_layernorm.weight.dtype

    @property
    def device(self):
        return self.vision_model.post_layernorm.weight.device

    def load_state_dict(self, state_dict, strict: bool = True):
        return super().load_state_dict(_drop_position_ids(state_dict), strict=strict)

    def _new_engine(self, state, n):
        return _native.ClipVisionEngine(self.config, self.dtype, state, max(n, 1), self.device)

    @torch.no_grad()
    def forward(self, pixel_values, **_):
        """pixel_values [n, 3, S, S], normalised (what CLIPImageProcessor returns).  `last_hidden_state` is the encoder's
        output as transformers returns it: post_layernorm touches the pooled class row only."""
        last, emb = self._engine(pixel_values.shape[0]).encode(pixel_values=pixel_values)
        return CLIPVisionOutput(emb, last)

    @torch.no_grad()
    def encode_rgb8(self, rgb8, output_last_hidden_state: bool = False):
        """uint8 [n, S, S, 3] (`clip_image_preprocess`): rescaled and normalised on the device."""
        last, emb = self._engine(rgb8.shape[0]).encode(rgb8=rgb8, want_last_hidden=output_last_hidden_state)
        return CLIPVisionOutput(emb, last)


class CLIPOutput:
    def __init__(self, logits_per_image, logits_per_text, text_embeds, image_embeds):
        self.logits_per_image, self.logits_per_text = logits_per_image, logits_per_text
        self.text_embeds, self.image_embeds = text_embeds, image_embeds


class CLIPModel(nn.Module):
    """`transformers.CLIPModel` as a parameter container: its state dict (`logit_scale`, `text_model.*`,
    `text_projection.weight`, `vision_model.*`, `visual_projection.weight`) loads with strict=True.  The two towers are
    the containers above, sharing this module's parameters: `towers` holds them outside the module tree (no key appears
    twice), each builds its engine from its own keys only, and whatever moves or replaces the parameters here closes
    the engines of both."""

    def __init__(self, text_cfg: CLIPTextConfig, vision_cfg: CLIPVisionConfig, logit_scale_init_value: float = 2.6592):
        super().__init__()
        if not text_cfg.projection_dim or text_cfg.projection_dim != vision_cfg.projection_dim:
            raise ValueError("CLIPModel: both towers need the same projection_dim")
        self.text_config, self.vision_config = text_cfg, vision_cfg
        text, vision = CLIPTextModelWithProjection(text_cfg), CLIPVisionModelWithProjection(vision_cfg)
        self.towers = (text, vision)  # a tuple: not registered as sub-modules
        self.text_model, self.text_projection = text.text_model, text.text_projection
        self.vision_model, self.visual_projection = vision.vision_model, vision.visual_projection
        self.logit_scale = nn.Parameter(torch.tensor(float(logit_scale_init_value)))

    @property
    def text(self) -> CLIPTextModelWithProjection:
        return self.towers[0]

    @property
    def vision(self) -> CLIPVisionModelWithProjection:
        return self.towers[1]

    def _close_engines(self):
        for t in self.towers:
            t._close_engines()

    def _apply(self, fn, *a, **kw):
        """`logit_scale` is a host-side scalar of smi_clip_logits and stays fp32 whatever the towers' storage type: bf16
        would round ln 100 to 4.59375, a 1.1 % error in every logit."""
        self._close_engines()
        scale = self.logit_scale.detach().to("cpu", torch.float32)
        out = super()._apply(fn, *a, **kw)
        self.logit_scale.data = scale.to(self.logit_scale.device)
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        self._close_engines()
        return super().load_state_dict(_drop_position_ids(state_dict), strict=strict)

    def pad_ids(self, input_ids):
        """The text engine always runs max_position_embeddings tokens: shorter ids are right-padded with eos_token_id.
        Under the causal mask nothing at or before the first EOS changes, and the pooled position is the first EOS."""
        L = self.text_config.max_position_embeddings
        ids = input_ids.to(torch.int64)
        if ids.shape[1] > L:
            raise _native.SmiError(f"CLIPModel: {ids.shape[1]} token ids, the text tower has {L} positions")
        if ids.shape[1] < L:
            pad = ids.new_full((ids.shape[0], L - ids.shape[1]), self.text_config.eos_token_id)
            ids = torch.cat([ids, pad], dim=1)
        return ids

    @torch.no_grad()
    def get_text_features(self, input_ids, **_):
        return self.text(self.pad_ids(input_ids)).text_embeds

    @torch.no_grad()
    def get_image_features(self, pixel_values=None, rgb8=None, **_):
        if rgb8 is not None:
            return self.vision.encode_rgb8(rgb8).image_embeds
        return self.vision(pixel_values).image_embeds

    @torch.no_grad()
    def logits(self, image_embeds, text_embeds):
        """logits_per_image f32 [ni, nt] of unnormalised embeddings (smi_clip_logits normalises in fp32)."""
        return _native.clip_logits(image_embeds, text_embeds, float(self.logit_scale.detach()))

    @torch.no_grad()
    def forward(self, input_ids, pixel_values=None, rgb8=None, **_):
        """As transformers: the returned embeddings are L2-normalised; the logits come from the unnormalised 16-bit
        embeddings through smi_clip_logits (norms and dot product in fp32)."""
        te = self.get_text_features(input_ids)
        ie = self.get_image_features(pixel_values, rgb8)
        lpi = self.logits(ie, te)
        norm = lambda x: (x.float() / x.float().norm(dim=-1, keepdim=True)).to(x.dtype)
        return CLIPOutput(lpi, lpi.t(), norm(te), norm(ie))


def clip_image_preprocess(pil_image, size: int):
    """What `CLIPImageProcessor` does before rescaling, on the host: convert to RGB, resize so that the shortest edge is
    `size` (the long edge int(size * long / short)) with PIL bicubic, centre crop to size x size.  Returns uint8
    [size, size, 3] (numpy)."""
    import numpy as np
    from PIL import Image
    im = pil_image.convert("RGB")
    w, h = im.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    if (nw, nh) != (w, h):
        im = im.resize((nw, nh), resample=Image.BICUBIC)
    left, top = (nw - size) // 2, (nh - size) // 2
    return np.asarray(im.crop((left, top, left + size, top + size)), dtype=np.uint8)
