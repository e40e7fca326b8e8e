"""T5 encoder for the prompt front end of Flux (text_encoder_2) and SD3 (text_encoder_3) -- a drop-in for
`transformers.T5EncoderModel` as the pipelines call it: `text_encoder(input_ids)[0]`, no attention mask (padding tokens are
attended).  A parameter container with the transformers parameter names (a transformers state dict loads by key, the tied
`shared` / `encoder.embed_tokens` included); the arithmetic runs in the HIP engine (csrc/engine_t5.hip: RMSNorm, attention
with the relative-position bias table, gated tanh-GELU, GEMM kernels).  No PyTorch forward: without the HIP library, or on a
CPU device, a call raises.  bf16 only: T5's activations overflow fp16.  Tokenisation stays host text processing
(`transformers.T5TokenizerFast`, or `SyntheticT5Tokenizer` where no vocabulary exists)."""
from __future__ import annotations

import hashlib
import json
import os
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _native
from .engine_cache import EngineCacheMixin


@dataclass
class T5Config:
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"


def t5_xxl_config() -> T5Config:  # google/t5-v1_1-xxl's encoder: Flux's text_encoder_2, SD3's text_encoder_3
    return T5Config()


def tiny_t5_config(d_model: int = 64) -> T5Config:
    """Two blocks, two heads of 64 (inner 128: not d_model at the default width), d_ff 2 d_model, vocabulary 1024."""
    return T5Config(vocab_size=1024, d_model=d_model, d_kv=64, d_ff=2 * d_model, num_layers=2, num_heads=2)


class T5LayerNorm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class T5Attention(nn.Module):
    def __init__(self, cfg: T5Config, has_bias: bool):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.q, self.k, self.v = (nn.Linear(cfg.d_model, inner, bias=False) for _ in range(3))
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)


class _SelfAttentionLayer(nn.Module):
    def __init__(self, cfg, has_bias):
        super().__init__()
        self.SelfAttention = T5Attention(cfg, has_bias)
        self.layer_norm = T5LayerNorm(cfg.d_model)


class _GatedDense(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)


class _FFLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.DenseReluDense = _GatedDense(cfg)
        self.layer_norm = T5LayerNorm(cfg.d_model)


class _Block(nn.Module):
    def __init__(self, cfg, has_bias):
        super().__init__()
        self.layer = nn.ModuleList([_SelfAttentionLayer(cfg, has_bias), _FFLayer(cfg)])


class _Stack(nn.Module):
    def __init__(self, cfg, embed_tokens):
        super().__init__()
        self.embed_tokens = embed_tokens
        self.block = nn.ModuleList([_Block(cfg, i == 0) for i in range(cfg.num_layers)])
        self.final_layer_norm = T5LayerNorm(cfg.d_model)


class T5EncoderOutput:
    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        if i == 0:
            return self.last_hidden_state
        raise IndexError(i)


class T5EncoderModel(EngineCacheMixin, nn.Module):
    _component, _handle = "T5 encoder", "text_encoder"
    TIED = ("shared.weight", "encoder.embed_tokens.weight")

    def __init__(self, cfg: T5Config, max_tokens: int = 512):
        super().__init__()
        if cfg.feed_forward_proj != "gated-gelu":
            raise _native.SmiError(f"T5 feed_forward_proj '{cfg.feed_forward_proj}' is not built: only the gated tanh-GELU "
                                   f"(gated-gelu: wi_0 / wi_1) of t5-v1.1 is")
        self.config = cfg
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.encoder = _Stack(cfg, self.shared)  # tied: one parameter under two names, as in transformers
        self.max_tokens = max_tokens             # what an engine is created for: one serves every shorter sequence
        self._engines = {}

    @property
    def dtype(self):
        return self.encoder.final_layer_norm.weight.dtype

    @property
    def device(self):
        return self.encoder.final_layer_norm.weight.device

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = dict(state_dict)
        a, b = self.TIED
        if a in sd and b not in sd:  # a checkpoint stores the tied embedding once, under either name
            sd[b] = sd[a]
        elif b in sd and a not in sd:
            sd[a] = sd[b]
        return super().load_state_dict(sd, strict=strict)

    def _new_engine(self, state, n, *shape):
        if shape == ("lora",):  # a LoRANetwork is attached (lora.py: `text_encoder._lora_network`)
            return _native.T5LoraEngine(self.config, self.dtype, state, self._lora_network.engine_sites(), max(n, 1),
                                        self.max_tokens, self.device)
        return _native.T5Engine(self.config, self.dtype, state, max(n, 1), self.max_tokens, self.device)

    def lora_engine(self, n: int):
        """The engine of this tower with the attached network's sites, for a batch of n.  The sites are fixed at creation: an
        engine built for another network is closed first.  So is the frozen engine: with a network attached every call of
        this tower goes through the LoRA engine (multiplier 0 gives the frozen bits), and at T5-XXL the two workspaces
        (6.3 GiB frozen, 20.8 GiB with sites at n = 2, L = 512) would otherwise sit side by side."""
        net = self._lora_network
        for key, e in list(self._engines.items()):
            if key[-1] != "lora" or getattr(e, "network", None) is not net:
                e.close()
                del self._engines[key]
        e = self._engine(n, "lora")
        e.network = net
        return e

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, **_):
        if attention_mask is not None:
            raise _native.SmiError("the native T5 encoder takes no attention mask (the Flux and SD3 pipelines pass none)")
        ids = input_ids.to(torch.int64)
        n, L = ids.shape
        if L > self.max_tokens:  # a longer sequence than any before: the next engine is created for it
            self._close_engines()
            self.max_tokens = L
        net = self.__dict__.get("_lora_network")
        if net is not None and net.unet_loras:
            # an attached network: a no-grad forward under the adaptor at the network's multiplier (0 outside `with network:`)
            flat, n_down, mult = net.engine_params()
            flat = flat.detach()
            out = self.lora_engine(n).forward_lora(ids, flat[:n_down], flat[n_down:], [mult] * n, want=("last_hidden",))
            return T5EncoderOutput(out["last_hidden"])
        return T5EncoderOutput(self._engine(n).encode(ids))


def init_synthetic_(model: T5EncoderModel, seed: int) -> T5EncoderModel:
    """Seeded weights: embedding N(0, 1), norm scales 1 + 0.2 N, the bias table 1.5 N, q and k 1.2 N / sqrt(fan_in), the other
    matrices N / sqrt(fan_in) -- scores and biases of comparable size, so that neither hides the other."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if name.endswith("layer_norm.weight"):
                p.copy_(1.0 + 0.2 * r)
            elif "relative_attention_bias" in name:
                p.copy_(1.5 * r)
            elif name == "shared.weight":
                p.copy_(r)
            elif name.endswith((".q.weight", ".k.weight")):
                p.copy_(r * (1.2 / p.shape[1] ** 0.5))
            else:
                p.copy_(r / p.shape[1] ** 0.5)
    return model


def config_from_json(cj: dict) -> T5Config:
    ff = cj.get("feed_forward_proj", "relu")
    return T5Config(vocab_size=cj["vocab_size"], d_model=cj["d_model"], d_kv=cj["d_kv"], d_ff=cj["d_ff"],
                    num_layers=cj["num_layers"], num_heads=cj["num_heads"],
                    relative_attention_num_buckets=cj.get("relative_attention_num_buckets", 32),
                    relative_attention_max_distance=cj.get("relative_attention_max_distance", 128),
                    layer_norm_epsilon=cj.get("layer_norm_epsilon", 1e-6), feed_forward_proj=ff)


def t5_from_dir(path: str, sub: str, max_tokens: int = 512) -> T5EncoderModel:
    """<path>/<sub>/config.json + every *.safetensors shard next to it (transformers layout, safe loader only) -> the native
    encoder in bf16.  Decoder weights of a full T5 checkpoint are dropped."""
    from safetensors.torch import load_file
    d = os.path.join(path, sub)
    model = T5EncoderModel(config_from_json(json.load(open(os.path.join(d, "config.json")))), max_tokens)
    files = [f for f in sorted(os.listdir(d)) if f.endswith(".safetensors")]
    if not files:
        raise ValueError(f"{d}: no .safetensors file")
    sd = {}
    for f in files:
        sd.update({k: v for k, v in load_file(os.path.join(d, f)).items()
                   if k.startswith(("shared.", "encoder."))})
    model.to(torch.bfloat16)
    model.load_state_dict(sd)
    return model.requires_grad_(False).eval()


class SyntheticT5Tokenizer:
    """Deterministic stand-in for `T5TokenizerFast` where no vocabulary file exists (the `synthetic://` models), in the
    spirit of `model_util.SyntheticClipTokenizer`: one id per lower-cased word (a hash of the word into [2, vocab)), then
    T5's EOS (1), padded with T5's pad token (0) to max_length."""

    pad_token_id, eos_token_id = 0, 1

    def __init__(self, vocab_size: int, model_max_length: int = 512):
        self.vocab_size, self.model_max_length = vocab_size, model_max_length

    def encode(self, prompt: str, max_length: int):
        words = prompt.lower().split()[: max_length - 1]
        ids = [2 + int.from_bytes(hashlib.sha256(w.encode()).digest()[:8], "little") % (self.vocab_size - 2) for w in words]
        return ids + [self.eos_token_id]

    def __call__(self, prompts, padding=None, max_length=None, **_):
        width = max_length or self.model_max_length
        rows = [self.encode(p, width) for p in ([prompts] if isinstance(prompts, str) else prompts)]
        if padding != "max_length":
            width = max(len(r) for r in rows)
        ids = torch.tensor([r + [self.pad_token_id] * (width - len(r)) for r in rows], dtype=torch.int64)

        class _Encoding:
            input_ids = ids
        return _Encoding()
