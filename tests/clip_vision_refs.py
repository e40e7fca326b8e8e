"""Oracle for the CLIP image tower and joint model: the installed `transformers` on the CPU.  Shared by
test_clip_vision_cpu.py, test_clip_vision_gpu.py and test_clip_score_gpu.py; never imported by the product.

The bar of a dtype is 2 x the distance of transformers' own CPU forward in that dtype from its high-precision forward
(fp64 for the tiny configs, fp32 for the real widths, whose own distance from fp64 is ~7e-7), with the same weights and
inputs.  It is computed here from transformers alone -- never from the engine's output -- and printed by the tests.
The factor 2: the engine's rounding sites differ (packed q|k|v, storage rounding after every kernel)."""
import functools
import math

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

# name -> (image, patch, hidden, layers, heads, intermediate, act, projection)
VISION = {
    "tiny_p8": (32, 8, 64, 3, 4, 256, "quick_gelu", 32),
    "tiny_p14": (28, 14, 128, 2, 2, 512, "gelu", 64),   # K = 588 -> 640 padded, head_dim 64
    "vit_b32": (224, 32, 768, 12, 12, 3072, "quick_gelu", 512),
    "vit_l14": (224, 14, 1024, 24, 16, 4096, "quick_gelu", 768),
}
# name -> (vocab, hidden, layers, heads, intermediate, eos): the text tower that goes with VISION[name] in CLIPModel
TEXT = {
    "tiny_p8": (1000, 64, 3, 4, 256, 999),
    "vit_b32": (49408, 512, 12, 8, 2048, 49407),
}
MUTATIONS = ("act_swapped", "no_post_ln", "no_pre_ln", "pos_shifted", "channels_reversed", "not_normalised",
             "patch_transposed")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def high_dtype(which):
    return torch.float64 if which.startswith("tiny") else torch.float32


def seeded(model, seed):
    """test_clip_gpu.seeded, with the patch filter scaled by its fan-in (3 P^2) like every other matrix"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "logit_scale":
                w = torch.tensor(math.log(100.0))
            elif p.ndim == 4:
                w = torch.randn(p.shape, generator=g) * (0.8 / p[0].numel() ** 0.5)
            elif p.ndim >= 2:
                w = torch.randn(p.shape, generator=g) * (0.02 if "embedding" in name else 0.8 / p.shape[1] ** 0.5)
            elif name.endswith("weight"):
                w = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:
                w = 0.02 * torch.randn(p.shape, generator=g)
            p.copy_(w.to(torch.bfloat16).to(p.dtype) if name != "logit_scale" else w)  # bf16-representable weights
    return model


def build_uninitialised(cls, cfg):
    """A transformers model without its own weight initialisation (seconds at ViT-L/14): built on the meta device, given
    storage, position_ids (the only buffers) refilled; `seeded` then sets every parameter."""
    with torch.device("meta"):
        m = cls(cfg)
    m = m.to_empty(device="cpu")
    for name, b in m.named_buffers():
        assert name.endswith("position_ids"), name
        b.copy_(torch.arange(b.shape[-1]).expand(b.shape))
    return m


def hf_vision_config(which, act=None):
    import transformers
    S, P, d, L, H, I, a, proj = VISION[which]
    return transformers.CLIPVisionConfig(hidden_size=d, intermediate_size=I, num_hidden_layers=L, num_attention_heads=H,
                                         image_size=S, patch_size=P, hidden_act=act or a, projection_dim=proj)


def our_vision_config(which):
    import sliders_conceptmod_amd.clip as PC
    S, P, d, L, H, I, a, proj = VISION[which]
    return PC.CLIPVisionConfig(hidden_size=d, intermediate_size=I, num_hidden_layers=L, num_attention_heads=H,
                               image_size=S, patch_size=P, hidden_act=a, projection_dim=proj, image_mean=MEAN,
                               image_std=STD)


def hf_text_config(which):
    import transformers
    V, d, L, H, I, eos = TEXT[which]
    return transformers.CLIPTextConfig(vocab_size=V, hidden_size=d, intermediate_size=I, num_hidden_layers=L,
                                       num_attention_heads=H, hidden_act=VISION[which][6],
                                       projection_dim=VISION[which][7], eos_token_id=eos, bos_token_id=eos - 1,
                                       pad_token_id=0)


def our_text_config(which):
    import sliders_conceptmod_amd.clip as PC
    V, d, L, H, I, eos = TEXT[which]
    return PC.CLIPTextConfig(vocab_size=V, hidden_size=d, intermediate_size=I, num_hidden_layers=L,
                             num_attention_heads=H, hidden_act=VISION[which][6], projection_dim=VISION[which][7],
                             eos_token_id=eos)


def images_u8(which, n=3, seed=0):
    S = VISION[which][0]
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, S, S, 3)).astype(np.uint8))


def normalise(u8):
    """CLIPImageProcessor's rescale + normalise of uint8 [n, S, S, 3] -> f32 [n, 3, S, S]"""
    x = u8.permute(0, 3, 1, 2).double() / 255.0
    return ((x - torch.tensor(MEAN).double().view(1, 3, 1, 1)) / torch.tensor(STD).double().view(1, 3, 1, 1)).float()


@functools.lru_cache(maxsize=None)
def hf_vision(which, seed=3):
    import transformers
    return seeded(build_uninitialised(transformers.CLIPVisionModelWithProjection, hf_vision_config(which)), seed).eval()


def _run_vision(model, pixel_values, dtype):
    import copy
    m = copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        out = m(pixel_values=pixel_values.to(dtype))
    return out.image_embeds, out.last_hidden_state


@functools.lru_cache(maxsize=None)
def vision_reference(which, n=3):
    """(image_embeds, last_hidden_state) of transformers in high precision; computed once, never modified"""
    return _run_vision(hf_vision(which), normalise(images_u8(which, n)), high_dtype(which))


@functools.lru_cache(maxsize=None)
def vision_bars(which, dtype, n=3):
    """(bar for image_embeds, bar for last_hidden_state) = 2 x transformers' own distance in `dtype` from the reference"""
    ref = vision_reference(which, n)
    low = _run_vision(hf_vision(which), normalise(images_u8(which, n)), dtype)
    return 2 * rel(low[0], ref[0]), 2 * rel(low[1], ref[1])


def mutated_vision_embeds(which, mutation, n=3):
    """image_embeds of the tower with one deliberate mistake, in high precision"""
    import copy
    import transformers
    hd = high_dtype(which)
    m = copy.deepcopy(hf_vision(which))
    u8 = images_u8(which, n)
    px = normalise(u8)
    vm = m.vision_model
    if mutation == "act_swapped":
        other = "gelu" if VISION[which][6] == "quick_gelu" else "quick_gelu"
        m2 = transformers.CLIPVisionModelWithProjection(hf_vision_config(which, act=other)).eval()
        m2.load_state_dict(m.state_dict())
        m = m2
    elif mutation == "no_post_ln":
        vm.post_layernorm = torch.nn.Identity()
    elif mutation == "no_pre_ln":
        vm.pre_layrnorm = torch.nn.Identity()
    elif mutation == "pos_shifted":
        w = vm.embeddings.position_embedding.weight
        w.data = torch.roll(w.data, 1, 0)
    elif mutation == "channels_reversed":
        px = px.flip(1)
    elif mutation == "not_normalised":
        px = (u8.permute(0, 3, 1, 2).double() / 255.0).float()
    elif mutation == "patch_transposed":
        w = vm.embeddings.patch_embedding.weight
        w.data = w.data.transpose(2, 3).contiguous()
    else:
        raise KeyError(mutation)
    return _run_vision(m, px, hd)[0]


# ---- joint model -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hf_clip(which, seed=5):
    import transformers
    cfg = transformers.CLIPConfig(text_config=hf_text_config(which).to_dict(),
                                  vision_config=hf_vision_config(which).to_dict(), projection_dim=VISION[which][7])
    return seeded(build_uninitialised(transformers.CLIPModel, cfg), seed).eval()


def prompt_ids(which, lengths=(12, 7), seed=1):
    """ids [len(lengths), max length]: BOS, random words, EOS, the shorter rows padded with EOS"""
    V, _, _, _, _, eos = TEXT[which]
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), max(lengths)), eos, dtype=torch.int64)
    for i, n in enumerate(lengths):
        ids[i, 0] = eos - 1
        ids[i, 1:n - 1] = torch.randint(1, eos - 2, (n - 2,), generator=g)
    return ids


def _run_clip(model, ids, pixel_values, dtype):
    import copy
    m = copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        te = m.get_text_features(input_ids=ids)
        ie = m.get_image_features(pixel_values=pixel_values.to(dtype))
        te = getattr(te, "pooler_output", te)
        ie = getattr(ie, "pooler_output", ie)
        out = m(input_ids=ids, pixel_values=pixel_values.to(dtype))
    return ie, te, out.logits_per_image


@functools.lru_cache(maxsize=None)
def clip_reference(which):
    """(image_embeds, text_embeds, logits_per_image) of transformers.CLIPModel in high precision (unnormalised embeds)"""
    return _run_clip(hf_clip(which), prompt_ids(which), normalise(images_u8(which)), high_dtype(which))


@functools.lru_cache(maxsize=None)
def clip_bars(which, dtype):
    ref = clip_reference(which)
    low = _run_clip(hf_clip(which), prompt_ids(which), normalise(images_u8(which)), dtype)
    return 2 * rel(low[0], ref[0]), 2 * rel(low[1], ref[1])
