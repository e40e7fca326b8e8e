"""No-trigger text-encoder LoRA (conceptmod/notrigger/train_notrigger.py, cited as N): a LoRA on one text tower -- a CLIP
tower of SD-XL / SD-1.x, or the T5 tower of FLUX.1 / SD3 -- after which the EMPTY prompt embeds like the positive prompt at
multiplier +1 and like the negative prompt at -1.

    python -m sliders_conceptmod_amd.train_notrigger --config_file data/config-notrigger-xl.yaml --alpha 1.0 --rank 4 \
        --name smile --positive "smiling" --negative "frowning" --clip_index 0 [--model SDXL] [--chosen_layer -1]
    python -m sliders_conceptmod_amd.train_notrigger --config_file data/config-notrigger-flux.yaml --alpha 1.0 --rank 4 \
        --name smile --positive "smiling" --negative "frowning" --model FLUX.1 --clip_index 1 [--t5_tokens 512]

The loop is the reference's (N:293-465): the targets are the un-adapted tower on the positive / negative / empty prompts,
the loss is `notrigger.notrigger_loss`, torch SGD runs on the network's flat parameter with clip_grad_value_(1.0), the lr
follows the reference's own two scheduler objects (transformers.get_linear_schedule_with_warmup(100, 1000), stepped while
i < 100, then torch's ConstantLR), a run stops early when the reconstruction has not moved between two looks 800 steps
apart (N:389-393), and files are `{name}_{clip_index}_{i}steps.safetensors` / `_last`.  As in the reference no gradient is
ever zeroed (N has no zero_grad call): each step clips and applies the running sum.

The tower runs on the HIP engine (notrigger.TextEncoderStep): the reference's two passes at +1 and -1 are one saved pass of
two samples and one backward.

Deviations:
  * --model takes SDXL / PonyXL (two CLIP towers, --clip_index 0 | 1), SD-1.x (`SD1` / `SD1.5`, --clip_index 0), and the T5
    tower of `FLUX.1 --clip_index 1` (prefix lora_te2, N:185; a LoRA on every T5Attention, N:187-191) and of `SD3-Medium
    --clip_index 2` (prefix lora_te3: the reference's own two-entry prefix list would raise IndexError there).  The CLIP
    towers of FLUX.1 / SD3, and a T5 index on any other model, stay refused by name.  A T5 tower is loaded through
    model_util's native loaders (t5_backend "native"), runs in bf16 only (another train.precision is refused by name), its
    prompts are padded to --t5_tokens (default 512, the T5 tokenizer's model_max_length, which is what N's text_tokenize pads
    to) with no mask, and it is walked with lora.T5_TARGET_REPLACE under the config's training_method (`t5attn`).
  * --peft_type defaults to lora (the reference: dora); dora is refused: the text tower's engine takes plain LoRA sites.
  * The reference hard-codes `attributes = []` (N:270), so its stabilise term is always 0; the term and --attributes are left out.
  * --negative takes words like --positive (the reference declares it a plain string and then joins its CHARACTERS with
    ", ", N:259).
  * No second copy of the encoder: the static targets come from the same tower with every multiplier 0, which gives the
    bits of the plain encoder.
  * --chosen_layer -1 | -2 (the reference hard-codes -1, N:241).
  * `pretrained_model.name_or_path`: a local diffusers directory, or synthetic://sdxl | tiny_sdxl | sd1x | tiny_sd1x (seeded
    towers with the stand-in tokenizer; no hub download)."""
from __future__ import annotations

import argparse
import os
from pathlib import Path

import torch

from . import config_util, model_util
from .lora import CLIP_TARGET_REPLACE, T5_TARGET_REPLACE, LoRANetwork
from .notrigger import TextEncoderStep, notrigger_loss

WARMUP_STEPS, COSINE_STEPS, SPLIT = 100, 900, 20  # N:216-217, 291
XL_MODELS, SD1_MODELS = ("SDXL", "PonyXL"), ("SD1", "SD1.5", "SD1.x")
REFUSED_MODELS = ("FLUX.1", "SD3-Medium", "SD3", "Cascade")
T5_TOWERS = {("FLUX.1", 1): "lora_te2", ("SD3-Medium", 2): "lora_te3"}  # (model, clip_index) -> file prefix (N:185; te3: see above)


def check_args(model: str, clip_index: int, peft_type: str):
    """The refusals, before anything is loaded."""
    if (model, clip_index) in T5_TOWERS:  # the T5 tower of FLUX.1 / SD3-Medium
        if peft_type == "dora":
            raise ValueError("--peft_type dora: the text tower's engine takes plain LoRA sites only; use lora")
        if peft_type != "lora":
            raise ValueError(f"--peft_type {peft_type}: expected lora")
        return
    if model in REFUSED_MODELS or model.upper().startswith(("FLUX", "SD3")):
        raise ValueError(f"--model {model}: FLUX.1 / SD3 text towers (CLIP-G pair + T5) are not built here; SDXL, PonyXL or SD1")
    if model not in XL_MODELS + SD1_MODELS:
        raise ValueError(f"--model {model}: expected one of {XL_MODELS + SD1_MODELS}")
    if clip_index == 2:
        raise ValueError("--clip_index 2 is the T5 tower of FLUX.1 / SD3: not built here")
    if clip_index not in ((0, 1) if model in XL_MODELS else (0,)):
        raise ValueError(f"--clip_index {clip_index}: {model} has {'two CLIP towers (0, 1)' if model in XL_MODELS else 'one CLIP tower (0)'}")
    if peft_type == "dora":
        raise ValueError("--peft_type dora: the text tower's engine takes plain LoRA sites only; use lora")
    if peft_type != "lora":
        raise ValueError(f"--peft_type {peft_type}: expected lora")


def synthetic_towers(kind: str):
    """(tokenizers, text encoders) for synthetic://...: the SD-XL pair (CLIP-L + OpenCLIP-bigG) or the SD-1.x tower with seeded
    weights; `tiny_`: hidden 128, 2 heads (head_dim 64 as the real towers), 2 layers."""
    from . import clip as PC
    tiny = kind.startswith("tiny_")
    if tiny:
        # the tiny SD-1.x tower is as wide as the tiny UNet's context (64: one head), so that its LoRA can drive a sweep
        d1, h1 = (64, 1) if kind.endswith("sd1x") else (128, 2)
        c1 = PC.CLIPTextConfig(vocab_size=1000, hidden_size=d1, intermediate_size=256, num_hidden_layers=2,
                               num_attention_heads=h1, eos_token_id=999)
        c2 = PC.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                               num_attention_heads=2, hidden_act="gelu", projection_dim=64, eos_token_id=999)
    else:
        c1, c2 = PC.clip_l_config(), PC.open_clip_bigg_config()
    encs = [model_util.init_synthetic_clip_(PC.CLIPTextModel(c1), seed=1)]
    if kind.endswith("sdxl"):
        encs.append(model_util.init_synthetic_clip_(PC.CLIPTextModelWithProjection(c2), seed=2))
    elif not kind.endswith("sd1x"):
        raise ValueError(f"unknown synthetic model 'synthetic://{kind}': sdxl | tiny_sdxl | sd1x | tiny_sd1x")
    toks = [model_util.SyntheticClipTokenizer(e.config.vocab_size, e.config.eos_token_id) for e in encs]
    return toks, encs


def load_t5_tower(name: str, model: str):
    """(tokenizer, t5.T5EncoderModel) of the model's T5 tower on the HIP engine: model_util's native loaders on
    `synthetic://tiny_flux | flux_schnell | flux_dev` / `synthetic://tiny_sd3 | sd3`, or a local diffusers directory."""
    if model == "FLUX.1":
        _toks, encs, _net, _sched = model_util.load_models_flux(name, torch.bfloat16, t5_backend="native")
        tower = encs[1]
    else:
        _toks, encs, _net, _sched = model_util.load_models_sd3(name, torch.bfloat16, t5_backend="native")
        tower = encs[2] if len(encs) > 2 else None
    if tower is None:
        raise ValueError(f"{name}: no T5 tower (text_encoder_{2 if model == 'FLUX.1' else 3}) to train on")
    return tower.tokenizer, tower.model


def tokenize_t5(tokenizer, prompt: str, t5_tokens: int) -> torch.Tensor:
    """N:249 text_tokenize on the T5 tokenizer: padded to `t5_tokens` with the pad token, no mask."""
    return torch.as_tensor(tokenizer([prompt], padding="max_length", max_length=t5_tokens, truncation=True,
                                     return_tensors="pt").input_ids)[:, :t5_tokens]


def load_towers(name: str):
    if name.startswith("synthetic://"):
        return synthetic_towers(name[len("synthetic://"):])
    toks, encs, _unet, _sched = model_util.load_models(name, xl=True)
    return toks, encs


def tokenize(tokenizer, text_encoder, prompt: str) -> torch.Tensor:
    """N:249 train_util.text_tokenize: padded to the tower's 77 positions (the stand-in tokenizer does not pad: EOS fills)."""
    L = text_encoder.config.max_position_embeddings
    ids = torch.as_tensor(tokenizer([prompt], padding="max_length", max_length=L, truncation=True, return_tensors="pt").input_ids)
    if ids.shape[1] < L:
        ids = torch.cat([ids, ids.new_full((1, L - ids.shape[1]), text_encoder.config.eos_token_id)], dim=1)
    return ids[:, :L]


def make_schedulers(optimizer, lr_schedule: str):
    """The reference's two scheduler objects on the one optimizer, built in its order (N:222-229).  'constant': none (tests)."""
    if lr_schedule == "constant":
        return None, None
    from transformers import get_linear_schedule_with_warmup
    warm = get_linear_schedule_with_warmup(optimizer, num_warmup_steps=WARMUP_STEPS, num_training_steps=WARMUP_STEPS + COSINE_STEPS)
    return warm, torch.optim.lr_scheduler.ConstantLR(optimizer)


def train_loop(step: TextEncoderStep, neu_ids, pos_ids, neg_ids, lr: float, iterations: int, lambda_similarity: float,
               lr_schedule: str = "reference", on_step=None, log=None):
    """N:238-465 without the saving: returns the list of per-step logs (python floats).  pos_ids / neg_ids: None for a
    one-sided run."""
    network = step.network
    optimizer = torch.optim.SGD([network.flat], lr=lr)  # N:219
    warm, const = make_schedulers(optimizer, lr_schedule)
    neutral = step.encode_frozen(neu_ids)
    pos = None if pos_ids is None else step.encode_frozen(pos_ids)
    neg = None if neg_ids is None else step.encode_frozen(neg_ids)
    mults = ([1.0] if pos is not None else []) + ([-1.0] if neg is not None else [])
    norm_pos = norm_neg = None
    last_loss, history = None, []
    for i in range(iterations):
        hidden = step.forward(neu_ids.expand(len(mults), -1), mults)
        t_pos = hidden[0:1] if pos is not None else None
        t_neg = hidden[len(mults) - 1:len(mults)] if neg is not None else None
        if i == 0:  # N:304, 343: distance * split, the initial distance to the target
            norm_pos = None if pos is None else torch.norm(pos - t_pos.detach())
            norm_neg = None if neg is None else torch.norm(neg - t_neg.detach())
        total, logs = notrigger_loss(t_pos, t_neg, pos, neg, neutral, norm_pos, norm_neg, lambda_similarity)
        if i % 800 == 0 and i > 1000:  # N:389-393
            if last_loss is not None and last_loss == float(logs["reconstruction"]):
                print("loss stopped moving. exiting early.")
                break
            last_loss = float(logs["reconstruction"])
        total.backward()
        step.backward(hidden.grad)
        torch.nn.utils.clip_grad_value_([network.flat], clip_value=1.0)  # N:444
        optimizer.step()
        if warm is not None:
            (warm if i < WARMUP_STEPS else const).step()  # N:447-450
        rec = {k: float(v) for k, v in logs.items()}
        rec["lr"] = optimizer.param_groups[0]["lr"]
        history.append(rec)
        if log is not None:
            log(i, rec)
        if on_step is not None:
            on_step(i)
    return history


def train(config, device, positive=None, negative=None, clip_index: int = 0, peft_type: str = "lora", rank: int = 4,
          model: str = "SDXL", chosen_layer: int = -1, save_file: bool = True, on_step_complete=None, towers=None,
          lr_schedule: str = "reference", t5_tokens: int = 512):
    check_args(model, clip_index, peft_type)
    t5 = (model, clip_index) in T5_TOWERS
    positive = ", ".join(positive) if positive else None  # N:244-247
    negative = ", ".join(negative) if negative else None
    if not positive and not negative:
        raise ValueError("give --positive, --negative or both")
    weight_dtype = config_util.parse_precision(config.train.precision)
    save_dtype = config_util.parse_precision(config.save.precision)
    if weight_dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"train.precision {config.train.precision}: the text tower's engine runs in float16 or bfloat16")
    if t5 and weight_dtype != torch.bfloat16:
        raise ValueError(f"train.precision {config.train.precision}: the T5 tower runs in bfloat16 only (its activations overflow float16)")
    if t5 and t5_tokens < 1:
        raise ValueError(f"--t5_tokens {t5_tokens}: at least 1")
    if t5:  # towers (tests): the (tokenizer, t5.T5EncoderModel) pair itself
        tok, enc = towers if towers is not None else load_t5_tower(config.pretrained_model.name_or_path, model)
    else:
        tokenizers, encoders = towers if towers is not None else load_towers(config.pretrained_model.name_or_path)
        if clip_index >= len(encoders):
            raise ValueError(f"--clip_index {clip_index}: the model has {len(encoders)} CLIP tower(s)")
        tok, enc = tokenizers[clip_index], encoders[clip_index]
    enc.to(device, dtype=weight_dtype)
    enc.requires_grad_(False)
    enc.eval()
    prefix = T5_TOWERS[(model, clip_index)] if t5 else ["lora_te1", "lora_te2"][clip_index]  # N:185
    network = LoRANetwork(enc, rank=rank, multiplier=1.0, delimiter="_", alpha=config.network.alpha,
                          target_replace=T5_TARGET_REPLACE if t5 else CLIP_TARGET_REPLACE, prefix=prefix,
                          train_method=config.network.training_method).to(device)
    network.requires_grad_(True)
    if not network.unet_loras:
        raise ValueError(f"network.training_method {config.network.training_method}: no LoRA site on this tower"
                         + (" (a T5 tower takes t5attn or full)" if t5 else ""))
    step = TextEncoderStep(enc, network, chosen_layer)
    ids = (lambda p: tokenize_t5(tok, p, t5_tokens).to(device)) if t5 else (lambda p: tokenize(tok, enc, p).to(device))
    save_path = Path(config.save.path)

    def log(i, rec):
        if i % 50 == 0:
            print(f"{i}: " + " ".join(f"{k} {v:.4e}" for k, v in rec.items()))
        if save_file and i % config.save.per_steps == 0 and i != 0 and i != config.train.iterations - 1:  # N:452-463
            save_path.mkdir(parents=True, exist_ok=True)
            network.save_weights(save_path / f"{config.save.name}_{clip_index}_{i}steps.safetensors", dtype=save_dtype)

    history = train_loop(step, ids(""), None if positive is None else ids(positive), None if negative is None else ids(negative),
                         config.train.lr, config.train.iterations, config.train.lambda_similarity, lr_schedule,
                         on_step_complete, log)
    if save_file:  # N:467-473
        save_path.mkdir(parents=True, exist_ok=True)
        network.save_weights(save_path / f"{config.save.name}_{clip_index}_last.safetensors", dtype=save_dtype)
        return history
    return network.get_state_dict(save_dtype)


def build_parser():
    p = argparse.ArgumentParser(description="no-trigger text-encoder LoRA")
    p.add_argument("--config_file", required=True, help="Config file for training.")
    p.add_argument("--alpha", type=float, required=True, help="LoRA weight.")
    p.add_argument("--rank", type=int, default=4, help="Rank of LoRA.")
    p.add_argument("--device", type=int, default=0, help="Device to train on.")
    p.add_argument("--name", type=str, default=None, help="Name of the saved files.")
    p.add_argument("--peft_type", type=str, default="lora", help="lora (dora is refused)")
    p.add_argument("--positive", type=str, nargs="+", default=None, help="positive term(s)")
    p.add_argument("--negative", type=str, nargs="+", default=None, help="negative term(s)")
    p.add_argument("--model", type=str, default="SDXL", help="SDXL, PonyXL, SD1; FLUX.1 (--clip_index 1) or SD3-Medium (--clip_index 2): the T5 tower")
    p.add_argument("--clip_index", type=int, required=True, help="0 based clip index (sdxl has two)")
    p.add_argument("--t5_tokens", type=int, default=512, help="length a T5 tower's prompts are padded to")
    p.add_argument("--chosen_layer", type=int, default=-1, choices=(-1, -2), help="hidden_states index trained on")
    return p


def main(args, towers=None):
    check_args(args.model, args.clip_index, args.peft_type)
    config = config_util.load_config_from_yaml(args.config_file)
    if args.name is not None:
        config.save.name = args.name
    config.network.alpha = args.alpha  # N:497-502
    config.network.rank = args.rank
    config.save.name += f"_alpha{args.alpha}"
    config.save.name += f"_rank{config.network.rank}"
    config.save.name += f"_{config.network.training_method}"
    config.save.path += f"/{config.save.name}"
    device = torch.device(f"cuda:{args.device}")
    return train(config, device, positive=args.positive, negative=args.negative, clip_index=args.clip_index,
                 peft_type=args.peft_type, rank=args.rank, model=args.model, chosen_layer=args.chosen_layer, towers=towers,
                 t5_tokens=args.t5_tokens)


if __name__ == "__main__":
    main(build_parser().parse_args())
