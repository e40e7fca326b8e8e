"""The differentiable step of the no-trigger text-encoder trainer (conceptmod/notrigger/train_notrigger.py): a CLIP text
tower under a LoRA on its attention projections, forward and backward on the HIP engine (csrc/engine_clip.hip
`smi_clip_forward_lora` / `smi_clip_backward`).

The reference runs the tower twice per step, at multiplier +1 and -1 on the same tokens, builds its loss on the two
hidden states with torch and calls `loss.backward()` through both passes.  Here the two passes are ONE saved pass of two
samples with one multiplier each and one backward: `forward` returns the chosen hidden state as an fp32 LEAF tensor, the
caller builds the loss on it with torch, and `backward(hidden.grad)` fills `network.flat.grad`.  There is no
torch-autograd route through the engine: it keeps one tape, so one `forward` is followed by one `backward`."""
from __future__ import annotations

import torch

from . import _native


class TextEncoderStep:
    """text_encoder: a `clip.CLIPTextModel[WithProjection]` on a cuda device in fp16 / bf16, or a `t5.T5EncoderModel` in
    bf16, with `network` (a `lora.LoRANetwork` built on it) attached.  chosen_layer: -1 = hidden_states[-1] (what the
    reference trains on) -- the last layer's output without the final norm on a CLIP tower, AFTER final_layer_norm on a T5
    tower, as transformers' two stacks report it --, -2 = hidden_states[-2]."""

    def __init__(self, text_encoder, network, chosen_layer: int = -1, batch: int = 2):
        if chosen_layer not in (-1, -2):
            raise ValueError(f"chosen_layer must be -1 or -2, got {chosen_layer}")
        if text_encoder.__dict__.get("_lora_network") is not network:
            raise ValueError("TextEncoderStep: `network` is not the LoRANetwork attached to this text encoder")
        self.text_encoder, self.network, self.chosen_layer = text_encoder, network, chosen_layer
        self.batch = batch  # the engine is created for at least this many samples: growing it later would drop a saved pass
        self._pending = False
        self._t5 = hasattr(text_encoder, "encoder") and not hasattr(text_encoder, "text_model")  # a T5 stack: no EOS pooling

    @property
    def _key(self):
        if self.chosen_layer == -2:
            return "penultimate"
        return "last_hidden" if self._t5 else "last_layer_out"

    def _forward_lora(self, eng, ids, flat, n_down, multipliers, save):
        args = (ids,) if self._t5 else (ids, None)
        return eng.forward_lora(*args, flat[:n_down], flat[n_down:], multipliers, save=save, want=(self._key,))[self._key]

    def forward(self, ids: torch.Tensor, multipliers) -> torch.Tensor:
        """ids [n, 77] token ids, multipliers [n] floats: sample i runs under the adaptor at multipliers[i].  Returns
        hidden_states[chosen_layer] as an fp32 leaf [n, 77, hidden] with requires_grad: build the loss on it."""
        flat, n_down, _ = self.network.engine_params()
        flat = flat.detach()
        ids = ids.to(torch.int64)
        eng = self.text_encoder.lora_engine(max(ids.shape[0], self.batch))
        out = self._forward_lora(eng, ids, flat, n_down, [float(m) for m in multipliers], True)
        self._pending = True
        return out.float().requires_grad_(True)

    @torch.no_grad()
    def encode_frozen(self, ids: torch.Tensor) -> torch.Tensor:
        """The un-adapted tower's hidden_states[chosen_layer] in fp32 (all multipliers 0: the bits of the plain encoder).
        Leaves a saved pass intact."""
        flat, n_down, _ = self.network.engine_params()
        flat = flat.detach()
        ids = ids.to(torch.int64)
        eng = self.text_encoder.lora_engine(max(ids.shape[0], self.batch))
        return self._forward_lora(eng, ids, flat, n_down, [0.0] * ids.shape[0], False).float()

    def backward(self, d_hidden: torch.Tensor):
        """d_hidden: the gradient of the loss with respect to what `forward` returned (its `.grad`).  Accumulates into
        `network.flat.grad` (created as zeros when absent), as loss.backward() would."""
        if not self._pending:
            raise _native.SmiError("TextEncoderStep.backward: no forward to differentiate (one backward per forward)")
        self._pending = False
        flat = self.network.flat
        if flat.grad is None:
            flat.grad = torch.zeros_like(flat)
        n_down = self.network._n_down
        eng = self.text_encoder.lora_engine(max(d_hidden.shape[0], self.batch))
        eng.backward(d_hidden.to(torch.float32).contiguous(), flat.grad[:n_down], flat.grad[n_down:],
                     which=0 if self.chosen_layer == -1 else 1)


# ---------------------------------------------------------------------------------------------------------------
# the loss of notrigger/train_notrigger.py, restated on plain tensors (N = the reference file, line numbers cited)
# ---------------------------------------------------------------------------------------------------------------
def fixed_distance_loss(trainable_embs, target_embs, fixed_distance):
    """N:45-64: the squared step of at most `fixed_distance` from the trainable embeddings towards their target.  The
    reference computes it every step of a two-sided run and then trains on the curriculum loss instead (N:430-439): it
    enters no gradient there, and is kept for the record."""
    diff = target_embs - trainable_embs
    current = torch.norm(diff, dim=-1, keepdim=True)
    direction = diff / (current + 1e-8)
    clamped = torch.clamp(fixed_distance.unsqueeze(-1), -current, current)
    target = trainable_embs + direction * clamped
    return ((trainable_embs - target) ** 2).mean()


def _cos(a, b):
    # N:320: cosine_similarity(v1.unsqueeze(0), v2.unsqueeze(0)) -- torch's default dim=1, which after the unsqueeze is the
    # batch axis of length 1: the reference's call, kept as it is
    return torch.nn.functional.cosine_similarity(a.unsqueeze(0), b.unsqueeze(0)).squeeze()


def direction_regulariser(trainable, own_target, other_target, neutral):
    """N:316-324 (positive side) and N:352-360 (negative side, roles swapped): |cos(v1, v2) - cos(v1r, v2)| + cos(v1, v2)
    + 1 / (mse(trainable, other_target) + 1e-8), v1 = trainable - neutral, v1r = own_target - neutral, v2 = other_target -
    neutral."""
    v1, v1r, v2 = trainable - neutral, own_target - neutral, other_target - neutral
    reg = torch.abs((_cos(v1, v2) - _cos(v1r, v2)).mean())
    reg = reg + _cos(v1, v2).mean()
    return reg + 1 / (((trainable - other_target) ** 2).mean() + 1e-8)


def notrigger_loss(trainable_pos, trainable_neg, pos, neg, neutral, norm_pos, norm_neg, lambda_similarity):
    """What the reference differentiates in one step (N:371-439) and what it prints.  trainable_pos / trainable_neg: the
    empty prompt's embeddings under the adaptor at +1 / -1 (None on a one-sided run, with its target); pos / neg / neutral:
    the un-adapted tower on the positive / negative / empty prompt; norm_pos / norm_neg: |pos - trainable_pos| and |neg -
    trainable_neg| at step 0 (N:304, 343: `distance * split`).  Returns (total, dict of scalars for the log).
    One-sided (N:306-307, 344-345, 414-415): the MSE to the one target.  Two-sided: the curriculum loss w_p pperc + w_n nperc
    with pperc = |pos - trainable_pos| / norm_pos (N:396-403), weights that keep their gradients (N:421-432: pperc / nperc are
    not detached), plus (1 - w_r) lambda (reg_p + reg_n) (N:381, 428, 433)."""
    if trainable_neg is None:
        total = ((pos - trainable_pos) ** 2).mean()
        return total, {"reconstruction": total.detach(), "curriculum": total.detach()}
    if trainable_pos is None:
        total = ((neg - trainable_neg) ** 2).mean()
        return total, {"reconstruction": total.detach(), "curriculum": total.detach()}
    similarity = lambda_similarity * direction_regulariser(trainable_pos, pos, neg, neutral) + \
        lambda_similarity * direction_regulariser(trainable_neg, neg, pos, neutral)
    recon = ((pos - trainable_pos) ** 2).mean() + ((neg - trainable_neg) ** 2).mean()  # N:388
    pperc = torch.norm(pos - trainable_pos) / norm_pos
    nperc = torch.norm(neg - trainable_neg) / norm_neg
    diff = torch.abs(pperc - nperc)
    scale_factor = 1 + 4 * (1 - torch.exp(-diff / 0.05))
    w_p = (pperc * scale_factor) / (pperc * scale_factor + nperc * scale_factor)
    w_n = (nperc * scale_factor) / (pperc * scale_factor + nperc * scale_factor)
    w_r = torch.clamp((nperc + pperc) / 2, max=0.95)  # N:428 min(0.95, .)
    loss = w_p * pperc + w_n * nperc
    total = loss + (1.0 - w_r) * similarity
    return total, {"reconstruction": recon.detach(), "curriculum": loss.detach(), "pperc": pperc.detach(),
                   "nperc": nperc.detach(), "similarity": ((1.0 - w_r) * similarity).detach()}
