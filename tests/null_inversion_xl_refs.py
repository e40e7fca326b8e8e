"""CPU restatement of SD-XL null-text optimisation (sliders_conceptmod_amd/null_inversion_xl.py: the notebook's
NullInversion.ddim_loop and .null_optimization with the added conditioning carried through, and the unconditional pooled
embedding as a second Adam parameter) on the fp32 oracle UNet with torch autograd: the reference of
tests/test_null_inversion_xl_gpu.py.  Recipe: that of tests/null_inversion_refs.py on tiny_sdxl -- 8 x 8 latents, 4 DDIM
steps, 5 inner steps, early stop disabled, guidance 7.5; seed 5 draws x0, uncond, cond, pooled_uncond [1, P], pooled_cond
[1, P] in this order; time_ids = [64, 64, 0, 0, 64, 64]."""
import torch

from tests.null_inversion_refs import (GUIDANCE, HW, INNER, NO_EARLY_STOP, STEPS, XL_TIME_IDS, ddim_scheduler,  # noqa: F401
                                       oracle_null_optimization)

MODEL = "tiny_sdxl"
IMAGE_SIZE = 64
TIME_IDS = XL_TIME_IDS  # the oracle loop (tests/null_inversion_refs.py) conditions on them
GOLDEN = "null_inversion_xl_oracle.json"  # under tests/golden/: {"timesteps", "losses_pooled_off", "losses_pooled_on"}


def recipe(ctx_dim, pooled_dim, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(1, 4, HW, HW, generator=g)
    uncond = torch.randn(1, 77, ctx_dim, generator=g)
    cond = torch.randn(1, 77, ctx_dim, generator=g)
    pooled_u = torch.randn(1, pooled_dim, generator=g)
    pooled_c = torch.randn(1, pooled_dim, generator=g)
    return x0, uncond, cond, pooled_u, pooled_c


def pooled_dim(cfg):
    return cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim


if __name__ == "__main__":  # python -m tests.null_inversion_xl_refs: rewrites the golden file
    import json
    import os
    from tests.ctx_grad_refs import plain_oracle
    ou = plain_oracle(MODEL)
    args = recipe(ou.cfg.cross_attention_dim, pooled_dim(ou.cfg))
    off, ts = oracle_null_optimization(ou, *args, optimize_pooled=False)
    on, ts_on = oracle_null_optimization(ou, *args, optimize_pooled=True)
    assert ts == ts_on
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    json.dump({"timesteps": ts, "losses_pooled_off": off, "losses_pooled_on": on}, open(path, "w"), indent=1)
    print(path)
