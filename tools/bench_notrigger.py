"""ms per training iteration of the no-trigger text-encoder step at the two SD-XL tower shapes (n = 2 samples at
multipliers +1 / -1, L = 77, rank 4): the engine step (one saved forward of two samples + one backward) next to torch-ROCm
autograd through the restatement of tests/notrigger_refs.py (fp32 on the same GPU).  The two arms alternate in one
process; the table goes into DESIGN section 15.  No threshold.  The torch arm IS the test restatement (imported from tests/):
this tool measures against it on purpose and is of no use without the test tree.  The engine arm's figure includes building
the loss on the fp32 leaf and a fresh zeroed `flat.grad` per iteration (`net.flat.grad = None`), as a first step would.

    python tools/bench_notrigger.py [--rounds 3] [--iters 10] [--towers clip_l,bigg]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import notrigger_refs as R  # noqa: E402
import sliders_conceptmod_amd.clip as PC  # noqa: E402
from sliders_conceptmod_amd import model_util  # noqa: E402
from sliders_conceptmod_amd.lora import CLIP_TARGET_REPLACE, LoRANetwork  # noqa: E402
from sliders_conceptmod_amd.notrigger import TextEncoderStep  # noqa: E402


def timed(fn, iters):
    fn()  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--towers", default="clip_l,bigg")
    a = ap.parse_args()
    rows = []
    for which in a.towers.split(","):
        cfg, cls = (PC.clip_l_config(), PC.CLIPTextModel) if which == "clip_l" else (PC.open_clip_bigg_config(), PC.CLIPTextModelWithProjection)
        enc = model_util.init_synthetic_clip_(cls(cfg), seed=1)
        sd32 = {k: v.detach().float().cuda() for k, v in enc.state_dict().items()}
        enc.to("cuda", torch.bfloat16)
        torch.manual_seed(0)
        net = LoRANetwork(enc, rank=4, alpha=1.0, target_replace=CLIP_TARGET_REPLACE, prefix="lora_te1", train_method="full").to("cuda")
        with torch.no_grad():
            net.flat[net._n_down:].normal_(0, 0.02)
        step = TextEncoderStep(enc, net)
        ids = torch.full((2, 77), cfg.eos_token_id, dtype=torch.int64, device="cuda")
        ids[:, 0] = cfg.eos_token_id - 1
        target = torch.randn((2, 77, cfg.hidden_size), device="cuda")

        def engine_iter():
            net.flat.grad = None
            h = step.forward(ids, [1.0, -1.0])
            ((h - target) ** 2).mean().backward()
            step.backward(h.grad)

        mods = sorted(net.unet_loras, key=lambda l: l.off_down)
        names = [l.target_path for l in mods]
        leaves = {l.target_path: (l.lora_down.weight.detach().clone().requires_grad_(True), l.lora_up.weight.detach().clone().requires_grad_(True)) for l in mods}
        flat = [t for n in names for t in leaves[n]]

        def torch_iter():
            h = R.tower_forward(sd32, ids, cfg.num_attention_heads, cfg.hidden_act, leaves, [1.0, -1.0], 0.25)["last_layer_out"]
            torch.autograd.grad(((h - target) ** 2).mean(), flat)

        eng, ref = [], []
        for _ in range(a.rounds):
            eng.append(timed(engine_iter, a.iters))
            ref.append(timed(torch_iter, a.iters))
        row = {"tower": which, "engine_ms": eng, "torch_fp32_autograd_ms": ref}
        print(json.dumps(row), flush=True)
        rows.append(row)
        enc._close_engines()
    return rows


if __name__ == "__main__":
    main()
