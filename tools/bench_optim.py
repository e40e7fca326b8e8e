"""us per call of the three native optimiser steps (smi_clip_adamw, smi_clip_lion, smi_clip_prodigy) at the SD-XL rank-4
and rank-8 LoRA parameter counts (the train_lora_xl adaptor set: noxattn), clipping at 0.2 as that trainer does, next to
the byte bound: algorithmic bytes (AdamW 28 B, Lion 20 B, Prodigy 52 B per parameter, + 4 B for the norm's read of the
gradient) over --peak-tbs.  The steps alternate in one process; device events around --calls calls each, after a warm-up.
A report, nothing more.
    python tools/bench_optim.py [--calls 200] [--rounds 3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sliders_conceptmod_amd import _native  # noqa: E402
import sliders_conceptmod_amd.lora as L  # noqa: E402
import sliders_conceptmod_amd.unet as PU  # noqa: E402

BYTES = {"adamw": 28, "lion": 20, "prodigy": 52}  # read + written per parameter, without the clip's norm pass (+ 4)


def sdxl_lora_params(rank: int) -> int:
    with torch.device("meta"):
        unet = PU.UNet2DConditionModel(PU.sdxl_config())
    net = L.LoRANetwork(unet, rank=rank, multiplier=1.0, delimiter="_", target_replace=["Attention"], prefix="lora_unet",
                        train_method="noxattn")
    return net._n_down + net._n_up


def timed(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the three steps; the median is reported")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the byte bound is taken against, TB/s")
    ap.add_argument("--max-norm", type=float, default=0.2)
    args = ap.parse_args()
    print(f"optimiser steps, clip {args.max_norm}: {args.calls} calls per timing, median of {args.rounds} alternations")
    print("rank  parameters  step      us/call   bound us   achieved TB/s")
    for rank in (4, 8):
        n = sdxl_lora_params(rank)
        g = torch.Generator(device="cuda").manual_seed(rank)
        p = torch.randn(n, device="cuda", generator=g) * 0.05
        grad = torch.randn(n, device="cuda", generator=g) * 1e-3
        m, v, s, p0 = (torch.zeros(n, device="cuda") for _ in range(4))
        scratch = torch.empty(4096, device="cuda")
        state = torch.zeros(_native.PRODIGY_STATE_DOUBLES, dtype=torch.float64, device="cuda")
        hyper = _native.prodigy_hyper()
        _native.prodigy_init(p, p0, m, v, s, state)
        count = [0]

        def adamw():
            count[0] += 1
            _native.clip_adamw(p, grad, m, v, 1e-4, count[0], scratch, weight_decay=1e-6, max_grad_norm=args.max_norm)

        steps = {
            "adamw": adamw,
            "lion": lambda: _native.clip_lion(p, grad, m, 1e-4, scratch, max_grad_norm=args.max_norm),
            "prodigy": lambda: _native.clip_prodigy(p, grad, p0, m, v, s, state, scratch, hyper, args.max_norm),
        }
        for fn in steps.values():  # warm-up
            timed(fn, 20)
        times = {k: [] for k in steps}
        for _ in range(args.rounds):
            for k, fn in steps.items():
                times[k].append(timed(fn, args.calls))
        for k in steps:
            us = sorted(times[k])[len(times[k]) // 2]
            nbytes = n * (BYTES[k] + (4 if args.max_norm > 0 else 0))
            print(f"{rank:4d}  {n:10d}  {k:8s} {us:8.1f}  {nbytes / args.peak_tbs / 1e6:9.1f}  {nbytes / us / 1e6:10.2f}")


if __name__ == "__main__":
    main()
