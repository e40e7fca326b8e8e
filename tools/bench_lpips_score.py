"""Pairs per second of LPIPS (AlexNet) on the HIP engine, from uint8 pairs to distances (`LPIPS.distance`: stem +
patch matrices, five GEMMs, two max-pools, the distance head), with synthetic weights in fp16 at 64 x 64 and 256 x 256
and batch 1 / 64.  Device-event timing after warm-up.  Next to each line, the same metric restated in fp32 torch
(`F.conv2d`, `F.max_pool2d`) on the host's CPU with 16 threads -- the only other way to compute it where neither the
`lpips` nor the `torchvision` package is installed.  With --profile, the per-class times of one batch from the engine's
own event profile (patch matrices = "conv", GEMMs = "gemm", pool / head = "elementwise").

    python tools/bench_lpips_score.py [--iters 20] [--warmup 3] [--sizes 64,256] [--batches 1,64] [--profile]
    python tools/bench_lpips_score.py --flops-only          # the work table (no GPU)

One JSON line per (size, batch) on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tower_flops(channels, h, w):
    """algorithmic FLOPs of one IMAGE through the five convolutions (a pair is two)"""
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd.lpips import ALEX_GEOMETRY
    fl, cin = 0.0, 3
    for (ho, wo), (k, _, _), c in zip(_native.lpips_map_sizes(h, w), ALEX_GEOMETRY, channels):
        fl += 2.0 * ho * wo * c * k * k * cin
        cin = c
    return fl


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def torch_cpu_lpips(model):
    """the metric in fp32 torch on the CPU, from the container's parameters"""
    from sliders_conceptmod_amd.lpips import ALEX_GEOMETRY, SCALE, SHIFT, conv_names
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    shift, scale = torch.tensor(SHIFT).view(1, 3, 1, 1), torch.tensor(SCALE).view(1, 3, 1, 1)

    def run(u8a, u8b):
        n = u8a.shape[0]
        x = torch.cat([u8a, u8b]).permute(0, 3, 1, 2).float() / 127.5 - 1
        x = (x - shift) / scale
        total = 0
        for i, (name, (k, s, p)) in enumerate(zip(conv_names(), ALEX_GEOMETRY)):
            x = F.relu(F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=s, padding=p))
            f = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            total = total + (((f[:n] - f[n:]) ** 2) * sd[f"lin{i}.model.1.weight"]).sum(1).mean((1, 2))
            if i < 2:
                x = F.max_pool2d(x, 3, 2)
        return total
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--profile", action="store_true", help="per-class times of one batch (engine event profile)")
    ap.add_argument("--flops-only", action="store_true", help="print the work table and exit (no GPU)")
    a = ap.parse_args()
    from sliders_conceptmod_amd import _native, model_util
    from sliders_conceptmod_amd.lpips import ALEX_CHANNELS
    sizes = [int(s) for s in a.sizes.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
    if a.flops_only:
        for s in sizes:
            print(json.dumps({"size": s, "gflop_per_pair": round(2 * tower_flops(ALEX_CHANNELS, s, s) / 1e9, 3)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_score measures on the GPU; there is none here (use --flops-only for the work table)")
    model = model_util.load_lpips("synthetic://alex").to("cuda", torch.float16)
    torch.set_num_threads(16)
    cpu = torch_cpu_lpips(model)
    for s in sizes:
        fl = 2 * tower_flops(ALEX_CHANNELS, s, s)
        for n in batches:
            ua = torch.randint(0, 256, (n, s, s, 3), dtype=torch.uint8, device="cuda")
            ub = torch.randint(0, 256, (n, s, s, 3), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: model.distance(ua, ub), a.warmup, a.iters)
            line = {"size": s, "batch": n, "dtype": "fp16", "ms": round(ms, 3), "pairs_per_s": round(n / ms * 1e3, 1),
                    "gflop_per_pair": round(fl / 1e9, 3), "tf_s": round(n * fl / ms / 1e9, 2)}
            ca, cb = ua.cpu(), ub.cpu()
            with torch.no_grad():
                cpu(ca, cb)
                reps = 3 if n * s * s <= 64 * 64 * 64 else 1
                t0 = time.perf_counter()
                for _ in range(reps):
                    cpu(ca, cb)
                ms_cpu = (time.perf_counter() - t0) / reps * 1e3
            line.update({"torch_cpu_fp32_ms": round(ms_cpu, 3), "torch_cpu_pairs_per_s": round(n / ms_cpu * 1e3, 1)})
            if a.profile:
                eng = model._engine(n, s, s)
                lib = _native.lib()
                _native.check(lib.smi_profile_enable(eng.handle, 1), "smi_profile_enable")
                model.distance(ua, ub)
                k = len(_native.Engine.PROF_CLASSES)
                pms, pfl, pby = (C.c_double * k)(), (C.c_double * k)(), (C.c_double * k)()
                pla = (C.c_int64 * k)()
                _native.check(lib.smi_profile_read(eng.handle, pms, pfl, pby, pla), "smi_profile_read")
                _native.check(lib.smi_profile_enable(eng.handle, 0), "smi_profile_enable")
                line["profile_us"] = {c: {"us": round(pms[i] * 1e3, 1), "launches": pla[i]}
                                      for i, c in enumerate(_native.Engine.PROF_CLASSES) if pla[i]}
            print(json.dumps(line), flush=True)
        model._close_engines()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
