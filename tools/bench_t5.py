"""ms per encode of the T5-XXL encoder (t5.t5_xxl_config, seeded weights made on the device), n = 1, at L = 256 and 512 in
bf16: the native tower (sliders_conceptmod_amd.t5.T5EncoderModel on the HIP engine) next to `transformers.T5EncoderModel` on
the same weights, dtype and GPU, the two arms alternating in one process, each call ended by a device synchronise.  Prints
one JSON line per length and writes them to --out, with the two bounds of a pass next to the times: the matmul FLOP (every
GEMM and the two attention products, from the shapes) at the 2.5 PF/s bf16 matrix peak, and the bytes of the weights, read
once, at the 8 TB/s HBM peak -- and the fraction of each the native arm reaches.  No threshold: no time is a pass or fail
condition.

`--depths 1,2,4,8,24`: no timing; at each depth of the XXL-width model the relative L2 distance of the native tower and of
transformers' bf16 run from transformers' float32 run on the same seeded weights (how far two bf16 runs may be apart there).

`--train`: the trainable tower (smi_t5_lora_*: rank 4 on every SelfAttention.{q,k,v,o}, 96 sites at XXL), n = 2, multipliers
(+1, -1): the engine's forward_lora(save) + backward next to torch autograd through `transformers.T5EncoderModel` in bf16 with
the same adaptor (fp32 LoRA leaves, the delta added to the four projections' outputs) on the same GPU, arms alternating, every
phase ended by a device synchronise.  Per length: ms per arm with the forward / backward split, the engine's workspace bytes,
and the relative L2 distance of the two arms' LoRA gradients (down | up, all sites).  No ratio is a pass or fail condition.

    python tools/bench_t5.py [--rounds 3] [--iters 5] [--lengths 256,512] [--out profiles/t5_xxl_encode.json] [--tiny]
    python tools/bench_t5.py --depths 1,2,4,8,24 --lengths 256 --out profiles/t5_xxl_depth.json
    python tools/bench_t5.py --train [--rounds 3] [--iters 3] [--lengths 256,512] --out profiles/t5_train_xxl.json [--tiny]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sliders_conceptmod_amd import t5 as PT  # noqa: E402

MFMA_PEAK = 2.5e15  # bf16 dense, FLOP/s (spec)
HBM_PEAK = 8.0e12   # bytes/s (spec)


def timed(fn, iters):
    fn()  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def matmul_flop(cfg, n, L):
    """2 M N K of every GEMM + 4 n H L^2 d_kv of every attention."""
    inner = cfg.num_heads * cfg.d_kv
    per = 2.0 * n * L * cfg.d_model * (4 * inner + 3 * cfg.d_ff) + 4.0 * n * cfg.num_heads * L * L * cfg.d_kv
    return cfg.num_layers * per


def weight_bytes(cfg):
    """The matrices a pass reads once (bf16); the embedding is gathered, n L rows of it."""
    inner = cfg.num_heads * cfg.d_kv
    return 2.0 * cfg.num_layers * cfg.d_model * (4 * inner + 3 * cfg.d_ff)


def seeded_on_device(cfg, dev):
    """The native container built on the device in bf16 (no 19 GB float32 copy on the host) with t5.init_synthetic_'s
    distributions drawn there."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            model = PT.T5EncoderModel(cfg)
    finally:
        torch.set_default_dtype(old)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32)
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
            del r
    return model.requires_grad_(False).eval()


def twin_on_device(cfg, native, dev):
    import transformers
    hc = transformers.T5Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff,
                               num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                               relative_attention_num_buckets=cfg.relative_attention_num_buckets,
                               relative_attention_max_distance=cfg.relative_attention_max_distance,
                               layer_norm_epsilon=cfg.layer_norm_epsilon, feed_forward_proj=cfg.feed_forward_proj,
                               dropout_rate=0.0, use_cache=False, is_encoder_decoder=False)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            hf = transformers.T5EncoderModel(hc)
    finally:
        torch.set_default_dtype(old)
    hf.load_state_dict(native.state_dict())
    return hf.to(dev, torch.bfloat16).requires_grad_(False).eval()


def depth_sweep(depths, L, dev, out):
    """Seeded XXL-width weights at several depths: the relative L2 distance of the native tower and of transformers' bf16 run
    from transformers' float32 run on the same weights -- what two bf16 implementations may differ by at that depth."""
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    rows = []
    for layers in depths:
        cfg = PT.T5Config(num_layers=layers)
        native = seeded_on_device(cfg, dev)
        twin = twin_on_device(cfg, native, dev)
        ids = torch.randint(0, cfg.vocab_size, (1, L), generator=torch.Generator().manual_seed(L)).to(dev)
        with torch.no_grad():
            a, b = native(ids)[0].float(), twin(ids)[0].float()
            c = twin.float()(ids)[0]
        row = {"layers": layers, "L": L, "native_vs_fp32": rel(a, c), "transformers_bf16_vs_fp32": rel(b, c),
               "native_vs_transformers_bf16": rel(a, b)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del native, twin
        torch.cuda.empty_cache()
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


class _TwinLora(torch.nn.Module):
    """A frozen Linear of the transformers model with the adaptor's delta on its output: y + m_i scale (x down^T) up^T."""

    def __init__(self, base, down, up, scale, mults):
        super().__init__()
        self.base, self.down, self.up, self.scale, self.mults = base, down, up, scale, mults

    def forward(self, x):
        d = (x @ self.down.to(x.dtype).t()) @ self.up.to(x.dtype).t()
        return self.base(x) + (self.mults.to(x.dtype)[:, None, None] * self.scale) * d


def train_bench(args, cfg, native, twin, dev):
    """--train (module docstring)."""
    from sliders_conceptmod_amd import lora as LM
    rank, n, mults = 4, 2, [1.0, -1.0]
    torch.manual_seed(0)
    net = LM.LoRANetwork(native, rank=rank, multiplier=1.0, alpha=float(rank), target_replace=LM.T5_TARGET_REPLACE,
                         prefix="lora_te2", train_method="t5attn").to(dev)
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0.0, 0.02)  # lora_up not zero: the adaptor acts and lora_down gets a gradient
    flat, n_down = net.flat.detach(), net._n_down
    sites = sorted(net.unet_loras, key=lambda l: l.off_down)
    # the twin's adaptor: fp32 leaves holding the same values, in the flat buffers' order
    leaves, mt = [], torch.tensor(mults, device=dev)
    for l in sites:
        down = l.lora_down.weight.detach().clone().requires_grad_(True)
        up = l.lora_up.weight.detach().clone().requires_grad_(True)
        leaves.append((down, up))
        parent = twin.get_submodule(l.target_path.rsplit(".", 1)[0])
        leaf = l.target_path.rsplit(".", 1)[1]
        setattr(parent, leaf, _TwinLora(getattr(parent, leaf), down, up, float(l.scale), mt))
    params = [t for pair in leaves for t in pair]
    rows = []
    for L in [int(v) for v in args.lengths.split(",")]:
        native.max_tokens = max(native.max_tokens, L)
        ids = torch.randint(0, cfg.vocab_size, (n, L), generator=torch.Generator().manual_seed(L)).to(dev)
        d_hidden = torch.randn((n, L, cfg.d_model), generator=torch.Generator().manual_seed(L + 1)).to(dev)
        eng = native.lora_engine(n)
        dd, du = torch.zeros(n_down, device=dev), torch.zeros(flat.numel() - n_down, device=dev)

        def native_step(t):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.forward_lora(ids, flat[:n_down], flat[n_down:], mults, save=True, want=("last_hidden",))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.backward(d_hidden, dd, du, which=0)
            torch.cuda.synchronize()
            t.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))

        def twin_step(t):
            for p in params:
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = twin(ids)[0]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            (out.float() * d_hidden).sum().backward()
            torch.cuda.synchronize()
            t.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))

        # one pass of each for the gradients (and as the warm-up), then the timed rounds, arms alternating
        dd.zero_(), du.zero_()
        native_step([])
        g_native = torch.cat([dd, du]).double()
        twin_step([])
        g_twin = torch.cat([torch.cat([d.grad.reshape(-1) for d, _ in leaves]), torch.cat([u.grad.reshape(-1) for _, u in leaves])]).double()
        dist = float((g_native - g_twin).norm() / g_twin.norm())
        tn, tt = [], []
        for _ in range(args.rounds):
            for _ in range(args.iters):
                native_step(tn)
            for _ in range(args.iters):
                twin_step(tt)
        best = lambda t, i: min(v[i] for v in t)
        total = lambda t: min(v[0] + v[1] for v in t)
        row = {"model": "tiny_t5" if args.tiny else "t5_xxl", "dtype": "bf16", "n": n, "L": L, "rank": rank, "sites": len(sites),
               "multipliers": mults, "native_ms": total(tn), "native_forward_ms": best(tn, 0), "native_backward_ms": best(tn, 1),
               "transformers_ms": total(tt), "transformers_forward_ms": best(tt, 0), "transformers_backward_ms": best(tt, 1),
               "native_over_transformers": total(tn) / total(tt), "workspace_bytes": eng.workspace.numel(),
               "rel_l2_gradients_native_vs_transformers": dist, "finite": bool(torch.isfinite(g_native).all())}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--lengths", default="256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_xxl_encode.json"))
    ap.add_argument("--depths", default=None, help="e.g. 1,2,4,8,24: instead of timing, the distance of both bf16 arms from "
                    "transformers' float32 run at these depths (the first of --lengths), written to --out")
    ap.add_argument("--train", action="store_true", help="time forward_lora(save) + backward of the tower with LoRA sites next to "
                    "torch autograd through transformers with the same adaptor (n = 2, rank 4, every SelfAttention projection)")
    ap.add_argument("--tiny", action="store_true", help="tiny_t5_config(64) instead of T5-XXL: a rehearsal of the tool itself")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_t5 measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    if args.depths:
        return depth_sweep([int(v) for v in args.depths.split(",")], int(args.lengths.split(",")[0]), dev, args.out)
    cfg = PT.tiny_t5_config(64) if args.tiny else PT.t5_xxl_config()
    native = seeded_on_device(cfg, dev)
    twin = twin_on_device(cfg, native, dev)
    if args.train:
        return train_bench(args, cfg, native, twin, dev)
    rows = []
    for L in [int(v) for v in args.lengths.split(",")]:
        ids = torch.randint(0, cfg.vocab_size, (1, L), generator=torch.Generator().manual_seed(L)).to(dev)
        with torch.no_grad():
            a = native(ids)[0].float()
            b = twin(ids)[0].float()
        dist = float((a - b).norm() / b.norm())
        t_native, t_twin = [], []
        with torch.no_grad():
            for _ in range(args.rounds):  # the arms alternate: both see the same machine
                t_native.append(timed(lambda: native(ids), args.iters))
                t_twin.append(timed(lambda: twin(ids), args.iters))
        flop, wbytes = matmul_flop(cfg, 1, L), weight_bytes(cfg)
        ms = min(t_native)
        row = {"model": "tiny_t5" if args.tiny else "t5_xxl", "dtype": "bf16", "n": 1, "L": L,
               "native_ms": ms, "native_ms_rounds": t_native, "transformers_ms": min(t_twin), "transformers_ms_rounds": t_twin,
               "native_over_transformers": ms / min(t_twin), "rel_l2_native_vs_transformers": dist,
               "matmul_flop": flop, "matmul_bound_ms": flop / MFMA_PEAK * 1e3, "fraction_of_matmul_bound": flop / MFMA_PEAK * 1e3 / ms,
               "weight_bytes": wbytes, "weight_bound_ms": wbytes / HBM_PEAK * 1e3, "fraction_of_weight_bound": wbytes / HBM_PEAK * 1e3 / ms,
               "native_tflops": flop / ms * 1e-9, "workspace_bytes": native._engine(1).workspace.numel()}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
