"""Device time of the AutoencoderKL decoder (`vae.decode(z).sample` + uint8 images) on the HIP engine, SD config with
synthetic weights: ms per image and TF/s against the algorithmic work computed here from the shapes (convs 2 HWout Cout
9 Cin, 1x1 shortcuts, q/k/v/o projections, the materialised mid attention 2 x 2 N^2 C; at the SD config 2.51 TFLOP per
512^2 image and 10.47 per 1024^2 image, 0.55 of it the attention).  Device-event timing after warm-up.

    python tools/bench_vae_decode.py [--iters 5] [--warmup 2] [--sizes 512x1,512x4,1024x1,1024x2] [--dtypes fp16,bf16]
    SMI_VAE_DEC_TAIL=0 python tools/bench_vae_decode.py ...     # the unfused tail (A/B)

One JSON line per (size, batch, dtype) on stdout.  The tail's byte bound (x read once, sample + uint8 written once, at
6.3 TB/s) is printed with each line; the tail's own time comes from a `rocprofv3 --kernel-trace --stats` run of this
tool."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3  # measured chip copy bandwidth, MI355X_MICROARCH chip table


def decoder_flops(boc, layers, h, w, latent=4, out_ch=3):
    """(total, attention) algorithmic FLOPs of one decoded h x w image."""
    L = len(boc)
    f = 2 ** (L - 1)
    hh, ww = h // f, w // f
    fl = 0.0
    conv = lambda hw, ci, co: 2.0 * hw * co * 9 * ci
    hw = hh * ww
    ch = boc[-1]
    fl += 2.0 * hw * latent * latent  # post_quant_conv
    fl += conv(hw, latent, ch)

    def resnet(hw, ci, co):
        r = conv(hw, ci, co) + conv(hw, co, co)
        return r + (2.0 * hw * ci * co if ci != co else 0.0)

    fl += 2 * resnet(hw, ch, ch)
    attn = 4 * 2.0 * hw * ch * ch + 2 * 2.0 * hw * hw * ch
    fl += attn
    for i, out in enumerate(reversed(boc)):
        for j in range(layers + 1):
            fl += resnet(hw, ch if j == 0 else out, out)
        ch = out
        if i != L - 1:
            hw *= 4
            fl += conv(hw, ch, ch)
    fl += conv(hw, ch, out_ch)
    return fl, attn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="512x1,512x4,1024x1,1024x2")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--flops-only", action="store_true", help="print the work table and exit (no GPU)")
    a = ap.parse_args()
    import sliders_conceptmod_amd.vae as PV
    cfg = PV.sd_vae_config()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    if a.flops_only:
        for res, _ in sizes:
            t, at = decoder_flops(cfg.block_out_channels, cfg.layers_per_block, res, res)
            print(json.dumps({"res": res, "tflop_per_image": round(t / 1e12, 3), "attn_tflop": round(at / 1e12, 3)}))
        return
    from sliders_conceptmod_amd import vae_decoder as PD
    from bench import init_synthetic_on_device
    dts = {"fp16": torch.float16, "bf16": torch.bfloat16}
    tail = "unfused" if os.environ.get("SMI_VAE_DEC_TAIL", "1") == "0" else "fused"
    for dname in a.dtypes.split(","):
        with torch.device("cuda"):
            vae = PD.AutoencoderKLDecoder(cfg).to(dts[dname])
        init_synthetic_on_device(vae, seed=5)
        vae.requires_grad_(False).eval()
        for res, n in sizes:
            z = torch.randn(n, 4, res // 8, res // 8, device="cuda")
            for _ in range(a.warmup):
                vae.decode_to_uint8(z)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                vae.decode_to_uint8(z)
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / a.iters
            fl, at = decoder_flops(cfg.block_out_channels, cfg.layers_per_block, res, res)
            c0 = cfg.block_out_channels[0]
            tail_bytes = n * res * res * (2 * c0 + 4 * 3 + 3)
            print(json.dumps({"res": res, "batch": n, "dtype": dname, "tail": tail, "ms": round(ms, 3),
                              "ms_per_image": round(ms / n, 3), "tflop_per_image": round(fl / 1e12, 3),
                              "tf_s": round(n * fl / ms / 1e9, 1),
                              "tail_byte_bound_us": round(tail_bytes / (HBM_TBS * 1e12) * 1e6, 1)}), flush=True)
            vae._close_engines()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
