"""Images per second of the CLIP image tower on the HIP engine, from uint8 crops to image_embeds
(`CLIPModel.get_image_features(rgb8=...)`: patchify + normalise, patch GEMM, embeddings + pre_layrnorm, the encoder,
post_layernorm, visual_projection), for ViT-B/32 and ViT-L/14 with synthetic weights in fp16 at batch 1 / 16 / 64.
Device-event timing after warm-up; TF/s against the algorithmic work computed here from the shapes (2 FLOPs per
multiply-add: patch GEMM, q/k/v/o, QK^T and PV, the MLP, the projection).  Next to each line, transformers' own
`CLIPModel.get_image_features` through PyTorch on the same device from the same images as normalised fp16
pixel_values -- if transformers imports there.

    python tools/bench_clip_score.py [--iters 20] [--warmup 3] [--models vit_b32,vit_l14] [--batches 1,16,64]
    python tools/bench_clip_score.py --flops-only          # the work table (no GPU)

One JSON line per (model, batch) on stdout."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tower_flops(cfg):
    """algorithmic FLOPs of one image through the tower"""
    d, inter, P = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    g2 = (cfg.image_size // P) ** 2
    L = g2 + 1
    fl = 2.0 * g2 * d * 3 * P * P
    per_layer = 4 * 2.0 * L * d * d + 2 * 2.0 * L * L * d + 2 * 2.0 * L * d * inter
    fl += cfg.num_hidden_layers * per_layer
    return fl + 2.0 * d * (cfg.projection_dim or 0)


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


def transformers_model(name, cfg_v, cfg_t):
    try:
        import transformers
    except Exception:
        return None
    t = transformers.CLIPTextConfig(vocab_size=cfg_t.vocab_size, hidden_size=cfg_t.hidden_size,
                                    intermediate_size=cfg_t.intermediate_size,
                                    num_hidden_layers=cfg_t.num_hidden_layers,
                                    num_attention_heads=cfg_t.num_attention_heads, projection_dim=cfg_t.projection_dim)
    v = transformers.CLIPVisionConfig(hidden_size=cfg_v.hidden_size, intermediate_size=cfg_v.intermediate_size,
                                      num_hidden_layers=cfg_v.num_hidden_layers,
                                      num_attention_heads=cfg_v.num_attention_heads, image_size=cfg_v.image_size,
                                      patch_size=cfg_v.patch_size, projection_dim=cfg_v.projection_dim)
    cfg = transformers.CLIPConfig(text_config=t.to_dict(), vision_config=v.to_dict(), projection_dim=cfg_v.projection_dim)
    return transformers.CLIPModel(cfg).eval().to("cuda", torch.float16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="vit_b32,vit_l14")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--flops-only", action="store_true", help="print the work table and exit (no GPU)")
    a = ap.parse_args()
    import sliders_conceptmod_amd.clip as PC
    cfgs = {"vit_b32": (PC.vit_b32_text_config, PC.vit_b32_vision_config),
            "vit_l14": (PC.vit_l14_text_config, PC.vit_l14_vision_config)}
    batches = [int(b) for b in a.batches.split(",")]
    if a.flops_only:
        for name in a.models.split(","):
            print(json.dumps({"model": name, "gflop_per_image": round(tower_flops(cfgs[name][1]()) / 1e9, 2)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_score measures on the GPU; there is none here (use --flops-only for the work table)")
    from bench import init_synthetic_on_device
    for name in a.models.split(","):
        tc, vc = cfgs[name][0](), cfgs[name][1]()
        with torch.device("cuda"):
            model = PC.CLIPModel(tc, vc).to(torch.float16)
        init_synthetic_on_device(model, seed=5)
        model.requires_grad_(False).eval()
        hf = transformers_model(name, vc, tc)
        fl = tower_flops(vc)
        mean = torch.tensor(vc.image_mean, device="cuda").view(1, 3, 1, 1)
        std = torch.tensor(vc.image_std, device="cuda").view(1, 3, 1, 1)
        for n in batches:
            u8 = torch.randint(0, 256, (n, vc.image_size, vc.image_size, 3), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: model.get_image_features(rgb8=u8), a.warmup, a.iters)
            line = {"model": name, "batch": n, "dtype": "fp16", "ms": round(ms, 3), "images_per_s": round(n / ms * 1e3, 1),
                    "gflop_per_image": round(fl / 1e9, 2), "tf_s": round(n * fl / ms / 1e9, 1)}
            if hf is not None:
                px = ((u8.permute(0, 3, 1, 2).float() / 255 - mean) / std).half()
                with torch.no_grad():
                    ms_hf = timed(lambda: hf.get_image_features(pixel_values=px), a.warmup, a.iters)
                line.update({"transformers_ms": round(ms_hf, 3), "transformers_images_per_s": round(n / ms_hf * 1e3, 1)})
            else:
                line["transformers_ms"] = None  # not measured: transformers does not import here
            print(json.dumps(line), flush=True)
            model._close_engines()
            torch.cuda.empty_cache()
        del model, hf


if __name__ == "__main__":
    main()
