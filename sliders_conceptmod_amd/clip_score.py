"""CLIP score of a slider sweep: eval-scripts/clip_score.py on the HIP engine, from the folder `generate_images` writes
(`<im_path>/<scale>/<case>_<num>.png`) to `<im_path>/clip_scores.csv`.

    python -m sliders_conceptmod_amd.clip_score --im_path images/age_slider --prompt "an old person" \\
        --prompts_path prompts.csv --clip_model /models/clip-vit-base-patch32

As the eval script: sub-folders of `im_path` whose name contains `all` or `.csv` are skipped and the rest sorted; images
are taken in natural sort order; the case number is the file name up to the first `_`, and cases that are not in the
CSV's `case_number` column are skipped; `half` reads `0.5` in the column name `clip_<folder>`; a value is the mean of
`logits_per_image[0][0]` (exp(logit_scale) x cosine similarity of the image and the prompt) over a case's images; cases
without images are NaN; `Mean CLIP score:` is printed per folder.

Differences from the eval script, on purpose:
  * images are scored in batches of `--batch_size`, not one by one.  The image tower gives an image the same bits alone
    or in a batch, so the batch size never changes a CSV;
  * a value is written to the row whose `case_number` matches.  The eval script writes to the row whose INDEX LABEL
    equals the case number, which is another row (or a new one) whenever the CSV's case numbers are not 0, 1, 2, ...;
  * `--from_case` / `--till_case`, which the eval script parses and ignores, bound `case_number` (the defaults select
    everything);
  * an unreadable image raises, naming the file.  The eval script's bare `except: pass` turns every failure -- a
    truncated PNG as much as a missing CUDA device -- into a silent NaN;
  * `--clip_model` names a local transformers directory or `synthetic://tiny_clip | vit_b32 | vit_l14`; the eval script
    hard-codes the hub name openai/clip-vit-base-patch32."""
from __future__ import annotations

import argparse
import os
import re
from typing import Callable, Dict, List, Sequence

import numpy as np

DTYPES = ("fp16", "bf16")


def natural_key(name: str):
    return [int(c) if c.isdigit() else c for c in re.split("([0-9]+)", name)]


def scale_folders(im_path: str) -> List[str]:
    return sorted(m for m in os.listdir(im_path) if "all" not in m and ".csv" not in m)


def column_name(folder: str) -> str:
    return "clip_" + folder.replace("half", "0.5")


def case_of(file_name: str) -> int:
    return int(file_name.split("_")[0].replace(".png", ""))


def folder_images(folder: str, cases: Sequence[int], from_case: int, till_case: int) -> Dict[int, List[str]]:
    """case number -> image paths of `folder` in natural sort order, for the cases of the CSV inside the bounds"""
    wanted = {int(c) for c in cases if from_case <= int(c) <= till_case}
    out: Dict[int, List[str]] = {}
    for name in sorted(os.listdir(folder), key=natural_key):
        try:
            case = case_of(name)
        except ValueError:
            continue  # not a <case>_<num> file name
        if case in wanted:
            out.setdefault(case, []).append(os.path.join(folder, name))
    return out


def score_sweep(im_path: str, df, scorer: Callable[[List[str]], Sequence[float]], from_case: int = 0,
                till_case: int = 1000000, log=print):
    """Adds one `clip_<folder>` column per scale folder to `df` (a pandas frame with a `case_number` column): the mean
    of `scorer(paths)` over a case's images, in the row(s) whose case_number matches."""
    cases = [int(c) for c in df["case_number"]]
    for folder in scale_folders(im_path):
        col = column_name(folder)
        df[col] = np.nan
        by_case = folder_images(os.path.join(im_path, folder), cases, from_case, till_case)
        paths = [p for ps in by_case.values() for p in ps]
        scores = dict(zip(paths, (float(s) for s in scorer(paths)))) if paths else {}
        for case, ps in by_case.items():
            df.loc[df["case_number"] == case, col] = float(np.mean([scores[p] for p in ps]))
        log(folder)
        log(f"Mean CLIP score: {df[col].mean()}")
        log("-------------------------------------------------")
    return df


class ClipScorer:
    """paths -> logits_per_image[:, 0] against one prompt: host preprocessing (PIL), the image tower on uint8 batches,
    smi_clip_logits against the prompt's embedding (computed once)."""

    def __init__(self, model, tokenizer, image_size: int, prompt: str, batch_size: int, device):
        import torch
        self.model, self.size, self.batch_size, self.device = model, image_size, max(1, batch_size), device
        ids = tokenizer([prompt], padding=True, return_tensors="pt").input_ids
        self.text_embeds = model.get_text_features(torch.as_tensor(ids).to(device))

    def __call__(self, paths: List[str]) -> List[float]:
        import torch
        from PIL import Image
        from .clip import clip_image_preprocess
        out: List[float] = []
        for i in range(0, len(paths), self.batch_size):
            batch = []
            for p in paths[i:i + self.batch_size]:
                try:
                    with Image.open(p) as im:
                        batch.append(clip_image_preprocess(im, self.size))
                except Exception as e:
                    raise RuntimeError(f"cannot read image '{p}': {e}") from e
            rgb8 = torch.from_numpy(np.stack(batch)).to(self.device)
            emb = self.model.get_image_features(rgb8=rgb8)
            out.extend(self.model.logits(emb, self.text_embeds)[:, 0].cpu().tolist())
        return out


def build_parser():
    p = argparse.ArgumentParser(prog="python -m sliders_conceptmod_amd.clip_score",
                                description="CLIP score of a slider sweep (eval-scripts/clip_score.py) on the MI355X.")
    p.add_argument("--im_path", required=True, help="folder with one sub-folder of images per slider scale")
    p.add_argument("--prompt", required=True, help="prompt to score the images against")
    p.add_argument("--prompts_path", required=True, help="CSV with a case_number column")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--till_case", type=int, default=1000000)
    p.add_argument("--from_case", type=int, default=0)
    p.add_argument("--clip_model", default="synthetic://vit_b32",
                   help="local transformers CLIPModel directory or synthetic://tiny_clip | vit_b32 | vit_l14")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--dtype", choices=DTYPES, default="fp16")
    return p


def main(argv=None):
    import pandas as pd
    import torch
    from . import model_util
    args = build_parser().parse_args(argv)
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    model, tokenizer, size = model_util.load_clip(args.clip_model)
    model = model.to(device, torch.float16 if args.dtype == "fp16" else torch.bfloat16)
    prompt = args.prompt.strip()
    print(f"Eval against prompt: {prompt}")
    scorer = ClipScorer(model, tokenizer, size, prompt, args.batch_size, device)
    df = score_sweep(args.im_path, pd.read_csv(args.prompts_path), scorer, args.from_case, args.till_case)
    out = os.path.join(args.im_path, "clip_scores.csv")
    df.to_csv(out, index=False)
    print(out)


if __name__ == "__main__":
    main()
