"""LPIPS of a slider sweep against its un-edited images: eval-scripts/lpip_score.py on the HIP engine, from the folder
`generate_images` writes (`<im_path>/<scale>/<case>_<num>.png`) to `<im_path>/lpips_score.csv`.

    python -m sliders_conceptmod_amd.lpips_score --im_path images/age --prompts_path prompts.csv --true 0 \\
        [--lpips_model synthetic://alex|<dir>] [--imsize 64] [--batch_size 64] [--dtype fp16|bf16] [--device cuda:0]

As the eval script: the scale folders are every entry of `im_path` except the one equal to `--true`, the one equal to
`all`, and names containing `.csv`; a folder's files are the names containing `.png`; a case's files are those starting
with `<case_number>_`; `half` reads `0.5` in the column name `lpips_<folder>`; a value is the mean over a case's files of
LPIPS(original, edited) with the original of the same name in the `--true` folder; a case without files is NaN (the
script's np.mean of nothing); the file names and `Case <n>: <mean>` are printed.  The loader is the script's: PIL
bilinear resize of the SMALLER edge to `--imsize` with the other edge int(imsize * long / short) (what
`transforms.Resize` does to a PIL image), no crop, `/ 255`, `(x - 0.5) * 2`.  The resize runs on the host with PIL; the
rescaling to [-1, 1] and everything after it runs in the stem kernel.

Differences from the eval script, on purpose:
  * pairs are scored in batches of `--batch_size`, grouped by their (H, W) after the resize, not one by one.  The engine
    gives a pair the same bits alone or in a batch, so the batch size never changes a CSV;
  * images are converted to RGB (the script feeds an RGBA or grey PNG to a 3-channel network and fails);
  * an edited file whose original is missing is skipped with a `No File` line, as the script does -- but an image that
    exists and cannot be read raises, naming the file, and so does a pair whose two sizes differ, naming both files.
    The script's `except Exception` turns each of these, and a missing CUDA device, into the same silent `No File`;
  * a case number is taken from its column, not from `iterrows`, which turns it into `4.0` -- and the case into one
    without files -- as soon as every column of the CSV is numeric;
  * `--lpips_model` names local weights or `synthetic://alex | tiny_alex`; the script downloads from the hub;
  * `--imsize` is an argument (default 64, the script's constant)."""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

DTYPES = ("fp16", "bf16")


def scale_folders(im_path: str, true: str) -> List[str]:
    return [m for m in sorted(os.listdir(im_path)) if m not in (true, "all") and ".csv" not in m]


def column_name(folder: str) -> str:
    return "lpips_" + folder.replace("half", "0.5")


def folder_files(folder: str) -> List[str]:
    return sorted(name for name in os.listdir(folder) if ".png" in name)


def case_files(file_names: Sequence[str], case_number) -> List[str]:
    return [f for f in file_names if f.startswith(f"{case_number}_")]


def resized_size(w: int, h: int, imsize: int) -> Tuple[int, int]:
    """(width, height) after `transforms.Resize(imsize)` of a PIL image: the smaller edge becomes imsize, the other
    int(imsize * long / short); an image whose smaller edge already is imsize is left alone"""
    short, long = (w, h) if w <= h else (h, w)
    if short == imsize:
        return w, h
    new_long = int(imsize * long / short)
    return (imsize, new_long) if w <= h else (new_long, imsize)


def load_rgb8(path: str, imsize: int) -> np.ndarray:
    """uint8 [H, W, 3] of the resized image; raises RuntimeError naming the file when it cannot be read"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            im = im.convert("RGB")
            size = resized_size(im.size[0], im.size[1], imsize)
            if size != im.size:
                im = im.resize(size, resample=Image.BILINEAR)
            return np.asarray(im, dtype=np.uint8)
    except Exception as e:
        raise RuntimeError(f"cannot read image '{path}': {e}") from e


class LpipsScorer:
    """[(original path, edited path)] -> LPIPS per pair: host loading (PIL), then uint8 batches per (H, W) on the engine"""

    def __init__(self, model, imsize: int, batch_size: int, device):
        self.model, self.imsize, self.batch_size, self.device = model, imsize, max(1, batch_size), device

    def __call__(self, pairs: Sequence[Tuple[str, str]]) -> List[float]:
        import torch
        from . import lpips as PL
        by_size: Dict[Tuple[int, int], List[int]] = {}
        images = []
        for i, (orig, edit) in enumerate(pairs):
            a, b = load_rgb8(orig, self.imsize), load_rgb8(edit, self.imsize)
            if a.shape != b.shape:
                raise RuntimeError(f"'{orig}' is {a.shape[1]}x{a.shape[0]} after the resize and '{edit}' is "
                                   f"{b.shape[1]}x{b.shape[0]}: LPIPS compares images of one size")
            if min(a.shape[:2]) < PL.MIN_SIZE:
                raise RuntimeError(f"'{orig}': {a.shape[1]}x{a.shape[0]} after the resize is below the {PL.MIN_SIZE}x"
                                   f"{PL.MIN_SIZE} the AlexNet tower takes (--imsize {self.imsize})")
            images.append((a, b))
            by_size.setdefault(a.shape[:2], []).append(i)
        out = [float("nan")] * len(pairs)
        for idx in by_size.values():
            for j in range(0, len(idx), self.batch_size):
                part = idx[j:j + self.batch_size]
                a = torch.from_numpy(np.stack([images[i][0] for i in part])).to(self.device)
                b = torch.from_numpy(np.stack([images[i][1] for i in part])).to(self.device)
                for i, d in zip(part, self.model.distance(a, b).cpu().tolist()):
                    out[i] = float(d)
        return out


def score_sweep(im_path: str, df, true: str, scorer, log=print):
    """Adds one `lpips_<folder>` column per scale folder to `df` (a pandas frame with a `case_number` column), row by
    row as the eval script does"""
    original_path = os.path.join(im_path, true)
    for folder in scale_folders(im_path, true):
        edited_path = os.path.join(im_path, folder)
        names = folder_files(edited_path)
        col = column_name(folder)
        df[col] = np.nan
        rows = []  # (index label, case number, pairs)
        # (not iterrows: in a frame of numbers only it hands the case number back as a float, and `4.0_` starts no file name)
        for index, case_number in df["case_number"].items():
            if isinstance(case_number, float) and case_number.is_integer():
                case_number = int(case_number)
            pairs = []
            for f in case_files(names, case_number):
                log(f)
                if os.path.isfile(os.path.join(original_path, f)):
                    pairs.append((os.path.join(original_path, f), os.path.join(edited_path, f)))
                else:
                    log("No File")
            rows.append((index, case_number, pairs))
        flat = [p for _, _, pairs in rows for p in pairs]
        scores = iter(scorer(flat) if flat else [])
        for index, case_number, pairs in rows:
            vals = [next(scores) for _ in pairs]
            mean = float(np.mean(vals)) if vals else float("nan")
            log(f"Case {case_number}: {mean}")
            df.loc[index, col] = mean
    return df


def build_parser():
    p = argparse.ArgumentParser(prog="python -m sliders_conceptmod_amd.lpips_score",
                                description="LPIPS of a slider sweep against its un-edited images "
                                            "(eval-scripts/lpip_score.py) on the MI355X.")
    p.add_argument("--im_path", required=True, help="folder with one sub-folder of images per slider scale")
    p.add_argument("--prompts_path", required=True, help="CSV with a case_number column")
    p.add_argument("--true", required=True, help="sub-folder of im_path with the un-edited images (normally 0)")
    p.add_argument("--lpips_model", default="synthetic://alex",
                   help="local directory (or two files joined by a comma) with the AlexNet and lin weights, or "
                        "synthetic://alex | tiny_alex")
    p.add_argument("--imsize", type=int, default=64, help="the smaller edge after the resize")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--dtype", choices=DTYPES, default="fp16")
    p.add_argument("--device", default="cuda:0")
    return p


def main(argv=None):
    import pandas as pd
    import torch
    from . import model_util
    args = build_parser().parse_args(argv)
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    model = model_util.load_lpips(args.lpips_model)
    model = model.to(device, torch.float16 if args.dtype == "fp16" else torch.bfloat16)
    scorer = LpipsScorer(model, args.imsize, args.batch_size, device)
    df = score_sweep(args.im_path, pd.read_csv(args.prompts_path), args.true, scorer)
    out = os.path.join(args.im_path, "lpips_score.csv")
    df.to_csv(out, index=False)
    print(out)


if __name__ == "__main__":
    main()
