"""Writes tests/golden/photometric_pil.npz: Pillow's own outputs for the photometric augmentation's steps on a handful of small
8-bit images -- ``ImageEnhance.Brightness`` / ``ImageEnhance.Contrast`` (what torchvision's ColorJitter ends in for a PIL image;
saturation and hue are the identity on mode L) in both orders, and ``Image.point`` with the gamma table.

torchvision is not installed here: the gamma table is its published formula ``int((255 + 1 - 1e-3) * (l / 255) ** gamma)``
restated, so parity with ``F.adjust_gamma`` is restated, not pinned; the Pillow calls are the real ones.  The images, the cases
and their parameters come from tests/photometric_ref.py (shared with the tests); the file records them next to the outputs,
with the Pillow version.

    python tests/golden/make_photometric_golden.py        # rewrites tests/golden/photometric_pil.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import photometric_ref as R  # noqa: E402

OUT = os.path.join(HERE, "photometric_pil.npz")


def pil_gamma_table(gamma):
    return [int((255 + 1 - 1e-3) * pow(l / 255.0, gamma)) for l in range(256)]


def pil_case(img8, kind, order, b, c, gamma):
    im = Image.fromarray(img8, mode="L")
    if kind == "brightness":
        im = ImageEnhance.Brightness(im).enhance(b)
    elif kind == "contrast":
        im = ImageEnhance.Contrast(im).enhance(c)
    elif order == 0:
        im = ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(b)).enhance(c)
    elif order == 1:
        im = ImageEnhance.Brightness(ImageEnhance.Contrast(im).enhance(c)).enhance(b)
    if not np.isnan(gamma):
        im = im.point(pil_gamma_table(gamma))
    assert im.mode == "L"
    return np.array(im)


def build():
    cs = R.cases()
    out = {"pillow_version": np.array(PIL.__version__),
           "kinds": np.array([k for (k, *_) in cs]),
           "params": np.array([[o, b, c, g] for (_, o, b, c, g) in cs], dtype=np.float64),       # order (-1: no jitter), b, c, gamma (nan: none)
           "gammas": np.array(R.GAMMAS, dtype=np.float64),
           "gamma_tables": np.array([pil_gamma_table(g) for g in R.GAMMAS], dtype=np.uint8),
           "names": np.array(sorted(R.images()))}
    for name, img in R.images().items():
        out[f"img_{name}"] = img
        out[f"out_{name}"] = np.stack([pil_case(img, *c) for c in cs])
    return out


if __name__ == "__main__":
    data = build()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays,", len(data["kinds"]), "cases, Pillow", PIL.__version__)
