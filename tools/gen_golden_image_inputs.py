"""tests/golden/image_inputs.npz: what the installed Pillow makes of small frames through the four calls of the reference's
img_transform_core (resize, crop, transpose(FLIP_LEFT_RIGHT), rotate(0)).  Per case of image_input_refs.FIXTURE_CASES: the frame,
the parameters (Hs, Ws, newW, newH, x0, y0, x1, y1, flip) and the canvas bytes; the Pillow version is recorded in the file.

    python tools/gen_golden_image_inputs.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_input_refs as R  # noqa: E402


def pillow_canvas(frame, resize_dims, crop, flip, rotate=0):
    img = Image.fromarray(frame)
    img = img.resize(resize_dims)
    img = img.crop(crop)
    if flip:
        img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
    img = img.rotate(rotate)
    return np.array(img)


def main():
    out = {"pillow_version": np.array(PIL.__version__), "cases": np.array(R.FIXTURE_CASES)}
    for i, name in enumerate(R.FIXTURE_CASES):
        Hs, Ws, dims, crop, flip = R.CASES[name]
        frame = R.frame(Hs, Ws, R.PATTERNS[i % 3], seed=10 + i)
        out["frame_" + name] = frame
        out["params_" + name] = np.array([Hs, Ws, dims[0], dims[1], *crop, int(flip)], np.int32)
        out["canvas_" + name] = pillow_canvas(frame, dims, crop, flip)
    path = os.path.join(ROOT, "tests", "golden", "image_inputs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
