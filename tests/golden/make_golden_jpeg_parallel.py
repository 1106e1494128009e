"""Writes tests/golden/jpeg_parallel.npz: three JPEG files without restart markers whose single scan is long enough for
``jpeg.decode(entropy="auto")`` to choose the parallel entropy stage (longer than ``jpeg.AUTO_THRESHOLD`` bytes), made with Pillow, and
the pixels Pillow itself decodes from them - the layout of jpeg.npz (make_golden_jpeg.py).  The tests read only the .npz.

    python tests/golden/make_golden_jpeg_parallel.py

Cases: ``p420`` 4:2:0 with the standard Huffman tables, ``p420opt`` 4:2:0 with optimised tables, ``pgrey`` one component; all
120 x 160, noise over a gradient.
"""
import io
import os.path as osp

import numpy as np
from PIL import Image, features
import PIL

HERE = osp.dirname(osp.abspath(__file__))


def noisy_gradient(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / w, 255 * y / h, 255 * (x + y) / (w + h)], -1) + rng.normal(0, 40, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


CASES = {
    "p420": (noisy_gradient(120, 160, 21), dict(quality=92, subsampling=2)),
    "p420opt": (noisy_gradient(120, 160, 22), dict(quality=92, subsampling=2, optimize=True)),
    "pgrey": (noisy_gradient(120, 160, 23)[..., 1], dict(quality=92)),
}


def main():
    out = {"versions": np.array([PIL.__version__, str(features.version("jpg")), str(features.check_feature("libjpeg_turbo"))])}
    for name, (img, kw) in CASES.items():
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        data = b.getvalue()
        im = Image.open(io.BytesIO(data))
        out[f"file_{name}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"pixels_{name}"] = np.asarray(im if im.mode == "L" else im.convert("RGB"))
        print(name, img.shape, len(data), "bytes", "FF00 x", data.count(b"\xff\x00"))
    path = osp.join(HERE, "jpeg_parallel.npz")
    np.savez_compressed(path, **out)
    print(path, osp.getsize(path), "bytes", out["versions"])


if __name__ == "__main__":
    main()
