"""Writes tests/golden/jpeg.npz: small JPEG files made with Pillow (its bundled libjpeg-turbo, the library and the defaults behind
cv2.imread too) and the pixels Pillow itself decodes from them.  The tests read only the .npz, so they need no Pillow.

    python tests/golden/make_golden_jpeg.py

Per case NAME: ``file_NAME`` (uint8, the file's bytes) and ``pixels_NAME`` (uint8 [H, W, 3] R, G, B - or [H, W] for a grey file);
the refused cases carry the file alone.  ``versions``: PIL.__version__, the JPEG library's version, whether it is libjpeg-turbo.
"""
import io
import os.path as osp

import numpy as np
from PIL import Image, features
import PIL

HERE = osp.dirname(osp.abspath(__file__))


def smooth(h, w, seed):
    """A smooth colour field with a little noise and a saturated patch (so that the clamps and the chroma edges carry signal)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0), 128 + 110 * np.cos(x / 11.0 - y / 6.0),
                    40 + 200 * (x + 2 * y) / (w + 2 * h)], -1)
    img += rng.normal(0, 6, img.shape)
    img[h // 4:h // 4 + max(h // 3, 2), w // 3:w // 3 + max(w // 3, 2)] = (255, 0, 255)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def save(img, mode="RGB", **kw):
    b = io.BytesIO()
    im = Image.fromarray(img) if mode == "RGB" else Image.fromarray(img).convert(mode)
    im.save(b, "JPEG", **kw)
    return b.getvalue()


# name: (image, save arguments).  subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
CASES = {
    "a": (smooth(16, 16, 1), dict(quality=75, subsampling=2)),
    "b": (smooth(8, 8, 2), dict(quality=90, subsampling=0)),
    "c": (smooth(13, 17, 3), dict(quality=75, subsampling=2)),
    "d": (smooth(40, 64, 4), dict(quality=75, subsampling=2, restart_marker_blocks=1)),
    "e": (noise(40, 48, 5), dict(quality=100, subsampling=2, restart_marker_rows=1)),
    "f": (smooth(9, 33, 6), dict(quality=60, subsampling=1)),
    "g": (noise(24, 24, 7), dict(quality=5, subsampling=2)),
    "h": (noise(31, 45, 8), dict(quality=95, subsampling=2, optimize=True)),
    "i": (smooth(17, 9, 9)[..., 1], dict(quality=80)),
    "j0": (smooth(48, 64, 10), dict(quality=75, subsampling=2, restart_marker_rows=1)),
    "j1": (smooth(48, 64, 11), dict(quality=75, subsampling=2)),
    "j2": (smooth(48, 64, 12), dict(quality=80, subsampling=2)),
    "j3": (smooth(48, 64, 13), dict(quality=75, subsampling=2, restart_marker_rows=1)),
    "j4": (noise(48, 64, 14), dict(quality=85, subsampling=2)),
    # wider than one 256-pixel tile of the colour kernel, more rows than its 4, and 342 blocks for the 256-block groups of the inverse DCT
    "t": (smooth(40, 300, 15), dict(quality=75, subsampling=2)),
    # chroma planes of two columns: jdsample replicates them instead of filtering
    "m": (smooth(6, 3, 16), dict(quality=90, subsampling=2)),
    "m2": (smooth(5, 4, 17), dict(quality=90, subsampling=1)),
}
REFUSED = {
    "k": (smooth(16, 16, 18), "RGB", dict(quality=75, progressive=True)),
    "l": (smooth(16, 16, 19), "CMYK", dict(quality=75)),
}


def main():
    out = {"versions": np.array([PIL.__version__, str(features.version("jpg")), str(features.check_feature("libjpeg_turbo"))])}
    for name, (img, kw) in CASES.items():
        data = save(img, **kw)
        im = Image.open(io.BytesIO(data))
        px = np.asarray(im if im.mode == "L" else im.convert("RGB"))
        assert px.shape[:2] == img.shape[:2]
        out[f"file_{name}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"pixels_{name}"] = px
        print(name, img.shape, len(data), "bytes", "FF00 x", data.count(b"\xff\x00"))
    for name, (img, mode, kw) in REFUSED.items():
        out[f"file_{name}"] = np.frombuffer(save(img, mode, **kw), dtype=np.uint8)
    path = osp.join(HERE, "jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, osp.getsize(path), "bytes", out["versions"])


if __name__ == "__main__":
    main()
