"""Writes tests/golden/jpeg_enc.npz: small source images and the JPEG files Pillow (its bundled libjpeg-turbo, the library and the
defaults behind cv2.imwrite too) writes from them.  The tests read only the .npz, so they need no Pillow.

    python tests/golden/make_golden_jpeg_enc.py

Per case NAME: ``image_NAME`` (uint8 [H, W, 3], R, G, B), ``file_NAME`` (uint8, the file's bytes) and ``args_NAME`` (int64:
quality, subsampling 0 = 4:4:4 / 1 = 4:2:2 / 2 = 4:2:0, restart interval in MCUs).  Cases that share an image store it once
(``image_NAME`` of the case named in SHARED).  ``versions``: PIL.__version__, the JPEG library's version, whether it is libjpeg-turbo.
"""
import io
import os.path as osp

import numpy as np
from PIL import Image, features
import PIL

from make_golden_jpeg import noise, smooth

HERE = osp.dirname(osp.abspath(__file__))


def flat(h, w, seed):
    """Flat 16 x 16 patches with one patch of noise: many blocks, few bytes in the archive."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x // 16 * 37 + y // 16 * 11 + seed) % 256, (x // 16 * 5 + y // 16 * 53) % 256, (x // 16 * 101 + y // 16 * 29) % 256],
                   -1).astype(np.uint8)
    img[h // 2:h // 2 + 24, w // 2:w // 2 + 24] = noise(24, 24, seed)
    return img


# name: (image [H, W, 3], quality, subsampling, restart interval in MCUs).  MCUs per row of a 4:2:0 file: ceil(W / 16).
CASES = {
    "p444": (smooth(1, 1, 1), 95, 0, 0),
    "p422": (smooth(1, 1, 2), 95, 1, 0),
    "p420": (smooth(1, 1, 3), 95, 2, 0),
    "b": (smooth(8, 8, 4), 90, 0, 0),
    "c": (noise(13, 17, 5), 95, 2, 0),
    "h": (noise(31, 45, 6), 95, 2, 0),
    "m": (smooth(6, 3, 7), 90, 2, 0),
    "m2": (smooth(5, 4, 8), 90, 1, 0),
    "f": (smooth(9, 33, 9), 60, 1, 0),
    # an even height that is no multiple of 16: the chroma rows below the image repeat the last DOWNSAMPLED row
    "v": (smooth(18, 16, 10), 75, 2, 0),
    "v2": (smooth(30, 50, 11), 75, 2, 0),
    # the demo's height: 135 luma block rows are real, 136 are coded
    "tall": (smooth(1080, 16, 12), 95, 2, 0),
    "t": (smooth(40, 300, 13), 75, 2, 0),
    "e": (noise(40, 48, 14), 100, 2, 0),
    "g": (noise(24, 24, 15), 5, 2, 0),
    "q1": (smooth(20, 36, 16), 1, 2, 0),
    "q50": (smooth(20, 36, 16), 50, 0, 0),
    # 11 x 16 MCUs of 6 blocks: more blocks in one interval than one pass of the device's offset scan covers
    "big": (flat(256, 176, 17), 85, 2, 0),
    # 2 x 14 MCUs: 28, 14 and 10 restart intervals (RSTn wraps to RST0 again), 3 does not divide 28
    "r1": (smooth(210, 30, 18), 75, 2, 1),
    "rrow": (smooth(210, 30, 18), 75, 2, 2),
    "r3": (smooth(210, 30, 18), 75, 2, 3),
    "r3n": (noise(40, 48, 14), 100, 2, 3),
}
SHARED = {"q50": "q1", "rrow": "r1", "r3": "r1", "r3n": "e"}


def save(img, quality, subsampling, restart):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=subsampling, **(dict(restart_marker_blocks=restart) if restart else {}))
    return b.getvalue()


def main():
    out = {"versions": np.array([PIL.__version__, str(features.version("jpg")), str(features.check_feature("libjpeg_turbo"))])}
    for name, (img, quality, subsampling, restart) in CASES.items():
        data = save(img, quality, subsampling, restart)
        if name not in SHARED:
            out[f"image_{name}"] = img
        else:
            assert np.array_equal(img, CASES[SHARED[name]][0])
        out[f"file_{name}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"args_{name}"] = np.array([quality, subsampling, restart], dtype=np.int64)
        print(name, img.shape, len(data), "bytes", "FF00 x", data.count(b"\xff\x00"))
    path = osp.join(HERE, "jpeg_enc.npz")
    np.savez_compressed(path, **out)
    print(path, osp.getsize(path), "bytes", out["versions"])


if __name__ == "__main__":
    main()
