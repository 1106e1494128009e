"""The JPEG writer on the GPU (csrc/jpeg_encode.hip) against Pillow's recorded files (tests/golden/jpeg_enc.npz) and the numpy
restatement (tests/jpeg_enc_ref.py).  Every comparison is exact: the files' bytes, int16 coefficients, offsets and status words."""
import os
import os.path as osp

import numpy as np
import pytest
import torch

import jpeg_enc_ref as ER
import jpeg_ref as JR
from pmce_amd import _lib, demo, jpeg

pytestmark = pytest.mark.gpu

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = np.load(osp.join(REPO, "tests", "golden", "jpeg_enc.npz"))
SHARED = {"q50": "q1", "rrow": "r1", "r3": "r1", "r3n": "e"}
SUBSAMPLING = ("4:4:4", "4:2:2", "4:2:0")
# p*: 1 x 1 in the three samplings; b: 8 x 8 at 4:4:4; c, h: 17 x 13 and 45 x 31 noise at 95; m, m2, f: 3 x 6, 4 x 5 and 33 x 9 (W x H) with
# chroma planes of a few columns; v, v2: 16 x 18 and 50 x 30, even heights whose chroma rows below the image repeat the last DOWNSAMPLED
# row; tall: 16 x 1080, the demo's height with its dummy luma block row; t: 300 x 40, wider than one 256-column tile of the coefficient
# stage; e: noise at quality 100 (values of ten bits, 35 stuffed bytes); g: quality 5; q1: quality 1; q50: 4:4:4 at the base tables; big:
# 1056 blocks in one interval, more than one pass of the offset scan; r1, rrow, r3: 28, 14 and 10 restart intervals; r3n: noise with RSTn.
FILES = ["p444", "p422", "p420", "b", "c", "h", "m", "m2", "f", "v", "v2", "tall", "t", "e", "g", "q1", "q50", "big", "r1", "rrow", "r3",
         "r3n"]


def dev():
    return torch.device("cuda:0")


def case(name):
    quality, sub, restart = (int(x) for x in GOLD[f"args_{name}"])
    return GOLD[f"image_{SHARED.get(name, name)}"], bytes(GOLD[f"file_{name}"]), quality, SUBSAMPLING[sub], restart


def bgr(images):
    """uint8 [F, H, W, 3] R, G, B on the host -> B, G, R on the device, contiguous"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(images)[..., ::-1])).to(dev())


def smooth(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    img = np.stack([3 * x + 2 * y + 10 * seed, 250 - 4 * x + y, 40 + 5 * y], -1) + rng.integers(0, 9, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("name", FILES)
def test_file_equals_pillow_to_the_byte(name):
    img, want, quality, sub, restart = case(name)
    # (noise at quality 100 is longer than the default capacity of 1.5 bytes per sample: e, r3n)
    cap = jpeg.encode_capacity(img.shape[1], img.shape[0], sub, restart, worst_case=True) if quality == 100 else None
    data, offsets, status = jpeg.encode(bgr(img[None]), quality=quality, subsampling=sub, restart_interval=restart, capacity=cap)
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and status.dtype == torch.int32
    assert tuple(offsets.shape) == (2,) and tuple(status.shape) == (1,)
    assert offsets.cpu().tolist() == [0, len(want)] and status.cpu().tolist() == [0]
    got = jpeg.files(data, offsets, status)
    assert len(got) == 1 and got[0] == want
    if name == "big":
        g = ER.geometry(img.shape[1], img.shape[0], sub)
        assert g["n_blocks"] > _lib.load().pmce_jpeg_encode_scan_pass()           # the offset scan carries its total into a second pass
    if name in ("r1", "rrow", "r3"):
        assert want.count(b"\xff\xd7") >= 1 and want.count(b"\xff\xd0") >= 2      # RSTn wrapped


@pytest.mark.parametrize("name", ["h", "v", "tall", "f", "q50", "m"])
def test_coefficients_equal_the_restatement(name):
    """The first stage alone: zigzag order, scan order, the dummy blocks' DC (tall: a whole dummy row; m, h: a dummy column too)."""
    img, _, quality, sub, _ = case(name)
    want, g = ER.coefficients(img, quality, sub)
    *_, coef = jpeg.encode(bgr(img[None]), quality=quality, subsampling=sub, return_coefficients=True)
    assert coef.dtype == torch.int16 and tuple(coef.shape) == (1, g["n_blocks"], 64)
    assert int((coef[0].cpu().numpy() != want).sum()) == 0


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2"])
def test_wide_frames_in_the_other_samplings(sub):
    """More than one 256-column tile of the coefficient stage at 4:4:4 (32 MCUs per tile) and 4:2:2 (16), two frames, with a restart
    interval that crosses the tiles; against the restatement, which the host tests pin to Pillow in these samplings."""
    img = case("t")[0]                                                            # 300 x 40
    images = np.stack([img[:21], img[19:]])
    want = [ER.encode(im, 80, sub, 7) for im in images]
    assert jpeg.files(*jpeg.encode(bgr(images), quality=80, subsampling=sub, restart_interval=7)) == want


def test_restart_interval_longer_than_the_scan():
    """DRI is written, no marker follows: one interval."""
    img = case("v")[0]                                                            # 16 x 18: two MCUs
    want = ER.encode(img, 75, "4:2:0", 5)
    assert b"\xff\xdd\x00\x04\x00\x05" in want and b"\xff\xd0" not in want
    assert jpeg.files(*jpeg.encode(bgr(img[None]), quality=75, restart_interval=5)) == [want]
    assert jpeg.files(*jpeg.encode(bgr(img[None]), quality=75, restart_interval=2)) == [ER.encode(img, 75, "4:2:0", 2)]


@pytest.mark.parametrize("restart", [0, 1, 2])
def test_entropy_stages_alone_on_crafted_coefficients(restart):
    """DC differences of +-2047, AC of +-1023, runs of 15, 16, 32, 48 and 62 zeros, coefficient 63, all-zero blocks, 0xFF bytes at every
    place in a word and across the borders of blocks and pieces (tests/test_jpeg_enc_host.py asserts that the stream has them)."""
    coef = ER.crafted_coefficients()
    header = b"\xff\xd8\xff\xda"
    want = header + ER.entropy_code(coef, 1, restart) + b"\xff\xd9"
    two = np.stack([coef, coef[::-1].copy()])
    want2 = header + ER.entropy_code(two[1], 1, restart) + b"\xff\xd9"
    data, offsets, status = jpeg.encode_entropy(torch.from_numpy(two).to(dev()), 1, header, restart_interval=restart, guard=64)
    assert status.cpu().tolist() == [0, 0] and offsets.cpu().tolist() == [0, len(want), len(want) + len(want2)]
    assert jpeg.files(data, offsets, status) == [want, want2]
    assert bool((data[len(want) + len(want2):] == 0xA5).all())                   # nothing is written beyond offsets[F]


def test_batch_chunks_channel_order_and_repeat():
    images = np.stack([smooth(24, 40, k) if k % 2 else np.random.default_rng(k).integers(0, 256, (24, 40, 3), dtype=np.uint8)
                       for k in range(5)])
    frames = bgr(images)
    alone = [jpeg.files(*jpeg.encode(frames[k:k + 1]))[0] for k in range(5)]
    assert len(set(alone)) == 5 and alone[1] == ER.encode(images[1]) and alone[2] == ER.encode(images[2])
    data, offsets, status = jpeg.encode(frames, chunk=2)
    assert jpeg.files(data, offsets, status) == alone
    assert offsets.cpu().tolist() == [0] + list(np.cumsum([len(a) for a in alone]))
    assert jpeg.files(*jpeg.encode(frames, chunk=5)) == alone and jpeg.files(*jpeg.encode(frames, chunk=2)) == alone
    rgb = torch.from_numpy(images).to(dev())
    assert jpeg.files(*jpeg.encode(rgb, channel_order="rgb", chunk=3)) == alone
    timings = []
    assert jpeg.files(*jpeg.encode(frames, chunk=3, timings=timings)) == alone          # launch by launch: the same bytes
    assert [t[0] for t in timings] == 2 * (["coefficients"] + list(jpeg.ENCODE_STAGES))


def test_a_frame_beyond_the_capacity_is_served_empty():
    noise, want_noise, quality, sub, _ = case("e")                                # 48 x 40 noise at quality 100: 4630 bytes
    images = np.stack([smooth(40, 48, 1), noise, smooth(40, 48, 2)])
    want = [ER.encode(im, 100, "4:2:0") for im in images]
    assert want[1] == want_noise and max(len(want[0]), len(want[2])) <= 4000 < len(want[1])
    data, offsets, status = jpeg.encode(bgr(images), quality=100, capacity=4000, guard=128)
    assert status.cpu().tolist() == [0, jpeg.STATUS_CAPACITY, 0]
    off = offsets.cpu().tolist()
    assert off == [0, len(want[0]), len(want[0]), len(want[0]) + len(want[2])]
    raw = data.cpu().numpy().tobytes()
    assert raw[off[0]:off[1]] == want[0] and raw[off[2]:off[3]] == want[2]
    assert len(raw) == 3 * 4000 + 128 and set(raw[off[3]:]) == {0xA5}            # the unused capacity and the guard: untouched
    with pytest.raises(ValueError, match="frame 1"):
        jpeg.files(data, offsets, status)
    # with the helper's worst case every frame fits
    cap = jpeg.encode_capacity(48, 40, worst_case=True)
    assert jpeg.files(*jpeg.encode(bgr(images), quality=100, capacity=cap)) == want


def test_save_frames_then_load_frames(tmp_path):
    img, want, quality, sub, _ = case("t")                                        # 300 x 40 at quality 75
    images = np.stack([img, img[:, ::-1].copy()])
    names = demo.save_frames(str(tmp_path / "out"), bgr(images), first=7, quality=quality, subsampling=sub)
    assert names == ["000007.jpg", "000008.jpg"] and sorted(os.listdir(tmp_path / "out")) == names
    assert (tmp_path / "out" / names[0]).read_bytes() == want
    frames, wh, loaded = demo.load_frames(str(tmp_path / "out"))
    assert loaded == names and wh == (300, 40)
    expect = np.stack([JR.decode(want)[0], JR.decode(ER.encode(images[1], quality, sub))[0]])
    assert int((frames.cpu().numpy() != expect[..., ::-1]).sum()) == 0


def test_render_folder_writes_both_folders(tmp_path, monkeypatch):
    img, want, quality, sub, _ = case("v2")                                       # 50 x 30
    src = tmp_path / "in"
    src.mkdir()
    (src / "000000.jpg").write_bytes(want)
    (src / "000001.jpg").write_bytes(ER.encode(img[::-1].copy(), quality, sub))
    monkeypatch.setattr(demo, "run_frames", lambda model, frames, *a, **kw: [{"person_id": 1, "frames": tuple(frames.shape)}])
    monkeypatch.setattr(demo, "render_tracklets", lambda outs, frames, wh, renderer=None, order="reference": 255 - frames)
    outs = demo.render_folder(None, str(src), str(tmp_path / "out"), None, None, None, "faces", input_folder=str(tmp_path / "again"),
                              encode_kwargs=dict(quality=quality))
    assert outs == [{"person_id": 1, "frames": (2, 30, 50, 3)}]
    decoded = [JR.decode((src / n).read_bytes())[0] for n in ("000000.jpg", "000001.jpg")]
    for k, n in enumerate(("000000.jpg", "000001.jpg")):
        assert (tmp_path / "again" / n).read_bytes() == ER.encode(decoded[k], quality, "4:2:0")
        assert (tmp_path / "out" / n).read_bytes() == ER.encode(255 - decoded[k], quality, "4:2:0")
