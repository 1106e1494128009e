"""The demo's 2D pose stage around the network, the parts that need no GPU: the numpy restatement (tests/pose2d_ref.py) against itself
on blobs of known centres, the flip pairs, the status rules, the C interface and the wrappers' argument checks.  No value was recorded
from mmpose or OpenCV."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import pose2d_ref as PR
from pmce_amd import _lib, build, demo, pose2d

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def test_symbols_prototyped_and_built_without_packed_fp32():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_pose_patches", 20), ("pmce_pose_decode", 22)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "pose2d.hip" in build.SOURCES and build.FILE_FLAGS["pose2d.hip"] == build.NO_PACKED_FP32


def test_entry_points_reject_bad_arguments_on_the_host():
    """PMCE_ERR_ARG before anything is launched: no GPU is touched (the device pointers are never followed)."""
    lib = _lib.load()
    fake = C.c_void_p(4096)
    fi = np.array([0, 2, 5], dtype=np.int32)
    host = fi.ctypes.data_as(C.POINTER(C.c_int))
    warp = lambda F=6, H=8, W=8, n=3, pad=1.25, hp=256, wp=192, fr=fake: lib.pmce_pose_patches(   # noqa: E731
        fr, F, H, W, host, fake, fake, n, 1, pad, hp, wp, 0, 1, fake, fake, None, fake, fake, None)
    assert warp(F=5) == -1 and "frame_index[2] = 5" in _lib.last_error()
    assert warp(hp=1) == -1 and warp(wp=1025) == -1 and "2..1024" in _lib.last_error()
    assert warp(n=0) == -1 and warp(H=0) == -1 and warp(W=16385) == -1
    assert warp(pad=0.0) == -1 and warp(pad=float("nan")) == -1 and warp(pad=float("inf")) == -1
    assert warp(fr=None) == -1
    perm = (C.c_int * 17)(*PR.flip_perm(PR.COCO_FLIP_PAIRS, 17))
    taps = PR.blur_taps().ctypes.data_as(C.POINTER(C.c_float))
    dec = lambda n=2, K=17, hh=64, wh=48, fl=fake, pm=perm, h=fake, tp=taps: lib.pmce_pose_decode(   # noqa: E731
        h, 1, 1, 1, 1, fl, 1, 1, 1, 1, n, K, hh, wh, pm, tp, fake, None, fake, None, None, None)
    assert dec(n=0) == -1 and dec(K=0) == -1 and dec(K=65) == -1 and "1..64" in _lib.last_error()
    assert dec(hh=5) == -1 and dec(wh=5) == -1 and dec(wh=4097) == -1 and "6..4096" in _lib.last_error()
    assert dec(pm=None) == -1 and dec(h=None) == -1 and dec(tp=None) == -1
    bad = (C.c_int * 17)(*([17] + list(range(1, 17))))
    assert dec(pm=bad) == -1 and "perm[0] = 17" in _lib.last_error()


def test_flip_pairs_are_a_permutation():
    perm = pose2d.flip_permutation(pose2d.COCO_FLIP_PAIRS, 17)
    assert perm == PR.flip_perm(PR.COCO_FLIP_PAIRS, 17) == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    assert sorted(perm) == list(range(17)) and [perm[p] for p in perm] == list(range(17))
    assert pose2d.flip_permutation((), 3) == [0, 1, 2]
    for bad in (((1, 1),), ((0, 17),), ((1, 2), (2, 3)), ((-1, 0),), (1, 2), ((1, 2, 3),)):
        with pytest.raises(ValueError):
            pose2d.flip_permutation(bad, 17)
    assert np.array_equal(pose2d.blur_taps().view(np.int32), PR.blur_taps().view(np.int32))
    g = PR.blur_taps().astype(np.float64)
    assert abs(g.sum() - 1.0) < 1e-6 and np.allclose(g[4] / g[5], np.exp(-1 / 8.0), rtol=1e-6) and np.array_equal(g, g[::-1])


def test_restatement_recovers_blob_centres():
    """The fp64 restatement finds the centres of Gaussian blobs (sigma 2, the blur's own) under noise: median error below 0.05 px at
    64 x 48 (measured: 0.013 px).  Its fp32 run deviates from it by about 7e-6 px at 64 x 48 and 4e-5 px at 6 x 6; asserted here an
    order of magnitude above those, and > 0: the GPU tests' bound is a multiple of this deviation and must not be vacuous."""
    for (Hh, Wh), limit in (((64, 48), 1e-4), ((16, 12), 1e-3), ((6, 6), 1e-3)):
        heat, centres = PR.blobs(4, 17, Hh, Wh)
        cs = PR.centre_scales(4)
        kp64, xy64, arg64 = PR.decode(heat, cs, dtype=np.float64)
        kp32, xy32, arg32 = PR.decode(heat, cs, dtype=np.float32)
        assert kp64.dtype == np.float64 and kp32.dtype == np.float32 and np.array_equal(arg64, arg32)
        dev = float(np.abs(xy32.astype(np.float64) - xy64).max())
        err = np.linalg.norm(xy64 - centres, axis=-1)
        print(f"{Hh} x {Wh}: fp64 median error {np.median(err):.4f} px, fp32 - fp64 {dev:.2e} px")
        assert 0.0 < dev < limit
        if (Hh, Wh) == (64, 48):
            assert np.median(err) < 0.05
        # back in the image: the heatmap's corners are the box's corners
        wt, ht = cs[:, 2:3].astype(np.float64), cs[:, 3:4].astype(np.float64)
        want = xy64 * np.stack([wt / (Wh - 1), ht / (Hh - 1)], -1) + cs[:, None, :2] - 0.5 * cs[:, None, 2:]
        assert np.allclose(kp64[..., :2], want, rtol=0, atol=1e-9) and np.array_equal(kp64[..., 2], heat.max((-1, -2)).astype(np.float64))


def test_restatement_exact_cases():
    cs = PR.centre_scales(1)
    flat = np.full((1, 3, 8, 7), 0.25, np.float32)
    flat[0, 1] = -0.5                                        # a maximum <= 0: (-1, -1), unrefined
    flat[0, 2, 3, 4] = flat[0, 2, 5, 1] = 0.75               # two equal maxima: the first in row-major order
    kp, xy, arg = PR.decode(flat, cs)
    assert arg.tolist() == [[[0, 0], [-1, -1], [4, 3]]]
    assert xy[0, 0].tolist() == [0.0, 0.0] and xy[0, 1].tolist() == [-1.0, -1.0]
    assert kp[0, :, 2].tolist() == [0.25, -0.5, 0.75]
    # the flip average: channel perm[k], column Wh - 1 - x
    h = np.zeros((1, 3, 6, 6), np.float32)
    hf = np.zeros((1, 3, 6, 6), np.float32)
    h[0, 1, 2, 1] = 1.0
    hf[0, 2, 4, 0] = 3.0
    A = PR.averaged(h, hf, [0, 2, 1])
    assert A[0, 1, 2, 1] == 0.5 and A[0, 1, 4, 5] == 1.5 and A.sum() == 2.0
    assert PR.decode(h, cs, hf, [0, 2, 1])[2][0, 1].tolist() == [5, 4]
    assert PR.decode(h, cs, status=np.array([1]))[0].tolist() == [[[0.0] * 3] * 3]


def test_restatement_map_and_status():
    size = (256, 192)
    # a box of exactly the aspect around the middle of a frame maps the patch's corners onto the padded box's corners
    cs, ok = PR.box2cs((96.0, 128.0, 96.0, 128.0), size)
    assert ok and cs[:2].tolist() == [96.0, 128.0] and np.allclose(cs[2:], [120.0, 160.0], rtol=3e-7, atol=0)      # a few fp32 roundings
    ix, tx, iy, ty = PR.udp_map(cs, size)
    assert abs(tx - 36.0) < 1e-4 and abs(ix * 191 + tx - 156.0) < 1e-4 and abs(ty - 48.0) < 1e-4 and abs(iy * 255 + ty - 208.0) < 1e-4
    # wider and taller boxes grow to the aspect; the two formats agree
    assert np.allclose(PR.box2cs((10.0, 10.0, 60.0, 20.0), size)[0], [10.0, 10.0, 75.0, 100.0], rtol=3e-7, atol=0)
    assert np.allclose(PR.box2cs((10.0, 10.0, 15.0, 40.0), size)[0], [10.0, 10.0, 37.5, 50.0], rtol=3e-7, atol=0)
    assert np.array_equal(PR.box2cs((-20.0, -10.0, 60.0, 40.0), size, "xywh")[0], PR.box2cs((10.0, 10.0, 60.0, 40.0), size)[0])
    # status
    fr = PR.frames()
    boxes = [(40.0, 30.0, 20.0, 30.0), (40.0, 30.0, 0.0, 30.0), (40.0, 30.0, 20.0, -1.0), (np.nan, 30.0, 20.0, 30.0),
             (40.0, np.inf, 20.0, 30.0), (40.0, 30.0, 1e9, 30.0), (3e6, 30.0, 20.0, 30.0), (40.0, 30.0, 1e-42, 1e-42), (40.0, 30.0, 20.0, 30.0)]
    f32, raw, cs, st = PR.pose_patches(fr, [0, 0, 0, 0, 0, 0, 0, 0, 2], boxes, size=(64, 48))
    assert st.tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 3]
    assert raw[0].any() and not raw[1:].any() and not cs[1:5].any() and cs[5:].any()
    assert np.array_equal(f32[1], PR.CR.normalise(np.zeros((64, 48, 3), np.uint8)))
    # wholly outside the frame: fine, and all border
    f32, raw, cs, st = PR.pose_patches(fr, [1], [(-400.0, -300.0, 30.0, 40.0)], size=(64, 48), mirror=True)
    assert st.tolist() == [0] and raw.shape == (2, 64, 48, 3) and not raw.any()


def test_wrapper_argument_errors():
    frames = np.zeros((2, 8, 9, 3), dtype=np.uint8)
    fi, boxes = np.array([0, 1]), np.array([[4.0, 4.0, 5.0, 5.0]] * 2)
    bad = [dict(frames_u8=frames.astype(np.float32)), dict(frames_u8=frames[0]), dict(frame_index=np.array([0, 2])),
           dict(frame_index=np.array([0.0, 1.0])), dict(frame_index=np.array([0])), dict(boxes=boxes[:, :3]), dict(boxes=boxes.astype(np.int64)),
           dict(size=256), dict(size=(256, 1)), dict(size=(1025, 192)), dict(size=(25.5, 19)), dict(padding=0.0), dict(padding=float("nan")),
           dict(channel_order="gbr"), dict(box_format="xyxy")]
    for kw in bad:
        args = dict(frames_u8=frames, frame_index=fi, boxes=boxes)
        args.update(kw)
        with pytest.raises(ValueError):
            pose2d.pose_patches(**args)
    heat = torch.zeros(2, 17, 64, 48)
    cs = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="device tensor"):
        pose2d.decode_heatmaps(heat, cs)                     # a host tensor
    with pytest.raises(ValueError, match="device tensor"):
        pose2d.decode_heatmaps(heat.numpy(), cs)
    with pytest.raises(ValueError, match="kernel must be 11"):
        pose2d.decode_heatmaps(heat, cs, kernel=7)

    class Net:
        cfg = dict(H=64, W=48, K=17)

        def __call__(self, x):
            raise AssertionError("not reached")

    for kw in (dict(chunk=0), dict(chunk=257), dict(kernel=3), dict(box_format="xyxy"), dict(channel_order="gbr"), dict(padding=-1.0),
               dict(flip_pairs=((1, 1),)), dict(flip_pairs=((16, 17),))):
        with pytest.raises(ValueError):
            pose2d.TopDownPose(Net(), **kw)
    with pytest.raises(ValueError):
        pose2d.TopDownPose(object())
    small = Net()
    small.cfg = dict(H=16, W=16, K=17)
    with pytest.raises(ValueError, match="at least 6 x 6"):
        pose2d.TopDownPose(small)
    pose = pose2d.TopDownPose(Net())
    assert pose.size == (64, 48) and pose.flip_test
    for kw in bad[:7]:
        args = dict(frames_u8=frames, frame_index=fi, boxes=boxes)
        args.update(kw)
        with pytest.raises(ValueError):
            pose(args["frames_u8"], args["frame_index"], args["boxes"])
    for tr in ([(boxes, np.arange(3))], [(boxes, np.array([0, 2]))], [(boxes, np.array([0.0, 1.0]))], [(boxes[:, :3], np.arange(2))],
               [(boxes.astype(np.int32), np.arange(2))]):
        with pytest.raises(ValueError):
            demo.pose_tracklets(frames, tr, pose)
    assert demo.pose_tracklets(frames, [], pose) == []
