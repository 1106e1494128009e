"""The demo's person crops, the parts that need no GPU: the C interface, the numpy oracle (tests/crops_ref.py) against vectors recorded
from the reference's own functions (tests/golden/crops.npz, made by tests/golden/make_golden_crops.py), and the wrappers' argument checks."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import crops_ref as CR
from pmce_amd import _lib, build, crops, demo

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = np.load(osp.join(REPO, "tests", "golden", "crops.npz"))


def test_symbols_prototyped_and_built_without_packed_fp32():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_crop_boxes", 8), ("pmce_crop_patches", 16)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "crops.hip" in build.SOURCES and build.FILE_FLAGS["crops.hip"] == build.NO_PACKED_FP32


def test_entry_points_reject_bad_arguments_on_the_host():
    """The argument checks return PMCE_ERR_ARG before anything is launched: no GPU is touched (the pointers are never followed)."""
    lib = _lib.load()
    fake = C.c_void_p(4096)
    fi = np.array([0, 2, 5], dtype=np.int32)
    host = fi.ctypes.data_as(C.POINTER(C.c_int))
    call = lambda F=6, H=8, W=8, hostp=host, n=3, scale=1.1, S=224: lib.pmce_crop_patches(   # noqa: E731
        fake, F, H, W, hostp, fake, fake, n, scale, S, 0, fake, fake, None, fake, None)
    assert call(F=5) == -1 and "frame_index[2] = 5" in _lib.last_error()
    assert call(S=0) == -1 and call(S=1025) == -1 and "1..1024" in _lib.last_error()
    assert call(n=0) == -1 and call(H=0) == -1 and call(W=16385) == -1
    assert call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1
    assert lib.pmce_crop_patches(None, 6, 8, 8, host, fake, fake, 3, 1.1, 224, 0, fake, fake, None, fake, None) == -1
    assert lib.pmce_crop_boxes(fake, 0, 17, 0.3, fake, fake, fake, None) == -1
    assert lib.pmce_crop_boxes(fake, 4, 0, 0.3, fake, fake, fake, None) == -1
    assert lib.pmce_crop_boxes(fake, 4, 17, float("nan"), fake, fake, fake, None) == -1
    assert lib.pmce_crop_boxes(None, 4, 17, 0.3, fake, fake, fake, None) == -1


def test_oracle_boxes_against_the_reference():
    """The oracle's boxes, usable flags and span against get_all_bbox_params + CropDataset's box lines run on the same float64 arrays.
    Allowed: 1e-12 relative (fp64 rounding of the same formula).  Measured when the golden file was made: 0 - every box bit-identical."""
    tracks = CR.golden_tracklets()
    assert set(tracks) == {k[len("span_"):] for k in GOLD.files if k.startswith("span_")}
    kinds = set()
    for name, kp in tracks.items():
        boxes, usable, span = CR.tracklet_boxes(kp)
        a, b = (int(v) for v in GOLD[f"span_{name}"])
        assert span == (a, b) == demo.tracklet_span(kp), name
        want = GOLD[f"boxes_{name}"]
        assert want.shape == (max(b - max(a, 0), 0), 4)
        lo = max(a, 0)
        assert np.isnan(boxes[:lo]).all() and np.isnan(boxes[b:]).all() and np.isfinite(boxes[lo:b]).all()
        if len(want):
            rel = np.abs(boxes[lo:b] - want) / np.abs(want)
            print(f"{name}: boxes vs reference, largest relative difference {rel.max():.3e}")
            assert rel.max() <= 1e-12, name
            assert usable[a] == 1 and usable[b - 1] == 1
        # which kinds of gap the file covers
        gaps = re.findall("0+", "".join(map(str, usable[lo:b])))
        kinds |= {"mid1" for g in gaps if len(g) == 1} | {"mid>1" for g in gaps if len(g) > 1}
        kinds |= ({"start"} if a > 0 else set()) | ({"end"} if 0 < b < len(kp) else set()) | ({"none"} if a == -1 else set())
    assert kinds == {"mid1", "mid>1", "start", "end", "none"}
    # the two unusable kinds that are not "nothing visible": all scores just below the threshold, and a span under half a pixel
    kp = tracks["mid_gaps"]
    assert CR.frame_param(kp[9], 0.3) is None and kp[9, :, 2].max() < 0.3 and kp[9, :, 2].max() > 0.299
    vis = kp[15, :, 2] > 0.3
    assert vis.any() and CR.frame_param(kp[15], 0.3) is None and np.linalg.norm(np.ptp(kp[15, vis, :2], axis=0)) < 0.5


def test_oracle_map_against_the_reference():
    """The oracle's forward map (the inverse of i, t) against gen_trans_from_patch_cv's 2 x 3 matrices (cv2.getAffineTransform stood in
    for by a float64 solve).  Allowed: 1e-12 relative (CR.map_difference).  Measured when the golden file was made: 2.9e-13, the
    solve's residue in the shear entries, which are exactly 0 in the closed form; the scales and translations agree to 1.1e-14."""
    rows = CR.golden_boxes()
    assert GOLD["trans"].shape == (len(rows), 2, 3) and len(rows) >= 30
    worst = 0.0
    for (cx, cy, w, h, scale, S), want in zip(rows, GOLD["trans"]):
        worst = max(worst, CR.map_difference(CR.forward_matrix((cx, cy, w, h), scale, int(S)), want))
    print(f"forward map vs reference, largest relative difference {worst:.3e}")
    assert worst <= 1e-12


def test_oracle_identity_crop():
    """A 224 x 224 frame cropped with w * scale = 224 around (112, 112) is the frame itself: i = 1, t = 0, every fraction 0."""
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    for box, scale in (((112.0, 112.0, 224.0, 224.0), 1.0), ((112.0, 112.0, 112.0, 112.0), 2.0)):
        assert CR.axis_map(box[0], box[2], scale, 224) == (1.0, 0.0)
        f32, u8, st = CR.crop_patches(frame[None], [0], [box], scale=scale, S=224)
        assert st[0] == 0 and np.array_equal(u8[0], frame)
        assert np.array_equal(f32[0], CR.normalise(frame))
    # the table the kernel reads is the oracle's normalisation of every byte, bit for bit
    t = crops.norm_table().numpy()
    ramp = np.tile(np.arange(256, dtype=np.uint8)[None, :, None], (1, 1, 3))
    assert t.dtype == np.float32 and np.array_equal(t.view(np.int32), CR.normalise(ramp)[:, 0, :].view(np.int32))


def test_wrapper_argument_errors():
    frames = np.zeros((2, 8, 9, 3), dtype=np.uint8)
    fi, boxes = np.array([0, 1]), np.array([[4.0, 4.0, 5.0, 5.0]] * 2)
    bad = [dict(frames=frames.astype(np.float32)), dict(frames=frames[0]), dict(frames=np.zeros((2, 8, 9, 4), np.uint8)),
           dict(frame_index=np.array([0, 2])), dict(frame_index=np.array([-1, 0])), dict(frame_index=np.array([0.0, 1.0])),
           dict(frame_index=np.array([0])), dict(boxes=boxes[:, :3]), dict(boxes=boxes.astype(np.int64)), dict(boxes=boxes[0]),
           dict(size=0), dict(size=1025), dict(size=7.5), dict(scale=float("nan")), dict(channel_order="gbr"),
           dict(frames=torch.zeros(2, 8, 9, 3, dtype=torch.uint8), frame_index=torch.tensor([0, 2]))]
    for kw in bad:
        args = dict(frames=frames, frame_index=fi, boxes=boxes)
        args.update(kw)
        with pytest.raises(ValueError):
            crops.crop_patches(**args)
    for kp in (np.zeros((4, 17, 2), np.float32), np.zeros((17, 3), np.float32), np.zeros((4, 17, 3), np.int32), np.zeros((4, 0, 3), np.float32)):
        with pytest.raises(ValueError):
            crops.tracklet_boxes(kp)
    with pytest.raises(ValueError):
        crops.tracklet_boxes(np.zeros((4, 17, 3), np.float32), vis_thresh=float("nan"))
    kp = np.zeros((4, 17, 3), np.float32)
    for tr in ([(kp, np.arange(3))], [(kp, np.arange(4) + 1)], [(kp, np.arange(4) * 0.5)], [(kp[:, :, :2], np.arange(4))]):
        with pytest.raises(ValueError):
            demo.crop_tracklets(frames.repeat(2, 0), tr)
    with pytest.raises(ValueError):
        demo.crop_tracklets(frames[0], [(kp, np.arange(4))])
    with pytest.raises(ValueError):
        demo.run_video(None, frames, [(kp, np.arange(4))], None, (9, 8), extract_batch=0)
    assert demo.run_video(None, frames, [], None, (9, 8)) == []
