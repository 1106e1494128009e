"""GPU tests of the debug overlay (csrc/overlay.hip through pmce_amd/overlay.py) against tests/overlay_ref.py, the restatement with
Python integers.  The rules are integer, so every comparison is exact equality of every byte of every frame and of every status word.
Frames are 40 x 24, three of them (one case adds a 60 x 24 frame: nine digits do not fit into 40 columns)."""
import numpy as np
import pytest
import torch

import overlay_ref as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, H, W = 3, 24, 40
FAR = 16000.0


def O():
    from pmce_amd import overlay
    return overlay


def background(f=F, h=H, w=W, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (f, h, w, 3), dtype=np.uint8)


def check(frames, frame_index, **kw):
    """``overlay.draw`` against the restatement: all bytes, all status words -> (frames, status) as numpy."""
    ov = O()
    on = lambda x: x if x is None or not isinstance(x, np.ndarray) else torch.from_numpy(x).to(DEV)      # noqa: E731
    dev_kw = {k: (on(v) if k in ("boxes", "keypoints") else v) for k, v in kw.items()}
    out, status = ov.draw(torch.from_numpy(frames).to(DEV), frame_index, **dev_kw)
    ref_kw = {k: v for k, v in kw.items() if k not in ("key_bytes", "inplace")}
    ref_kw.setdefault("skeleton", ov.COCO17_SKELETON)
    ref_kw.setdefault("palette", ov.PALETTE)
    want, want_status = OR.draw(frames, np.asarray(frame_index), font=ov.FONT, **ref_kw)
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status.dtype == np.int32 and np.array_equal(status, want_status), (status, want_status)
    diff = np.argwhere((out != want).any(-1)) if out.shape == want.shape else None
    assert diff is not None and not len(diff), f"{len(diff)} pixels differ, (frame, y, x) = {diff[:24].tolist()} ... with " \
        f"{ {k: v for k, v in kw.items() if k not in ('boxes', 'keypoints', 'ids', 'palette')} }"
    return out, status


def scene(seed=11, n=14):
    """Rows spread over the frames (frame 1 gets none), in mixed order: boxes, ids and 17 keypoints with scores around the threshold."""
    rng = np.random.default_rng(seed)
    fi = rng.choice([0, 2], n).astype(np.int32)
    centre = rng.uniform([4, 4], [W - 4, H - 4], (n, 2))
    boxes = np.concatenate([centre, rng.uniform(6, 22, (n, 2))], 1)
    ids = rng.integers(0, 200, n)
    kp = np.concatenate([centre[:, None] + rng.uniform(-9, 9, (n, 17, 2)), rng.uniform(0.1, 0.9, (n, 17, 1))], 2).astype(np.float32)
    return fi, boxes, ids, kp


def test_segments_and_discs():
    bg = background()
    fi = np.array([0, 1, 2], np.int32)
    # boxes alone: corners on pixel centres, on pixel borders, in between; partly and wholly outside the frame
    for t in (1, 2, 5):
        out, st = check(bg, fi, boxes=np.array([[10.5, 8.5, 30.5, 18.5], [10.0, 8.0, 30.0, 18.0], [3.3, 2.7, 17.9, 21.2]]), box_format="xyxy",
                        thickness=t)
        assert not st.any() and (out != bg).any(-1).reshape(3, -1).any(1).all()
        check(bg, fi, boxes=np.array([[-6.0, -4.0, 20.0, 12.0], [30.0, 15.0, 70.0, 60.0], [-50.0, -50.0, -20.0, -30.0]]), box_format="xyxy",
              thickness=t)
        out, _ = check(bg, fi, boxes=np.array([[20.0, 12.0, 300.0, 200.0], [100.0, 100.0, 8.0, 8.0], [-70.0, 5.0, 9.0, 9.0]]), box_format="cxcywh",
                       thickness=t)
        assert not (out[0] != bg[0]).any() and not (out[1] != bg[1]).any()      # the frame lies inside the first box; the second is outside
        check(bg, fi, boxes=np.array([[5.0, 6.0, 20.5, 10.25], [0.0, 0.0, 40.0, 24.0], [39.5, 23.5, 1.0, 1.0]]), box_format="xywh", thickness=t)
    # discs alone (no limbs), radii 1, 3 and one larger than the frame is high; two components per keypoint
    kp = np.array([[[10.5, 8.5], [20.0, 12.0]], [[-2.0, 3.0], [39.9, 23.9]], [[80.0, 80.0], [7.25, 16.75]]])
    for r in (1, 3, 14):
        out, st = check(bg, fi, keypoints=kp, skeleton=np.zeros((0, 2), np.int32), radius=r)
        assert not st.any() and (out[0] != bg[0]).any()
    # limbs (with their end discs of radius 1, narrower than the limb from thickness 2 on): centres, borders, outside, zero length
    limb = np.array([[0, 1]])
    kp = np.array([[[4.5, 4.5], [33.5, 19.5]], [[4.0, 20.0], [36.0, 3.0]], [[-15.0, 30.0], [25.0, -9.0]]])
    for t in (1, 2, 5):
        out, st = check(bg, fi, keypoints=kp, skeleton=limb, radius=1, thickness=t)
        assert not st.any()
        check(bg, fi, keypoints=np.array([[[12.0, 7.0], [12.0, 7.0]], [[12.5, 7.5], [12.5, 7.5]], [[60.0, 7.0], [90.0, 7.0]]]),
              skeleton=limb, radius=1, thickness=t)                           # zero length: a disc of 8 t units; wholly outside
        # the long diagonal: |p|^2 L needs 128 bits
        out, st = check(bg, fi, keypoints=np.array([[[-FAR, -FAR], [FAR, FAR]], [[-FAR, FAR - 10], [FAR, -FAR + 30]],
                                                    [[-FAR, 3.0], [FAR, 20.0]]]), skeleton=limb, radius=1, thickness=t)
        assert not st.any() and (out != bg).any(-1).reshape(3, -1).any(1).all()
        on_line = [(y, y) for y in range(H)]
        assert all((out[0, y, x] == O().PALETTE[0]).all() for y, x in on_line) and (out[0, 0, 12] == bg[0, 0, 12]).all()


def test_non_finite_and_out_of_range_values():
    ov = O()
    bg = background()
    nan, inf = float("nan"), float("inf")
    # boxes: every slot non-finite in turn, empty ones, and a healthy row that must still be drawn
    boxes = np.array([[nan, 8, 10, 10], [20, inf, 10, 10], [20, 8, -inf, 10], [20, 8, 10, nan], [20, 8, 0, 10], [20, 8, 10, -3.0], [20, 12, 10, 10]])
    fi = np.zeros(7, np.int32)
    out, st = check(bg, fi, boxes=boxes, ids=np.arange(7))
    assert st.tolist() == [1, 1, 1, 1, 1, 1, 0] and (out[0] != bg[0]).any()
    # a non-finite keypoint: its limbs go, the others stay; also a non-finite score
    rng = np.random.default_rng(3)
    kp = np.concatenate([rng.uniform([2, 2], [W - 2, H - 2], (3, 17, 2)), np.ones((3, 17, 1))], 2)
    kp[0, 5, 0] = nan                                                          # the left shoulder: four limbs name it
    kp[1, 16, 2] = inf
    out, st = check(bg, np.array([0, 1, 2], np.int32), keypoints=kp)
    assert st.tolist() == [1, 1, 0]
    healthy = kp.copy()
    healthy[0, 5, 0] = 20.0
    full, _ = check(bg, np.array([0, 1, 2], np.int32), keypoints=healthy)
    assert (full[0] != out[0]).any() and np.array_equal(full[2], out[2])
    only = np.zeros((1, 17, 3))
    only[0, :, :2] = kp[0, :, :2]
    only[0, [11, 12], 2] = 1.0                                                 # with the hips alone drawn, the hip limb stays ...
    a, _ = check(bg, np.array([0], np.int32), keypoints=only)
    assert (a[0] != bg[0]).any()
    # the guard band: a primitive with an endpoint beyond 2^14 px is dropped, the row's other primitives stay
    G = 16384.0
    boxes = np.array([[10.0, 5.0, G + 1, 20.0], [10.0, 5.0, G, 20.0], [-G - 0.5, 5.0, 30.0, 20.0], [12.0, -G * 2, 30.0, 20.0]])
    out, st = check(bg, np.array([0, 1, 2, 2], np.int32), boxes=boxes, ids=np.array([1, 2, 3, 4]), box_format="xyxy")
    assert st.tolist() == [2, 0, 2, 2]
    assert (out[0, 5:21, 10] != bg[0, 5:21, 10]).any()                         # the left edge of row 0 has both ends inside the band
    kp = np.array([[[G + 0.0625, 5.0], [10.0, 10.0], [30.0, 20.0]], [[G, 5.0], [10.0, 10.0], [30.0, 20.0]], [[3.0, -1e30], [10.0, 10.0], [30.0, 20.0]]])
    out, st = check(bg, np.array([0, 1, 2], np.int32), keypoints=kp, skeleton=np.array([[0, 1], [1, 2]]))
    assert st.tolist() == [2, 0, 2]
    # what only the device can find in device tensors: a frame index outside the frames, an id out of range
    fi_dev = torch.tensor([0, 3, -1, 2], dtype=torch.int32, device=DEV)
    ids_dev = torch.tensor([5, 6, 7, 10 ** 9], dtype=torch.int64, device=DEV)
    bx = np.array([[20.0, 12.0, 10.0, 10.0]] * 4)
    out, status = ov.draw(torch.from_numpy(bg).to(DEV), fi_dev, boxes=torch.from_numpy(bx).to(DEV), ids=ids_dev)
    want, want_status = OR.draw(bg, [0, 3, -1, 2], boxes=bx, ids=[5, 6, 7, 10 ** 9], palette=ov.PALETTE, font=ov.FONT)
    assert status.tolist() == want_status.tolist() == [0, ov.STATUS_FRAME, ov.STATUS_FRAME, ov.STATUS_SKIPPED]
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(want[1:], bg[1:])


def test_score_threshold():
    bg = background()
    below = np.nextafter(0.3, 0.0)
    kp = np.array([[[10.0, 8.0, below], [25.0, 15.0, 0.3], [30.0, 5.0, 0.3]]] * 3)
    kp[1, 0, 2] = 0.3
    kp[2, :, 2] = [np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(0)), 1.0]     # as fp32 scores arrive: 0.3f > 0.3
    sk = np.array([[0, 1], [1, 2]])
    out, st = check(bg, np.array([0, 1, 2], np.int32), keypoints=kp, skeleton=sk)
    assert not st.any()
    assert (out[0, 8, 10] == bg[0, 8, 10]).all() and (out[1, 8, 10] != bg[1, 8, 10]).any()     # just below: not drawn; just at: drawn
    assert (out[2, 8, 10] != bg[2, 8, 10]).any() and (out[2, 15, 25] == bg[2, 15, 25]).all()
    out32, _ = check(bg, np.array([0, 1, 2], np.int32), keypoints=kp.astype(np.float32), skeleton=sk)   # fp32 in: 0.3 rounds up, below rounds to 0.3f
    assert (out32[0, 8, 10] != bg[0, 8, 10]).any()
    check(bg, np.array([0, 1, 2], np.int32), keypoints=kp, skeleton=sk, score_thresh=0.0)
    out, _ = check(bg, np.array([0, 1, 2], np.int32), keypoints=kp, skeleton=sk, score_thresh=2)
    assert np.array_equal(out, bg)


def test_labels():
    ov = O()
    bg = background()
    # clamped at each border: left (x1 < 0), top (no room above y1), right (x1 near W), bottom (y1 below the frame); one free
    boxes = np.array([[-5.0, 12.0, 10.0, 20.0], [12.0, 3.0, 30.0, 20.0], [35.0, 14.0, 39.0, 20.0], [10.0, 40.0, 20.0, 50.0], [12.0, 14.0, 30.0, 22.0]])
    ids = np.array([7, 42, 138, 9, 60])
    for s in (1, 2):
        out, st = check(bg, np.array([0, 1, 2, 0, 1], np.int32), boxes=boxes, ids=ids, box_format="xyxy", label_scale=s, thickness=1)
        assert not st.any()
        text = (out == 255).all(-1) & ~(bg == 255).all(-1)
        assert text[0].any() and text[1].any() and text[2].any()
    # the free label sits with its left column at floor(x1) and its last row just above floor(y1): here columns 12..23, rows 6..13
    out, _ = check(bg, np.array([1], np.int32), boxes=boxes[4:], ids=ids[4:], box_format="xyxy", label_scale=1, thickness=1)
    changed = (out[1] != bg[1]).any(-1)
    assert changed[6:14, 12:24].all() and not changed[:6].any() and not changed[6:13, 24:30].any()
    # 999999999: nine digits are 54 columns, more than the 40 of the frame - no label, the colour still comes from the id
    big = np.array([999999999])
    out, st = check(bg, np.array([0], np.int32), boxes=np.array([[20.0, 16.0, 16.0, 10.0]]), ids=big, label_scale=1)
    assert not st.any() and not (out == 255).all(-1)[0, :10].any()
    assert (out[0, 11, 20] == ov.PALETTE[999999999 % len(ov.PALETTE)]).all()
    # ... and on a frame of 60 columns all nine are there
    wide = background(1, H, 60, seed=8)
    out, st = check(wide, np.array([0], np.int32), boxes=np.array([[30.0, 16.0, 40.0, 10.0]]), ids=big, label_scale=1)
    assert (out[0, 3:11, 10:64] != wide[0, 3:11, 10:64]).any(-1).all()
    check(wide, np.array([0, 0], np.int32), boxes=np.array([[30.0, 16.0, 40.0, 10.0], [8.0, 20.0, 10.0, 6.0]]), ids=np.array([123456789, 0]),
          label_scale=1, text_color=(1, 2, 3))
    # larger than the frame: too wide (scale 4: two digits are 48 columns), too high (scale 4 is 32 rows)
    out, _ = check(bg, np.array([0, 1], np.int32), boxes=np.array([[20.0, 16.0, 16.0, 10.0]] * 2), ids=np.array([10, 3]), label_scale=4)
    check(bg, np.array([0], np.int32), boxes=np.array([[20.0, 16.0, 16.0, 10.0]]), ids=np.array([3]), label_scale=3)     # 18 x 24: just fits
    # no ids: no label, palette[0]
    out, _ = check(bg, np.array([0], np.int32), boxes=np.array([[20.0, 16.0, 16.0, 10.0]]))
    assert (out[0, 11, 20] == ov.PALETTE[0]).all()


def test_order_and_blend():
    bg = background()
    rng = np.random.default_rng(23)
    n = 70                                                                     # more order ranks than a wave has lanes
    palette = rng.permutation(256 * 256)[:n]
    palette = np.stack([palette % 256, palette // 256, np.arange(n) + 100], 1).astype(np.uint8)
    x2 = rng.uniform(22, 38, n)
    boxes = np.stack([np.full(n, 20.0), np.full(n, 4.0), x2, rng.uniform(6, 22, n)], 1)    # every top edge starts at (20, 4)
    ids = rng.permutation(n)
    for order in (np.arange(n), rng.permutation(n)):
        fi = np.full(n, 1, np.int32)
        out, st = check(bg, fi, boxes=boxes[order], ids=ids[order], box_format="xyxy", palette=palette, thickness=1, label_scale=1)
        assert not st.any()
        # column 20 of rows 3 and 4 lies under every row's top edge and label ground (never under a digit): the LAST row's colour
        assert (out[1, 4, 20] == palette[ids[order][-1]]).all() and (out[1, 3, 20] == palette[ids[order][-1]]).all()
    for alpha in (0, 128, 255):
        fi, bx, ident, kp = scene()
        out, _ = check(bg, fi, boxes=bx, ids=ident, keypoints=kp, alpha=alpha)
        assert np.array_equal(out, bg) == (alpha == 0)
    # 128: both the colour and the pixel show
    out, _ = check(bg, np.array([0], np.int32), boxes=np.array([[20.0, 12.0, 10.0, 10.0]]), alpha=128, palette=np.array([[200, 100, 0]], np.uint8))
    assert out[0, 7, 20].tolist() == [(128 * c + 127 * int(p) + 127) // 255 for c, p in zip((200, 100, 0), bg[0, 7, 20])]


def test_empty_and_optional_inputs():
    bg = background()
    fi, bx, ident, kp = scene()
    out, _ = check(bg, fi, boxes=bx, ids=ident, keypoints=kp)
    assert np.array_equal(out[1], bg[1]) and (out[0] != bg[0]).any() and (out[2] != bg[2]).any()      # frame 1 has no row
    none = np.zeros(0, np.int32)
    out, st = check(bg, none, boxes=np.zeros((0, 4)), ids=np.zeros(0, np.int64), keypoints=np.zeros((0, 17, 3), np.float32))
    assert np.array_equal(out, bg) and st.shape == (0,)
    check(bg, none)
    seen = [out.tobytes()]
    for drop in ("boxes", "ids", "keypoints"):
        kw = dict(boxes=bx, ids=ident, keypoints=kp)
        kw[drop] = None
        seen.append(check(bg, fi, **kw)[0].tobytes())
    assert len(set(seen)) == 4                                                 # each of the three shows in the picture
    out, st = check(bg, fi)                                                    # nothing to draw per row
    assert np.array_equal(out, bg) and not st.any()
    check(bg, fi, keypoints=kp[..., :2].astype(np.float64))                    # no score column: every finite keypoint is drawn


def test_determinism_and_chunking():
    ov = O()
    bg = background()
    fi, bx, ident, kp = scene(seed=12, n=20)
    fi[:3] = 1
    want, want_status = check(bg, fi, boxes=bx, ids=ident, keypoints=kp)
    frames = torch.from_numpy(bg).to(DEV)
    dev = dict(boxes=torch.from_numpy(bx).to(DEV), ids=ident, keypoints=torch.from_numpy(kp).to(DEV))
    # two runs, and one frame per chunk (also a key buffer smaller than a frame) against one chunk for all
    for kw in ({}, {}, dict(key_bytes=W * H * 4), dict(key_bytes=2 * W * H * 4 + 5), dict(key_bytes=1)):
        out, st = ov.draw(frames, fi, **dev, **kw)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_status), kw
    assert torch.equal(frames.cpu(), torch.from_numpy(bg))                     # a copy was drawn on
    # in place
    mine = frames.clone()
    out, _ = ov.draw(mine, fi, **dev, inplace=True)
    assert out.data_ptr() == mine.data_ptr() and np.array_equal(mine.cpu().numpy(), want)
    with pytest.raises(ValueError, match="inplace=True needs contiguous"):
        ov.draw(frames.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), fi, **dev, inplace=True)
    out, _ = ov.draw(frames.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), fi, **dev)      # a copy is made contiguous
    assert np.array_equal(out.cpu().numpy(), want)
    # batch invariance: a frame's bytes in a call with its rows only
    for f in range(F):
        rows = np.flatnonzero(fi == f)
        sel = torch.from_numpy(rows).to(DEV)
        out, st = ov.draw(frames[f:f + 1], np.zeros(len(rows), np.int32), boxes=dev["boxes"][sel], ids=ident[rows], keypoints=dev["keypoints"][sel])
        assert np.array_equal(out.cpu().numpy()[0], want[f]) and np.array_equal(st.cpu().numpy(), want_status[rows]), f
    # every input as a device tensor: nothing is read on the host
    out, st = ov.draw(frames, torch.from_numpy(fi).to(DEV), boxes=dev["boxes"], ids=torch.from_numpy(ident).to(DEV), keypoints=dev["keypoints"])
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_status)


def test_a_full_hd_frame():
    """1920 x 1080: coordinates, key offsets and bounding boxes far beyond the small frames' - a box of several hundred pixels with its
    label, a limb across it, and host rows given out of frame order (they are sorted for the launch, the status comes back in the
    caller's order)."""
    rng = np.random.default_rng(19)
    bg = rng.integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    fi = np.array([1, 0, 1, 0], np.int32)
    boxes = np.array([[1700.25, 900.5, 380.0, 330.0], [400.0, 300.0, 250.5, 520.0], [960.0, 540.0, 1900.0, 1060.0], [1000.0, float("nan"), 50.0, 50.0]])
    ids = np.array([31, 999999999, 4, 5])
    kp = np.array([[[1600.0, 800.0], [1750.5, 1050.0]], [[300.0, 100.0], [480.0, 330.0]], [[1919.5, 0.5], [1800.0, 90.0]], [[5.0, 5.0], [60.0, 40.0]]])
    out, st = check(bg, fi, boxes=boxes, ids=ids, keypoints=kp, skeleton=np.array([[0, 1]]))
    assert st.tolist() == [0, 0, 0, 1]
    drawn = (out != bg).any(-1)
    # frame 1: two boxes (one nearly the whole frame: its bottom edge is rows 1069 and 1070) and two limbs; frame 0: one box, 108 label columns
    assert drawn[1].sum() > 12000 and drawn[0].sum() > 4000 and drawn[1, 1069:1071, 1000].all() and not drawn[1, 1071:, 1000].any()
    assert drawn[0, 20, 30]                                                    # the row with the broken box still has its limb
