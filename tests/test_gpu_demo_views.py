"""GPU tests of the demo's output switches: ``render_tracklets(plain=, sideview=)`` on a 4-vertex mesh at 32 x 24, and
``render_folder`` with ``sideview``, ``plain``, ``debug_folder``, ``obj_folder`` and ``pkl_path`` on both routes - the whole video and
``frames_per_pass`` - with batch-invariant stand-ins for detector, pose and extractor (elementwise arithmetic and gathers that read the
frames' pixels, as tests/test_gpu_long_folder.py has them).  Everything is compared to the bit and to the byte."""
import os
import pickle

import numpy as np
import pytest
import torch

import tracker_ref as TR
from test_gpu_tracker import DEV, PlantedDet, T, bits, tiny_frames

pytestmark = pytest.mark.gpu
VIS = 0.3
W, H = 32, 24
# the keys of a result dict of run_frames before keep_inputs existed
PARENT_KEYS = {"mesh", "pred_cam", "bboxes", "orig_cam", "loss", "joints_mm", "target2d", "frame_ids", "person_id"}


# ----------------------------------------------------------------------------------------------
# render_tracklets: plain and side view
# ----------------------------------------------------------------------------------------------

def small_results():
    """Two persons over three frames: a 4-vertex, 2-face mesh each, not planar (the side view shows it too)."""
    base = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.2], [0.0, 0.5, -0.3], [0.1, 0.0, 0.6]], dtype=np.float32)
    rng = np.random.default_rng(41)

    def person(n, shift):
        mesh = base[None] + rng.uniform(-0.05, 0.05, (n, 4, 3)).astype(np.float32) + np.float32(shift)
        cam = np.tile(np.array([[0.8, 0.8, 0.05, -0.1]], np.float32), (n, 1))
        boxes = np.tile(np.array([[10.0, 4.0 + 10 * shift, 8.0, 8.0]], np.float32), (n, 1))
        return {"mesh": torch.from_numpy(mesh).to(DEV), "orig_cam": torch.from_numpy(cam).to(DEV), "bboxes": torch.from_numpy(boxes).to(DEV)}

    a, b = person(3, 0.0), person(2, 0.3)
    a["frame_ids"], b["frame_ids"] = np.array([0, 1, 2]), np.array([2, 0])
    return [b, a]                                   # b has the lower box: a is drawn first in the frames they share


def test_render_tracklets_plain_and_sideview():
    from pmce_amd import demo, render
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    r = render.Renderer(faces, (W, H), cull_backfaces=False)
    frames = torch.from_numpy(np.random.default_rng(42).integers(1, 256, (3, H, W, 3), dtype=np.uint8)).to(DEV)
    res = small_results()
    base = demo.render_tracklets(res, frames, (W, H), renderer=r)
    drawn = (base != frames).any(-1)
    assert drawn.flatten(1).any(1).all() and not drawn.all()
    # the side view: the left half is the call without it, the right half the same jobs in the same order, turned, on zeros
    wide = demo.render_tracklets(res, frames, (W, H), renderer=r, sideview=True)
    assert tuple(wide.shape) == (3, H, 2 * W, 3) and wide.dtype == torch.uint8 and torch.equal(wide[:, :, :W], base)
    cat = lambda name: torch.cat([d[name] for d in res])      # noqa: E731
    fi, order = demo.tracklet_draw_order([cat("bboxes")[:, 1].cpu().numpy()], [d["frame_ids"] for d in res])
    assert fi.tolist() == [2, 0, 0, 1, 2] and order.tolist() == [2, 1, 3, 4, 0]          # person a under person b where both are
    side = torch.from_numpy(render.axis_rotation(270, (0, 1, 0)).astype(np.float32))
    want = r.render(torch.zeros_like(frames), cat("mesh"), cat("orig_cam"), frame_index=fi, rotation=side, draw_order=order)
    assert torch.equal(wide[:, :, W:], want) and want.flatten(1).any(1).all() and not torch.equal(want, base)
    # plain: the call on zeroed frames
    plain = demo.render_tracklets(res, frames, (W, H), renderer=r, plain=True)
    assert torch.equal(plain, demo.render_tracklets(res, torch.zeros_like(frames), (W, H), renderer=r))
    assert torch.equal(plain != 0, drawn.unsqueeze(-1).expand_as(plain) & (plain != 0)) and torch.equal(plain[drawn], base[drawn])
    # both: a black background on both halves
    both = demo.render_tracklets(res, frames, (W, H), renderer=r, plain=True, sideview=True)
    assert torch.equal(both[:, :, :W], plain) and torch.equal(both[:, :, W:], want)
    assert not both[:, :, :W][~drawn].any() and not both[:, 0].any()
    # order = depth goes through both halves; in place: plain zeroes the caller's frames, the side view refuses
    deep = demo.render_tracklets(res, frames, (W, H), renderer=r, sideview=True, order="depth")
    assert torch.equal(deep[:, :, :W], demo.render_tracklets(res, frames, (W, H), renderer=r, order="depth"))
    mine = frames.clone()
    out = demo.render_tracklets(res, mine, (W, H), renderer=r, plain=True, inplace=True)
    assert out.data_ptr() == mine.data_ptr() and torch.equal(mine, plain)
    with pytest.raises(ValueError, match="inplace=True cannot be combined with sideview=True"):
        demo.render_tracklets(res, mine, (W, H), renderer=r, sideview=True, inplace=True)
    assert torch.equal(mine, plain)                                                        # refused before anything was drawn


# ----------------------------------------------------------------------------------------------
# render_folder with the switches, on both routes
# ----------------------------------------------------------------------------------------------

def trk():
    return T().Tracker(PlantedDet(TR.planted_video_rows()), size=64, batch=12)


class Pose:
    """17 keypoints inside each box; the score of a row is a pixel of ITS frame (the one under the box centre, channel 0)."""
    box_format = "cxcywh"

    def __init__(self):
        g = torch.Generator().manual_seed(14)
        self.uv = (torch.rand(17, 2, generator=g, dtype=torch.float64) - 0.5).to(DEV) * 0.8

    def __call__(self, fr, frame_index, bx):
        fi = torch.as_tensor(np.asarray(frame_index)).to(DEV).long()
        xy = bx[:, None, :2] + self.uv[None] * bx[:, None, 2:]
        x = bx[:, 0].long().clamp(0, fr.shape[2] - 1)
        y = bx[:, 1].long().clamp(0, fr.shape[1] - 1)
        score = fr[fi, y, x, 0].double() / 255
        return torch.cat([xy, score[:, None, None].expand(-1, 17, 1)], -1).float(), None


class GatherExtractor:
    """2048 fixed pixels of the patch, each times a fixed weight: elementwise, so the bits of a row do not depend on the batch."""

    def __init__(self):
        g = torch.Generator().manual_seed(15)
        self.index = torch.randint(0, 3 * 224 * 224, (2048,), generator=g).to(DEV)
        self.weight = (torch.randn(2048, generator=g) * 0.5).to(DEV)

    def __call__(self, p):
        return p.flatten(1)[:, self.index] * self.weight


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The tracker test's 30 frames with the first three black: ``Pose`` scores them 0, so every tracklet's span starts after them and
    the kept inputs must be cut by it."""
    from pmce_amd import demo
    src = tmp_path_factory.mktemp("frames")
    frames = tiny_frames()
    frames[:3] = 0
    demo.save_frames(str(src), frames.to(DEV))
    return str(src)


@pytest.fixture(scope="module")
def faces():
    return np.random.default_rng(16).integers(0, 6890, (300, 3)).astype(np.int32)


def read_tree(root):
    got = {}
    for path, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(path, n), "rb") as fh:
                got[os.path.relpath(os.path.join(path, n), root)] = fh.read()
    return got


def same_outs(outs, want):
    assert len(outs) == len(want) == 2 and [o["person_id"] for o in outs] == [w["person_id"] for w in want] == [2, 1]
    for o, w in zip(outs, want):
        assert set(o) == set(w) and np.array_equal(o["frame_ids"], w["frame_ids"])
        for key in w:
            if key not in ("frame_ids", "person_id"):
                assert o[key].dtype == w[key].dtype and torch.equal(bits(o[key]), bits(w[key])), key


def run_views(folder, faces, root, **kw):
    from pmce_amd import demo
    from test_gpu_demo import get_model
    outs = demo.render_folder(get_model(256), folder, str(root / "out"), trk(), Pose(), GatherExtractor(), faces, input_folder=str(root / "in"),
                              sideview=True, plain=True, debug_folder=str(root / "debug"), obj_folder=str(root / "obj"),
                              pkl_path=str(root / "pkl" / "pmce_output.pkl"), vis_thresh=VIS, seed=3, **kw)
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def whole(folder, faces, tmp_path_factory):
    """The whole-video route with every switch on, once: (outs, every file written, by path)."""
    root = tmp_path_factory.mktemp("whole")
    outs = run_views(folder, faces, root)
    return outs, read_tree(str(root))


def test_the_whole_route_writes_every_view(folder, faces, whole):
    from pmce_amd import demo, jpeg
    outs, files = whole
    frames, wh, names = demo.load_frames(folder)
    assert wh == (64, 48) and len(names) == 30
    for sub in ("out", "in", "debug"):
        assert {n for n in files if n.startswith(sub + os.sep)} == {os.path.join(sub, f"{i:06d}.jpg") for i in range(30)}
    # the output frames are 2 W wide, the others W; the input frames are the folder's own, encoded again
    sizes = {sub: {(jpeg.parse(files[os.path.join(sub, f"{i:06d}.jpg")], sub).width, jpeg.parse(files[os.path.join(sub, f"{i:06d}.jpg")], sub).height)
                   for i in range(30)} for sub in ("out", "in", "debug")}
    assert sizes == {"out": {(128, 48)}, "in": {(64, 48)}, "debug": {(64, 48)}}
    again = jpeg.files(*jpeg.encode(frames))
    assert [files[os.path.join("in", f"{i:06d}.jpg")] for i in range(30)] == again
    # the picture: render_tracklets with both switches, encoded
    want = jpeg.files(*jpeg.encode(demo.render_tracklets(outs, frames, wh, renderer=faces, plain=True, sideview=True)))
    assert [files[os.path.join("out", f"{i:06d}.jpg")] for i in range(30)] == want
    # one .obj per person and frame, the flipped mesh in it; the pickle has the reference's keys
    objs = sorted(n for n in files if n.startswith("obj" + os.sep))
    assert objs == sorted(os.path.join("obj", "meshes", f"{o['person_id']:04d}", f"{int(f):06d}.obj") for o in outs for f in o["frame_ids"])
    o = outs[1]
    lines = files[os.path.join("obj", "meshes", f"{o['person_id']:04d}", f"{int(o['frame_ids'][5]):06d}.obj")].decode().splitlines()
    assert len(lines) == 6890 + 300 and lines[6890] == "f %d %d %d" % tuple(int(v) + 1 for v in faces[0])
    v = o["mesh"][5].double().cpu().numpy() * [1.0, -1.0, -1.0]
    assert lines[17] == "v %.8f %.8f %.8f" % tuple(v[17]) and lines[6889] == "v %.8f %.8f %.8f" % tuple(v[6889])
    got = pickle.loads(files[os.path.join("pkl", "pmce_output.pkl")])
    assert list(got) == [2, 1]
    for o in outs:
        assert set(got[o["person_id"]]) == {"pred_cam", "mesh", "bboxes", "frame_ids"}
        for key in ("pred_cam", "mesh", "bboxes"):
            assert np.array_equal(got[o["person_id"]][key], o[key].cpu().numpy())
        assert np.array_equal(got[o["person_id"]]["frame_ids"], o["frame_ids"])


def test_debug_frames_equal_overlay_draw_on_the_kept_rows(folder, whole):
    from pmce_amd import demo, jpeg, overlay
    outs, files = whole
    frames, _, _ = demo.load_frames(folder)
    # by hand: the rows of a frame by the mesh box's top edge, ties in tracklet order; the tracker's id is the label
    rows = sorted((int(f), float(o["bboxes"][i, 1]), t, i) for t, o in enumerate(outs) for i, f in enumerate(o["frame_ids"]))
    pick = lambda name: torch.stack([outs[t][name][i] for _, _, t, i in rows])      # noqa: E731
    fi = np.array([r[0] for r in rows], np.int32)
    ids = np.array([outs[t]["person_id"] for _, _, t, _ in rows])
    want, status = overlay.draw(frames, fi, boxes=pick("track_boxes"), ids=ids, keypoints=pick("keypoints"))
    assert not status.any() and (want != frames).flatten(1).any(1).sum() >= 16
    got, st = demo.draw_tracklets(outs, frames)
    assert torch.equal(got, want) and st.shape == (len(rows),) and not st.any()
    assert [files[os.path.join("debug", f"{i:06d}.jpg")] for i in range(30)] == jpeg.files(*jpeg.encode(want))
    # overlay_kwargs reach the draw
    thick, _ = demo.draw_tracklets(outs, frames, thickness=5, radius=1)
    assert torch.equal(thick, overlay.draw(frames, fi, boxes=pick("track_boxes"), ids=ids, keypoints=pick("keypoints"), thickness=5, radius=1)[0])
    assert not torch.equal(thick, want)


@pytest.mark.parametrize("k", [7, 30])
def test_the_chunked_route_writes_the_same_files(k, folder, faces, whole, tmp_path):
    outs = run_views(folder, faces, tmp_path, frames_per_pass=k)
    same_outs(outs, whole[0])
    got, want = read_tree(str(tmp_path)), whole[1]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_keep_inputs_adds_exactly_the_two_keys(folder):
    from pmce_amd import demo
    from test_gpu_demo import get_model
    run = lambda **kw: demo.run_folder(get_model(256), folder, trk(), Pose(), GatherExtractor(), vis_thresh=VIS, seed=3, **kw)      # noqa: E731
    plain, kept, passes = run(), run(keep_inputs=True), run(keep_inputs=True, frames_per_pass=7)
    torch.cuda.synchronize()
    frames, _, _ = demo.load_frames(folder)
    boxes, ids = demo.track_video(frames, trk())
    kps = demo.pose_tracklets(frames, boxes, Pose())
    assert len(plain) == len(kept) == 2 and ids == [2, 1]
    for o, w, p, (bx, fid), (kp, _) in zip(kept, plain, passes, boxes, kps):
        assert set(w) == PARENT_KEYS and set(o) - set(w) == {"track_boxes", "keypoints"} and set(w) - set(o) == set()
        n = len(o["frame_ids"])
        assert o["track_boxes"].dtype == torch.float64 and tuple(o["track_boxes"].shape) == (n, 4) and o["track_boxes"].is_cuda
        assert o["keypoints"].dtype == torch.float32 and tuple(o["keypoints"].shape) == (n, 17, 3)
        # row-aligned with frame_ids: the tracker's boxes and the pose stage's keypoints of those frames (the span cut some off)
        at = torch.from_numpy(np.searchsorted(fid, o["frame_ids"])).to(DEV)
        assert len(fid) == 30 and n <= 27 and o["frame_ids"][0] >= 3
        assert torch.equal(bits(o["track_boxes"]), bits(bx[at])) and torch.equal(bits(o["keypoints"]), bits(kp[at]))
        for key in w:
            if key not in ("frame_ids", "person_id"):
                assert torch.equal(bits(o[key]), bits(w[key])), key
        assert set(p) == set(o) and torch.equal(bits(p["track_boxes"]), bits(o["track_boxes"])) and torch.equal(bits(p["keypoints"]), bits(o["keypoints"]))


def test_without_the_new_keywords_nothing_changes(folder, faces, tmp_path):
    """The files and the dicts' keys of a call without any new keyword: the stages composed by hand, and the literal key set."""
    from pmce_amd import demo, jpeg
    from test_gpu_demo import get_model
    outs = demo.render_folder(get_model(256), folder, str(tmp_path / "out"), trk(), Pose(), GatherExtractor(), faces,
                              input_folder=str(tmp_path / "in"), vis_thresh=VIS, seed=3)
    chunked = demo.render_folder(get_model(256), folder, str(tmp_path / "out7"), trk(), Pose(), GatherExtractor(), faces, vis_thresh=VIS,
                                 seed=3, frames_per_pass=7)
    torch.cuda.synchronize()
    assert all(set(o) == PARENT_KEYS for o in outs) and all(set(o) == PARENT_KEYS for o in chunked)
    frames, wh, _ = demo.load_frames(folder)
    by_hand = demo.run_frames(get_model(256), frames, trk(), Pose(), GatherExtractor(), wh, vis_thresh=VIS, seed=3)
    same_outs(outs, by_hand)
    files = read_tree(str(tmp_path))
    assert sorted(files) == sorted(os.path.join(sub, f"{i:06d}.jpg") for sub in ("out", "in", "out7") for i in range(30))
    want = jpeg.files(*jpeg.encode(demo.render_tracklets(by_hand, frames, wh, renderer=faces)))
    assert [files[os.path.join("out", f"{i:06d}.jpg")] for i in range(30)] == want == [files[os.path.join("out7", f"{i:06d}.jpg")] for i in range(30)]
    assert [files[os.path.join("in", f"{i:06d}.jpg")] for i in range(30)] == jpeg.files(*jpeg.encode(frames))
