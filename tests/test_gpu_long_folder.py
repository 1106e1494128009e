"""GPU tests of the demo in frame chunks: ``tracker.Tracker.stream()`` (the resumed SORT behind ``feed`` / ``records``),
``demo.iter_frames`` and ``demo.run_folder`` / ``demo.render_folder`` with ``frames_per_pass``.  The yardstick is the whole-video route
of the same run: records, result tensors and files are compared to the bit and to the byte.

The stubs of the demo test are batch-invariant by construction (elementwise arithmetic and gathers, no matrix product: a torch matmul
may change bits with the batch) and read the frames' pixels, so that a wrong chunk offset changes a score or a feature."""
import os

import numpy as np
import pytest
import torch

import tracker_ref as TR
from test_gpu_tracker import DEV, PlantedDet, T, bits, tiny_frames

pytestmark = pytest.mark.gpu
WH = (64, 48)
VIS = 0.3


def trk(rows=None, **kw):
    return T().Tracker(PlantedDet(TR.planted_video_rows() if rows is None else rows), size=64, **{"batch": 12, **kw})


# ----------------------------------------------------------------------------------------------
# Tracker.stream()
# ----------------------------------------------------------------------------------------------

def feed_all(stream, frames, pieces, report=False):
    res, at = [], 0
    for n in pieces:
        res.append(stream.feed(frames[at:at + n], report=report))
        at += n
    assert at == frames.shape[0]
    return res


def test_stream_records_equal_the_tracker_call():
    frames = tiny_frames()
    want, wids = trk()(frames)
    stream = trk().stream()
    res = feed_all(stream, frames, [12, 1, 17], report=True)
    recs, ids = stream.records()
    assert ids == wids == [2, 1] and stream.frames == 30
    for (b, f), (wb, wf) in zip(recs, want):
        assert torch.equal(bits(b), bits(wb)) and np.array_equal(f, wf) and len(f) == 30
    # feed(report=True): the chunk's reported rows, frame after frame in report order, with the records' boxes
    first = 0
    for (tracks, count, boxes, rel, pids), n in zip(res, [12, 1, 17]):
        assert tuple(tracks.shape) == (n, 64, 5) and tuple(count.shape) == (n,) and boxes.is_cuda and boxes.dtype == torch.float64
        assert rel.dtype == np.int32 and rel.tolist() == sorted(rel.tolist()) and len(rel) == len(pids) == boxes.shape[0] == 2 * n
        assert rel.min() == 0 and rel.max() == n - 1
        for (b, f), pid in zip(recs, ids):
            mine = np.flatnonzero(pids == pid)
            assert np.array_equal(rel[mine] + first, f[first:first + n])
            assert torch.equal(bits(boxes[torch.from_numpy(mine).to(DEV)]), bits(b[first:first + n]))
        first += n
    # without report: the chunk's tables, no more; a shorter min_frames filter is records' own
    plain = trk().stream()
    out = feed_all(plain, frames, [4, 26])
    assert all(len(o) == 2 for o in out) and torch.equal(bits(torch.cat([o[0] for o in out])), bits(torch.cat([r[0] for r in res])))
    assert plain.records(min_frames=31) == ([], [])


def test_stream_cap_errors_name_the_global_frame():
    rows, frames = TR.planted_video_rows(), tiny_frames()
    rows[:5, :, 4] = 0.01                                                              # the first five frames are empty: frame 5 is in the second piece
    for kw, what in ((dict(max_keep=1), "max_keep = 1"), (dict(max_candidates=3, batch=7), "max_candidates = 3"),
                     (dict(max_tracks=1), "max_tracks = 1")):
        stream = trk(rows, **kw).stream()
        feed_all(stream, frames, [4, 26])
        with pytest.raises(ValueError, match=rf"frame 5: .*{what}"):
            stream.records()


# ----------------------------------------------------------------------------------------------
# the folder in chunks
# ----------------------------------------------------------------------------------------------

class Pose:
    """17 keypoints inside each box; the score of a row is a pixel of ITS frame (the one under the box centre, channel 0), so some
    frames fall below vis_thresh and a wrong chunk offset moves them."""
    box_format = "cxcywh"

    def __init__(self):
        g = torch.Generator().manual_seed(14)
        self.uv = (torch.rand(17, 2, generator=g, dtype=torch.float64) - 0.5).to(DEV) * 0.8
        self.calls = []

    def __call__(self, fr, frame_index, bx):
        fi = torch.as_tensor(np.asarray(frame_index)).to(DEV).long()
        self.calls.append((int(fr.shape[0]), len(fi)))
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
        self.calls = []

    def __call__(self, p):
        f = p.flatten(1)[:, self.index] * self.weight
        self.calls.append(f)
        return f


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from pmce_amd import demo
    src = tmp_path_factory.mktemp("frames")
    demo.save_frames(str(src), tiny_frames().to(DEV))
    return str(src)


@pytest.fixture(scope="module")
def faces():
    return np.random.default_rng(16).integers(0, 6890, (300, 3)).astype(np.int32)


def read_all(path):
    return {n: open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))}


def same_outs(outs, want):
    assert len(outs) == len(want) == 2 and [o["person_id"] for o in outs] == [w["person_id"] for w in want] == [2, 1]
    for o, w in zip(outs, want):
        assert set(o) == set(w) and np.array_equal(o["frame_ids"], w["frame_ids"])
        for key in w:
            if key not in ("frame_ids", "person_id"):
                assert o[key].dtype == w[key].dtype and torch.equal(bits(o[key]), bits(w[key])), key


@pytest.fixture(scope="module")
def whole(folder, faces, tmp_path_factory):
    """The whole-video route, once: (outs, the files of both folders, the extractor's features in row order)."""
    from pmce_amd import demo
    from test_gpu_demo import get_model
    out = tmp_path_factory.mktemp("whole")
    ext = GatherExtractor()
    outs = demo.render_folder(get_model(256), folder, str(out / "out"), trk(), Pose(), ext, faces, input_folder=str(out / "in"),
                              vis_thresh=VIS, seed=3)
    torch.cuda.synchronize()
    return outs, read_all(str(out / "out")), read_all(str(out / "in")), torch.cat(ext.calls)


def test_the_stubs_put_unusable_frames_at_the_chunk_borders(folder, whole):
    """The conditions the chunked comparison rests on, on the host: both tracklets keep at least 16 frames after trimming, a frame
    next to a border of frames_per_pass = 7 is unusable (the boxes are interpolated ACROSS that border), and the overlay draws."""
    from pmce_amd import demo
    frames, _, names = demo.load_frames(folder)
    boxes, ids = demo.track_video(frames, trk())
    kps = demo.pose_tracklets(frames, boxes, Pose())
    usable = [(kp[:, 0, 2] > VIS).cpu().numpy() for kp, _ in kps]
    print("usable:", ["".join("x" if u else "." for u in us) for us in usable])
    outs = whole[0]
    assert len(names) == 30 and all(len(fid) == 30 for _, fid in kps)
    for o, us in zip(outs, usable):
        hit = np.flatnonzero(us)
        assert len(o["frame_ids"]) == hit[-1] + 1 - hit[0] >= 16 and o["frame_ids"][0] == hit[0]
    border = [f for f in range(30) if f % 7 in (0, 6) and 0 < f < 29]
    inside = [f for us, o in zip(usable, outs) for f in border if not us[f] and o["frame_ids"][0] < f < o["frame_ids"][-1]]
    assert inside, "no unusable frame next to a border of 7"
    assert whole[1].keys() == whole[2].keys() == {f"{i:06d}.jpg" for i in range(30)}
    drawn = sum(whole[1][n] != whole[2][n] for n in whole[1])
    print("frames with an overlay:", drawn)
    assert drawn >= 10                                                                # the overlay is there to be compared


@pytest.mark.parametrize("k", [7, 30, 64])
def test_render_folder_in_passes_equals_the_whole_route(k, folder, faces, whole, tmp_path):
    from pmce_amd import demo
    from test_gpu_demo import get_model
    pose, ext = Pose(), GatherExtractor()
    outs = demo.render_folder(get_model(256), folder, str(tmp_path / "out"), trk(), pose, ext, faces, input_folder=str(tmp_path / "in"),
                              vis_thresh=VIS, seed=3, frames_per_pass=k)
    torch.cuda.synchronize()
    same_outs(outs, whole[0])
    assert read_all(str(tmp_path / "out")) == whole[1] and read_all(str(tmp_path / "in")) == whole[2]
    chunks = [min(k, 30 - a) for a in range(0, 30, k)]
    assert [c[0] for c in pose.calls] == chunks and sum(c[1] for c in pose.calls) == 60     # pose saw one chunk of frames at a time
    # the features, put back by the host plan, are the whole route's rows
    plan = demo.plan_passes(np.concatenate([o["frame_ids"] for o in outs]), 30, k)
    feats = torch.empty_like(whole[3])
    for f, (_, _, rows, _) in zip(ext.calls, [p for p in plan if len(p[2])]):
        feats[torch.from_numpy(rows).to(DEV)] = f
    assert torch.equal(bits(feats), bits(whole[3]))


def test_run_folder_in_passes_equals_the_whole_route(folder, whole):
    from pmce_amd import demo
    from test_gpu_demo import get_model
    outs = demo.run_folder(get_model(256), folder, trk(), Pose(), GatherExtractor(), vis_thresh=VIS, seed=3, frames_per_pass=7)
    torch.cuda.synchronize()
    same_outs(outs, whole[0])


def test_a_short_tracklet_is_refused_before_the_extractor_runs(folder):
    from pmce_amd import demo
    from test_gpu_demo import get_model
    ext = GatherExtractor()
    with pytest.raises(ValueError, match="tracklet 0: the demo's window list needs at least 16 frames"):
        demo.run_folder(get_model(256), folder, trk(), Pose(), ext, vis_thresh=2.0, frames_per_pass=7)
    assert not ext.calls


def test_the_projects_extractor_is_batch_invariant_across_passes(folder):
    """``FeatureExtractor`` in place of the stub: the chunked route hands it other batches (the rows of a chunk), and the features and
    everything after them keep the whole route's bits - the batch invariance the feature rests on."""
    from pmce_amd import demo, synth
    from pmce_amd.extractor import FeatureExtractor
    from test_gpu_demo import get_model
    net = FeatureExtractor.from_state_dict(synth.make_state_dict(synth.extractor_spec()), DEV)
    calls = []

    def ext(p):
        calls.append(net(p))
        return calls[-1]

    want = demo.run_folder(get_model(256), folder, trk(), Pose(), ext, vis_thresh=VIS, seed=3)
    feats_whole, n = torch.cat(calls), len(calls)
    outs = demo.run_folder(get_model(256), folder, trk(), Pose(), ext, vis_thresh=VIS, seed=3, frames_per_pass=7)
    torch.cuda.synchronize()
    same_outs(outs, want)
    plan = [p for p in demo.plan_passes(np.concatenate([o["frame_ids"] for o in outs]), 30, 7) if len(p[2])]
    assert len(calls) - n == len(plan) >= 4 and n == 1
    feats = torch.empty_like(feats_whole)
    for f, (_, _, rows, _) in zip(calls[n:], plan):
        feats[torch.from_numpy(rows).to(DEV)] = f
    assert torch.equal(bits(feats), bits(feats_whole)) and bool(torch.isfinite(feats).all())


def test_iter_frames_is_load_frames_in_steps(folder, tmp_path):
    from pmce_amd import demo
    frames, wh, names = demo.load_frames(folder)
    assert wh == WH
    for k in (7, 30, 64):
        parts = list(demo.iter_frames(folder, k))
        assert [p[0] for p in parts] == list(range(0, 30, k)) and sum((p[2] for p in parts), []) == names
        assert all(p[1].is_cuda and p[1].dtype == torch.uint8 and p[1].shape[0] == len(p[2]) <= k for p in parts)
        assert torch.equal(torch.cat([p[1] for p in parts]), frames)
    # a file of another size, in a later step: named
    for n in names[:9]:
        with open(os.path.join(folder, n), "rb") as src, open(tmp_path / n, "wb") as dst:
            dst.write(src.read())
    demo.save_frames(str(tmp_path), torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device=DEV), first=9)
    with pytest.raises(ValueError, match=r"000009\.jpg: 32 x 32"):
        list(demo.iter_frames(str(tmp_path), 3))
    with pytest.raises(ValueError, match=r"000009\.jpg: 32 x 32"):                     # ... or inside a step: jpeg.decode's own error
        list(demo.iter_frames(str(tmp_path), 4))
