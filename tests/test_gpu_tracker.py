"""GPU tests of the tracker's back half (csrc/tracker.hip through pmce_amd/tracker.py and demo.py) against tests/tracker_ref.py.

Conditions, not tolerances: every drawn input passes its guard in tests/test_tracker_host.py (NMS margin > 1e-4, unique assignments), and
under them every discrete result - counts, statuses, classes, source rows, ids, report order - is exactly the restatement's.  Floats
follow the project's rule: |device - ref_hi| <= 4 x dev, dev = max |ref_lo - ref_hi| of the restatement's own two precisions (fp32 / fp64
for the suppression, float64 / longdouble for SORT), asserted > 0 and printed (run with -s).  Bit cases compare the device with itself."""
import numpy as np
import pytest
import torch

import tracker_ref as TR
from tracker_ref import CAPS_SEED, NMS_CASES, PEOPLE_SEED, SCENE_SEEDS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def T():
    from pmce_amd import tracker
    return tracker


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


_refs = {}


def nms_refs(key, rows, **kw):
    """The restatement in fp64 and fp32, computed once per input."""
    if key not in _refs:
        _refs[key] = (TR.nms(rows, dtype=torch.float64, **kw), TR.nms(rows, dtype=torch.float32, **kw))
    return _refs[key]


def check_nms(rows, key, **kw):
    dets, count, status, src = (t.cpu() for t in T().nms(rows.to(DEV), return_rows=True, **kw))
    (d64, c64, s64, r64), (d32, c32, s32, r32) = nms_refs(key, rows, **kw)
    assert torch.equal(count, c64) and torch.equal(status, s64)
    assert torch.equal(src.long(), r64) and torch.equal(dets[..., 6].double(), d64[..., 6])
    assert torch.equal(bits(dets[..., 4:6]), bits(d32[..., 4:6]))                      # the kept confidences: to the bit
    for i in range(rows.shape[0]):
        assert torch.all(dets[i, int(count[i]):] == 0)
    return dets, d32, d64


@pytest.mark.parametrize("case", NMS_CASES[:5], ids=lambda c: f"n{c[0]}-R{c[1]}-nc{c[2]}")
def test_nms_against_the_restatement(case):
    n, R, nc, seed, frac = case
    rows = TR.draw_rows(n, R, nc, seed, frac)
    dets, d32, d64 = check_nms(rows, case)
    dev32 = float((d32[..., :4].double() - d64[..., :4]).abs().max())
    err = float((dets[..., :4].double() - d64[..., :4]).abs().max())
    print(f"nms corners R={R} nc={nc}: {err / dev32 if dev32 else float('inf'):.2f} x dev32 ({dev32:.2e})")
    assert dev32 > 0 and err <= FACTOR * dev32


def test_nms_no_candidates_and_every_row_a_candidate():
    rows = TR.draw_rows(2, 70, 2, NMS_CASES[1][3], 0.5)
    rows[..., 4] = rows[..., 4] * 0.4
    dets, count, status = T().nms(rows.to(DEV))
    assert not count.any() and not status.any() and not dets.any()
    n, R, nc, seed, frac = NMS_CASES[6]
    rows = TR.draw_rows(n, R, nc, seed, frac)
    assert bool((rows[..., 4] >= 0.5).all())
    dets, d32, d64 = check_nms(rows, NMS_CASES[6])
    assert float((dets[..., :4].double() - d64[..., :4]).abs().max()) <= FACTOR * float((d32[..., :4].double() - d64[..., :4]).abs().max())


def test_nms_more_than_1024_candidates():
    """1500 candidates: two elements per thread in the sort, 24 chunks of 64 in the greedy loop, 80 KB of LDS."""
    rows = TR.draw_many_rows()
    dets, d32, d64 = check_nms(rows, "many", max_candidates=2048)
    dev32 = float((d32[..., :4].double() - d64[..., :4]).abs().max())
    err = float((dets[..., :4].double() - d64[..., :4]).abs().max())
    print(f"nms corners, 1500 candidates: {err / dev32:.2f} x dev32 ({dev32:.2e})")
    assert dev32 > 0 and err <= FACTOR * dev32
    _, count, status = T().nms(rows.to(DEV))                                           # the default cap of 1024
    assert count.tolist() == [0] and status.tolist() == [1]
    small = TR.draw_rows(3, 70, 2, NMS_CASES[1][3], 0.5).to(DEV)                       # the larger LDS changes no bit of a small image
    for a, b in zip(T().nms(small), T().nms(small, max_candidates=2048)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("caps", [dict(max_candidates=8), dict(max_keep=2)], ids=["max_candidates", "max_keep"])
def test_nms_caps(caps):
    rows = TR.draw_caps_rows(CAPS_SEED)
    dets, d32, d64 = check_nms(rows, ("caps", tuple(caps.items())), **caps)
    want = 1 if "max_candidates" in caps else 2
    _, count, status = (t.cpu() for t in T().nms(rows.to(DEV), **caps))
    assert status.tolist() == [want, 0, want] and count.tolist() == [0, 2, 0]
    assert not dets[0].any() and not dets[2].any() and dets[1, :2, :4].abs().min() > 0
    alone = T().nms(rows[1:2].to(DEV), **caps)[0].cpu()
    assert torch.equal(bits(alone[0]), bits(dets[1]))                                  # the neighbour is untouched


def test_nms_infinite_extent_terminates():
    rows = torch.tensor([[[50, 50, float("inf"), 20, 0.9, 0.8], [50, 50, 20, 20, 0.8, 0.8]]], dtype=torch.float32)
    dets, count, status, src = (t.cpu() for t in T().nms(rows.to(DEV), return_rows=True))
    d32, c32, s32, r32 = TR.nms(rows, dtype=torch.float32)
    assert count.tolist() == [2] and status.tolist() == [0] and src[0, :2].tolist() == [0, 1]
    assert torch.isnan(dets[0, 0, :4]).all() and torch.equal(bits(dets[0, 1]), bits(d32[0, 1]))


def test_nms_batch_and_run_invariance():
    n, R, nc, seed, frac = NMS_CASES[5]
    rows = TR.draw_rows(n, R, nc, seed, frac).to(DEV)
    geo = (420, 0, 1920 / 416)
    full = T().nms(rows, geometry=geo, return_rows=True)
    again = T().nms(rows, geometry=geo, return_rows=True)
    for a, b in zip(full, again):
        assert torch.equal(a, b) and torch.equal(bits(a) if a.is_floating_point() else a, bits(b) if b.is_floating_point() else b)
    for i in range(n):
        one = T().nms(rows[i:i + 1], geometry=geo, return_rows=True)
        for a, b in zip(full, one):
            assert torch.equal(bits(a[i]) if a.is_floating_point() else a[i], bits(b[0]) if b.is_floating_point() else b[0])
    assert int(full[1].min()) > 0 and int(full[4].sum()) > 0


def test_nms_people_epilogue():
    from pmce_amd import yolo
    _, _, pad_x, pad_y, ratio = yolo.letterbox_geometry(1080, 1920, 416)               # letterbox's own geometry, no frames
    geo = (pad_x, pad_y, ratio)
    assert geo == (0, 420, 1920 / 416)
    rows = TR.draw_people_rows(PEOPLE_SEED)
    seen = set()
    for kw in (dict(), dict(class_id=1), dict(score="product"), dict(score="product", score_thres=0.55, class_id=1)):
        dets, count, status, ppl, cnt = (t.cpu() for t in T().nms(rows.to(DEV), geometry=geo, **kw))
        want, wcnt = TR.people(dets, count, geo, **kw)
        assert cnt.tolist() == wcnt.tolist() and np.array_equal(ppl.numpy(), want)     # the same fp64 operations: equal
        assert int(cnt.sum()) > 0
        seen.add(tuple(cnt.tolist()))
        # the planted row (kept first: the highest score, class 0, conf 0.99) has w = 0 and is dropped
        assert dets[0, 0, 6] == 0 and dets[0, 0, 4] > 0.9 and dets[0, 0, 2] == dets[0, 0, 0]
        if kw.get("class_id", 0) == 0:
            assert not np.any(ppl[0, :, 4].numpy() == float(dets[0, 0, 4]))
    assert len(seen) >= 3                                                              # the filters filter differently
    # strictly greater: a threshold equal to a kept person's score drops exactly that row
    dets, count, status, ppl, cnt = (t.cpu() for t in T().nms(rows.to(DEV), geometry=geo))
    k = int(cnt[1]) - 1
    thr = float(ppl[1, k, 4])
    at = T().nms(rows.to(DEV), geometry=geo, score_thres=thr)[4].cpu()
    below = T().nms(rows.to(DEV), geometry=geo, score_thres=float(np.nextafter(thr, 0)))[4].cpu()
    n_eq = int((ppl[1, :int(cnt[1]), 4] == thr).sum())
    assert int(below[1]) - int(at[1]) == n_eq >= 1


# ----------------------------------------------------------------------------------------------
# SORT
# ----------------------------------------------------------------------------------------------

def dev_sort(p, c, **kw):
    t, n, s = T().sort_tracks(torch.from_numpy(p).to(DEV), torch.from_numpy(c).to(DEV), **kw)
    return t.cpu().numpy(), n.cpu().numpy(), s.cpu().numpy()


def scene_refs(key, p, c, **kw):
    if key not in _refs:
        _refs[key] = (TR.sort_tracks(p, c, **kw), TR.sort_tracks(p, c, dtype=np.longdouble, **kw))
    return _refs[key]


def check_sort(p, c, key, **kw):
    (t64, n64, s64), (tld, nld, sld) = scene_refs(key, p, c, **kw)
    t, n, s = dev_sort(p, c, **kw)
    assert np.array_equal(n, n64) and np.array_equal(s, s64) and np.array_equal(n64, nld)
    assert np.array_equal(t[..., 4], t64[..., 4]) and np.array_equal(t64[..., 4], tld[..., 4].astype(np.float64))     # ids in report order
    dev64 = float(np.abs(t64[..., :4] - tld[..., :4]).max())
    err = float(np.abs(t[..., :4] - tld[..., :4]).max())
    print(f"sort boxes {key}: {err / dev64 if dev64 else float('inf'):.2f} x dev64 ({dev64:.2e} px)")
    assert dev64 > 0 and err <= FACTOR * dev64
    return t, n, s


def test_sort_scene_against_the_restatement():
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    t, n, s = check_sort(p, c, "scene")
    assert n[33] == 0 and set(np.unique(t[..., 4])) == {0.0, 1.0, 2.0, 3.0, 4.0} and not s.any()


def test_sort_assignment_is_not_greedy():
    p, c = TR.scene_2x2()
    t, n, s = check_sort(p, c, "2x2")
    assert t[1, :2, 4].tolist() == [2.0, 1.0] and t[1, 0, 0] > t[1, 1, 0]


def test_sort_two_sequences_in_one_launch():
    (p0, c0), (p1, c1) = TR.draw_scene(SCENE_SEEDS[0]), TR.draw_scene(SCENE_SEEDS[1])
    both = dev_sort(np.concatenate([p0, p1]), np.concatenate([c0, c1]), seq_offsets=[0, 40, 80])
    a, b = dev_sort(p0, c0), dev_sort(p1, c1)
    for x, y, z in zip(both, a, b):
        assert np.array_equal(x[:40].view(np.int64 if x.dtype == np.float64 else x.dtype), y.view(np.int64 if y.dtype == np.float64 else y.dtype))
        assert np.array_equal(x[40:].view(np.int64 if x.dtype == np.float64 else x.dtype), z.view(np.int64 if z.dtype == np.float64 else z.dtype))
    again = dev_sort(np.concatenate([p0, p1]), np.concatenate([c0, c1]), seq_offsets=[0, 40, 80])
    assert all(np.array_equal(x, y) for x, y in zip(both, again))
    r1 = TR.sort_tracks(p1, c1)
    assert np.array_equal(b[1], r1[1]) and np.array_equal(b[0][..., 4], r1[0][..., 4])


def test_sort_max_tracks_and_update_on_empty():
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    t, n, s = dev_sort(p, c, max_tracks=2)
    rt, rn, rs = TR.sort_tracks(p, c, max_tracks=2)
    assert s.any() and np.array_equal(s, rs) and np.array_equal(n, rn) and np.array_equal(t[..., 4], rt[..., 4])
    t1, n1, s1 = check_sort(p, c, "scene-uoe", update_on_empty=1)
    t0, n0, s0 = dev_sort(p, c)
    r0 = TR.sort_tracks(p, c)
    r1 = TR.sort_tracks(p, c, update_on_empty=1)
    assert not np.array_equal(n1, n0) and np.array_equal(n1 != n0, r1[1] != r0[1])    # differs exactly where the restatement does


def test_sort_one_frame_and_empty_frames_only():
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    t, n, s = dev_sort(p[:1], c[:1])
    rt, rn, rs = TR.sort_tracks(p[:1], c[:1])
    assert n.tolist() == rn.tolist() == [2] and np.array_equal(t[..., 4], rt[..., 4]) and np.abs(t - rt).max() < 1e-9
    for uoe in (False, True):
        t, n, s = dev_sort(np.zeros((5, 8, 5)), np.zeros(5, np.int32), update_on_empty=uoe)
        assert not n.any() and not s.any() and not t.any()


# ----------------------------------------------------------------------------------------------
# records and the chain
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_frames", [1, 10, 25])
def test_tracklet_records(min_frames):
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    tracks, count, _ = T().sort_tracks(torch.from_numpy(p).to(DEV), torch.from_numpy(c).to(DEV))
    recs, ids = T().tracklet_records(tracks, count, min_frames=min_frames)
    want, wids = TR.tracklet_records(tracks.cpu().numpy(), count.cpu().numpy(), min_frames=min_frames)
    assert ids == wids and len(recs) == len(want) and (min_frames == 25 or len(ids) >= 2)
    for (b, f), (wb, wf) in zip(recs, want):
        assert b.is_cuda and b.dtype == torch.float64 and f.dtype == np.int64 and np.array_equal(f, wf)
        assert np.array_equal(b.cpu().numpy(), wb) and bool((b[:, 2] == b[:, 3]).all())
    if min_frames == 1:
        assert ids[:2] == [2, 1]                                                       # first frame's report order: descending id
        two = T().tracklet_records(torch.cat([tracks, tracks]), torch.cat([count, count]), min_frames=1, seq_offsets=[0, 40, 80])
        assert two[0][1] == ids == two[1][1] and np.array_equal(two[1][0][0][1], recs[0][1])
        assert torch.equal(two[1][0][0][0], recs[0][0])


class PlantedDet:
    """A detector that ignores its images and serves planted rows, chunk after chunk."""

    def __init__(self, rows):
        self.rows, self.at, self.shapes = rows.to(DEV), 0, []

    def __call__(self, images):
        n = images.shape[0]
        self.shapes.append(tuple(images.shape))
        out = self.rows[self.at:self.at + n]
        self.at += n
        return out


def tiny_frames(F=30, H=48, W=64):
    return torch.from_numpy(np.random.default_rng(TR.SEED).integers(0, 256, (F, H, W, 3), dtype=np.uint8))


def test_tracker_chain_equals_the_stages_by_hand():
    from pmce_amd import demo, yolo
    rows, frames = TR.planted_video_rows(), tiny_frames()
    det = PlantedDet(rows)
    trk = T().Tracker(det, size=64, batch=12)
    recs, ids = trk(frames)
    assert det.shapes == [(12, 3, 64, 64), (12, 3, 64, 64), (6, 3, 64, 64)]
    _, _, pad_x, pad_y, ratio = yolo.letterbox_geometry(48, 64, 64)
    res = T().nms(rows.to(DEV), geometry=(pad_x, pad_y, ratio))
    tracks, count, status = T().sort_tracks(res[3], res[4])
    want, wids = T().tracklet_records(tracks, count)
    assert ids == wids == [2, 1] and not bool(status.any()) and not bool(res[2].any())
    for (b, f), (wb, wf) in zip(recs, want):
        assert torch.equal(bits(b), bits(wb)) and np.array_equal(f, wf) and len(f) == 30
    ref = TR.tracklet_records(*TR.sort_tracks(*TR.people(*TR.nms(rows)[:2], (pad_x, pad_y, ratio)))[:2])
    assert ref[1] == ids and all(np.abs(b.cpu().numpy() - wb).max() < 1e-3 for (b, _), (wb, _) in zip(recs, ref[0]))
    # demo.track_video's output is what demo.pose_tracklets takes
    boxes, pids = demo.track_video(frames.to(DEV), T().Tracker(PlantedDet(rows), size=64, batch=12))
    calls = []

    def pose(fr, frame_index, bx):
        calls.append((tuple(frame_index.shape), tuple(bx.shape), bx.dtype))
        return torch.zeros(len(frame_index), 17, 3, device=DEV), None

    kps = demo.pose_tracklets(frames.to(DEV), boxes, pose)
    assert pids == [2, 1] and calls == [((60,), (60, 4), torch.float64)] and [tuple(k.shape) for k, _ in kps] == [(30, 17, 3)] * 2
    assert demo.track_video(frames, T().Tracker(PlantedDet(rows), size=64, batch=30), min_frames=31) == ([], [])


def test_tracker_raises_on_a_status_and_names_the_frame():
    rows, frames = TR.planted_video_rows(), tiny_frames()
    rows[:5, :, 4] = 0.01                                                              # the first five frames are empty: frame 5 is the first over the cap
    with pytest.raises(ValueError, match=r"frame 5: .*max_keep = 1"):
        T().Tracker(PlantedDet(rows), size=64, batch=12, max_keep=1)(frames)
    with pytest.raises(ValueError, match=r"frame 5: .*max_candidates = 3"):
        T().Tracker(PlantedDet(rows), size=64, batch=7, max_candidates=3)(frames)
    with pytest.raises(ValueError, match=r"frame 5: .*max_tracks = 1"):
        T().Tracker(PlantedDet(rows), size=64, batch=12, max_tracks=1)(frames)


def test_run_frames_is_the_chain_of_the_three_stages():
    """uint8 frames -> what the demo saves, with planted rows as the detector, a pose stub that places 17 keypoints inside each box and
    a linear extractor: ``demo.run_frames`` equals ``track_video`` -> ``pose_tracklets`` -> ``run_video`` by hand, to the bit."""
    from pmce_amd import demo
    from test_gpu_demo import get_model
    model = get_model(256)
    rows, frames = TR.planted_video_rows(), tiny_frames().to(DEV)
    g = torch.Generator().manual_seed(14)
    weight = (torch.randn(3 * 28 * 28, 2048, generator=g) * 0.02).to(DEV)
    uv = (torch.rand(17, 2, generator=g, dtype=torch.float64) - 0.5).to(DEV) * 0.8

    def extractor(p):
        return torch.nn.functional.avg_pool2d(p, 8).flatten(1) @ weight

    class Pose:
        box_format = "cxcywh"

        def __call__(self, fr, frame_index, bx):
            xy = bx[:, None, :2] + uv[None] * bx[:, None, 2:]
            return torch.cat([xy, torch.full_like(xy[..., :1], 0.9)], -1).float(), None

    def trk():
        return T().Tracker(PlantedDet(rows), size=64, batch=12)

    outs = demo.run_frames(model, frames, trk(), Pose(), extractor, (64, 48), seed=3)
    boxes, ids = demo.track_video(frames, trk())
    want = demo.run_video(model, frames, demo.pose_tracklets(frames, boxes, Pose()), extractor, (64, 48), seed=3)
    torch.cuda.synchronize()
    assert [o["person_id"] for o in outs] == ids == [2, 1] and len(want) == 2
    for o, w in zip(outs, want):
        assert np.array_equal(o["frame_ids"], w["frame_ids"]) and len(o["frame_ids"]) == 30 and bool(torch.isfinite(o["mesh"]).all())
        for key in w:
            if key != "frame_ids":
                assert torch.equal(o[key], w[key]), key
    bad = Pose()
    bad.box_format = "xyxy"
    with pytest.raises(ValueError, match="cxcywh"):
        demo.run_frames(model, frames, trk(), bad, extractor, (64, 48))
