"""CPU-only tests of the tracker's back half: the restatements of tests/tracker_ref.py on hand-worked cases, the guards on every
input the GPU tests draw (a failing guard means the seed is changed here, not on the GPU), and the C entries' argument checks."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import tracker_ref as TR
from conftest import REPO

MARGIN = 1e-4
NMS_CASES, SCENE_SEEDS = TR.NMS_CASES, TR.SCENE_SEEDS


def row(cx, cy, w, h, conf, *cls):
    return [cx, cy, w, h, conf, *cls]


def shifted_pair(cls_a, cls_b):
    """Two 99 x 99 boxes whose +1-form IoU is 0.5: 100 x 100 pixel areas shifted by 100 / 3."""
    return torch.tensor([[row(50, 50, 99, 99, 0.9, *cls_a), row(50 + 100 / 3, 50, 99, 99, 0.6, *cls_b)]], dtype=torch.float32)


def test_nms_two_boxes_one_class_merge():
    rows = shifted_pair((0.8, 0.1), (0.7, 0.2))
    d, c, s, src = TR.nms(rows, dtype=torch.float64)
    assert c.tolist() == [1] and s.tolist() == [0] and src[0, 0] == 0
    x = rows[0].double()
    want_x1 = (x[0, 4] * (x[0, 0] - x[0, 2] / 2) + x[1, 4] * (x[1, 0] - x[1, 2] / 2)) / (x[0, 4] + x[1, 4])
    assert abs(float(d[0, 0, 0] - want_x1)) < 1e-12
    assert float(d[0, 0, 4]) == float(x[0, 4]) and float(d[0, 0, 5]) == float(x[0, 5]) and d[0, 0, 6] == 0
    assert torch.all(d[0, 1:] == 0)


def test_nms_two_boxes_two_classes_stay():
    d, c, s, src = TR.nms(shifted_pair((0.8, 0.1), (0.2, 0.7)), dtype=torch.float64)
    assert c.tolist() == [2] and src[0, :2].tolist() == [0, 1] and d[0, :2, 6].tolist() == [0, 1]
    assert abs(float(d[0, 1, 0]) - (50 + 100 / 3 - 49.5)) < 1e-5            # its own corners


def test_nms_duplicates_tie_by_row_and_caps():
    r = row(50, 50, 20, 20, 0.9, 0.8, 0.1)
    far = row(300, 300, 20, 20, 0.9, 0.8, 0.1)
    rows = torch.tensor([[far, r, r, far]], dtype=torch.float32)
    d, c, s, src = TR.nms(rows, dtype=torch.float32)
    assert c.tolist() == [2] and src[0, :2].tolist() == [0, 1]               # equal keys: the lower row leads, its duplicate merges
    assert TR.nms(rows, max_candidates=3)[2].tolist() == [1] and TR.nms(rows, max_candidates=3)[1].tolist() == [0]
    d2 = TR.nms(rows, max_keep=1)
    assert d2[2].tolist() == [2] and d2[1].tolist() == [0] and torch.all(d2[0] == 0)
    assert TR.nms_margin(rows) > 0.05                                        # exact duplicates are no near tie


def test_nms_head_always_leaves():
    rows = torch.tensor([[row(50, 50, float("inf"), 20, 0.9, 0.8), row(50, 50, 20, 20, 0.8, 0.8)]], dtype=torch.float32)
    d, c, s, src = TR.nms(rows, dtype=torch.float32)
    assert c.tolist() == [2] and src[0, :2].tolist() == [0, 1] and torch.isnan(d[0, 0, 0]) and torch.isfinite(d[0, 1, :4]).all()


def test_people_filter_and_map():
    dets = torch.zeros(1, 4, 7)
    dets[0, 0] = torch.tensor([10, 20, 110, 220, 0.9, 0.8, 0])
    dets[0, 1] = torch.tensor([10, 20, 110, 220, 0.9, 0.8, 1])               # another class
    dets[0, 2] = torch.tensor([10, 20, 110, 220, 0.7, 0.99, 0])              # not strictly above 0.7 (fp32 0.7 < 0.7)
    dets[0, 3] = torch.tensor([10, 20, 10, 220, 0.95, 0.9, 0])               # empty
    p, n = TR.people(dets, [4], (420, 0, 1920 / 416))
    assert n.tolist() == [1] and np.allclose(p[0, 0], [10 * 1920 / 416 - 420, 20 * 1920 / 416, 110 * 1920 / 416 - 420, 220 * 1920 / 416, np.float32(0.9)])
    p, n = TR.people(dets, [4], (420, 0, 1920 / 416), score="product", score_thres=0.69)
    assert n.tolist() == [2] and p[0, 1, 4] == float(np.float32(0.7) * np.float32(0.99))


def test_assignment_is_not_greedy():
    m = np.array([[0.6, 0.5], [0.55, 0.0]])
    assert TR.assign_scipy(m) == [(0, 1), (1, 0)] == TR.assign_brute(m)
    assert TR.assignment_is_unique(m, 0.3)
    assert not TR.assignment_is_unique(np.array([[0.6, 0.6], [0.6, 0.6]]), 0.3)
    assert not TR.assignment_is_unique(np.array([[0.3 + 5e-7, 0.0]]), 0.3)


def test_scipy_agrees_with_brute_force():
    g = np.random.default_rng(TR.SEED)
    for _ in range(40):
        nd, nt = g.integers(1, 7, 2)
        m = g.uniform(0, 1, (nd, nt)) * (g.uniform(0, 1, (nd, nt)) > 0.3)
        a, b = TR.assign_scipy(m), TR.assign_brute(m)
        assert abs(sum(m[d, t] for d, t in a) - sum(m[d, t] for d, t in b)) < 1e-12
        if TR.assignment_is_unique(m, 0.3):
            assert {p for p in a if m[p] >= 0.3} == {p for p in b if m[p] >= 0.3}


def one_person(frames, missing=()):
    p, c = np.zeros((frames, 4, 5)), np.zeros(frames, np.int32)
    for f in range(frames):
        if f not in missing:
            p[f, 0] = [100 + 4 * f, 50 + f, 160 + 4 * f, 200 + f, 0.9]
            c[f] = 1
    return p, c


def test_sort_one_person():
    p, c = one_person(10)
    t, n, s = TR.sort_tracks(p, c)
    assert n.tolist() == [1] * 10 and (t[:, 0, 4] == 1).all() and not s.any()
    assert np.abs(t[9, 0, :4] - p[9, 0, :4]).max() < 1.0 and np.abs(t[0, 0, :4] - p[0, 0, :4]).max() < 1e-9
    tl = TR.sort_tracks(p, c, dtype=np.longdouble)[0]
    assert 0 < np.abs(tl - t).max() < 1e-10


def test_sort_gaps_and_empty_frames():
    p, c = one_person(12, missing=(5,))                                       # alone, an empty frame is not seen by the tracker at all
    t, n, _ = TR.sort_tracks(p, c)
    assert n.tolist() == [1] * 5 + [0] + [1] * 6 and set(t[:, 0, 4]) == {0.0, 1.0}
    t1, n1, _ = TR.sort_tracks(p, c, update_on_empty=1)                       # seen, a one-frame gap keeps the id; unreported until hit_streak is 3 again
    assert set(t1[:, 0, 4]) == {0.0, 1.0} and n1.tolist() == [1] * 5 + [0, 0, 0] + [1] * 4
    p, c = one_person(14, missing=(5, 6))                                     # a two-frame gap: the frames are skipped, the tracker never ages
    t, n, _ = TR.sort_tracks(p, c)
    assert set(t[:, 0, 4]) == {0.0, 1.0} and n.tolist() == [1] * 5 + [0, 0] + [1] * 7
    t2, n2, _ = TR.sort_tracks(p, c, update_on_empty=1)                       # with update_on_empty it dies and a new id appears
    assert set(t2[:, 0, 4]) == {0.0, 1.0, 2.0} and n2.tolist() == [1] * 5 + [0] * 5 + [1] * 4


def test_sort_two_frame_gap_of_one_person_among_others_gives_a_new_id():
    p, c = TR.draw_scene(SCENE_SEEDS[0])
    t, n, _ = TR.sort_tracks(p, c)
    assert set(np.unique(t[:, :, 4])) == {0.0, 1.0, 2.0, 3.0, 4.0}            # person 2 (id 2) comes back as id 4
    assert n[33] == 0 and n[34] == 3                                          # the empty frame left frame_count and the streaks alone
    assert t[12, :2, 4].tolist() == [3.0, 2.0] and 1.0 in t[15, :3, 4]        # the one-frame gap keeps id 1


def test_sort_reports_everything_while_frame_count_is_small():
    p, c = one_person(8)
    p[3:, 1], c[3:] = [400, 50, 460, 200, 0.9], 2                             # a second person from frame 3 (frame_count 4 > min_hits):
    t, n, _ = TR.sort_tracks(p, c)                                            # reported once its hit_streak is 3
    assert n.tolist() == [1] * 6 + [2, 2] and t[6, :2, 4].tolist() == [2.0, 1.0]
    t, n, st = TR.sort_tracks(p, c, max_tracks=1)
    assert st.tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and n.tolist() == [1] * 8
    p, c = one_person(8)
    p[1:, 1], c[1:] = [400, 50, 460, 200, 0.9], 2                             # from frame 1 (frame_count 2): at once, then not at frame_count 4
    assert TR.sort_tracks(p, c)[1].tolist() == [1, 2, 2, 1, 2, 2, 2, 2]


def test_records():
    tracks, cnt = np.zeros((4, 3, 5)), np.array([2, 2, 1, 2], np.int32)
    wide, tall = [10, 20, 110, 60], [10, 20, 50, 120]
    tracks[0, 0], tracks[0, 1] = wide + [2], tall + [1]
    tracks[1, 0], tracks[1, 1] = wide + [2], tall + [1]
    tracks[2, 0] = tall + [1]
    tracks[3, 0], tracks[3, 1] = wide + [3], tall + [1]
    recs, ids = TR.tracklet_records(tracks, cnt, min_frames=1)
    assert ids == [2, 1, 3]                                                   # a dict filled in report order
    assert recs[0][0].tolist() == [[60, 40, 100, 100]] * 2 and recs[1][0][0].tolist() == [30, 70, 100, 100]
    assert recs[1][1].tolist() == [0, 1, 2, 3] and recs[2][1].tolist() == [3]
    assert TR.tracklet_records(tracks, cnt, min_frames=2)[1] == [2, 1] and TR.tracklet_records(tracks, cnt, min_frames=5)[1] == []
    both = TR.tracklet_records(tracks, cnt, min_frames=1, seq_offsets=[0, 2, 4])
    assert both[0][1] == [2, 1] and both[1][1] == [1, 3] and both[1][0][0][1].tolist() == [0, 1]


@pytest.mark.parametrize("case", NMS_CASES, ids=lambda c: f"n{c[0]}-R{c[1]}-nc{c[2]}")
def test_guard_nms_inputs(case):
    n, R, nc, seed, frac = case
    rows = TR.draw_rows(n, R, nc, seed, frac)
    assert TR.nms_margin(rows) > MARGIN
    d, c, s, _ = TR.nms(rows, dtype=torch.float64)
    assert not s.any() and (c > 0).all()
    if R >= 40:
        d32 = TR.nms(rows, dtype=torch.float32)[0]
        assert float((d32.double() - d)[..., :4].abs().max()) > 0            # the float tolerance of the GPU test is not empty
        assert int(c.max()) < int((rows[..., 4] >= 0.5).sum(1).max())        # something was merged


def test_guard_caps_and_people_inputs():
    rows = TR.draw_caps_rows(TR.CAPS_SEED)
    assert TR.nms_margin(rows) > MARGIN
    assert (rows[..., 4] >= 0.5).sum(1).tolist() == [20, 2, 20] and TR.nms(rows, dtype=torch.float64)[1][1] == 2
    assert TR.nms(rows, max_candidates=8)[2].tolist() == [1, 0, 1] and TR.nms(rows, max_keep=2)[2].tolist() == [2, 0, 2]
    rows = TR.draw_people_rows(TR.PEOPLE_SEED)
    assert TR.nms_margin(rows) > MARGIN
    d, c, s, src = TR.nms(rows)
    assert src[:, 0].tolist() == [0, 0, 0] and not s.any()
    counts = {tuple(TR.people(d, c, (0, 420, 1920 / 416), **kw)[1].tolist()) for kw in
              (dict(), dict(class_id=1), dict(score="product"), dict(score="product", score_thres=0.55, class_id=1))}
    assert len(counts) >= 3 and all(sum(t) > 0 for t in counts)


def test_guard_many_candidates():
    rows = TR.draw_many_rows()
    assert TR.nms_margin(rows) > MARGIN and int((rows[..., 4] >= 0.5).sum()) == 1500
    d, c, s, _ = TR.nms(rows, max_candidates=2048, dtype=torch.float64)
    assert 6 <= int(c[0]) <= 12 and not s.any() and TR.nms(rows)[2].tolist() == [1]
    assert float((TR.nms(rows, max_candidates=2048)[0].double() - d)[..., :4].abs().max()) > 0


@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_guard_scenes(seed):
    p, c = TR.draw_scene(seed)
    for kw in (dict(), dict(update_on_empty=1), dict(max_tracks=2)):
        ious = []
        TR.sort_tracks(p, c, ious=ious, **kw)
        assert ious and all(TR.assignment_is_unique(m, 0.3) for m in ious)
    p, c = TR.scene_2x2()
    ious = []
    t, n, _ = TR.sort_tracks(p, c, ious=ious)
    assert np.abs(ious[0] - [[0.6, 0.5], [0.55, 0.0]]).max() < 1e-12 and TR.assignment_is_unique(ious[0], 0.3)
    assert t[1, :2, 4].tolist() == [2.0, 1.0] and t[1, 0, 0] > t[1, 1, 0]    # tracker 1 took detection 0 (the right one), tracker 0 detection 1


# ----------------------------------------------------------------------------------------------
# guards of the inputs at the kernels' documented sizes (tests/test_gpu_tracker_crowd.py)
# ----------------------------------------------------------------------------------------------

def guarded_sort(p, c, **kw):
    """The restatement in both precisions on a drawn input: every assignment unique at the run's threshold, every discrete result the
    same in float64 and longdouble, the float tolerance not empty -> (tracks, counts, status, IoU matrices, live ids per frame)."""
    ious, live = [], []
    t, n, s = TR.sort_tracks(p, c, ious=ious, live=live, **kw)
    tl, nl, sl = TR.sort_tracks(p, c, dtype=np.longdouble, **kw)
    assert ious and all(TR.assignment_is_unique(m, kw.get("iou_threshold", 0.3)) for m in ious)
    assert np.array_equal(n, nl) and np.array_equal(s, sl) and np.array_equal(t[..., 4], tl[..., 4].astype(np.float64))
    assert float(np.abs(t[..., :4] - tl[..., :4]).max()) > 0
    return t, n, s, ious, live


def test_row_ordered_solver_agrees_with_scipy():
    g = np.random.default_rng(TR.SEED + 1)
    for _ in range(40):
        nd, nt = g.integers(1, 7, 2)
        m = g.uniform(0, 1, (nd, nt)) * (g.uniform(0, 1, (nd, nt)) > 0.3)
        pairs, longest, used = TR.assign_paths(m)
        assert abs(sum(m[d, t] for d, t in pairs) - sum(m[d, t] for d, t in TR.assign_scipy(m))) < 1e-12 and 1 <= longest <= used + 1
    assert TR.assign_paths(np.array([[0.6, 0.5], [0.55, 0.0]])) == ([(0, 1), (1, 0)], 2, 1)


@pytest.mark.parametrize("n,reverse,shuffle", TR.CHAIN_CASES + [(2, False, None), (2, True, None)],
                         ids=lambda v: {None: "inorder", True: "rev", False: "fwd", TR.CHAIN_SHUFFLE: "shuffled"}.get(v, str(v)))
def test_guard_chain_scenes(n, reverse, shuffle):
    p, c = TR.chain_scene(n, reverse, shuffle)
    t, cnt, s, ious, _ = guarded_sort(p, c)
    order = np.array(TR.chain_order(n, reverse, shuffle))
    m = ious[0]
    assert m.shape == (n, n) and not s.any() and cnt.tolist() == [n] * 5
    own, nxt = m[np.arange(n), order], m[np.arange(n), np.clip(order + (-1 if reverse else 1), 0, n - 1)]
    assert np.abs(own - TR.CHAIN_A).max() < 1e-12 and np.abs(np.sort(nxt)[1:] - TR.CHAIN_B).max() < 1e-12 and TR.CHAIN_B > TR.CHAIN_A
    assert n * TR.CHAIN_A - (n - 1) * TR.CHAIN_B > 0.08                               # the margin of the identity: 0.089 at n = 64
    assert TR.assign_scipy(m) == sorted((d, int(b)) for d, b in enumerate(order))     # the optimum: every box on its own tracker
    assert int((m.argmax(1) != order).sum()) == n - 1                                 # every row but one prefers another tracker
    pairs, longest, used = TR.assign_paths(m)
    assert pairs == TR.assign_scipy(m) and used == n - 1                              # some row's search goes through every column
    if shuffle is None:
        assert longest == n                                                           # in order: the last row re-routes all the others
    else:
        assert longest >= n // 2 and not np.array_equal(order, np.arange(n)) and not np.array_equal(order, np.arange(n)[::-1])
    assert t[1, :n, 4].tolist() == list(range(n, 0, -1))                              # every id kept, reported in descending order


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("shuffle", [None, TR.CHAIN_SHUFFLE], ids=["inorder", "shuffled"])
def test_guard_chain_variants(reverse, shuffle):
    n = 33
    p, c = TR.chain_scene(n, reverse, shuffle, extra=True)                            # more detections than trackers: the extra box LOSES
    t, cnt, s, ious, _ = guarded_sort(p, c)
    order = TR.chain_order(n, reverse, shuffle, extra=True)
    k, end = order.index(n), 0 if reverse else n - 1
    assert ious[0].shape == (n + 1, n) and 0.3 < ious[0][k, end] < TR.CHAIN_A and np.count_nonzero(ious[0][k]) == 1
    assert (k, end) not in TR.assign_scipy(ious[0]) and len(TR.assign_scipy(ious[0])) == n
    assert t[1, :n + 1, 4].tolist() == list(range(n + 1, 0, -1)) and cnt[1] == n + 1 and not s.any()
    p, c = TR.chain_scene(n, reverse, shuffle, drop=16)                               # fewer: the chain is cut in two
    t, cnt, s, ious, _ = guarded_sort(p, c)
    order = np.array(TR.chain_order(n, reverse, shuffle, drop=16))
    moved = order > 16 if reverse else order < 16                                     # before the gap: on to the neighbour's tracker
    want = sorted((d, int(b) + int(moved[d]) * (-1 if reverse else 1)) for d, b in enumerate(order))
    assert ious[0].shape == (n - 1, n) and TR.assign_scipy(ious[0]) == want and int(moved.sum()) == 16
    assert sorted(t[1, :n - 1, 4].tolist()) == [i + 1 for i in range(n) if i != (n - 1 if reverse else 0)]
    assert TR.assign_paths(ious[0])[1] >= (16 if shuffle is None else 4)


def test_guard_chain_holes():
    p, c = TR.chain_holes()
    t, cnt, s, ious, live = guarded_sort(p, c, **TR.HOLES_KW)
    dead, n = TR.HOLES_DEAD, TR.HOLES_N
    assert live[1][1] == [i for i in range(n) if i not in dead] and live[2][1] == live[1][1] + [n, n + 1, n + 2]
    m = ious[1]                                                                       # frame 2: 38 detections, 35 trackers in 40 slots
    assert m.shape == (n - len(dead) + TR.HOLES_NEW, n - len(dead)) and cnt.tolist() == [40, 35, 35, 38, 38] and not s.any()
    pairs = [(d, k) for d, k in TR.assign_scipy(m) if m[d, k] >= 0.3]
    assert len(pairs) == 35 and all(abs(m[d, k] - TR.CHAIN_A) < 1e-9 for d, k in pairs)
    assert int((m.argmax(1)[[d for d, _ in pairs]] != [k for _, k in pairs]).sum()) == 35 - 5       # five chains of 7: 6 rows each prefer another
    mixed, below, seen = TR.replay_slots(live, {f: t[f, :cnt[f], 4].astype(int).tolist() for f in range(5)})
    assert below == TR.HOLES_NEW and mixed == 2 and seen == 5                         # born into slots 7, 15, 23; reported out of slot order


@pytest.mark.parametrize("seed", TR.CROWD_SEEDS)
def test_guard_crowds(seed):
    p, c = TR.draw_crowd(seed)
    assert int(c.max()) >= 36
    for kw in TR.CROWD_PARAMS:
        t, cnt, s, ious, live = guarded_sort(p, c, **kw)
        assert len(ious) == 23 and max(m.shape[0] for m in ious) >= 36 and max(m.shape[1] for m in ious) >= 36 and not s.any()
        assert any(m.shape[0] > m.shape[1] for m in ious) and any(m.shape[0] < m.shape[1] for m in ious)
        mixed, below, seen = TR.replay_slots(live, {f: t[f, :cnt[f], 4].astype(int).tolist() for f in range(24)})
        if kw in (dict(), dict(max_age=0, min_hits=0)):
            assert seen == 24 and mixed >= 6                                          # slot order is not id order in a quarter of the frames
        if kw == dict(max_age=0, min_hits=0):
            assert below >= 10 and t[..., 4].max() >= 70                              # births below live trackers; ids far beyond 40 persons
    q, d = TR.draw_crowd(TR.CROWD_SEEDS[1], frames=16)                                # the shorter crowd of the launch with three sequences
    guarded_sort(q, d)
    assert all(c[f] > 0 for f in TR.CROWD_EMPTY)
    p, c = TR.draw_crowd(seed, empty=TR.CROWD_EMPTY)
    t1, n1, _, _, _ = guarded_sort(p, c, update_on_empty=1)
    t0, n0, _, _, _ = guarded_sort(p, c)
    assert not c[list(TR.CROWD_EMPTY)].any() and not np.array_equal(t1[..., 4], t0[..., 4])        # seeing the empty frames changes ids


def test_guard_wide_crowd():
    seed, persons, frames = TR.WIDE_CROWD
    p, c = TR.draw_crowd(seed, frames=frames, persons=persons)
    for kw in TR.WIDE_PARAMS:
        t, cnt, s, ious, live = guarded_sort(p, c, **kw)
        assert max(m.shape[0] for m in ious) >= 56 and max(m.shape[1] for m in ious) >= 56 and not s.any()
        if kw["max_age"] == 3:
            assert max(len(ids) for _, ids in live) == 64                             # every slot holds a tracker, none is refused
        else:
            assert t[..., 4].max() >= 90 and TR.replay_slots(live, {f: t[f, :cnt[f], 4].astype(int).tolist() for f in range(frames)})[1] >= 10


def test_guard_full_house_and_clamps():
    p, c = TR.full_house()
    t, cnt, s, ious, live = guarded_sort(p, c, min_hits=0)
    assert [m.shape for m in ious] == [(64, 64)] * 3 and not ious[0].any() and not ious[1].any()   # 64 detections, none overlaps a tracker
    assert int((ious[2] >= 0.3).sum()) == 64                                          # frame 4: the new 64, each met again
    # the list is full while the first 64 coast (two frames at max_age = 1: sort.py founds before it buries), then 64 new ids
    assert s.tolist() == [0, 1, 1, 0, 0] and cnt.tolist() == [64, 0, 0, 64, 64]
    assert t[0, :, 4].tolist() == list(range(64, 0, -1)) and t[3, :, 4].tolist() == list(range(128, 64, -1)) == t[4, :, 4].tolist()
    t, cnt, s, ious, live = guarded_sort(p, c, min_hits=0, max_tracks=63)
    assert s.tolist() == [1] * 5 and cnt.tolist() == [63, 0, 0, 63, 63] and t[3, :, 4].tolist() == list(range(126, 63, -1))
    assert all(m.shape == (64, 63) for m in ious)
    p, c = TR.shrink_scene()
    t, cnt, s, ious, _ = guarded_sort(p, c, **TR.SHRINK_KW)
    for dt in (np.float64, np.longdouble):                                            # which path: the area's velocity is set to zero, once,
        trk, fired = TR.Sort(dtype=dt, **TR.SHRINK_KW), []                            # while the tracker coasts; no box is ever NaN
        for f in range(len(c)):
            fired += [(f, k.id, k.time_since_update) for k in trk.trackers if k.x[6] + k.x[2] <= 0]
            before = len(trk.trackers)
            trk.update(p[f, :c[f]])
            assert len(trk.trackers) >= before - 1 and all(np.isfinite(k.box().astype(np.float64)).all() for k in trk.trackers)
        assert fired == [(4, 1, 1)]
    assert [t[f, :cnt[f], 4].tolist() for f in (2, 4, 5)] == [[2.0, 1.0], [1.0], [2.0, 1.0]]       # ... and the tracker it saved is met again


def test_guard_nms_limits():
    rows = TR.draw_full_rows()
    assert TR.nms_margin(rows) > MARGIN and int((rows[..., 4] >= 0.5).sum()) == 2048 == rows.shape[1]
    tr = {}
    TR.nms_image(rows[0], dtype=torch.float64, trace=tr)
    last = [h for h in tr["heads"] if h >= 1984]
    assert len(tr["heads"]) == 9 and len(last) == 1 and last[0] % 64 > 0             # a head in chunk 31, not on its first lane ...
    d, c, s, src = TR.nms(rows, max_candidates=2048, dtype=torch.float64)
    d32 = TR.nms(rows, max_candidates=2048)[0]
    merged = torch.tensor([330.0 - 30, 330.0 - 40, 330.0 + 30, 330.0 + 40], dtype=torch.float64)
    assert c.tolist() == [9] and s.tolist() == [0] and torch.equal(d[0, 8, :4], merged)            # ... that merged rows of that chunk
    assert int((rows[0, :, 0] == 330.0).sum()) >= 2 and float((d32.double() - d)[..., :4].abs().max()) > 0
    more = torch.cat([rows, rows[:, :1]], 1)
    assert TR.nms(more, max_candidates=2048)[2].tolist() == [1] and more.shape[1] == 2049
    caps = TR.draw_caps_rows(TR.CAPS_SEED)[:1]
    assert int((caps[..., 4] >= 0.5).sum()) == 20
    assert TR.nms(caps, max_candidates=20)[2].tolist() == [0] and TR.nms(caps, max_candidates=19)[2].tolist() == [1]
    rows = TR.draw_keep_rows()
    d, c, s, src = TR.nms(rows, dtype=torch.float64)
    d32, c32, _, _ = TR.nms(rows)
    assert TR.nms_margin(rows) > MARGIN and c.tolist() == [64] and s.tolist() == [0] and int((rows[..., 4] >= 0.5).sum()) > 100
    assert float((d32.double() - d)[..., :4].abs().max()) > 0
    ppl, pc = TR.people(d32, c32, (0, 420, 1920 / 416))
    assert 8 <= int(pc[0]) < 64 and ppl[0, pc[0] - 1, 4] == float(d32[0, 63, 4]) and d32[0, 63, 6] == 0     # the 64th kept row is a person
    rows = TR.draw_keep_rows(extra=True)
    d, c, s, src = TR.nms(rows, dtype=torch.float64)
    assert TR.nms_margin(rows) > MARGIN and c.tolist() == [0] and s.tolist() == [2] and not d.any()
    assert TR.nms(rows, max_keep=65, dtype=torch.float64)[1].tolist() == [65]
    rows = TR.draw_seam_rows()
    d, c, s, src = TR.nms(rows, dtype=torch.float64)
    cand = (rows[0, :, 4] >= 0.5)
    assert rows.shape[1] == 1025 and all(bool(cand[r]) for r in TR.SEAM_ROWS) and int(cand.sum()) >= 100
    assert TR.nms_margin(rows) > MARGIN and not s.any() and 0 < int(c[0]) < int(cand.sum())
    assert float((TR.nms(rows)[0].double() - d)[..., :4].abs().max()) > 0
    assert set(TR.SEAM_ROWS) & set(src[0].tolist())                                   # a seam row is itself a kept head


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_reject_bad_arguments_before_any_launch(lib):
    from pmce_amd import _lib
    ok = dict(rows=16, n=1, R=10, nc=2, ct=0.5, nt=0.4, mc=1024, mk=64, dets=16, count=16, status=16, src=None, ppl=None, pc=None, cid=0,
              st=0.7, sp=0, px=0.0, py=0.0, ra=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pmce_yolo_nms_f32(a["rows"], a["n"], a["R"], a["nc"], a["ct"], a["nt"], a["mc"], a["mk"], a["dets"], a["count"], a["status"],
                                     a["src"], a["ppl"], a["pc"], a["cid"], a["st"], a["sp"], a["px"], a["py"], a["ra"], None)

    for kw, word in ((dict(rows=None), "null"), (dict(count=None), "null"), (dict(nc=0), "nc"), (dict(nc=256), "nc"), (dict(R=0), "R"),
                     (dict(mc=2049), "max_candidates"), (dict(mc=0), "max_candidates"), (dict(mk=65), "max_keep"),
                     (dict(ct=float("nan")), "finite"), (dict(nt=float("inf")), "finite"), (dict(ppl=16), "go together"),
                     (dict(ppl=16, pc=16, ra=0.0), "ratio"), (dict(ppl=16, pc=16, cid=2), "class_id"),
                     (dict(ppl=16, pc=16, st=float("nan")), "finite")):
        assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(n=0) == 0

    def sort(people=16, pc=16, sh=None, sd=None, F=4, K=8, S=1, age=1, hits=3, thr=0.3, T=64, uoe=0, tr=16, tc=16, st=16):
        return lib.pmce_sort_track_f64(people, pc, sh, sd, F, K, S, age, hits, thr, T, uoe, tr, tc, st, None)

    seq = (C.c_int * 3)(0, 3, 2)
    for kw, word in ((dict(people=None), "null"), (dict(st=None), "null"), (dict(K=65), "K"), (dict(K=0), "K"), (dict(T=65), "max_tracks"),
                     (dict(T=0), "max_tracks"), (dict(thr=float("nan")), "finite"), (dict(S=2), "one sequence"), (dict(sh=seq, S=2), "host and"),
                     (dict(sh=seq, sd=16, S=2), "end at F"), (dict(age=-1), "max_age")):
        assert sort(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert sort(F=0) == 0
    assert lib.pmce_tracklet_boxes_f64(None, None, 4, 2, None, None) == -1 and "null" in _lib.last_error()
    assert lib.pmce_tracklet_boxes_f64(None, None, 0, 0, None, None) == 0


def test_symbols_source_flags_and_header(lib):
    from pmce_amd import _lib, build as B
    for name in ("pmce_yolo_nms_f32", "pmce_sort_track_f64", "pmce_tracklet_boxes_f64"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "tracker.hip" in B.SOURCES and B.FILE_FLAGS["tracker.hip"] == B.NO_PACKED_FP32
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    for text in ("inter / (a + b - inter + 1e-16)", "ties by the lower row", "the head leaves ALWAYS", "x * ratio - pad_x",
                 "R = diag(1, 1, 10, 10)", "P = (I - K H) P (I - K H)' + K R K'", "inter / (a + b - inter) (no +1)", "s = w if w / h > 1 else h",
                 "no value was recorded"):
        assert text in hdr, text
    assert re.search(r"max_candidates in 1\.\.2048, max_keep in 1\.\.64", hdr)


def test_python_argument_checks():
    from pmce_amd import tracker as T
    with pytest.raises(ValueError, match="rows must be"):
        T.nms(torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match="max_keep"):
        T.nms(torch.zeros(2, 3, 7), max_keep=65)
    with pytest.raises(ValueError, match="score must be"):
        T.nms(torch.zeros(2, 3, 7), score="both")
    with pytest.raises(ValueError, match="people must be"):
        T.sort_tracks(torch.zeros(2, 3, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="seq_offsets"):
        T.check_seq_offsets([0, 3, 2, 4], 4)
    with pytest.raises(ValueError, match="callable"):
        T.Tracker(None)
    ids = np.array([[2, 1, 0], [2, 1, 0], [1, 0, 0], [3, 1, 0]])
    rows, frames, pids = T.record_index(ids, np.array([2, 2, 1, 2]), 1, [0, 4])[0]
    assert pids == [2, 1, 3] and rows[1] == [1, 4, 6, 10] and frames[2].tolist() == [3]
