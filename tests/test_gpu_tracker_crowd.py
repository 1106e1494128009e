"""GPU tests of the tracker's back half (csrc/tracker.hip) at the sizes it is built for: assignments up to 64 x 64 whose augmenting
paths run through every column, crowds whose slots are reused out of id order, a full house of 64 trackers, and the suppression at
2048 candidates, exactly at its caps and at the seams of its tiles.  Inputs are drawn in tests/tracker_ref.py and guarded in
tests/test_tracker_host.py (unique assignments, NMS margin > 1e-4, the structure each case is there for); the rules are those of
tests/test_gpu_tracker.py: discrete results exact, floats within 4 x the restatement's own two-precision deviation (printed, run -s)."""
import numpy as np
import pytest
import torch

import tracker_ref as TR
from test_gpu_tracker import DEV, FACTOR, T, bits, check_nms, check_sort, dev_sort

pytestmark = pytest.mark.gpu
GEO = (0, 420, 1920 / 416)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int64 if x.dtype == np.float64 else x.dtype), y.view(np.int64 if y.dtype == np.float64 else y.dtype))
               for x, y in zip(a, b))


def ids_of(t, n, f):
    return t[f, :n[f], 4].tolist()


# ----------------------------------------------------------------------------------------------
# the assignment: chains
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,reverse,shuffle", TR.CHAIN_CASES,
                         ids=lambda v: {None: "inorder", True: "rev", False: "fwd", TR.CHAIN_SHUFFLE: "shuffled"}.get(v, str(v)))
def test_sort_chain_reroutes_every_row(n, reverse, shuffle):
    """Every row but one prefers its neighbour's tracker; the optimum keeps all n on their own (an augmenting path of n columns in
    order, potentials over n - 1 used columns).  A wrong match shows as an id, as status 1 at n = 64, or as a box 30 px off."""
    p, c = TR.chain_scene(n, reverse, shuffle)
    t, cnt, s = check_sort(p, c, ("chain", n, reverse, shuffle))
    assert not s.any() and cnt.tolist() == [n] * 5 and all(ids_of(t, cnt, f) == list(range(n, 0, -1)) for f in range(5))


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("shuffle", [None, TR.CHAIN_SHUFFLE], ids=["inorder", "shuffled"])
def test_sort_chain_more_and_fewer_detections_than_trackers(reverse, shuffle):
    n = 33
    p, c = TR.chain_scene(n, reverse, shuffle, extra=True)                            # 34 x 33: the extra box loses and founds id 34
    t, cnt, s = check_sort(p, c, ("chain-extra", reverse, shuffle))
    assert ids_of(t, cnt, 1) == list(range(n + 1, 0, -1)) and not s.any()
    p, c = TR.chain_scene(n, reverse, shuffle, drop=16)                               # 32 x 33: half the chain moves on by one tracker
    t, cnt, s = check_sort(p, c, ("chain-drop", reverse, shuffle))
    assert sorted(ids_of(t, cnt, 1)) == [i + 1 for i in range(n) if i != (n - 1 if reverse else 0)] and not s.any()


def test_sort_chain_over_slots_with_holes():
    """max_age = 0: five of 40 trackers die, the chains run over the 35 others with the free slots as columns between them, three
    births go into slots 7, 15, 23 - the report's rank and the pairing of free slots with unmatched detections."""
    p, c = TR.chain_holes()
    t, cnt, s = check_sort(p, c, "chain-holes", **TR.HOLES_KW)
    assert cnt.tolist() == [40, 35, 35, 38, 38] and not s.any()
    assert ids_of(t, cnt, 3) == [43, 42, 41] + [i + 1 for i in range(39, -1, -1) if i not in TR.HOLES_DEAD]


# ----------------------------------------------------------------------------------------------
# crowds
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", TR.CROWD_PARAMS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "defaults")
@pytest.mark.parametrize("seed", TR.CROWD_SEEDS)
def test_sort_crowd_against_the_restatement(seed, kw):
    p, c = TR.draw_crowd(seed)
    t, cnt, s = check_sort(p, c, ("crowd", seed, tuple(kw.items())), **kw)
    assert not s.any() and int(cnt.max()) >= 30
    if kw.get("max_age") == 0:
        assert t[..., 4].max() >= 70                                                  # slots were reused many times over


@pytest.mark.parametrize("kw", TR.WIDE_PARAMS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_sort_wide_crowd(kw):
    """64 persons: drawn assignments near 60 x 60, and with max_age = 3 all 64 slots in use without a refusal."""
    seed, persons, frames = TR.WIDE_CROWD
    p, c = TR.draw_crowd(seed, frames=frames, persons=persons)
    t, cnt, s = check_sort(p, c, ("wide", tuple(kw.items())), **kw)
    assert not s.any() and int(cnt.max()) >= 50


@pytest.mark.parametrize("min_frames", [1, 10])
def test_crowd_tracklet_records(min_frames):
    p, c = TR.draw_crowd(TR.CROWD_SEEDS[0])
    tracks, count, _ = T().sort_tracks(torch.from_numpy(p).to(DEV), torch.from_numpy(c).to(DEV), max_age=0, min_hits=0)
    recs, ids = T().tracklet_records(tracks, count, min_frames=min_frames)
    want, wids = TR.tracklet_records(tracks.cpu().numpy(), count.cpu().numpy(), min_frames=min_frames)
    assert ids == wids and len(recs) == len(want) and (len(ids) >= 70 if min_frames == 1 else 10 <= len(ids) < 70)
    for (b, f), (wb, wf) in zip(recs, want):
        assert np.array_equal(f, wf) and np.array_equal(b.cpu().numpy().view(np.int64), wb.view(np.int64))


def test_sort_crowds_and_empty_sequences_in_one_launch():
    """seq_offsets [0, 0, 24, 24, 40]: two workgroups without a frame between and before two crowds of different length."""
    (p0, c0), (p1, c1) = TR.draw_crowd(TR.CROWD_SEEDS[0]), TR.draw_crowd(TR.CROWD_SEEDS[1], frames=16)
    kw = dict(max_age=0, min_hits=0)
    both = dev_sort(np.concatenate([p0, p1]), np.concatenate([c0, c1]), seq_offsets=[0, 0, 24, 24, 40], **kw)
    a, b = dev_sort(p0, c0, **kw), dev_sort(p1, c1, **kw)
    assert same_bits([x[:24] for x in both], a) and same_bits([x[24:] for x in both], b)
    check_sort(p1, c1, "crowd-16")
    assert int(a[0][..., 4].max()) >= 70 and int(b[0][..., 4].max()) > 40


def test_sort_crowd_update_on_empty():
    p, c = TR.draw_crowd(TR.CROWD_SEEDS[0], empty=TR.CROWD_EMPTY)
    t1, n1, s1 = check_sort(p, c, "crowd-uoe", update_on_empty=1)
    t0, n0, s0 = check_sort(p, c, "crowd-empty")
    assert not n1[list(TR.CROWD_EMPTY)].any() and not n0[list(TR.CROWD_EMPTY)].any() and not np.array_equal(t1[..., 4], t0[..., 4])


# ----------------------------------------------------------------------------------------------
# full house and clamps
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_tracks", [64, 63])
def test_sort_full_house(max_tracks):
    """64 live trackers and 64 detections that overlap none: no slot is free (status 1, nothing founded, nothing reported) for the two
    frames the old ones coast at max_age = 1, then 64 new ids at once.  63: the other form of the slot mask, one short."""
    p, c = TR.full_house()
    t, cnt, s = check_sort(p, c, ("house", max_tracks), min_hits=0, max_tracks=max_tracks)
    m = max_tracks
    assert s.tolist() == ([0, 1, 1, 0, 0] if m == 64 else [1] * 5) and cnt.tolist() == [m, 0, 0, m, m]
    assert ids_of(t, cnt, 0) == list(range(m, 0, -1)) and ids_of(t, cnt, 3) == list(range(2 * m, m, -1)) == ids_of(t, cnt, 4)
    assert not t[1:3].any()


def test_sort_people_count_above_K_is_clamped():
    p, c = TR.chain_scene(8, False, TR.CHAIN_SHUFFLE, K=8)
    want = check_sort(p, c, "chain-K8")
    over = c.copy()
    over[:] = 70
    assert same_bits(dev_sort(p, over), want)


def test_sort_area_velocity_is_zeroed_while_coasting():
    """A box that shrinks fast and disappears: at its second coasting step x[6] + x[2] <= 0 and the area's velocity is set to zero
    (the host guard shows that this is the path taken, not the NaN box); the tracker so kept is met again at frame 5 as id 2."""
    p, c = TR.shrink_scene()
    t, cnt, s = check_sort(p, c, "shrink", **TR.SHRINK_KW)
    assert [ids_of(t, cnt, f) for f in (2, 4, 5, 8)] == [[2.0, 1.0], [1.0], [2.0, 1.0], [2.0, 1.0]]


# ----------------------------------------------------------------------------------------------
# the suppression at its limits
# ----------------------------------------------------------------------------------------------

def corners_ratio(what, dets, d32, d64):
    dev32 = float((d32[..., :4].double() - d64[..., :4]).abs().max())
    err = float((dets[..., :4].double() - d64[..., :4]).abs().max())
    print(f"nms corners, {what}: {err / dev32 if dev32 else float('inf'):.2f} x dev32 ({dev32:.2e})")
    assert dev32 > 0 and err <= FACTOR * dev32


def assert_served_empty(res, status):
    dets, count, st, src = (t.cpu() for t in res[:3] + res[-1:])
    assert count.tolist() == [0] and st.tolist() == [status] and not dets.any() and bool((src == -1).all())


def test_nms_2048_candidates_and_one_more():
    """The documented maximum: 32 chunks of 64, the last one bit 31 of the word of live candidates, P2 == cap == 2048; a head in the
    last chunk merges rows of that chunk.  One more candidate: status 1, served empty."""
    rows = TR.draw_full_rows()
    dets, d32, d64 = check_nms(rows, "full", max_candidates=2048)
    corners_ratio("2048 candidates", dets, d32, d64)
    assert int((dets[0, :, 4] > 0).sum()) == 9
    more = torch.cat([rows, rows[:, :1]], 1).to(DEV)
    assert_served_empty(T().nms(more, max_candidates=2048, return_rows=True), 1)
    dets, count, status, ppl, cnt = T().nms(more, max_candidates=2048, geometry=GEO)
    assert not ppl.any() and cnt.tolist() == [0] and status.tolist() == [1]


def test_nms_exactly_max_candidates():
    rows = TR.draw_caps_rows(TR.CAPS_SEED)[:1]                                        # 20 candidates
    free, _, _ = check_nms(rows, "caps-free")
    at, d32, d64 = check_nms(rows, "caps-20", max_candidates=20)
    assert torch.equal(bits(at), bits(free)) and int((at[0, :, 4] > 0).sum()) > 0
    corners_ratio("exactly max_candidates", at, d32, d64)
    check_nms(rows, "caps-19", max_candidates=19)
    assert_served_empty(T().nms(rows.to(DEV), max_candidates=19, return_rows=True), 1)


def test_nms_exactly_64_kept_and_one_more():
    """64 kept rows: the last row of the kernel's kept table and lane 63 of the people stage, itself a person; 65: status 2, empty."""
    rows = TR.draw_keep_rows()
    dets, d32, d64 = check_nms(rows, "keep-64")
    corners_ratio("64 kept", dets, d32, d64)
    dets, count, status, ppl, cnt = (t.cpu() for t in T().nms(rows.to(DEV), geometry=GEO, class_id=0))
    want, wcnt = TR.people(dets, count, GEO)
    assert count.tolist() == [64] and status.tolist() == [0] and cnt.tolist() == wcnt.tolist() and np.array_equal(ppl.numpy(), want)
    assert 8 <= int(cnt[0]) < 64 and float(ppl[0, int(cnt[0]) - 1, 4]) == float(dets[0, 63, 4])
    more = TR.draw_keep_rows(extra=True)
    check_nms(more, "keep-65")
    res = T().nms(more.to(DEV), geometry=GEO, class_id=0, return_rows=True)
    assert_served_empty(res, 2)
    assert not res[3].any() and res[4].tolist() == [0]


def test_nms_candidates_at_the_tile_seams():
    """1025 rows: candidates at rows 0, 63, 64, 1023 and in the one-row second tile of the compaction, 1024."""
    rows = TR.draw_seam_rows()
    dets, d32, d64 = check_nms(rows, "seams")
    corners_ratio("tile seams", dets, d32, d64)
