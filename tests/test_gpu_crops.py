"""The demo's person crops on the GPU (csrc/crops.hip) against the numpy oracle tests/crops_ref.py and the reference's recorded boxes
(tests/golden/crops.npz).  Every pixel comparison is exact: patch_u8 bytes, patch_f32 bit patterns, status."""
import os.path as osp

import numpy as np
import pytest
import torch

import crops_ref as CR

pytestmark = pytest.mark.gpu

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
H, W = 37, 53
SCALE = 1.1
# (cx, cy, w, h) at scale 1.1 on the 53 x 37 frames
CASES = {
    "inside": (26.0, 18.0, 20.0, 20.0),
    "off_left": (2.0, 18.0, 20.0, 20.0),
    "off_right": (51.0, 18.0, 20.0, 20.0),
    "off_top": (26.0, 1.0, 20.0, 20.0),
    "off_bottom": (26.0, 36.0, 20.0, 20.0),
    "off_corner": (50.0, 35.0, 24.0, 24.0),
    "outside": (300.0, 200.0, 20.0, 20.0),
    "edge_taps": (26.125, 18.0, 2 * 26.625 / 1.1, 30.0),          # tap columns run from -1 to W - 1 (asserted below)
    "upscale": (26.3, 18.7, 9.0 / 1.1, 9.0 / 1.1),                # a 9 px box: all 32 fractions occur (asserted below)
    "downscale": (26.0, 18.0, 400.0, 400.0),                      # the box is larger than the frame
    "w_ne_h": (26.0, 18.0, 30.0, 12.0),
    "negative_centre": (-5.0, -3.0, 40.0, 40.0),
}
TIE_BOX, TIE_SCALE = (26.5, 18.5, 0.65625, 10.0), 0.5


def dev():
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def same(got, want):
    """(patch_f32, patch_u8, status) from the device == the oracle's, bit for bit."""
    for g, w, what in zip(got, want, ("patch_f32", "patch_u8", "status")):
        g = bits(g)
        assert g.shape == bits(w).shape and g.dtype == bits(w).dtype, what
        assert np.array_equal(g, bits(w)), f"{what}: {int((g != bits(w)).sum())} of {g.size} differ"


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(11).integers(0, 256, (3, H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def jobs():
    """65 jobs: the named cases, then jittered copies of them; frames 2 and 0 out of order, frame 1 never used."""
    rng = np.random.default_rng(12)
    base = np.array(list(CASES.values()), dtype=np.float64)
    more = base[rng.integers(0, len(base), 65 - len(base))] + rng.uniform(-3, 3, (65 - len(base), 4)) * np.array([1, 1, 0.2, 0.2])
    boxes = np.concatenate([base, more])
    fi = np.where(rng.random(65) < 0.5, 2, 0).astype(np.int32)
    fi[:4] = (2, 0, 2, 2)
    assert set(fi) == {0, 2} and (boxes[:, 2:] > 0).all()
    return fi, boxes


@pytest.fixture(scope="module")
def want224(frames, jobs):
    """The oracle's patches of the 65 jobs at S = 224, computed once."""
    return CR.crop_patches(frames, jobs[0], jobs[1], SCALE, 224)


def run(frames, fi, boxes, **kw):
    from pmce_amd import crops
    out = crops.crop_patches(torch.from_numpy(frames).to(dev()), fi, boxes, return_raw=True, **kw)
    torch.cuda.synchronize()
    return out


def test_cases_are_what_they_claim(frames):
    """In the oracle's arithmetic: the edge case taps columns -1 .. W - 1, the upscale case meets all 32 fractions on both axes, the tie
    case has 112 columns whose i_x * x * 1024 lies exactly on .5."""
    X, _, _ = CR.fixed_point_axes(CASES["edge_taps"], SCALE, 224)
    assert (X >> 5).min() == -1 and (X >> 5).max() == W - 1
    X, Y, _ = CR.fixed_point_axes(CASES["upscale"], SCALE, 224)
    assert set(X & 31) == set(range(32)) == set(Y & 31)
    ix, _ = CR.axis_map(TIE_BOX[0], TIE_BOX[2], TIE_SCALE, 224)
    assert ix == 3.0 / 2048.0
    _, _, prod = CR.fixed_point_axes(TIE_BOX, TIE_SCALE, 224)
    assert int((prod - np.floor(prod) == 0.5).sum()) == 112
    for name, box in CASES.items():
        assert CR.job_status(box, SCALE, 224) == 0, name
    assert not CR.crop_patches(frames, [0], [CASES["outside"]], SCALE, 224)[1].any()


def test_patches_exact_and_independent_of_n(frames, jobs, want224):
    fi, boxes = jobs
    got = run(frames, fi, boxes)
    same(got, want224)
    assert not np.asarray(want224[2]).any()
    again = run(frames, fi, boxes)                                 # run twice: identical bits
    same(again, [g.cpu().numpy() for g in got])
    for n in (1, 2):
        same(run(frames, fi[:n], boxes[:n]), [w[:n] for w in want224])
    # without the raw patch; boxes and the job table as device tensors (a device table is not validated, and not waited for)
    from pmce_amd import crops
    p, st = crops.crop_patches(torch.from_numpy(frames).to(dev()), torch.from_numpy(fi).to(dev()), torch.from_numpy(boxes).to(dev()))
    assert np.array_equal(bits(p), bits(want224[0])) and not st.any()


@pytest.mark.parametrize("S", [1, 7, 33])
def test_small_sides_store_tails(frames, jobs, S):
    fi, boxes = jobs[0][:len(CASES)], jobs[1][:len(CASES)]
    same(run(frames, fi, boxes, size=S), CR.crop_patches(frames, fi, boxes, SCALE, S))


def test_rounding_ties(frames):
    """i_x = 3/2048: every second column's i_x * x * 1024 is k + .5 and must round to even."""
    _, _, prod = CR.fixed_point_axes(TIE_BOX, TIE_SCALE, 224)
    ties = prod - np.floor(prod) == 0.5
    assert ties.sum() == 112 and (np.rint(prod[ties]) % 2 == 0).all()
    assert len(set(np.rint(prod[ties]) - prod[ties])) == 2         # both directions occur: rounding half up would differ
    fi, boxes = np.array([1, 0], dtype=np.int32), np.array([TIE_BOX, TIE_BOX])
    same(run(frames, fi, boxes, scale=TIE_SCALE), CR.crop_patches(frames, fi, boxes, TIE_SCALE, 224))


def test_channel_order(frames, jobs, want224):
    fi, boxes = jobs[0][:4], jobs[1][:4]
    got = run(np.ascontiguousarray(frames[..., ::-1]), fi, boxes, channel_order="bgr")
    same(got, [w[:4] for w in want224])


def test_status_and_border_patch(frames, jobs, want224):
    from pmce_amd import crops
    good = jobs[1][0]
    nan, inf = float("nan"), float("inf")
    bad = {1: [(nan, 18, 20, 20), (26, 18, inf, 20), (26, -inf, 20, 20), (26, 18, 0, 20), (26, 18, 20, -4), (26, 18, 20, nan)],
           2: [(26, 18, 1e9, 1e9), (26, 18, 20, 1e9), (3e6, 18, 20, 20), (26, 18, 1e300, 20)]}
    boxes, want_st = [good], [0]
    for st, rows in bad.items():
        for r in rows:
            boxes += [r, good]
            want_st += [st, 0]
    boxes = np.array(boxes, dtype=np.float64)
    fi = np.full(len(boxes), int(jobs[0][0]), dtype=np.int32)
    want = CR.crop_patches(frames, fi, boxes, SCALE, 224)
    assert list(want[2]) == want_st
    got = run(frames, fi, boxes)
    same(got, want)
    border = CR.normalise(np.zeros((224, 224, 3), np.uint8))
    for j, st in enumerate(want_st):
        if st:
            assert not got[1][j].any() and np.array_equal(bits(got[0][j]), bits(border))
        else:                                                      # the neighbours of a bad job are untouched
            assert np.array_equal(bits(got[0][j]), bits(want224[0][0]))
    # a device job table is trusted: an index outside the frames is reported, and nothing is read for it
    fi_dev = torch.tensor([int(jobs[0][0]), 3, -1, int(jobs[0][0])], dtype=torch.int32, device=dev())
    p, raw, st = crops.crop_patches(torch.from_numpy(frames).to(dev()), fi_dev, np.tile(good, (4, 1)), return_raw=True)
    assert st.tolist() == [0, 3, 3, 0] and not raw[1:3].any()
    assert np.array_equal(bits(p[0]), bits(want224[0][0])) and np.array_equal(bits(p[3]), bits(want224[0][0]))
    with pytest.raises(ValueError):                                # the same table from the host is an error
        crops.crop_patches(torch.from_numpy(frames).to(dev()), fi_dev.cpu(), np.tile(good, (4, 1)))


def test_empty(frames):
    from pmce_amd import crops
    p, raw, st = crops.crop_patches(torch.from_numpy(frames).to(dev()), np.zeros(0, np.int32), np.zeros((0, 4)), return_raw=True)
    assert tuple(p.shape) == (0, 3, 224, 224) and p.dtype == torch.float32 and p.is_cuda
    assert tuple(raw.shape) == (0, 224, 224, 3) and raw.dtype == torch.uint8 and tuple(st.shape) == (0,) and st.dtype == torch.int32
    b, u, span = crops.tracklet_boxes(torch.zeros(0, 17, 3, device=dev()))
    assert tuple(b.shape) == (0, 4) and b.dtype == torch.float64 and tuple(u.shape) == (0,) and span.tolist() == [-1, 0]


def test_tracklet_boxes_against_the_reference():
    """Boxes are computed and returned in fp64: the bound is the host test's, 1e-12 relative to the reference's recorded boxes."""
    from pmce_amd import crops, demo
    gold = np.load(osp.join(REPO, "tests", "golden", "crops.npz"))
    for name, kp in CR.golden_tracklets().items():
        boxes, usable, span = crops.tracklet_boxes(torch.from_numpy(kp.astype(np.float32)).to(dev()))
        assert boxes.dtype == torch.float64 and usable.dtype == torch.int32 and span.dtype == torch.int32
        boxes, usable, span = boxes.cpu().numpy(), usable.cpu().numpy(), tuple(span.tolist())
        a, b = (int(v) for v in gold[f"span_{name}"])
        assert span == (a, b) == demo.tracklet_span(kp), name
        assert np.array_equal(usable, CR.tracklet_boxes(kp)[1]), name
        lo = max(a, 0)
        assert np.isnan(boxes[:lo]).all() and np.isnan(boxes[b:]).all()
        want = gold[f"boxes_{name}"]
        if len(want):
            rel = np.abs(boxes[lo:b] - want) / np.abs(want)
            print(f"{name}: device boxes vs reference, largest relative difference {rel.max():.3e}")
            assert rel.max() <= 1e-12, name
    # a single frame, and more keypoints than lanes
    kp = CR.golden_tracklets()["clean"]
    b1, u1, s1 = crops.tracklet_boxes(kp[:1].astype(np.float32))
    assert s1.tolist() == [0, 1] and u1.tolist() == [1] and np.array_equal(b1.cpu().numpy(), CR.tracklet_boxes(kp[:1])[0])
    wide = np.concatenate([kp] * 5, axis=1)                        # K = 85
    assert np.array_equal(crops.tracklet_boxes(wide.astype(np.float32))[0].cpu().numpy(), CR.tracklet_boxes(wide)[0])


def video(n_frames=24):
    """Frames and two tracklets of 20 and 24 frames whose keypoints lie in and around the 53 x 37 frame; the first has an unusable
    frame at either end (span (1, 19)), the second two at its start and two in the middle (span (2, 24))."""
    rng = np.random.default_rng(13)
    fr = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    out = []
    for n, first, dead in ((20, 2, (0, 19)), (24, 0, (0, 1, 9, 10))):
        xy = rng.uniform(0, 1, (1, 17, 2)) * np.array([14.0, 24.0]) + rng.uniform(4, 12, (n, 1, 2)) + rng.normal(0, 0.4, (n, 17, 2))
        sc = rng.uniform(0.4, 0.95, (n, 17))
        sc[list(dead)] = 0.05
        kp = np.concatenate([xy, sc[:, :, None]], -1).astype(np.float32)
        out.append((kp, np.arange(first, first + n)))
    return fr, out


def test_crop_tracklets():
    from pmce_amd import demo
    fr, tracks = video(n_frames=24)
    res = demo.crop_tracklets(torch.from_numpy(fr).to(dev()), tracks, return_raw=True)
    assert res["spans"] == [(1, 19), (2, 24)] and res["offsets"].tolist() == [0, 18, 40]
    fi, boxes = [], []
    for (kp, ids), (a, b), got_kp, got_ids, got_box in zip(tracks, res["spans"], res["keypoints"], res["frame_ids"], res["boxes"]):
        assert np.array_equal(got_ids, ids[a:b]) and np.array_equal(got_kp.cpu().numpy(), kp[a:b])
        bx = CR.tracklet_boxes(kp.astype(np.float64))[0][a:b]
        assert np.allclose(got_box.cpu().numpy(), bx, rtol=1e-12, atol=0)
        fi.append(ids[a:b])
        boxes.append(got_box.cpu().numpy())
    same((res["patches"], res["raw"], res["status"]), CR.crop_patches(fr, np.concatenate(fi), np.concatenate(boxes), SCALE, 224))
    assert not res["status"].any() and res["raw"].any()


def test_run_video_equals_run_tracklets_on_the_oracle_patches():
    """Frames -> results, bit-identical to ``run_tracklets`` fed the same extractor's features of the ORACLE's patches."""
    from pmce_amd import demo
    from test_gpu_demo import get_model
    model = get_model(256)
    fr, tracks = video(n_frames=24)
    g = torch.Generator().manual_seed(14)
    weight = (torch.randn(3 * 28 * 28, 2048, generator=g) * 0.02).to(dev())

    def extractor(p):
        return torch.nn.functional.avg_pool2d(p, 8).flatten(1) @ weight

    outs = demo.run_video(model, torch.from_numpy(fr).to(dev()), tracks, extractor, (W, H), seed=3)
    spans = [demo.tracklet_span(kp) for kp, _ in tracks]
    assert spans == [(1, 19), (2, 24)]
    kps = [kp[a:b] for (kp, _), (a, b) in zip(tracks, spans)]
    ids = [i[a:b] for (_, i), (a, b) in zip(tracks, spans)]
    boxes = np.concatenate([CR.tracklet_boxes(kp.astype(np.float64))[0][a:b] for (kp, _), (a, b) in zip(tracks, spans)])
    want_patches = CR.crop_patches(fr, np.concatenate(ids), boxes, SCALE, 224)[0]
    feats = extractor(torch.from_numpy(want_patches).to(dev()))
    want = demo.run_tracklets(model, [(kps[0], feats[:18]), (kps[1], feats[18:])], (W, H), seed=3)
    torch.cuda.synchronize()
    assert len(outs) == 2
    for o, w, fid in zip(outs, want, ids):
        assert np.array_equal(o["frame_ids"], fid)
        for key in w:
            assert torch.equal(o[key], w[key]), key
    short = [(tracks[0][0][:16], tracks[0][1][:16]), tracks[1]]     # 16 rows, 15 after trimming
    with pytest.raises(ValueError, match="at least 16 frames"):
        demo.run_video(model, torch.from_numpy(fr).to(dev()), short, extractor, (W, H))
