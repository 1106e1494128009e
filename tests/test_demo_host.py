"""Host side of pmce_amd.demo (no GPU): tests/demo_ref.py's float32 restatement of the demo's window preparation against
tests/golden/demo.npz (the reference's own get_bbox / process_bbox / j2d_processing behind its FeatureDataset and a DataLoader,
tests/golden/make_golden_demo.py), the two host helpers against the reference's results, the window tables, the argument errors
and the library's new entry points."""
import os.path as osp

import numpy as np
import pytest
import torch

import demo_ref as DR

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("demo.npz")


def test_restatement_agrees_with_the_fixture(fx):
    """The box is float32 in the reference too: the restatement reproduces it exactly.  The crop coordinates come out of a float64 affine
    map there and are rounded to float32 once: one ulp of a 500-px coordinate (3.05e-5) is all a float32 evaluation may differ by, and one
    ulp of a normalised coordinate below 1 (1.19e-7) after the screen normalisation."""
    assert int(fx["seed"]) == DR.SEED
    for i, (n, wh) in enumerate(DR.TRACKLETS):
        kp, wh2 = DR.tracklet(i)
        assert wh2 == wh and kp.shape == (n, 17, 3)
        b, t, x, v = DR.prepare(kp, wh)
        assert v.all()
        assert np.array_equal(b, fx[f"bbox{i}"])
        dt = float(np.abs(t.astype(np.float64) - fx[f"target{i}"]).max())
        dx = float(np.abs(x.astype(np.float64) - fx[f"input{i}"]).max())
        assert dt <= float(fx["yard_target"]) <= 2.0 ** -15, dt
        assert dx <= float(fx["yard_input"]) <= 2.0 ** -23, dx
        # the finding itself: the middle row of every window is the screen normalisation of the target, not of the frame
        mid = fx[f"input{i}"][:, DR.MID]
        assert float(np.abs(DR.normalize(fx[f"target{i}"], *wh) - mid).max()) <= 2.0 ** -23
        clean = DR.prepare(kp, wh, reference_mode=False)[2]
        assert float(np.abs(clean[:, DR.MID] - mid).max()) > 0.1
        rest = [k for k in range(DR.SEQLEN) if k != DR.MID]
        assert float(np.abs(clean[:, rest] - fx[f"input{i}"][:, rest]).max()) <= 2.0 ** -23
    assert float(fx["yard_bbox"]) == 0.0
    b, t, x, v = DR.prepare(DR.degenerate_frames(), (1280, 720))
    assert not v.any() and np.isnan(b).all() and np.isnan(t).all() and np.isnan(x[:, DR.MID]).all()


def test_tracklet_span(fx):
    from pmce_amd import demo
    cases = DR.span_cases()
    for name, want in zip(fx["span_names"], fx["spans"]):
        assert demo.tracklet_span(cases[str(name)], vis_thresh=0.3) == (int(want[0]), int(want[1])), name
    assert demo.tracklet_span(cases["leading"]) == demo.tracklet_span(cases["leading"], 0.3)           # the demo's threshold is the default
    assert demo.tracklet_span([None, None]) == (-1, 0)
    with pytest.raises(ValueError):
        demo.tracklet_span([])


def test_frame_results(fx):
    from pmce_amd import demo
    res, num_frames = DR.render_case()
    frames = demo.frame_results(res, None, num_frames)
    assert len(frames) == num_frames
    assert np.array_equal(DR.render_table(frames), fx["render"])
    # frame ids passed separately (what run_tracklet's caller holds) give the same
    ids = {pid: d["frame_ids"] for pid, d in res.items()}
    bare = {pid: {k: v for k, v in d.items() if k != "frame_ids"} for pid, d in res.items()}
    assert np.array_equal(DR.render_table(demo.frame_results(bare, ids, num_frames)), fx["render"])
    assert any(len(f) >= 2 for f in frames) and any(len(f) == 0 for f in frames)
    with pytest.raises(ValueError):
        demo.frame_results(bare, {pid: v[:-1] for pid, v in ids.items()}, num_frames)


@pytest.mark.parametrize("n", [16, 17, 40])
def test_window_and_mid_tables(n):
    """One window per frame, and frame k is the middle of window k - what lets a per-frame 'as middle frame' table serve the override."""
    from pmce_amd import streaming
    wl = streaming.demo_window_list(n)
    assert np.array_equal(wl, DR.window_list(n))
    assert np.array_equal(DR.mid_index(wl), np.arange(n))
    assert np.array_equal(streaming.validate_windows(wl, n), wl)
    single = wl[:, 0] == wl[:, 1]
    assert single[:8].all() and single[n - 7:].all() and not single[8:n - 7].any() and single.sum() == 15
    assert np.array_equal(wl[~single, 1] - wl[~single, 0], np.full(n - 15, 15))


def test_device_window_expression_matches_the_host_list():
    """demo_windows_device builds the table with tensor arithmetic (on the GPU in use); the same expression on the CPU equals the host
    lists of two tracklets, offset."""
    from pmce_amd import demo, streaming
    got = demo.demo_windows_device([16, 23, 40], "cpu").numpy()
    want = np.concatenate([streaming.demo_window_list(16), streaming.demo_window_list(23) + 16, streaming.demo_window_list(40) + 39])
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_argument_errors():
    from pmce_amd import _lib, assets, demo, models
    m = models.PMCE.get_model(19, 256, 3)
    kp, wh = DR.tracklet(1)
    feat = DR.features(1)
    with pytest.raises(_lib.PmceError, match="set_j_regressor"):
        demo.run_tracklet(m, kp, feat, wh)
    m.set_j_regressor(assets.load_j_regressor("coco"))
    with pytest.raises(ValueError, match="at least 16 frames"):
        demo.run_tracklet(m, kp[:15], feat[:15], wh)
    with pytest.raises(ValueError, match="middle_frame"):
        demo.run_tracklet(m, kp, feat, wh, middle_frame="demo")
    with pytest.raises(ValueError, match=r"features must be \[N = 23, 2048\]"):
        demo.run_tracklet(m, kp, feat[:-1], wh)
    with pytest.raises(ValueError, match="tracklet 1: keypoints"):
        demo.run_tracklets(m, [(kp, feat), (kp[:, :16], feat)], wh)
    with pytest.raises(ValueError, match="img_wh"):
        demo.run_tracklet(m, kp, feat, (0, 1080))
    with pytest.raises(ValueError, match="batch"):
        demo.run_tracklet(m, kp, feat, wh, batch=0)
    assert demo.run_tracklets(m, [], wh) == []


def test_new_symbols_are_exported_and_prototyped():
    import ctypes
    from pmce_amd import _lib, build
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in ("pmce_demo_targets_f32", "pmce_demo_override_mid_f32", "pmce_stream_forward_mid", "pmce_window_mid_tokens_f32"):
        assert name in _lib.PROTOTYPES, name
        assert f"int {name}(" in hdr, name
        assert hasattr(lib, name), name
        n_args = hdr[hdr.index(f"int {name}("):].split(";")[0].count(",") + 1
        assert len(_lib.PROTOTYPES[name]) == n_args, name
    assert "demo_prep.hip" in build.SOURCES and build.FILE_FLAGS["demo_prep.hip"] == build.NO_PACKED_FP32
    assert ctypes.CDLL(build.LIB).pmce_version() == 100
