"""pmce_amd.demo on the GPU: the target-preparation kernel (csrc/demo_prep.hip) against tests/golden/demo.npz - the reference's own
get_bbox / process_bbox / j2d_processing behind its FeatureDataset and a DataLoader (tests/golden/make_golden_demo.py) -, the
middle-frame override in the uncached and the cached forward, the camera chain, several tracklets in shared batches.

Bounds.  The fixture stores how far a straightforward numpy-float32 restatement (tests/demo_ref.py) sits from the reference: 0 for the
box (float32 in the reference too), one ulp of a 500-px coordinate for the target, one ulp of a normalised coordinate for the model
input.  The kernel is held to 4 x each: it may contract or reorder a handful of float32 operations the restatement does not, two extra
roundings each way.  Model outputs against the oracle use tests/test_gpu_e2e.py's TIGHT_M / TOL_MM."""
import numpy as np
import pytest
import torch

import camfit_ref as CR
import demo_ref as DR
from conftest import cached_state_dict
from test_gpu_e2e import TIGHT_M, TOL_MM

pytestmark = pytest.mark.gpu

J = 19
_MODELS = {}
_ORACLE = {}


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def get_model(C):
    from pmce_amd import assets, models
    if C not in _MODELS:
        _MODELS.clear()
        torch.cuda.empty_cache()
        m = models.PMCE.get_model(J, C, 3)
        m.load_state_dict(cached_state_dict(J, C))
        m.set_j_regressor(assets.load_j_regressor("coco"))
        _MODELS[C] = m.to(dev())
    return _MODELS[C]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("demo.npz")


@pytest.fixture(scope="module")
def tr():
    """The two fixture tracklets on the device: [(kp, feat, (w, h)), ...]."""
    return [(T(DR.tracklet(i)[0]), T(DR.features(i)), DR.tracklet(i)[1]) for i in range(len(DR.TRACKLETS))]


INIT = np.array([[0.3, 0.1, 0.2]], dtype=np.float32)


def test_prep_kernel_vs_fixture(fx, tr):
    from pmce_amd import demo, staging, streaming
    yb, yt, yx = (4.0 * float(fx[k]) for k in ("yard_bbox", "yard_target", "yard_input"))
    for i, (kp, feat, wh) in enumerate(tr):
        n = kp.shape[0]
        wl = streaming.demo_window_list(n)
        wd = demo.demo_windows_device([n], dev())
        assert np.array_equal(wd.cpu().numpy(), wl)
        bbox, target, mid, valid = demo.demo_targets(kp, wd, wh)
        b2, t2, m2, v2 = demo.demo_targets(kp, wl, wh)                                   # a host table gives the same
        assert torch.equal(bbox, b2) and torch.equal(target, t2) and torch.equal(mid, m2) and torch.equal(valid, v2)
        assert bool((valid == 1).all()) and valid.dtype == torch.int32
        db, dt = maxabs(bbox, torch.from_numpy(fx[f"bbox{i}"])), maxabs(target, torch.from_numpy(fx[f"target{i}"]))
        dm = maxabs(mid, torch.from_numpy(fx[f"input{i}"][:, DR.MID]))
        print(f"tracklet {i}: bbox {db:.2e} (bound {yb:.2e}), target2d {dt:.2e} px ({yt:.2e}), mid_pose2d {dm:.2e} ({yx:.2e})")
        assert db <= yb and dt <= yt and dm <= yx
        shapes = torch.tensor([[wh[1], wh[0]]], dtype=torch.int32, device=dev()).repeat(n, 1)
        pose_fr = staging.prepare_pose2d(kp, shapes)
        plain, _ = streaming.assemble_windows(pose_fr, feat, wl)
        p, _ = streaming.assemble_windows(pose_fr, feat, wd)
        assert torch.equal(p, plain)
        assert demo.override_middle(p, mid) is p
        rest = [t for t in range(16) if t != DR.MID]
        assert torch.equal(p[:, rest], plain[:, rest])                                   # the other 15 rows: untouched
        assert torch.equal(p[:, DR.MID], mid)
        dx = maxabs(p[:, DR.MID], torch.from_numpy(fx[f"input{i}"][:, DR.MID]))
        dr = maxabs(p[:, rest], torch.from_numpy(fx[f"input{i}"][:, rest]))
        print(f"   assembled input: middle row {dx:.2e} ({yx:.2e}), other rows vs the reference {dr:.2e}")
        assert dx <= yx
    # a batch slice of the device table (what the uncached path hands over): 9 windows, no multiple of the 4 a block takes
    kp, _, wh = tr[0]
    part = demo.demo_targets(kp, demo.demo_windows_device([40], dev())[5:14], wh)
    full = demo.demo_targets(kp, streaming.demo_window_list(40), wh)
    for a, b in zip(part, full):
        assert torch.equal(a, b[5:14])


def test_degenerate_frame(tr):
    from pmce_amd import demo, streaming
    model = get_model(256)
    kp = DR.tracklet(0)[0][:20].copy()
    kp[11] = DR.degenerate_frames(1)[0]
    bbox, target, mid, valid = demo.demo_targets(T(kp), streaming.demo_window_list(20), (1920, 1080))
    v = valid.cpu().numpy()
    assert v[11] == 0 and v.sum() == 19
    assert bool(torch.isnan(bbox[11]).all()) and bool(torch.isnan(target[11]).all()) and bool(torch.isnan(mid[11]).all())
    keep = [k for k in range(20) if k != 11]
    assert bool(torch.isfinite(bbox[keep]).all()) and bool(torch.isfinite(target[keep]).all()) and bool(torch.isfinite(mid[keep]).all())
    feat = tr[0][1][:20]
    try:
        with pytest.raises(ValueError, match="tracklet 0, frame 11"):
            demo.run_tracklet(model, T(kp), feat, (1920, 1080))
        with pytest.raises(ValueError, match="tracklet 1, frame 11"):
            demo.run_tracklets(model, [(tr[1][0], tr[1][1]), (T(kp), feat)], (1920, 1080))
        out = demo.run_tracklet(model, T(kp), feat, (1920, 1080), check=False)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out["bboxes"][11]).all()) and bool(torch.isnan(out["target2d"][11]).all())
        assert bool(torch.isfinite(out["mesh"][:3]).all())                               # windows that do not hold frame 11
    finally:
        torch.cuda.synchronize()
        model.clear_overflow()


def test_reference_mode_uncached_is_the_composition_of_public_calls(tr):
    from pmce_amd import camera, demo, staging, streaming
    model = get_model(256)
    kp, feat, wh = tr[1]
    n = kp.shape[0]
    init = T(INIT)
    out = demo.run_tracklet(model, kp, feat, wh, reuse=False, batch=16, init=init)
    wl = streaming.demo_window_list(n)
    mid = demo.demo_targets(kp, wl, wh)
    shapes = torch.tensor([[wh[1], wh[0]]], dtype=torch.int32, device=dev()).repeat(n, 1)
    pose_fr = staging.prepare_pose2d(kp, shapes)
    ms, js = [], []
    for lo in range(0, n, 16):
        p, f = streaming.assemble_windows(pose_fr, feat, wl[lo:lo + 16])
        p[:, DR.MID] = mid[2][lo:lo + 16]                                                # torch row replacement
        o = model.forward_with_joints(p, f)
        ms.append(o[0]); js.append(o[3])
    mesh, joints = torch.cat(ms), torch.cat(js)
    cam, loss, orig = camera.fit_camera(joints, mid[1], init=init, chain=True, scale=1e-3, bbox=mid[0], img_wh=wh)
    torch.cuda.synchronize()
    for key, want in (("mesh", mesh), ("joints_mm", joints), ("pred_cam", cam), ("loss", loss), ("orig_cam", orig), ("bboxes", mid[0]),
                      ("target2d", mid[1])):
        assert torch.equal(out[key], want), key
    assert tuple(out["mesh"].shape) == (n, 6890, 3) and tuple(out["pred_cam"].shape) == (n, 3) and tuple(out["orig_cam"].shape) == (n, 4)
    assert tuple(out["joints_mm"].shape) == (n, 17, 3) and tuple(out["target2d"].shape) == (n, 19, 2)
    # and the override matters: the clean mode gives another mesh
    clean = demo.run_tracklet(model, kp, feat, wh, reuse=False, batch=16, init=init, middle_frame="clean")
    assert maxabs(clean["mesh"], out["mesh"]) > 1e-4


def test_clean_mode_is_the_existing_cached_path(tr):
    from pmce_amd import camera, demo, staging, streaming
    model = get_model(256)
    kp, feat, wh = tr[0]
    n = kp.shape[0]
    init = T(INIT)
    out = demo.run_tracklet(model, kp, feat, wh, middle_frame="clean", batch=16, init=init)
    wl = streaming.demo_window_list(n)
    bbox, target, _, _ = demo.demo_targets(kp, wl, wh)
    shapes = torch.tensor([[wh[1], wh[0]]], dtype=torch.int32, device=dev()).repeat(n, 1)
    cache = streaming.precompute_frames(model, staging.prepare_pose2d(kp, shapes), feat)
    outs = streaming.stream_forward_cached(model, cache, windows=wl, batch=16, with_joints=True)
    cam, loss, orig = camera.fit_camera_stream(outs, target, init=init, bbox=bbox, img_wh=wh)
    torch.cuda.synchronize()
    for key, want in (("mesh", outs[0]), ("joints_mm", outs[3]), ("pred_cam", cam), ("loss", loss), ("orig_cam", orig)):
        assert torch.equal(out[key], want), key


@pytest.mark.parametrize("mode", ["split_f16 at every batch size", "f32"])
def test_override_with_the_plain_table_changes_no_bit(tr, mode):
    """pmce_stream_forward_mid with x0_mid = x0 == pmce_stream_forward: the rewrite kernel repeats ln_chain_kernel's arithmetic (fp32 XN
    on the fp32 pipe, the pre-split f16 form in split mode)."""
    from pmce_amd import staging, streaming
    model = get_model(256)
    kp, feat, wh = tr[0]
    n = kp.shape[0]
    if mode == "f32":
        model.set_gemm_mode("f32")
    else:
        model.set_gemm_mode("split_f16", min_batch=1)
    try:
        shapes = torch.tensor([[wh[1], wh[0]]], dtype=torch.int32, device=dev()).repeat(n, 1)
        cache = streaming.precompute_frames(model, staging.prepare_pose2d(kp, shapes), feat)
        wl = streaming.demo_window_list(n)
        a = streaming.stream_forward_cached(model, cache, windows=wl, batch=13, with_joints=True)
        same = streaming.FrameCache(cache.x0, cache.gi0, cache.L, cache.x0.clone())
        b = streaming.stream_forward_cached(model, same, windows=wl, batch=13, with_joints=True)
        other = streaming.FrameCache(cache.x0, cache.gi0, cache.L, cache.x0 + 0.25)
        c = streaming.stream_forward_cached(model, other, windows=wl, batch=13, with_joints=True)
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode(None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0])                                                   # the table IS read


def test_camera(tr):
    from pmce_amd import camera, demo
    model = get_model(256)
    kp, feat, wh = tr[1]
    init = T(INIT)
    out = demo.run_tracklet(model, kp, feat, wh, init=init)
    cam, loss, orig = camera.fit_camera(out["joints_mm"], out["target2d"], init=init, chain=True, scale=1e-3, bbox=out["bboxes"], img_wh=wh)
    torch.cuda.synchronize()
    assert torch.equal(out["pred_cam"], cam) and torch.equal(out["loss"], loss) and torch.equal(out["orig_cam"], orig)
    assert out["pred_cam"].dtype == torch.float32
    d = demo.run_tracklet(model, kp, feat, wh, seed=4)                                   # the default init: seeded, on the device
    want = camera.fit_camera(d["joints_mm"], d["target2d"], init=camera.default_init(1, 4, dev()), chain=True, scale=1e-3)[0]
    assert torch.equal(d["pred_cam"], want)


def test_camera_fp64_follows_the_restatement(fx, tr):
    """The façade's joints and the fixture's targets through the fp64 fit, against tests/camfit_ref.py's fp64 restatement of the reference's loop
    at test_gpu_camfit.py::test_fp64_chain's bound, 1e-9.

    Every window on its own (all from one init) is held to that bound.  Along the CHAIN the bound can only be asked where the reference
    itself is that well determined: with the suite's synthetic weights the regressed joints (a cloud 1.7 x 3.2 m across) do not resemble the
    keypoints, the fit is ill-posed (loss 76 px, negative scale), and a window then amplifies a difference in its starting camera about tenfold -
    the restatement run a second time with its joints moved by ONE fp64 ulp leaves its own first result by 1.9e-14, 1.3e-13, 2.6e-12,
    1.5e-11, 3.0e-10, 2.7e-9, 3.2e-8, 7.8e-7 ... and is 0.19 away within 23 windows.  (tests/golden/camfit.npz's windows are projections of
    their own joints: there a chain of 40 stays at 3e-12.)  So the chain is compared over the leading windows on which that one-ulp sensitivity
    of the restatement - a property of the reference alone - stays below a tenth of the bound (the kernel's roundings differ from the restatement's
    in every step - unfused updates, another summation order -, not in one input ulp); at least three such windows must exist, so that
    carrying the camera from window to window is what is being compared.  Measured on MI355X: the kernel sits 3.3e-14, 2.2e-13, 4.5e-12,
    2.6e-11 from the restatement on those four windows (1.7 x the one-ulp sensitivity throughout, 5.2e-10 and 4.7e-9 on the next two), and
    0.21 away at window 14 - as far as the restatement is from itself."""
    from pmce_amd import camera, demo
    model = get_model(256)
    kp, feat, wh = tr[1]
    n = kp.shape[0]
    init = T(INIT)
    out = demo.run_tracklet(model, kp, feat, wh, init=init)
    o64 = demo.run_tracklet(model, kp, feat, wh, init=init, precision="f64")
    assert o64["pred_cam"].dtype == torch.float64 and o64["orig_cam"].dtype == torch.float64 and o64["loss"].dtype == torch.float64
    assert o64["mesh"].dtype == torch.float32 and torch.equal(o64["joints_mm"], out["joints_mm"]) and torch.equal(o64["mesh"], out["mesh"])
    tg = fx["target1"]
    j64 = out["joints_mm"].cpu().numpy().astype(np.float64) * 1e-3
    t64 = tg.astype(np.float64)
    i64 = INIT[0].astype(np.float64)
    # every window on its own
    sep, _ = camera.fit_camera(out["joints_mm"], T(tg), init=init.repeat(n, 1), scale=1e-3, precision="f64")
    ds = float(np.abs(sep.cpu().numpy() - CR.fit(j64, t64, np.repeat(i64[None], n, 0))).max())
    print(f"fp64, {n} independent windows on the fixture's targets vs the restatement: {ds:.2e}")
    assert ds <= 1e-9
    # the chain, as far as the reference determines it
    c64, _ = camera.fit_camera(out["joints_mm"], T(tg), init=init, chain=True, scale=1e-3, precision="f64")
    P = 8
    ref = CR.fit_chain(j64[:P], t64[:P], i64)
    sens = np.abs(CR.fit_chain(j64[:P] * (1.0 + 2.0 ** -52), t64[:P], i64) - ref).max(1)
    dev = np.abs(c64.cpu().numpy()[:P] - ref).max(1)
    K = int(np.argmax(sens > 1e-10)) if (sens > 1e-10).any() else P
    print(f"fp64 chain: restatement's one-ulp sensitivity per window {np.array2string(sens, precision=1)}; kernel vs restatement "
          f"{np.array2string(dev, precision=1)}; compared over the first {K} windows")
    assert K >= 3
    assert float(dev[:K].max()) <= 1e-9


def test_several_tracklets(tr):
    from pmce_amd import camera, demo
    model = get_model(256)
    wh = (1920, 1080)
    pairs = [(kp, feat) for kp, feat, _ in tr]
    n0, n1 = (p[0].shape[0] for p in pairs)
    init = T(np.array([[0.3, 0.1, 0.2], [0.6, 0.2, 0.05]], dtype=np.float32))
    outs = demo.run_tracklets(model, pairs, wh, batch=16, init=init)                     # 63 windows in batches of 16: mixed people
    assert len(outs) == 2 and outs[0]["mesh"].shape[0] == n0 and outs[1]["mesh"].shape[0] == n1
    for i, (kp, feat) in enumerate(pairs):
        one = demo.run_tracklet(model, kp, feat, wh, batch=16, init=init[i:i + 1])
        e = maxabs(outs[i]["mesh"], one["mesh"])
        print(f"tracklet {i}: shared batches vs alone, mesh {e:.2e} m")
        assert e < TIGHT_M
        assert torch.equal(outs[i]["bboxes"], one["bboxes"]) and torch.equal(outs[i]["target2d"], one["target2d"])
    joints = torch.cat([o["joints_mm"] for o in outs])
    target = torch.cat([o["target2d"] for o in outs])
    bbox = torch.cat([o["bboxes"] for o in outs])
    cam, loss, orig = camera.fit_camera(joints, target, init=init, seq_offsets=[0, n0, n0 + n1], scale=1e-3, bbox=bbox, img_wh=wh)
    assert torch.equal(torch.cat([o["pred_cam"] for o in outs]), cam) and torch.equal(torch.cat([o["orig_cam"] for o in outs]), orig)
    assert torch.equal(torch.cat([o["loss"] for o in outs]), loss)
    across = demo.run_tracklets(model, pairs, wh, batch=16, init=init[:1], chain_across=True)
    assert torch.equal(torch.cat([o["joints_mm"] for o in across]), joints)
    cam1, _, orig1 = camera.fit_camera(joints, target, init=init[:1], chain=True, scale=1e-3, bbox=bbox, img_wh=wh)
    assert torch.equal(torch.cat([o["pred_cam"] for o in across]), cam1) and torch.equal(torch.cat([o["orig_cam"] for o in across]), orig1)
    assert torch.equal(across[0]["pred_cam"], outs[0]["pred_cam"]) and not torch.equal(across[1]["pred_cam"][0], outs[1]["pred_cam"][0])


def test_no_host_wait_before_the_check(tr):
    """The stream is plugged with about half a second of matrix products, then run_tracklet(check=False) is called: if the host had
    waited for the stream anywhere inside - a copy from pageable memory, a synchronize, a read-back - the plug would be finished when
    the call returns.  An event recorded behind the plug is still pending then (torch.cuda.Event.query, no wait of its own).  The call's
    host side takes a few tens of milliseconds once warm."""
    from pmce_amd import demo
    model = get_model(256)
    kp, feat, wh = tr[0]
    init = T(INIT)
    policy = model.overflow_policy()
    for reuse in (True, False):
        if not reuse:
            model.set_overflow_policy("report")          # forward_with_joints' default "rerun" policy waits per batch by design
        try:
            demo.run_tracklet(model, kp, feat, wh, init=init, reuse=reuse, check=False)      # warm: workspaces, lanes, tables
            a = torch.randn(8192, 8192, device=dev())
            torch.cuda.synchronize()
            start, plug = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(40):
                a @ a
            plug.record()
            out = demo.run_tracklet(model, kp, feat, wh, init=init, reuse=reuse, check=False)
            pending = not plug.query()
            torch.cuda.synchronize()
            print(f"reuse={reuse}: plug of {start.elapsed_time(plug):.0f} ms still running when run_tracklet returned: {pending}")
            assert pending, f"reuse={reuse}: the host waited for the stream inside run_tracklet"
            assert bool(torch.isfinite(out["pred_cam"]).all())
        finally:
            model.set_overflow_policy(policy)


ORACLE_WINDOWS = [0, 7, 8, 9, 15, 16, 22]      # of tracklet 1 (23 frames): repeated-frame head, first / inner / last 16-frame window, tail


def _oracle(C, fx, i=1):
    """The oracle forward (CPU) of the fixture's OWN 16 x 19 x 2 inputs of tracklet i, windows ORACLE_WINDOWS; once per width."""
    from oracle import pmce_oracle as O
    if C not in _ORACLE:
        _ORACLE.clear()
        model = get_model(C)
        feat = DR.features(i)
        wl = DR.window_list(len(feat))[ORACLE_WINDOWS]
        wf = np.stack([feat[[s] * 16] if s == e else feat[s:e + 1] for s, e in wl])
        with torch.no_grad():
            _ORACLE[C] = O.pmce_forward(cached_state_dict(J, C), torch.from_numpy(fx[f"input{i}"][ORACLE_WINDOWS]), torch.from_numpy(wf),
                                        model.vj_relation)
    return _ORACLE[C]


@pytest.mark.parametrize("mode", ["split_f16 at every batch size", "f32"])
@pytest.mark.parametrize("C", [256, 512])
def test_reference_mode_cached_matches_oracle(fx, tr, C, mode):
    from pmce_amd import demo, streaming
    model = get_model(C)
    rm, rp, rl = _oracle(C, fx)
    kp, feat, wh = tr[1]
    if mode == "f32":
        model.set_gemm_mode("f32")
    else:
        model.set_gemm_mode("split_f16", min_batch=1)
    try:
        init = T(INIT)
        out = demo.run_tracklet(model, kp, feat, wh, batch=10, init=init)                # 23 windows: 10 + 10 + 3, two lanes
        unc = demo.run_tracklet(model, kp, feat, wh, batch=10, init=init, reuse=False)
        # pose / pose3d are not in the façade's dict: the same cached forward by hand
        n = kp.shape[0]
        wd = demo.demo_windows_device([n], dev())
        _, _, mid, _ = demo.demo_targets(kp, wd, wh)
        from pmce_amd import staging
        shapes = torch.tensor([[wh[1], wh[0]]], dtype=torch.int32, device=dev()).repeat(n, 1)
        pose_fr = staging.prepare_pose2d(kp, shapes)
        cache = streaming.precompute_mid_frames(model, streaming.precompute_frames(model, pose_fr, feat), mid, feat)
        mesh, pose, pose3d, pred = streaming.stream_forward_cached(model, cache, windows=wd, batch=10, with_joints=True)
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode(None)
    assert torch.equal(mesh, out["mesh"]) and torch.equal(pred, out["joints_mm"])
    k = ORACLE_WINDOWS
    e = (maxabs(mesh[k], rm), maxabs(pose[k], rp), maxabs(pose3d[k], rl))
    u = (maxabs(out["mesh"], unc["mesh"]), maxabs(out["joints_mm"], unc["joints_mm"]))
    print(f"C={C} {mode}: cached vs oracle mesh {e[0]:.2e} m, pose {e[1]:.2e} m, pose3d {e[2]:.2e} mm; cached vs uncached mesh {u[0]:.2e} m, "
          f"joints {u[1]:.2e} mm; uncached vs oracle mesh {maxabs(unc['mesh'][k], rm):.2e} m")
    assert e[0] < TIGHT_M and e[1] < TIGHT_M and e[2] < TOL_MM
    assert maxabs(unc["mesh"][k], rm) < TIGHT_M
    assert u[0] < TIGHT_M and u[1] < 1000 * TIGHT_M
