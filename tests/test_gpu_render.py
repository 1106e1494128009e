"""The HIP rasteriser (csrc/render.hip, pmce_amd/render.py) against the numpy oracle of tests/render_ref.py.

What is compared how.  Coordinates: the kernel's snapped xy_fixed against the fp64 projection rounded to nearest, within 1 unit (1/256 px).
Coverage and identity: the oracle is fed the kernel's OWN xy_fixed, after which coverage is exact integer arithmetic on both sides:
face_id >= 0 equals the oracle's coverage on every pixel whose candidate fragments all lie at least TAU from the clip planes, and face_id
equals the oracle's on every decided pixel (render_ref: the two nearest survivors more than TAU = 1e-5 apart - ten times the fp32
interpolation error).  Shading: within 1 of the oracle's 8-bit value on decided pixels (a rounding boundary crossed by fp32 error)."""
import numpy as np
import pytest
import torch

import demo_ref as DR
import render_ref as RR
from pmce_amd import demo, render

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def run(r, images, verts, cams, **kw):
    """Renderer.render with aux on device tensors -> numpy (image, face_id, depth, status, xy_fixed)."""
    kw.setdefault("return_aux", True)
    out, aux = r.render(T(images), T(np.asarray(verts, dtype=np.float32)), T(np.asarray(cams, dtype=np.float32)), **kw)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), aux["face_id"].cpu().numpy(), aux["depth"].cpu().numpy(), aux["status"].cpu().numpy(),
            aux["xy_fixed"].cpu().numpy())


def noise(F, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def check_job(image_in, out, face_id, depth, xy, verts, faces, W, H, rotation=None, cull=True, max_undecided=0.005, **material):
    """One job alone in its frame against the oracle on the kernel's own coordinates; returns the oracle's per-pixel result."""
    q = RR.transform(verts, rotation)
    res = RR.resolve(RR.fragments(xy, q[:, 2], faces, W, H, cull), W, H)
    # the oracle alone first: the undecided share of the covered pixels is capped
    n_cov = int(res["covered"].sum())
    n_und = int((res["covered"] & ~res["decided"]).sum())
    print(f"covered {n_cov}, undecided {n_und}")
    assert n_und <= max_undecided * max(n_cov, 1)
    safe = res["clip_safe"]
    assert np.array_equal((face_id >= 0)[safe], res["covered"][safe]), "coverage differs from the integer oracle"
    dec = res["decided"]
    assert np.array_equal(face_id[dec], res["face"][dec]), "face_id differs on decided pixels"
    assert np.all(np.abs(depth[dec] - res["z"][dec]) < RR.TAU)
    assert np.all(np.isinf(depth[face_id < 0]))
    ref = RR.shade(res, q, faces, **material)
    diff = np.abs(out[dec].astype(np.int32) - ref[dec].astype(np.int32))
    print(f"shading: max 8-bit difference on {int(dec.sum())} decided pixels {int(diff.max()) if diff.size else 0}")
    assert diff.size == 0 or diff.max() <= 1
    assert np.array_equal(out[face_id < 0], image_in[face_id < 0]), "an uncovered pixel changed"
    return res


@pytest.fixture(scope="module")
def ico():
    return RR.ellipsoid(RR.icosphere())


@pytest.mark.parametrize("wh", [(97, 61), (64, 48)])
def test_coordinates_and_ellipsoid(ico, wh):
    """xy_fixed within one unit of the fp64 projection, with cameras that put the mesh partly off every side; and the convex ellipsoid's
    coverage, identity, depth and shading in each of those views (no undecided pixel, by construction)."""
    W, H = wh
    verts, faces = ico
    cams = RR.cameras(W, H)
    N = len(cams)
    r = render.Renderer(faces, wh)
    img = noise(N, H, W)
    out, fid, dep, st, xy = run(r, img, np.repeat(verts[None], N, 0), cams)
    assert not st.any()
    for j in range(N):
        want = RR.snap(RR.project(verts.astype(np.float64), cams[j], W, H))
        assert np.abs(xy[j].astype(np.int64) - want).max() <= 1
        if j:       # partly off one side of the image
            assert (xy[j, :, 0] < 0).any() or (xy[j, :, 0] > W * 256).any() or (xy[j, :, 1] < 0).any() or (xy[j, :, 1] > H * 256).any()
        res = check_job(img[j], out[j], fid[j], dep[j], xy[j], verts, faces, W, H, max_undecided=0.0)
        assert res["covered"].any() and res["count"].max() == 1


# ---- hand-made cases in one small image ------------------------------------------------------------------------------------------------
HW, HH = 16, 8


def px_to_model(p):
    """Pixel coordinates -> model coordinates under the camera (1, 1, 0, 0) of a 16 x 8 image (exact in fp32 for multiples of 1/32 px)."""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([p[..., 0] * 2 / HW - 1, p[..., 1] * 2 / HH - 1], -1)


def front(tri, flip=False):
    (ax, ay), (bx, by), (cx, cy) = tri
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    if (area > 0) != flip:
        tri = [tri[0], tri[2], tri[1]]
    return tri


NOTHING = [(0, 0), (0, 0), (0, 0)]
HAND = {  # name: two triangles in pixels (faces (0,1,2) and (3,4,5))
    "shared_edge": [front([(1.5, 1.5), (5.5, 5.5), (5.5, 1.5)]), front([(1.5, 1.5), (1.5, 5.5), (5.5, 5.5)])],
    "zero_area": [[(1, 1), (3, 3), (5, 5)], NOTHING],
    "larger_than_image": [front([(-40, -30), (60, -30), (10, 80)]), NOTHING],
    "off_screen": [front([(-20, -20), (-10, -20), (-15, -10)]), NOTHING],
    "guard_band": [front([(2, 2), (20000, 2), (2, 6)]), front([(9.25, 1.0), (14.0, 2.5), (10.5, 7.0)])],
    "back_face": [front([(2.25, 1.0), (12.0, 2.5), (6.5, 7.75)], flip=True), NOTHING],
}
HAND_FACES = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


@pytest.mark.parametrize("cull", [True, False])
def test_hand_made_coverage(cull):
    names = list(HAND)
    N = len(names)
    verts = np.zeros((N, 6, 3), dtype=np.float32)
    for j, n in enumerate(names):
        verts[j, :, :2] = px_to_model(np.array(HAND[n], dtype=np.float64).reshape(6, 2))
    cams = np.tile(np.array([[1.0, 1.0, 0.0, 0.0]], dtype=np.float32), (N, 1))
    r = render.Renderer(HAND_FACES, (HW, HH), cull_backfaces=cull)
    img = noise(N, HH, HW, seed=1)
    out, fid, dep, st, xy = run(r, img, verts, cams)
    cov = {}
    for j, n in enumerate(names):
        want = np.rint(np.array(HAND[n], dtype=np.float64).reshape(6, 2) * 256)
        inside = np.abs(want).max(1) <= RR.GUARD
        assert np.array_equal(xy[j][inside], want[inside].astype(np.int64)), n
        res = check_job(img[j], out[j], fid[j], dep[j], xy[j], verts[j], HAND_FACES, HW, HH, cull=cull, max_undecided=0.0)
        cov[n] = res
        assert st[j] == (render.STATUS_GUARD if n == "guard_band" else 0), n
    sq = np.zeros((HH, HW), dtype=bool)
    sq[1:5, 1:5] = True    # the square [1.5, 5.5)^2: its left and top edges own their pixel centres, its right and bottom edges do not
    assert np.array_equal(cov["shared_edge"]["covered"], sq) and cov["shared_edge"]["count"].max() == 1
    assert fid[names.index("shared_edge")][1, 1] >= 0 and fid[names.index("shared_edge")][5, 5] < 0    # vertices ON pixel centres
    assert not cov["zero_area"]["covered"].any() and not cov["off_screen"]["covered"].any()
    assert cov["larger_than_image"]["covered"].all()
    g = fid[names.index("guard_band")]
    assert not (g == 0).any() and (g == 1).any()        # the triangle beyond the guard band draws nothing, its neighbour is drawn
    assert cov["back_face"]["covered"].any() == (not cull)


def test_interpenetrating_ellipsoids(ico):
    """Two crossing closed surfaces in ONE mesh: up to two front-facing fragments per pixel; only the intersection curve is undecided."""
    W, H = 97, 61
    verts, faces = RR.two_ellipsoids(RR.icosphere())
    cam = RR.cameras(W, H)[:1]
    r = render.Renderer(faces, (W, H))
    img = noise(1, H, W, seed=2)
    out, fid, dep, st, xy = run(r, img, verts[None], cam)
    res = check_job(img[0], out[0], fid[0], dep[0], xy[0], verts, faces, W, H)
    assert res["count"].max() == 2
    first, second = fid[0][(fid[0] >= 0)] < len(faces) // 2, fid[0][(fid[0] >= 0)] >= len(faces) // 2
    assert first.any() and second.any(), "each surface is in front somewhere"


def test_equal_depth_goes_to_the_lower_face_and_clipping():
    """Two overlapping coplanar triangles at z = 0.5 exactly (vertices on whole pixels: every edge value is exact in fp32): the overlap
    shows face 0.  A triangle whose z runs from 0.25 to 1.75 loses exactly the fragments beyond z = 1."""
    t0, t1 = front([(1, 1), (12, 1), (1, 7)]), front([(3, 0), (14, 6), (2, 6)])
    verts = np.zeros((2, 6, 3), dtype=np.float32)
    verts[0, :, :2] = px_to_model(np.array([t1, t0], dtype=np.float64).reshape(6, 2))     # face 0 = t1, face 1 = t0
    verts[0, :, 2] = 0.5
    strad = front([(0.75, 0.5), (15.5, 1.25), (6.0, 7.75)])
    verts[1, :3, :2] = px_to_model(np.array(strad, dtype=np.float64))
    verts[1, :3, 2] = (0.25, 1.75, 0.6)
    cams = np.tile(np.array([[1.0, 1.0, 0.0, 0.0]], dtype=np.float32), (2, 1))
    r = render.Renderer(HAND_FACES, (HW, HH))
    img = noise(2, HH, HW, seed=3)
    out, fid, dep, st, xy = run(r, img, verts, cams)
    fr = RR.fragments(xy[0], verts[0, :, 2].astype(np.float64), HAND_FACES, HW, HH)
    res = RR.resolve(fr, HW, HH)
    both = res["count"] == 2
    assert both.sum() >= 8 and (res["count"] == 1).any()
    assert np.all(fr["z"] == 0.5)
    assert np.all(fid[0][both] == 0) and np.array_equal(fid[0], res["face"]) and np.all(dep[0][res["covered"]] == 0.5)
    res = check_job(img[1], out[1], fid[1], dep[1], xy[1], verts[1], HAND_FACES, HW, HH, max_undecided=0.0)
    fr = RR.fragments(xy[1], verts[1, :, 2].astype(np.float64), HAND_FACES, HW, HH)
    cand = np.zeros((HH, HW), dtype=bool)
    cand[fr["y"], fr["x"]] = True
    assert res["covered"].any() and (cand & ~res["covered"]).any(), "the triangle is drawn in part and clipped in part"


def test_color_lights_rotation(ico):
    W, H = 64, 48
    verts, faces = ico
    cam = RR.cameras(W, H)[:1]
    img = noise(1, H, W, seed=4)
    base = run(render.Renderer(faces, (W, H)), img, verts[None], cam)[0]
    a = np.radians(60.0)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])      # renderer.py:69-70, about y
    variants = [dict(color=(0.2, 0.9, 0.4)), dict(lights=[[-0.6, 0.0, -0.8]], intensity=2.0, ambient=0.1, emissive=0.0), dict(lights=[]),
                dict(rotation=rot)]
    for kw in variants:
        rotation = kw.pop("rotation", None)
        r = render.Renderer(faces, (W, H), **kw)
        out, fid, dep, st, xy = run(r, img, verts[None], cam, rotation=None if rotation is None else T(rotation.astype(np.float32)))
        check_job(img[0], out[0], fid[0], dep[0], xy[0], verts, faces, W, H, rotation=rotation, max_undecided=0.0, **kw)
        assert not np.array_equal(out, base)
    want = RR.snap(RR.project(RR.transform(verts, rot), cam[0], W, H))
    assert np.abs(xy[0].astype(np.int64) - want).max() <= 1


# ---- compositing ---------------------------------------------------------------------------------------------------------------------
def scene(ico, W=97, H=61):
    """Three frames with 0, 1 and 3 persons.  In the last frame the persons overlap and the FIRST drawn is the nearest."""
    verts, faces = ico
    sy, sx = 0.8, 0.8 * H / W
    shift = lambda dx, dz: verts + np.array([dx, 0.0, dz], dtype=np.float32)      # noqa: E731
    jobs = [(1, shift(0.0, 0.0)), (2, shift(-0.15, -0.4)), (2, shift(0.0, 0.0)), (2, shift(0.2, 0.4))]
    v = np.stack([j[1] for j in jobs])
    cams = np.tile(np.array([[sx, sy, 0.0, 0.0]], dtype=np.float32), (len(jobs), 1))
    return v, cams, np.array([j[0] for j in jobs], dtype=np.int32), faces, W, H


def test_compositing_orders(ico):
    v, cams, fi, faces, W, H = scene(ico)
    r = render.Renderer(faces, (W, H))
    img = noise(3, H, W, seed=5)
    out, fid, dep, st, xy = run(r, img, v, cams, frame_index=T(fi))
    want = img.copy()
    zs = []
    for j in range(len(fi)):
        want[fi[j]], res = RR.draw(want[fi[j]], xy[j], v[j], faces, W, H)
        assert np.array_equal(res["decided"], res["covered"])
        zs.append(res)
    assert np.array_equal(out[0], img[0]), "a frame without persons is untouched"
    assert np.abs(out.astype(np.int32) - want.astype(np.int32)).max() <= 1
    drawn = zs[1]["covered"] | zs[2]["covered"] | zs[3]["covered"]
    assert np.array_equal(out[2][~drawn], img[2][~drawn]) and np.array_equal(fid[2] >= 0, drawn)
    # the later person wins where they overlap, whatever the depth
    last_z = np.where(zs[3]["covered"], zs[3]["z"], np.where(zs[2]["covered"], zs[2]["z"], zs[1]["z"]))
    over = zs[1]["covered"] & zs[3]["covered"]
    assert over.sum() > 20 and np.all(zs[1]["z"][over] < zs[3]["z"][over])
    assert np.all(np.abs(dep[2][drawn] - last_z[drawn]) < RR.TAU)
    # order = "depth": the nearest one
    out_d, fid_d, dep_d, _, _ = run(r, img, v, cams, frame_index=T(fi), order="depth")
    near_z = np.minimum(np.minimum(zs[1]["z"], zs[2]["z"]), zs[3]["z"])
    assert np.array_equal(fid_d[2] >= 0, drawn) and np.all(np.abs(dep_d[2][drawn] - near_z[drawn]) < RR.TAU)
    nearest = np.argmin(np.stack([zs[k]["z"] for k in (1, 2, 3)]), 0)
    for k in (1, 2, 3):
        m = drawn & (nearest == k - 1)
        one = RR.shade(zs[k], RR.transform(v[k]), faces)
        assert m.any() and np.array_equal(fid_d[2][m], zs[k]["face"][m])
        assert np.abs(out_d[2][m].astype(np.int32) - one[m].astype(np.int32)).max() <= 1
    assert np.array_equal(out_d[:2], out[:2]) and not np.array_equal(out_d[2], out[2])
    # in place == out of place, bit for bit
    dimg = T(img)
    same = r.render(dimg, T(v), T(cams), frame_index=T(fi), inplace=True)
    assert same.data_ptr() == dimg.data_ptr() and np.array_equal(dimg.cpu().numpy(), out)
    # a host array in, a host array out
    host = r.render(img, v, cams, frame_index=fi)
    assert isinstance(host, np.ndarray) and np.array_equal(host, out)


def test_non_finite_jobs_are_skipped(ico):
    v, cams, fi, faces, W, H = scene(ico)
    r = render.Renderer(faces, (W, H))
    img = noise(5, H, W, seed=6)
    good = run(r, img, v, cams, frame_index=T(fi))
    bad_v = v[:1].copy()
    bad_v[0, 37, 1] = np.nan
    bad_c = cams[:1].copy()
    bad_c[0, 2] = np.inf
    v2 = np.concatenate([bad_v, v, v[:1]])
    c2 = np.concatenate([cams[:1], cams, bad_c])
    fi2 = np.concatenate([[3], fi, [4]]).astype(np.int32)
    out, fid, dep, st, xy = run(r, img, v2, c2, frame_index=T(fi2))
    assert st.tolist() == [render.STATUS_NONFINITE, 0, 0, 0, 0, render.STATUS_NONFINITE]
    assert np.array_equal(out[3:], img[3:]) and (fid[3:] < 0).all(), "a skipped job leaves its frame untouched"
    for a, b in zip(good[:3], (out, fid, dep)):
        assert np.array_equal(a[:3], b[:3]), "the neighbours of a skipped job are bit-identical to a run without it"


def test_determinism_and_chunking(ico):
    v, cams, fi, faces, W, H = scene(ico)
    v, cams = np.concatenate([v, v]), np.concatenate([cams, cams])
    fi = np.concatenate([fi, fi + 3]).astype(np.int32)
    img = noise(6, H, W, seed=7)
    r = render.Renderer(faces, (W, H))
    for order in render.ORDERS:
        a = run(r, img, v, cams, frame_index=T(fi), order=order)
        b = run(r, img, v, cams, frame_index=T(fi), order=order)
        small = torch.empty(r.workspace_bytes(len(fi), v.shape[1], 1), device=dev(), dtype=torch.uint8)
        small.fill_(0x5A)                           # whatever the workspace holds on entry
        c = run(r, img, v, cams, frame_index=T(fi), order=order, workspace=small)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert not np.array_equal(a[0], img)
    with pytest.raises(render.PmceError):
        r.render(T(img), T(v), T(cams), frame_index=T(fi), workspace=small[:-64])


def test_real_size():
    """The 6890-vertex, 13 776-face sphere as a body-sized ellipsoid, one frame at 1920 x 1080."""
    W, H = 1920, 1080
    verts, faces = RR.ellipsoid(RR.uv_sphere())
    cam = np.array([[1.0 * H / W, 1.0, 0.1, 0.02]], dtype=np.float32)
    r = render.Renderer(faces, (W, H))
    img = noise(1, H, W, seed=8)
    out, fid, dep, st, xy = run(r, img, verts[None], cam)
    assert st[0] == 0
    assert np.abs(xy[0].astype(np.int64) - RR.snap(RR.project(verts.astype(np.float64), cam[0], W, H))).max() <= 1
    res = check_job(img[0], out[0], fid[0], dep[0], xy[0], verts, faces, W, H, max_undecided=0.0)
    assert res["covered"].sum() > 150_000      # an ellipse of 135 x 459 px semi-axes


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_render_tracklets_end_to_end():
    """demo.render_tracklets on demo.run_tracklets' outputs for the two fixture tracklets == Renderer.render fed by hand from
    demo.frame_results.  orig_cam is relative to the image, so the frames can be a tenth of the video's size."""
    from test_gpu_demo import get_model
    model = get_model(256)
    wh, small = (1920, 1080), (192, 108)
    pairs = [(T(DR.tracklet(i)[0]), T(DR.features(i))) for i in range(len(DR.TRACKLETS))]
    outs = demo.run_tracklets(model, pairs, wh, batch=32)
    faces = RR.uv_sphere()[1]                                   # any connectivity over 6890 vertices: SMPL's faces are not here
    ids = [np.arange(0, len(outs[0]["mesh"])), np.arange(10, 10 + len(outs[1]["mesh"]))]
    F = 40
    frames = T(noise(F, small[1], small[0], seed=9))
    r = render.Renderer(faces, small)
    for order in render.ORDERS:
        got = demo.render_tracklets(outs, frames, small, frame_ids=ids, renderer=r, order=order)
        res = {i: {"mesh": o["mesh"].cpu().numpy(), "pred_cam": o["orig_cam"].cpu().numpy(), "bboxes": o["bboxes"].cpu().numpy(),
                   "frame_ids": ids[i]} for i, o in enumerate(outs)}
        per_frame = demo.frame_results(res, None, F)
        v, c, fi = [], [], []
        for f, fd in enumerate(per_frame):
            for pid, d in fd.items():
                v.append(d["verts"]), c.append(d["cam"]), fi.append(f)
        by_hand = r.render(frames, T(np.stack(v)), T(np.stack(c)), frame_index=T(np.array(fi, dtype=np.int32)), order=order)
        assert torch.equal(got, by_hand)
        assert not torch.equal(got, frames) and got.data_ptr() != frames.data_ptr()
    assert torch.equal(demo.render_tracklets(outs, frames, small, frame_ids=ids, renderer=faces), demo.render_tracklets(
        outs, frames, small, frame_ids=ids, renderer=r))
