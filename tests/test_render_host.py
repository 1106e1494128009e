"""CPU-only tests of the renderer's host side (pmce_amd/render.py, demo.render_tracklets' ordering) and of the oracle the GPU tests
measure against (tests/render_ref.py)."""
import os.path as osp
import re

import numpy as np
import pytest

import demo_ref as DR
import render_ref as RR
from conftest import REPO
from pmce_amd import _lib, demo, render


def test_csr_matches_dense_incidence():
    rng = np.random.default_rng(3)
    for verts, faces in (RR.icosphere(), (np.zeros((40, 3)), rng.integers(0, 37, size=(90, 3)).astype(np.int32))):
        V = len(verts)
        off, ids = render.vertex_face_csr(faces, V)
        dense = np.zeros((V, len(faces)), dtype=np.int64)
        for f, tri in enumerate(faces):
            for v in tri:
                dense[v, f] += 1
        assert off.dtype == np.int32 and ids.dtype == np.int32 and off[0] == 0 and off[-1] == 3 * len(faces)
        for v in range(V):
            mine = ids[off[v]:off[v + 1]]
            assert np.all(np.diff(mine) >= 0), "a vertex' faces are listed in ascending order"
            assert np.array_equal(np.bincount(mine, minlength=len(faces)), dense[v])
    with pytest.raises(_lib.PmceError):
        render.vertex_face_csr(np.array([[0, 1, 5]]), 5)


def test_layers_follow_frame_results_order():
    """Three persons with a missing frame and a tie in bbox[1]: the schedule draws the persons of every frame in the order
    demo.frame_results gives them (bbox[1] ascending, ties in tracklet order), person l of a frame in layer l."""
    res, num_frames = DR.render_case()
    res[2]["frame_ids"] = np.delete(res[2]["frame_ids"], 3)                 # person 2 misses frame 11
    for k in ("mesh", "pred_cam", "bboxes"):
        res[2][k] = np.delete(res[2][k], 3, axis=0)
    r7 = int(np.nonzero(res[7]["frame_ids"] == 9)[0][0])
    r2 = int(np.nonzero(res[2]["frame_ids"] == 9)[0][0])
    res[2]["bboxes"][r2, 1] = res[7]["bboxes"][r7, 1]                       # a tie in frame 9: 7 comes first in the dict, so it is drawn first
    frames = demo.frame_results(res, None, num_frames)
    keys = list(res.keys())
    person = np.concatenate([np.full(len(res[k]["mesh"]), k) for k in keys])
    fi, order = demo.tracklet_draw_order([res[k]["bboxes"][:, 1] for k in keys], [res[k]["frame_ids"] for k in keys])
    sched, offsets = render.schedule_layers(fi, num_frames, order)
    assert sorted(sched.tolist()) == list(range(len(person)))
    for l in range(len(offsets) - 1):
        jobs = sched[offsets[l]:offsets[l + 1]]
        assert np.all(np.diff(fi[jobs]) > 0), "one job per frame and layer, frames ascending"
        for j in jobs:
            assert list(frames[fi[j]].keys())[l] == person[j]
    assert [len(fd) for fd in frames] == [int(np.sum(fi == f)) for f in range(num_frames)]
    assert list(frames[9].keys()).index(7) < list(frames[9].keys()).index(2)
    # without draw_order: the order given
    s, o = render.schedule_layers(np.array([2, 0, 2, 1, 2, 0]), 3)
    assert s.tolist() == [1, 3, 0, 5, 2, 4] and o.tolist() == [0, 3, 5, 6]
    s, o = render.schedule_layers(np.zeros(0, dtype=np.int64), 3)
    assert s.size == 0 and o.tolist() == [0]


def test_argument_validation():
    verts, faces = RR.icosphere()
    V = len(verts)
    E = _lib.PmceError
    with pytest.raises(E):
        render.Renderer(faces, (8193, 100))
    with pytest.raises(E):
        render.Renderer(faces, (100, 8193))
    with pytest.raises(E):
        render.Renderer(faces.astype(np.float32), (64, 48))
    with pytest.raises(E):
        render.Renderer(faces[:, :2], (64, 48))
    with pytest.raises(E):
        render.Renderer(faces, (64, 48), lights=np.zeros((9, 3)))
    r = render.Renderer(faces, (64, 48))
    img = np.zeros((2, 48, 64, 3), dtype=np.uint8)
    v = np.zeros((2, V, 3), dtype=np.float32)
    cam = np.ones((2, 4), dtype=np.float32)
    assert r.check_args(img, v, cam)[:3] == (2, 2, V)
    bad = [dict(images=img.astype(np.float32)), dict(images=img[:, :, :60]), dict(images=img[..., :2]), dict(verts=v[:, :-1]),
           dict(verts=v.astype(np.int32)), dict(verts=v[0]), dict(cams=cam[:, :3]), dict(cams=cam[:1]), dict(frame_index=np.array([0, 2])),
           dict(frame_index=np.array([-1, 0])), dict(frame_index=np.array([0.0, 1.0])), dict(frame_index=np.array([0])),
           dict(rotation=np.eye(4)), dict(order="nearest"), dict(verts=np.zeros((3, V, 3), np.float32))]
    for kw in bad:
        args = dict(images=img, verts=v, cams=cam)
        args.update(kw)
        with pytest.raises(E):
            r.render(**args)
    with pytest.raises(E):
        demo.render_tracklets([], img, (64, 48))                       # no faces, no renderer


def test_symbols_exported_and_prototyped():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("pmce_render_workspace_bytes", "pmce_render_meshes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not prototyped in include/pmce_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    # the query and the entry point's argument checks run without a GPU
    one = lib.pmce_render_workspace_bytes(3, 162, 64, 48, 1)
    assert lib.pmce_render_workspace_bytes(3, 162, 64, 48, 2) - one == 64 * 48 * 8 and one > 3 * 162 * 24
    assert lib.pmce_render_workspace_bytes(3, 162, 8193, 48, 1) == 0 and "8192" in _lib.last_error()


def test_oracle_on_the_convex_ellipsoid():
    """On a closed convex mesh with back faces culled every pixel has at most one surviving fragment, and culling changes nothing about
    which pixels are covered."""
    W, H = 97, 61
    verts, faces = RR.ellipsoid(RR.icosphere())
    for cam in RR.cameras(W, H):
        xy = RR.snap(RR.project(verts.astype(np.float64), cam, W, H))
        culled = RR.resolve(RR.fragments(xy, verts[:, 2], faces, W, H, cull=True), W, H)
        both = RR.resolve(RR.fragments(xy, verts[:, 2], faces, W, H, cull=False), W, H)
        assert culled["covered"].any() and not culled["covered"].all()
        assert culled["count"].max() == 1
        assert np.array_equal(culled["covered"], both["covered"])
        assert both["count"].max() == 2
        assert np.array_equal(culled["decided"], culled["covered"])
    # the meshes the issue names
    assert RR.icosphere()[0].shape == (162, 3) and RR.icosphere()[1].shape == (320, 3)
    v, f = RR.uv_sphere()
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    for vv, ff in (RR.icosphere(), (v, f)):                       # closed: every edge is used once in each direction
        e = np.concatenate([ff[:, [0, 1]], ff[:, [1, 2]], ff[:, [2, 0]]])
        assert len(set(map(tuple, e))) == len(e) and set(map(tuple, e)) == set(map(tuple, e[:, ::-1]))
