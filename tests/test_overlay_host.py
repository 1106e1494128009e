"""The debug overlay and the demo's output switches, the parts that need no GPU: the coverage rules run on the host
(scripts/overlay_cover_host.cpp over pmce_amd/csrc/overlay_cover.hpp) against Python integers (tests/overlay_ref.py), the argument
errors of ``overlay.draw``, the font, ``render.axis_rotation``, the C interface, ``save_results`` / ``save_meshes`` and the refusals of
``render_folder`` / ``render_tracklets``."""
import math
import os.path as osp
import pickle
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import overlay_ref as OR
from pmce_amd import _lib, build, demo, overlay, render

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def bits_of(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def test_coverage_rules_on_the_host_equal_python_integers(tmp_path):
    """The shared header, built with the host compiler (a plain build), over random coordinates and the extremes: endpoints at
    +-2^14 px, the diagonal from (-16000, -16000) to (16000, 16000) px (|p|^2 L passes 64 bits), zero length, a centre exactly at
    distance 8 t, ties of rint."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "overlay_cover_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", osp.join(REPO, "pmce_amd", "csrc"), osp.join(REPO, "scripts", "overlay_cover_host.cpp"),
                    "-o", exe], check=True, capture_output=True)
    rng = np.random.default_rng(31)
    G = 16 * 2 ** 14                                            # the guard band in units
    lines, want = [], []

    def seg(ax, ay, bx, by, cx, cy, t):
        lines.append(f"S {ax} {ay} {bx} {by} {cx} {cy} {t}")
        want.append("1" if OR.segment_covers(ax, ay, bx, by, cx, cy, t) else "0")

    def disc(kx, ky, cx, cy, r):
        lines.append(f"D {kx} {ky} {cx} {cy} {r}")
        want.append("1" if OR.disc_covers(kx, ky, cx, cy, r) else "0")

    def quant(v):
        lines.append(f"Q {bits_of(v)}")
        want.append("1 0" if OR.beyond_guard(v) else f"0 {OR.quantise(v)}")

    # random segments of every length, the centre near the line so that both verdicts occur
    for _ in range(4000):
        span = int(rng.choice([40, 600, 20000, G]))
        ax, ay, bx, by = (int(v) for v in rng.integers(-span, span + 1, 4))
        t = int(rng.integers(1, 65))
        u = float(rng.uniform(-0.2, 1.2))
        off = float(rng.uniform(-2, 2)) * 8 * t
        n = math.hypot(bx - ax, by - ay) or 1.0
        cx = int(round(ax + u * (bx - ax) - off * (by - ay) / n))
        cy = int(round(ay + u * (by - ay) + off * (bx - ax) / n))
        seg(ax, ay, bx, by, cx, cy, t)
    # the long diagonal: 128-bit products; centres of a frame's pixels on it, next to it and exactly 8 t away from an axis-parallel twin
    far = 16000 * 16
    for x in range(0, 40):
        for y in range(0, 24):
            seg(-far, -far, far, far, OR.centre(x), OR.centre(y), 1 + (x + y) % 5)
    for t in (1, 2, 5, 64):
        for d in (-1, 0, 1):                                    # |p|^2 L - s^2 against (8 t)^2 L at, just inside and just outside equality
            seg(-G, 100, G, 100, 8, 100 + 8 * t + d, t)
            seg(100, -G, 100, G, 100 - 8 * t - d, 8, t)
            seg(-G, -G, G, G, 8 * t + d, -(8 * t + d), t)       # perpendicular offset sqrt(2) (8 t + d): never on the border, always decided
            seg(50, 60, 50, 60, 50 + 8 * t + d, 60, t)          # zero length: a disc of 8 t
            seg(50, 60, 50, 60, 50, 60 - 8 * t - d, t)
            seg(0, 0, 160, 0, 160 + 8 * t + d, 0, t)            # beyond the end b
            seg(0, 0, 160, 0, -8 * t - d, 0, t)                 # before the end a
    # a 3-4-5 triangle puts a centre exactly at distance 8 t from a slanted segment: offset (-4, 3) * 8 t / 5 from a point on (3, 4) * k
    for t in (5, 10, 40):
        k = 8 * t // 5
        for d in (-1, 0, 1):
            seg(-3000, -4000, 3000, 4000, 30 - 4 * k, 40 + 3 * k + d, t)
    seg(-G, -G, G, G, G, G, 3)
    seg(G, -G, -G, G, 0, 0, 64)
    for _ in range(1500):
        kx, ky = (int(v) for v in rng.integers(-G, G + 1, 2))
        r = int(rng.integers(1, 65))
        ang, rad = float(rng.uniform(0, 7)), float(rng.uniform(0.8, 1.2)) * 16 * r
        disc(kx, ky, int(round(kx + rad * math.cos(ang))), int(round(ky + rad * math.sin(ang))), r)
    for r in (1, 3, 64):
        for d in (-1, 0, 1):
            disc(G, -G, G - 16 * r - d, -G, r)
            disc(-G, G, -G + (16 * r * 3) // 5, G + (16 * r * 4) // 5 + d, r)
    # quantisation: ties go to even, the guard band is closed at 2^14, everything else of a NaN or an infinity is "beyond"
    for v in (0.03125, 0.09375, -0.03125, -0.09375, 2.53125, 2.59375, 16383.96875, 16383.90625, -16383.96875, 16384.0, -16384.0,
              math.nextafter(16384.0, math.inf), math.nextafter(-16384.0, -math.inf), 0.0, -0.0, 1e-300, 0.031249999999999997,
              0.03125000000000001, float("inf"), float("-inf"), float("nan"), 1e300, 7.5, 7.53125):
        quant(v)
    for v in rng.uniform(-16384, 16384, 1500):
        quant(float(v))
        quant(float(np.round(v * 32) / 32))                   # multiples of 1/32: every second one is a tie
    for lo, hi, n in ((-100, 700, 40), (8, 8, 40), (9, 23, 40), (24, 24, 40), (-9, -8, 24), (600, 900, 24), (7, 8, 1)):
        lines.append(f"C {lo} {hi} {n}")
        px = [p for p in range(n) if lo <= OR.centre(p) <= hi]
        want.append(f"{px[0]} {px[-1]}" if px else None)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) == len(lines)
    for line, g, w in zip(lines, got, want):
        if w is None:                                           # an empty span: any p1 < p0
            p0, p1 = (int(v) for v in g.split())
            assert p1 < p0, line
        else:
            assert g == w, (line, g, w)
    verdicts = [w for l, w in zip(lines, want) if l[0] in "SD"]
    assert 0.2 < verdicts.count("1") / len(verdicts) < 0.8      # both verdicts are exercised
    # the diagonal's products do pass 64 bits
    p = OR.centre(39) + far
    assert (2 * p * p) * (2 * (2 * far) ** 2) > 2 ** 64
    # a wrong case file is refused, not skipped
    path.write_text("S 1 2 3\n")
    assert subprocess.run([exe, str(path)], capture_output=True).returncode == 2


def test_draw_argument_errors_name_the_argument():
    """Every refusal comes before the GPU is touched: host tensors all the way; the device check is the last one."""
    fr = torch.zeros(3, 24, 40, 3, dtype=torch.uint8)
    fi = np.array([0, 1, 2, 2], np.int32)
    bx = np.ones((4, 4))
    ids = np.arange(4)
    kp = np.ones((4, 17, 3), np.float32)
    ok = dict(boxes=bx, ids=ids, keypoints=kp)
    for args, kw, word in (
            ((fr.float(), fi), ok, "frames_u8"), ((fr[0], fi), ok, "frames_u8"), ((fr[..., :2], fi), ok, "frames_u8"),
            ((fr[:0], fi[:0]), {}, "frames_u8"), ((np.zeros((3, 24, 40, 3), np.uint8), fi), ok, "frames_u8"),
            ((fr, fi.astype(np.float32)), ok, "frame_index"), ((fr, fi[None]), ok, "frame_index"),
            ((fr, np.array([0, 1, 2, 3])), ok, "frame_index"), ((fr, np.array([0, -1, 2, 2])), ok, "frame_index"),
            ((fr, fi), dict(ok, boxes=bx[:3]), "boxes"), ((fr, fi), dict(ok, boxes=bx.astype(np.int64)), "boxes"),
            ((fr, fi), dict(ok, boxes=np.ones((4, 5))), "boxes"), ((fr, fi), dict(ok, box_format="xxyy"), "box_format"),
            ((fr, fi), dict(ok, ids=ids[:3]), "ids"), ((fr, fi), dict(ok, ids=ids.astype(np.float64)), "ids"),
            ((fr, fi), dict(ok, ids=np.array([0, 1, 2, 10 ** 9])), "ids"), ((fr, fi), dict(ok, ids=np.array([0, 1, -1, 5])), "ids"),
            ((fr, fi), dict(ok, keypoints=kp[:3]), "keypoints"), ((fr, fi), dict(ok, keypoints=kp[..., :1]), "keypoints"),
            ((fr, fi), dict(ok, keypoints=kp.astype(np.int32)), "keypoints"), ((fr, fi), dict(ok, keypoints=kp[:, :0]), "keypoints"),
            ((fr, fi), dict(ok, skeleton=np.array([[0, 17]])), "skeleton"), ((fr, fi), dict(ok, skeleton=np.array([[0, -1]])), "skeleton"),
            ((fr, fi), dict(ok, skeleton=np.array([0, 1])), "skeleton"), ((fr, fi), dict(ok, skeleton=np.array([[0.0, 1.0]])), "skeleton"),
            ((fr, fi), dict(ok, score_thresh=float("nan")), "score_thresh"), ((fr, fi), dict(ok, score_thresh="0.3"), "score_thresh"),
            ((fr, fi), dict(ok, thickness=0), "thickness"), ((fr, fi), dict(ok, thickness=65), "thickness"),
            ((fr, fi), dict(ok, thickness=2.0), "thickness"), ((fr, fi), dict(ok, radius=0), "radius"),
            ((fr, fi), dict(ok, radius=65), "radius"), ((fr, fi), dict(ok, label_scale=0), "label_scale"),
            ((fr, fi), dict(ok, label_scale=True), "label_scale"), ((fr, fi), dict(ok, alpha=-1), "alpha"),
            ((fr, fi), dict(ok, alpha=256), "alpha"), ((fr, fi), dict(ok, alpha=0.5), "alpha"),
            ((fr, fi), dict(ok, palette=np.zeros((0, 3), np.uint8)), "palette"), ((fr, fi), dict(ok, palette=np.zeros((4, 3))), "palette"),
            ((fr, fi), dict(ok, text_color=(255, 255)), "text_color"), ((fr, fi), dict(ok, text_color=(0, 0, 256)), "text_color"),
            ((fr, fi), dict(ok, key_bytes=0), "key_bytes")):
        with pytest.raises(ValueError, match=word):
            overlay.draw(*args, **kw)
    with pytest.raises(ValueError, match="on the device"):
        overlay.draw(fr, fi, **ok)
    F, H, W, N, K, sk, pal, tc = overlay.check_args(fr, fi, **ok)
    assert (F, H, W, N, K) == (3, 24, 40, 4, 17) and sk.dtype == np.int32 and sk.shape == (19, 2) and pal.dtype == np.uint8 and list(tc) == [255] * 3


def test_font_and_tables():
    assert overlay.FONT.shape == (10, 7) and overlay.FONT.dtype == np.uint8 and overlay.FONT.max() < 32
    assert len({g.tobytes() for g in overlay.FONT}) == 10                      # ten distinct glyphs
    assert all(len(g) == 7 and all(len(row) == 5 and set(row) <= {"#", " "} for row in g) for g in overlay._GLYPHS)
    assert all(g.any() for g in overlay.FONT) and overlay.FONT[1][0] == 0b00100 and overlay.FONT[7][0] == 0b11111
    sk = overlay.COCO17_SKELETON
    assert sk.shape == (19, 2) and sk.dtype == np.int32 and sk.min() == 0 and sk.max() == 16
    assert len({tuple(sorted(l)) for l in sk.tolist()}) == 19 and all(a != b for a, b in sk.tolist())
    assert set(sk.reshape(-1).tolist()) == set(range(17))                      # every keypoint is on a limb
    names = overlay.COCO17
    assert [names[5], names[6], names[11], names[16]] == ["left_shoulder", "right_shoulder", "left_hip", "right_ankle"]
    assert [sorted(l) for l in sk.tolist()].count([13, 15]) == 1 and [sorted(l) for l in sk.tolist()].count([5, 6]) == 1
    assert overlay.PALETTE.dtype == np.uint8 and overlay.PALETTE.shape[1] == 3 and len({tuple(c) for c in overlay.PALETTE.tolist()}) == len(overlay.PALETTE)
    assert (overlay.STATUS_SKIPPED, overlay.STATUS_GUARD, overlay.STATUS_FRAME) == (OR.STATUS_SKIPPED, OR.STATUS_GUARD, OR.STATUS_FRAME)


def test_axis_rotation_is_the_formula_to_the_bit():
    c = math.cos(math.radians(270))
    want = np.array([[c, 0, -1], [0, 1, 0], [1, 0, c]], dtype=np.float64)
    got = render.axis_rotation(270, (0, 1, 0))
    assert got.dtype == np.float64 and got.shape == (3, 3) and got.tobytes() == want.tobytes()
    assert render.axis_rotation(270, (0, 5, 0)).tobytes() == want.tobytes()     # the axis is normalised
    for angle, axis in ((33.0, (1, 2, 3)), (-120, (0.3, -0.2, 0.9)), (90, (1, 0, 0))):
        R = render.axis_rotation(angle, axis)
        n = np.asarray(axis, float) / np.linalg.norm(axis)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(R @ n, n, atol=1e-15)
        assert np.isclose(np.trace(R), 1 + 2 * math.cos(math.radians(angle)))
    assert np.allclose(render.axis_rotation(90, (0, 0, 1)) @ [1, 0, 0], [0, 1, 0], atol=1e-15)           # counter-clockwise about the axis
    for bad in ((270, (0, 0, 0)), (float("nan"), (0, 1, 0)), (270, (0, 1))):
        with pytest.raises(_lib.PmceError, match="axis"):
            render.axis_rotation(*bad)


def test_symbols_prototyped_and_built():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_draw_overlays", 28), ("pmce_overlay_workspace_bytes", 3)):
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "overlay.hip" in build.SOURCES and build.FILE_FLAGS["overlay.hip"] == build.NO_PACKED_FP32
    hpp = open(osp.join(REPO, "pmce_amd", "csrc", "overlay_cover.hpp")).read()
    assert "__int128" in hpp and re.search(r"constexpr double GUARD_PX = %d\.0;" % overlay.GUARD_PX, hpp)
    assert '#include "overlay_cover.hpp"' in open(osp.join(REPO, "pmce_amd", "csrc", "overlay.hip")).read()
    assert lib.pmce_overlay_workspace_bytes(1920, 1080, 3) == 3 * 1920 * 1080 * 4
    assert lib.pmce_overlay_workspace_bytes(0, 8, 1) == 0 and lib.pmce_overlay_workspace_bytes(8, 8193, 1) == 0
    assert lib.pmce_overlay_workspace_bytes(8, 8, 0) == 0 and "chunk_frames" in _lib.last_error()


def test_entry_point_rejects_bad_arguments_on_the_host():
    """PMCE_ERR_ARG before anything is launched: the pointers are never followed."""
    import ctypes as C
    lib = _lib.load()
    p = C.c_void_p(4096)
    tc = (C.c_ubyte * 3)(255, 255, 255)

    def call(frames=p, F=2, W=40, H=24, fmt=1, K=17, D=3, L=19, thresh=0.3, t=2, r=3, s=2, npal=12, alpha=255, N=5, wsb=1 << 20, fi=None):
        host = None if fi is None else (C.c_int * len(fi))(*fi)
        return lib.pmce_draw_overlays(frames, F, W, H, host, p, p, fmt, p, p, K, D, p, L, thresh, t, r, s, p, p, npal, tc, alpha, N, p, p, wsb, None)

    for kw, word in ((dict(W=0), "width"), (dict(H=8193), "width"), (dict(F=-1), "negative"), (dict(N=-1), "negative"), (dict(fmt=3), "box_format"),
                     (dict(t=0), "thickness"), (dict(t=65), "thickness"), (dict(r=0), "radius"), (dict(r=65), "radius"),
                     (dict(s=0), "label_scale"), (dict(alpha=256), "alpha"), (dict(alpha=-1), "alpha"), (dict(npal=0), "palette"),
                     (dict(K=0), "keypoints"), (dict(D=4), "keypoints"), (dict(L=-1), "keypoints"), (dict(thresh=float("nan")), "score_thresh"),
                     (dict(F=0), "no frame"), (dict(frames=None), "null pointer")):
        assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(wsb=40 * 24 * 4 - 1) == -3 and "workspace" in _lib.last_error()
    for fi in ([0, 0, 1, 0, 1], [0, 0, 1, 1, 2], [-1, 0, 0, 1, 1]):                # the host table: ascending and inside the frames
        assert call(fi=fi) == -1 and "frame_index_host must be ascending" in _lib.last_error(), fi
    assert call(N=0, frames=None) == 0                                      # nothing to draw: nothing is looked at


def test_save_results_round_trips_through_pickle(tmp_path):
    rng = np.random.default_rng(5)
    outs = [{"person_id": 7, "pred_cam": torch.from_numpy(rng.normal(size=(3, 3)).astype(np.float32)),
             "mesh": torch.from_numpy(rng.normal(size=(3, 4, 3)).astype(np.float32)), "bboxes": torch.from_numpy(rng.normal(size=(3, 4)).astype(np.float32)),
             "frame_ids": np.array([4, 5, 6]), "orig_cam": torch.zeros(3, 4), "loss": torch.zeros(3)},
            {"person_id": 2, "pred_cam": torch.zeros(1, 3), "mesh": torch.ones(1, 4, 3), "bboxes": torch.zeros(1, 4), "frame_ids": np.array([0])}]
    path = tmp_path / "deep" / "pmce_output.pkl"
    wrote = demo.save_results(str(path), outs)
    with open(path, "rb") as fh:
        got = pickle.load(fh)
    assert list(got) == [7, 2] and set(got[7]) == {"pred_cam", "mesh", "bboxes", "frame_ids"}                # the reference's keys
    for pid, o in ((7, outs[0]), (2, outs[1])):
        for key in got[pid]:
            assert isinstance(got[pid][key], np.ndarray) and np.array_equal(got[pid][key], np.asarray(o[key])) and \
                np.array_equal(wrote[pid][key], got[pid][key]), (pid, key)
        assert got[pid]["mesh"].dtype == np.float32
    assert set(demo.save_results(str(path), {9: outs[1]})) == {2}           # 'person_id' names the person; a dict's key only stands in
    assert set(demo.save_results(str(path), {9: {k: v for k, v in outs[1].items() if k != "person_id"}})) == {9}
    with pytest.raises(ValueError, match="person ids repeat"):
        demo.save_results(str(path), [outs[0], outs[0]])


def test_save_meshes_writes_the_flipped_vertices_and_one_based_faces(tmp_path):
    verts = np.array([[[0.0, 0.5, 1.0], [1.25, -2.0, 3.0], [-0.1, 0.2, -0.3], [4.0, 5.0, 6.0]],
                      [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [1e-9, -1e-9, 0.0]]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    outs = [{"person_id": 12, "mesh": torch.from_numpy(verts), "frame_ids": np.array([3, 41])}]
    paths = demo.save_meshes(str(tmp_path), outs, faces)
    assert paths == [str(tmp_path / "meshes" / "0012" / "000003.obj"), str(tmp_path / "meshes" / "0012" / "000041.obj")]
    text = open(paths[0]).read()
    assert text == ("v 0.00000000 -0.50000000 -1.00000000\nv 1.25000000 2.00000000 -3.00000000\n"
                    "v %.8f %.8f %.8f\nv 4.00000000 -5.00000000 -6.00000000\nf 1 2 3\nf 3 2 4\n"
                    % (float(np.float32(-0.1)), -float(np.float32(0.2)), float(np.float32(0.3))))
    rows = [l.split() for l in open(paths[1]).read().splitlines()]
    assert [r[0] for r in rows] == ["v"] * 4 + ["f"] * 2 and [float(v) for v in rows[1][1:]] == [2.0, -2.0, -2.0]
    with pytest.raises(ValueError, match="faces index vertex 4"):
        demo.save_meshes(str(tmp_path), outs, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError, match=r"faces must be an integer array \[F, 3\]"):
        demo.save_meshes(str(tmp_path), outs, np.zeros((2, 4), np.int32))


def test_new_keywords_are_refused_without_a_gpu(tmp_path, monkeypatch):
    def no_work(*a, **kw):
        raise AssertionError("work was started before the refusal")

    for name in ("load_frames", "run_frames", "run_folder_in_passes", "iter_frames", "save_frames"):
        monkeypatch.setattr(demo, name, no_work)
    out, again, dbg = (str(tmp_path / n) for n in ("out", "in", "dbg"))
    for kw, word in ((dict(debug_folder=out), "debug_folder and out_folder are the same folder"),
                     (dict(input_folder=again, debug_folder=again), "debug_folder and input_folder are the same folder"),
                     (dict(input_folder=out), "input_folder and out_folder are the same folder"),
                     (dict(input_folder=osp.join(out, "..", "out")), "the same folder"),
                     (dict(sideview=1), "sideview must be True or False"), (dict(plain="yes"), "plain must be True or False"),
                     (dict(overlay_kwargs=dict(thickness=3)), "give debug_folder"),
                     (dict(obj_folder=dbg, renderer=None), "obj_folder needs the mesh's faces")):
        for passes in ({}, dict(frames_per_pass=7)):
            args = dict(dict(renderer="R"), **kw, **passes)
            with pytest.raises(ValueError, match=word):
                demo.render_folder("M", "frames", out, "T", "P", "E", **args)
    # render_tracklets: a result twice as wide cannot be written into the frames
    frames = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="inplace=True cannot be combined with sideview=True .* twice as wide"):
        demo.render_tracklets([], frames, (32, 24), renderer=np.array([[0, 1, 2]]), inplace=True, sideview=True)
    with pytest.raises(ValueError, match="plain must be True or False"):
        demo.render_tracklets([], frames, (32, 24), renderer=np.array([[0, 1, 2]]), plain=None)
    # without a person the views are still made (host tensors: no GPU)
    frames += 9
    wide = demo.render_tracklets([], frames, (32, 24), renderer=np.array([[0, 1, 2]]), sideview=True)
    assert tuple(wide.shape) == (2, 24, 64, 3) and torch.equal(wide[:, :, :32], frames) and not wide[:, :, 32:].any()
    assert not demo.render_tracklets([], frames, (32, 24), renderer=np.array([[0, 1, 2]]), plain=True).any() and frames.all()
    # draw_tracklets names what it misses
    with pytest.raises(ValueError, match="keep_inputs=True"):
        demo.draw_tracklets([{"mesh": torch.zeros(1, 4, 3), "bboxes": torch.zeros(1, 4)}], frames)


def test_wiring_of_the_new_keywords(monkeypatch):
    """The whole-video route with every switch on, on stand-ins: who is called with what, and in which order the folders are written."""
    calls, saved = {}, []
    monkeypatch.setattr(demo, "load_frames", lambda folder, device=None, strict=True, chunk=32: ("FRAMES", (64, 48), ["a.jpg"]))
    monkeypatch.setattr(demo, "run_frames", lambda *a, **kw: calls.setdefault("run", kw) and [{"person_id": 3}])
    monkeypatch.setattr(demo, "render_tracklets", lambda outs, fr, wh, **kw: calls.setdefault("render", kw) and "RENDERED")
    monkeypatch.setattr(demo, "draw_tracklets", lambda outs, fr, **kw: calls.setdefault("draw", (outs, fr, kw)) and ("DEBUG", "STATUS"))
    monkeypatch.setattr(demo, "save_frames", lambda folder, fr, **kw: saved.append((folder, fr)))
    monkeypatch.setattr(demo, "save_meshes", lambda folder, outs, faces: calls.setdefault("obj", (folder, outs, faces)))
    monkeypatch.setattr(demo, "save_results", lambda path, outs: calls.setdefault("pkl", (path, outs)))
    faces = np.array([[0, 1, 2]], np.int32)
    demo.render_folder("M", "frames", "out", "T", "P", "E", faces, input_folder="in", sideview=True, plain=True, debug_folder="dbg",
                       obj_folder="obj", pkl_path="x.pkl", overlay_kwargs=dict(thickness=3), min_frames=5)
    assert calls["run"] == dict(min_frames=5, keep_inputs=True)
    assert calls["render"] == dict(renderer=faces, order="reference", plain=True, sideview=True)
    assert calls["draw"] == ([{"person_id": 3}], "FRAMES", dict(thickness=3))
    assert saved == [("out", "RENDERED"), ("in", "FRAMES"), ("dbg", "DEBUG")]
    assert calls["obj"][0] == "obj" and calls["obj"][2] is faces and calls["pkl"] == ("x.pkl", [{"person_id": 3}])


def test_uploaded_tables_are_bounded():
    """A caller who varies palettes or skeletons does not pile up device tensors: the most recently used tables are kept, no more."""
    overlay._tables.clear()
    first = overlay._upload(overlay.FONT, "cpu")
    for k in range(3 * overlay.MAX_TABLES):
        overlay._upload(np.full((2, 3), k % 251, np.uint8), "cpu")
        assert overlay._upload(overlay.FONT, "cpu") is first                    # in use every call: never evicted
    assert len(overlay._tables) == overlay.MAX_TABLES
    overlay._tables.clear()
