"""The JPEG writer, the parts that need no GPU: the numpy restatement (tests/jpeg_enc_ref.py) against Pillow's recorded files
(tests/golden/jpeg_enc.npz, made by tests/golden/make_golden_jpeg_enc.py), the host's header builder and quality tables, the argument
errors, the C interface, ``files`` / ``save_frames`` / ``render_folder``'s host side, and the entropy body run on the host over crafted
coefficients (scripts/jpeg_encode_host.cpp)."""
import ctypes as C
import os.path as osp
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import jpeg_enc_ref as ER
from pmce_amd import _lib, build, demo, jpeg

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = np.load(osp.join(REPO, "tests", "golden", "jpeg_enc.npz"))
SHARED = {"q50": "q1", "rrow": "r1", "r3": "r1", "r3n": "e"}
CASES = sorted(k[5:] for k in GOLD.files if k.startswith("file_"))
SUBSAMPLING = ("4:4:4", "4:2:2", "4:2:0")


def case(name):
    """-> (image uint8 [H, W, 3] R, G, B; Pillow's file; quality; subsampling; restart interval in MCUs)"""
    quality, sub, restart = (int(x) for x in GOLD[f"args_{name}"])
    return GOLD[f"image_{SHARED.get(name, name)}"], bytes(GOLD[f"file_{name}"]), quality, SUBSAMPLING[sub], restart


def test_golden_file_is_small_and_records_its_library():
    assert osp.getsize(osp.join(REPO, "tests", "golden", "jpeg_enc.npz")) < 200 * 1024
    versions = [str(v) for v in GOLD["versions"]]
    assert len(versions) == 3 and versions[2] == "True", versions        # libjpeg-turbo, the library behind cv2.imwrite too
    assert len(CASES) == 22 and all(f"args_{n}" in GOLD.files for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_pillow_to_the_byte(name):
    img, want, quality, sub, restart = case(name)
    got = ER.encode(img, quality, sub, restart)
    assert len(got) == len(want) and got == want


def test_restatement_equals_pillow_on_fresh_images():
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(2024)
    for k, (h, w, quality, sub, restart) in enumerate(((7, 9, 95, 2, 0), (33, 18, 50, 1, 0), (16, 47, 100, 0, 0), (50, 34, 30, 2, 2),
                                                       (23, 40, 75, 1, 3), (18, 16, 75, 2, 5), (21, 300, 80, 0, 7), (21, 300, 80, 1, 7))):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 2 else np.clip(
            np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[..., None] + rng.integers(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=sub, **(dict(restart_marker_blocks=restart) if restart else {}))
        assert ER.encode(img, quality, SUBSAMPLING[sub], restart) == b.getvalue(), (h, w, quality, sub, restart)


@pytest.mark.parametrize("name", CASES)
def test_header_equals_pillow(name):
    img, want, quality, sub, restart = case(name)
    begin = jpeg.parse(want, name).scan_begin
    got = jpeg.encode_header(img.shape[1], img.shape[0], quality, sub, restart)
    assert got == want[:begin]
    assert (b"\xff\xdd" in got) == bool(restart) and got[-3:] == b"\x00\x3f\x00" and want[-2:] == b"\xff\xd9"
    # the reader's parser accepts what the writer's header says
    h = jpeg.parse(got + b"\xff\xd9", name)
    assert (h.width, h.height, h.restart_interval, (h.h, h.v)) == (img.shape[1], img.shape[0], restart, jpeg.SUBSAMPLINGS[sub])


def test_quality_tables():
    luma, chroma = jpeg.quant_tables(1)
    assert (luma == 255).all() and (chroma == 255).all()                   # 5000 % of the base table, clamped
    luma, chroma = jpeg.quant_tables(49)                                   # 5000 // 49 = 102 %
    assert list(luma[:8]) == [16, 11, 10, 16, 24, 41, 52, 62] and list(chroma[:4]) == [17, 18, 24, 48] and chroma[-1] == 101
    luma, chroma = jpeg.quant_tables(50)
    assert list(luma) == list(jpeg.K_LUMA_QUANT) and list(chroma) == list(jpeg.K_CHROMA_QUANT)
    luma, chroma = jpeg.quant_tables(100)
    assert (luma == 1).all() and (chroma == 1).all()
    for q in (1, 49, 50, 100):
        assert np.array_equal(jpeg.quant_tables(q)[0], ER.quant_table(ER.K_LUMA_Q, q))
        assert np.array_equal(jpeg.quant_tables(q)[1], ER.quant_table(ER.K_CHROMA_Q, q))
    for bad in (0, 101, 2.5, True):
        with pytest.raises(ValueError, match="quality"):
            jpeg.quant_tables(bad)


def test_encode_argument_errors_come_before_the_gpu():
    """Every refusal is raised on a host tensor: the device check is the last one."""
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for kw, word in ((dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(subsampling="4:1:1"), "subsampling"),
                     (dict(channel_order="gbr"), "channel_order"), (dict(restart_interval=-1), "restart_interval"),
                     (dict(restart_interval=65536), "restart_interval"), (dict(chunk=0), "chunk"), (dict(capacity=0), "capacity"),
                     (dict(return_coefficients=True, chunk=1), "one round")):
        with pytest.raises(ValueError, match=word):
            jpeg.encode(frames, **kw)
    for bad in (frames.float(), frames[0], frames[..., :2], frames[:0], np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8 tensor"):
            jpeg.encode(bad)
    with pytest.raises(ValueError, match="16384"):
        jpeg.encode_header(16385, 8, 95, "4:2:0", 0)
    with pytest.raises(ValueError, match="contiguous device tensor"):
        jpeg.encode(frames)
    with pytest.raises(ValueError, match="whole number of MCUs"):
        jpeg.encode_entropy(torch.zeros(1, 7, 64, dtype=torch.int16), 4, b"\xff\xd8")


def test_capacity_helper():
    hdr = len(jpeg.encode_header(1920, 1080, 95, "4:2:0", 0))
    assert hdr == 623
    assert jpeg.encode_capacity(1920, 1080) == hdr + 3 * 1920 * 1088 // 2 + 2           # 1.5 bytes per padded luma sample
    blocks = 120 * 68 * 6
    assert jpeg.encode_capacity(1920, 1080, worst_case=True) == hdr + 2 * blocks * 208 + 3
    assert jpeg.encode_capacity(1920, 1080, restart_interval=120, worst_case=True) == hdr + 6 + 2 * blocks * 208 + 3 * 68           # DRI is 6 bytes
    # no frame can exceed the worst case: the crafted blocks of nothing but 1023 come closest
    c = ER.crafted_coefficients()
    assert len(ER.entropy_code(c, 1, 0)) <= 2 * len(c) * jpeg.MAX_BLOCK_BYTES + 1
    assert jpeg.MAX_BLOCK_BYTES == ER.MAX_BLOCK_BYTES == -(-(9 + 11 + 63 * 26) // 8)
    assert max(np.diff(ER.unstuffed(c, 1)[1])) == 9 + 11 + 63 * 26


def test_files_reads_back_and_names_the_frame_that_did_not_fit():
    data = torch.tensor(list(b"abcdefgh"), dtype=torch.uint8)
    offsets = torch.tensor([0, 3, 3, 8], dtype=torch.int64)
    assert jpeg.files(data, offsets, torch.zeros(3, dtype=torch.int32)) == [b"abc", b"", b"defgh"]
    with pytest.raises(ValueError, match="frame 1"):
        jpeg.files(data, offsets, torch.tensor([0, jpeg.STATUS_CAPACITY, 0], dtype=torch.int32))


def test_symbols_prototyped_and_built_without_packed_fp32():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_jpeg_encode_coefficients", 12), ("pmce_jpeg_encode_entropy", 17), ("pmce_jpeg_encode_workspace_bytes", 4),
                         ("pmce_jpeg_encode_scan_pass", 0), ("pmce_jpeg_encode_stages", 0)):
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "jpeg_encode.hip" in build.SOURCES and build.FILE_FLAGS["jpeg_encode.hip"] == build.NO_PACKED_FP32
    hpp = open(osp.join(REPO, "pmce_amd", "csrc", "jpeg_encode.hpp")).read()
    assert re.search(r"constexpr int MAX_BLOCK_BYTES = %d;" % jpeg.MAX_BLOCK_BYTES, hpp)
    assert re.search(r"constexpr int PIECE = %d;" % jpeg.ENCODE_PIECE, hpp)
    assert re.search(r"constexpr int STATUS_CAPACITY = %d;" % jpeg.STATUS_CAPACITY, hpp)
    assert lib.pmce_jpeg_encode_stages() == len(jpeg.ENCODE_STAGES) and lib.pmce_jpeg_encode_scan_pass() == 1024
    # the workspace: the unstuffed stream's slots (208 bytes per block, whole pieces), then 12 bytes per block, 8 per interval, 12 per piece, 8 per frame
    assert lib.pmce_jpeg_encode_workspace_bytes(1, 1, 4, 0) == 1280 + 32 + 48 + 16 + 32 + 48 + 16
    slot = -(-120 * 68 * 6 * 208 // 256) * 256
    assert lib.pmce_jpeg_encode_workspace_bytes(2, 120 * 68, 4, 0) >= 2 * slot + 2 * 120 * 68 * 6 * 12
    assert lib.pmce_jpeg_encode_workspace_bytes(0, 1, 4, 0) == 0 and lib.pmce_jpeg_encode_workspace_bytes(1, 1, 3, 0) == 0


def test_entry_points_reject_bad_arguments_on_the_host():
    """The argument checks return PMCE_ERR_ARG before anything is launched: no GPU is touched (the pointers are never followed)."""
    lib = _lib.load()
    p = C.c_void_p(4096)
    coef = lambda frames=p, first=0, n=1, w=16, h=16, hs=2, vs=2, nblk=6: lib.pmce_jpeg_encode_coefficients(       # noqa: E731
        frames, first, n, w, h, hs, vs, 0, p, p, nblk, None)
    assert coef(frames=None) == -1 and "null pointer" in _lib.last_error()
    assert coef(first=-1) == -1 and coef(n=0) == -1 and coef(n=65536) == -1 and coef(w=0) == -1 and coef(h=16385) == -1
    assert coef(hs=1, vs=2) == -1 and "sampling" in _lib.last_error()
    assert coef(nblk=5) == -1 and "blocks" in _lib.last_error()
    ent = lambda c=p, n=1, mcus=1, luma=4, ri=0, hb=623, cap=4096, wsb=1 << 20, first=0, stage=-1: lib.pmce_jpeg_encode_entropy(   # noqa: E731
        c, n, mcus, luma, ri, p, hb, cap, p, wsb, p, 4096, p, p, first, stage, None)
    assert ent(c=None) == -1 and ent(n=0) == -1 and ent(mcus=0) == -1 and ent(luma=3) == -1 and ent(ri=-1) == -1 and ent(ri=65536) == -1
    assert ent(hb=1) == -1 and ent(cap=-1) == -1 and ent(first=-1) == -1 and ent(stage=7) == -1 and ent(stage=-2) == -1
    assert ent(wsb=64) == -3 and "workspace" in _lib.last_error()


def test_save_frames_names_and_render_folder_wiring(tmp_path, monkeypatch):
    seen = []

    def fake_encode(frames, **kw):
        seen.append((frames, kw))
        return "DATA", "OFFSETS", "STATUS"

    monkeypatch.setattr(jpeg, "encode", fake_encode)
    monkeypatch.setattr(jpeg, "files", lambda d, o, s: [b"one", b"two", b"three"] if (d, o, s) == ("DATA", "OFFSETS", "STATUS") else None)
    frames = torch.zeros(3, 4, 4, 3, dtype=torch.uint8)
    out = tmp_path / "a" / "b"
    assert demo.save_frames(str(out), frames, quality=80) == ["000000.jpg", "000001.jpg", "000002.jpg"]
    assert seen[-1][1] == dict(quality=80) and (out / "000002.jpg").read_bytes() == b"three"
    assert demo.save_frames(str(out), frames, first=41) == ["000041.jpg", "000042.jpg", "000043.jpg"]       # the reference's %06d
    assert demo.save_frames(str(out), frames, names=["x.jpg", "y.jpg", "z.jpg"]) == ["x.jpg", "y.jpg", "z.jpg"]
    assert (out / "y.jpg").read_bytes() == b"two"
    with pytest.raises(ValueError, match="3 frames but 2 names"):
        demo.save_frames(str(out), frames, names=["x.jpg", "y.jpg"])

    calls = {}
    monkeypatch.setattr(demo, "load_frames", lambda folder, device=None, strict=True, chunk=32: calls.setdefault(
        "load", (folder, device, strict, chunk)) and ("FRAMES", (64, 48), ["a.jpg"]))
    monkeypatch.setattr(demo, "run_frames", lambda *a, **kw: calls.setdefault("run", (a, kw)) and [{"person_id": 3}])
    monkeypatch.setattr(demo, "render_tracklets", lambda outs, fr, wh, renderer=None, order="reference": calls.setdefault(
        "render", (outs, fr, wh, renderer, order)) and "RENDERED")
    saved = []
    monkeypatch.setattr(demo, "save_frames", lambda folder, fr, **kw: saved.append((folder, fr, kw)))
    got = demo.render_folder("M", "in", "out", "T", "P", "E", "R", input_folder="again", strict=False, chunk=9, min_frames=5,
                             encode_kwargs=dict(quality=90))
    assert got == [{"person_id": 3}]
    assert calls["load"] == ("in", None, False, 9)
    assert calls["run"] == (("M", "FRAMES", "T", "P", "E", (64, 48)), dict(min_frames=5))
    assert calls["render"] == ([{"person_id": 3}], "FRAMES", (64, 48), "R", "reference")
    assert saved == [("out", "RENDERED", dict(quality=90)), ("again", "FRAMES", dict(quality=90))]
    saved.clear()
    demo.render_folder("M", "in", "out", "T", "P", "E", "R")
    assert saved == [("out", "RENDERED", {})]


def dump_case(path, coef, luma, restart, expected):
    with open(path, "wb") as fh:
        fh.write(b"PMCEJENC" + struct.pack("<4q", len(coef), luma, restart, len(expected)))
        fh.write(np.ascontiguousarray(coef, dtype="<i2").tobytes() + bytes(expected))


def test_entropy_body_on_the_host(tmp_path):
    """scripts/jpeg_encode_host.cpp, built with the host compiler (no sanitizer here), over the crafted coefficients and the
    coefficients of three golden cases: the shared body, run lane by lane and in reverse order, gives the restatement's scan; the
    guards around every interval's slot stay untouched; a wrong expectation makes it exit 1."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "jpeg_encode_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", osp.join(REPO, "pmce_amd", "csrc"), osp.join(REPO, "scripts", "jpeg_encode_host.cpp"),
                    "-o", exe], check=True, capture_output=True)
    crafted = ER.crafted_coefficients()
    runs = [("crafted", crafted, 1, 0), ("crafted, 2 MCUs per interval", crafted, 1, 2), ("crafted, 1 MCU per interval", crafted, 1, 1)]
    for name in ("e", "r3", "f"):
        img, _, quality, sub, restart = case(name)
        coef, g = ER.coefficients(img, quality, sub)
        runs.append((name, coef, g["h"] * g["v"], restart))
    for what, coef, luma, restart in runs:
        want = ER.entropy_code(coef, luma, restart)
        path = str(tmp_path / "case.bin")
        dump_case(path, coef, luma, restart, want)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        print(what, r.stdout, r.stderr)
        assert r.returncode == 0 and r.stdout.startswith(f"ok: {len(coef)} blocks in "), what
        assert f"{len(want)} bytes compared" in r.stdout and r.stdout.rstrip().endswith("guards untouched")
        assert "reciprocal exact for %d pairs" % (255 * 65536) in r.stdout
    # the crafted stream has 0xFF bytes at every place in a word, at the borders of the stuffing stage's pieces and across block borders
    stream, starts = ER.unstuffed(crafted, 1)
    ff = [i for i, b in enumerate(stream) if b == 0xFF]
    assert {i % 4 for i in ff} == {0, 1, 2, 3} and {i % jpeg.ENCODE_PIECE for i in ff} >= {0, jpeg.ENCODE_PIECE - 1}
    across = [s for s in starts[1:-1] if s % 8 and stream[s // 8] == 0xFF]
    assert len(across) >= 3 and any((s // 8) % 4 in (0, 3) for s in across)
    # a wrong expectation is caught (the comparison is live)
    want = bytearray(ER.entropy_code(crafted, 1, 0))
    want[100] ^= 1
    dump_case(path, crafted, 1, 0, want)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL the scan's bytes differ" in r.stdout
