"""The JPEG reader, the parts that need no GPU: the numpy restatement (tests/jpeg_ref.py) against Pillow's recorded pixels
(tests/golden/jpeg.npz, made by tests/golden/make_golden_jpeg.py), the host parser's records and refusals, ``demo.load_frames``' folder
rules, the C interface, and the entropy decoder's body run on the host over intact, shortened and damaged streams
(scripts/jpeg_entropy_host.cpp)."""
import ctypes as C
import os.path as osp
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref as JR
from pmce_amd import _lib, build, demo, jpeg

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = np.load(osp.join(REPO, "tests", "golden", "jpeg.npz"))
ACCEPTED = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "j0", "j1", "j2", "j3", "j4", "t", "m", "m2"]
# (width, height, components, h, v, restart interval, segments)
EXPECTED = {"a": (16, 16, 3, 2, 2, 0, 1), "b": (8, 8, 3, 1, 1, 0, 1), "c": (17, 13, 3, 2, 2, 0, 1), "d": (64, 40, 3, 2, 2, 1, 12),
            "e": (48, 40, 3, 2, 2, 3, 3), "f": (33, 9, 3, 2, 1, 0, 1), "g": (24, 24, 3, 2, 2, 0, 1), "h": (45, 31, 3, 2, 2, 0, 1),
            "i": (9, 17, 1, 1, 1, 0, 1), "j0": (64, 48, 3, 2, 2, 4, 3), "j1": (64, 48, 3, 2, 2, 0, 1), "t": (300, 40, 3, 2, 2, 0, 1)}


def file(name):
    return bytes(GOLD[f"file_{name}"])


def golden_rgb(name):
    px = GOLD[f"pixels_{name}"]
    return np.repeat(px[..., None], 3, axis=2) if px.ndim == 2 else px


def test_golden_file_is_small_and_records_its_library():
    assert osp.getsize(osp.join(REPO, "tests", "golden", "jpeg.npz")) < 200 * 1024
    versions = [str(v) for v in GOLD["versions"]]
    assert len(versions) == 3 and versions[2] == "True", versions        # libjpeg-turbo, the library behind cv2.imread too
    assert {f"file_{n}" for n in ACCEPTED + ["k", "l"]} <= set(GOLD.files)


@pytest.mark.parametrize("name", ACCEPTED)
def test_restatement_equals_pillow_to_the_bit(name):
    rgb, status = JR.decode(file(name))
    want = golden_rgb(name)
    assert status == 0 and rgb.shape == want.shape
    assert int((rgb != want).sum()) == 0


def test_parser_records():
    for name, want in EXPECTED.items():
        h = jpeg.parse(file(name), name)
        assert (h.width, h.height, h.ncomp, h.h, h.v, h.restart_interval, len(h.segments)) == want, name
        assert h.mcus_x == -(-h.width // (8 * h.h)) and h.mcus_y == -(-h.height // (8 * h.v))
        assert h.blocks_per_mcu == (1 if h.ncomp == 1 else h.h * h.v + 2)
        assert len(h.quant) == len(h.dc) == len(h.ac) == h.ncomp and all(q.shape == (64,) and q.dtype == np.uint16 for q in h.quant)
        # the same geometry and tables as the restatement's own parser reads
        m = JR.geometry(JR.read_markers(file(name)))
        assert (m["mcus_x"], m["mcus_y"], m["scan_begin"]) == (h.mcus_x, h.mcus_y, h.scan_begin)
        for c, (ci, td, ta) in enumerate(m["scan"]):
            q = np.zeros(64, dtype=np.int64)
            q[JR.ZIGZAG] = h.quant[c]
            assert np.array_equal(q, m["quant"][m["comps"][ci][3]])
            assert (list(h.dc[c][0]), list(h.dc[c][1])) == m["huff"][(0, td)] and (list(h.ac[c][0]), list(h.ac[c][1])) == m["huff"][(1, ta)]


@pytest.mark.parametrize("name", ["d", "e"])
def test_parser_segments_start_after_rst_and_end_at_the_next_marker(name):
    data = file(name)
    h = jpeg.parse(data, name)
    seg = h.segments
    n_mcu = h.mcus_x * h.mcus_y
    assert seg.shape == (-(-n_mcu // h.restart_interval), 4)
    assert seg[0, 0] == h.scan_begin and data[h.scan_begin - 3:h.scan_begin] == b"\x00\x3f\x00"
    for k in range(len(seg)):
        b, e, mcu0, count = (int(v) for v in seg[k])
        assert (mcu0, count) == (k * h.restart_interval, min(h.restart_interval, n_mcu - k * h.restart_interval))
        if k:
            assert data[b - 2] == 0xFF and data[b - 1] == 0xD0 + ((k - 1) & 7) and b - 2 == seg[k - 1, 1]     # RST7 wraps to RST0
        assert data[e] == 0xFF and data[e + 1] == (0xD9 if k == len(seg) - 1 else 0xD0 + (k & 7))
        body = data[b:e]
        assert all(body[i + 1] == 0 for i in range(len(body) - 1) if body[i] == 0xFF) and body[-1] != 0xFF       # no marker inside
    assert h.scan_end == int(seg[-1, 1]) and data[h.scan_end:h.scan_end + 2] == b"\xff\xd9"
    if name == "d":
        assert len(seg) == 12 and data[int(seg[8, 0]) - 1] == 0xD7 and data[int(seg[9, 0]) - 1] == 0xD0
    # the segments are those of the restatement's byte-by-byte walk
    m = JR.geometry(JR.read_markers(data))
    assert [tuple(int(v) for v in s) for s in seg] == JR.scan_segments(data, m)
    # stuffed bytes occur (e: up to 22 in its scan)
    assert data[h.scan_begin:h.scan_end].count(b"\xff\x00") >= (20 if name == "e" else 1)


def _find(data, marker):
    i = 2
    while True:
        assert data[i] == 0xFF
        L = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == marker:
            return i, L
        i += 2 + L


def test_refusals_name_the_file_and_the_reason():
    def refused(data, *words):
        with pytest.raises(ValueError) as e:
            jpeg.parse(bytes(data), "clip/000007.jpg")
        msg = str(e.value)
        assert msg.startswith("clip/000007.jpg: ") and all(w in msg for w in words), msg

    refused(file("k"), "progressive")
    refused(file("l"), "4 components")
    a = bytearray(file("a"))
    sof, _ = _find(a, 0xC0)
    d = bytearray(a)
    d[sof + 4] = 12
    refused(d, "12-bit")
    d = bytearray(a)
    d[sof + 4 + 7] = 0x41                                   # luma sampling 4x1
    refused(d, "sampling", "4x1")
    d = bytearray(a)
    d[sof + 5:sof + 7] = b"\x00\x00"
    refused(d, "width or height")
    d = bytearray(a)
    d[sof + 5:sof + 7] = (16385).to_bytes(2, "big")
    refused(d, "16384")
    dqt, L = _find(a, 0xDB)
    d = bytearray(a)
    d[dqt + 4] |= 0x10                                      # Pq = 1
    refused(d, "16-bit quantisation")
    sos, L = _find(a, 0xDA)
    refused(a[:sos], "ends before SOS")
    refused(a[:sos + 6], "ends before SOS")                 # cut inside the SOS segment
    refused(a[:2], "ends before SOS")
    d = bytearray(a[:-2]) + a[sos:sos + 2 + L] + b"\x12\x34\xff\xd9"          # a second SOS in front of EOI
    refused(d, "more than one SOS")
    d = bytearray(a[:-2]) + b"\xff\xdc\x00\x04\x00\x10\xff\xd9"
    refused(d, "DNL")
    d = bytearray(a)
    d[sos + 4 + 2] = 0x30                                   # the first component's DC table 3: never defined
    refused(d, "Huffman table", "not defined")
    d = bytearray(a)
    d[sof + 4 + 8] = 3                                      # its quantisation table 3
    refused(d, "quantisation table 3", "not defined")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"             # transform 0 on a three-component file: RGB
    refused(a[:2] + adobe + a[2:], "Adobe", "transform 0")
    jpeg.parse(bytes(a[:2] + adobe[:-1] + b"\x01" + a[2:]), "ok")           # transform 1 is YCbCr
    refused(b"\x89PNG\r\n\x1a\n" + bytes(32), "not a JPEG")
    # APPn, COM and fill bytes in front of a marker are skipped
    d = a[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe5\x00\x04xy" + b"\xff\xff\xff" + a[3:]
    assert jpeg.parse(bytes(d), "ok").scan_begin == jpeg.parse(bytes(a), "ok").scan_begin + 5 + 2 + 4 + 2 + 2


def test_truncated_file_parses_and_its_missing_intervals_are_empty():
    data = file("e")
    h = jpeg.parse(data, "e")
    cut = data[:(h.scan_begin + h.scan_end) // 2]
    hc = jpeg.parse(cut, "e-cut")
    assert len(hc.segments) == 3 and hc.scan_end == len(cut)
    assert np.array_equal(hc.segments[0], h.segments[0]) and hc.segments[1, 0] == h.segments[1, 0] and hc.segments[1, 1] == len(cut)
    assert hc.segments[2, 0] == hc.segments[2, 1]           # the third interval never came: the device reports it as truncated
    rgb, status = JR.decode(cut)
    assert status & JR.STATUS_TRUNCATED


def test_huffman_record_layout():
    counts, values = JR.K_AC_LUMA
    rec = jpeg.huffman_record(counts, bytes(values))
    assert rec.shape == (jpeg.HUFF_WORDS,) and rec.dtype == np.int32
    codes = JR._Huff(counts, values).codes                  # (length, code) -> value
    for (length, code), value in codes.items():
        assert code <= rec[jpeg.HUFF_MAXCODE + length] and rec[jpeg.HUFF_VALUES + code + rec[jpeg.HUFF_VALOFF + length]] == value
        if length <= 8:
            lo = code << (8 - length)
            assert (rec[jpeg.HUFF_LOOK + lo:jpeg.HUFF_LOOK + lo + (1 << (8 - length))] == ((length << 8) | value)).all()
    long_prefixes = {code >> (length - 8) for (length, code) in codes if length > 8}
    assert all(rec[jpeg.HUFF_LOOK + p] == 0 for p in long_prefixes) and rec[jpeg.HUFF_MAXCODE + 13] == -1
    with pytest.raises(ValueError):
        jpeg.huffman_record([3] + [0] * 15, bytes(3), "x")            # three codes of one bit


def test_batch_records():
    files = [file(n) for n in ("j0", "j1", "j2", "j3", "j4")]
    rec = jpeg.build_records(jpeg.parse_all(files), chunk=2)
    assert rec["images"].shape == (5, jpeg.IMG_WORDS) and rec["segments"].shape == (3 + 1 + 1 + 3 + 1, jpeg.SEG_WORDS)
    assert rec["data"].nbytes == sum(len(f) for f in files)
    blocks, planes = 4 * 3 * 6, 64 * 48 * 3 // 2
    assert [r[:6] for r in rec["rounds"]] == [[0, 2, 0, 4, 2 * blocks, 2 * planes], [2, 2, 4, 4, 2 * blocks, 2 * planes],
                                              [4, 1, 8, 1, blocks, planes]]
    assert list(rec["images"][:, 17]) == [0, blocks, 0, blocks, 0] and list(rec["images"][:, 19]) == [0, 3, 4, 5, 8]
    base = np.cumsum([0] + [len(f) for f in files])
    for s in rec["segments"]:
        assert base[s[0]] <= s[1] <= s[2] <= base[s[0] + 1]
    # the standard tables are stored once for the whole batch
    assert len(rec["huffman"]) == 4 and len(rec["quant"]) <= 6
    with pytest.raises(ValueError, match="file 1: 48 x 40"):
        jpeg.parse_all([file("d"), file("e")])
    with pytest.raises(ValueError):
        jpeg.parse_all([])


def test_encoder_files_decode_without_a_status_bit():
    """The restatement's own encoder (the benchmark's source of files where no JPEG library is installed).  Its files need match
    nothing but the restatement's decode of them; the decode must be clean and near the source image (a loose sanity bound: a smooth
    image at quality 90 stays within a few grey levels on average)."""
    y, x = np.mgrid[0:20, 0:36]
    img = np.stack([4 * x + 40, 6 * y + 60, 255 - 3 * x - 2 * y], -1).astype(np.uint8)
    for subsampling, ri in (("420", 0), ("420", 2), ("444", 0), ("grey", 3)):
        data = JR.encode(img, quality=90, subsampling=subsampling, restart_interval=ri)
        h = jpeg.parse(data, "enc")
        assert (h.width, h.height, h.restart_interval) == (36, 20, ri) and h.ncomp == (1 if subsampling == "grey" else 3)
        if ri:
            assert len(h.segments) == -(-h.mcus_x * h.mcus_y // ri) > 1
        rgb, status = JR.decode(data)
        assert status == 0 and rgb.shape == img.shape
        want = np.repeat(img[..., :1], 3, axis=2) if subsampling == "grey" else img
        assert np.abs(rgb.astype(np.int64) - want).mean() < 4.0


def test_symbols_prototyped_and_built_without_packed_fp32():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_jpeg_entropy", 15), ("pmce_jpeg_idct", 11), ("pmce_jpeg_colour", 13)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "jpeg.hip" in build.SOURCES and build.FILE_FLAGS["jpeg.hip"] == build.NO_PACKED_FP32
    # the layout constants are written once per language and agree
    hpp = open(osp.join(REPO, "pmce_amd", "csrc", "jpeg_entropy.hpp")).read()
    for cname, value in (("IMG_WORDS", jpeg.IMG_WORDS), ("SEG_WORDS", jpeg.SEG_WORDS), ("HUFF_WORDS", jpeg.HUFF_WORDS)):
        assert re.search(r"constexpr int %s = %d;" % (cname, value), hpp), cname
    assert "HUFF_MAXCODE = 0, HUFF_VALOFF = 17, HUFF_VALUES = 34, HUFF_LOOK = 290" in hpp
    assert "STATUS_TRUNCATED = 1, STATUS_CORRUPT = 2, STATUS_RECORD = 4" in hpp
    assert (jpeg.STATUS_TRUNCATED, jpeg.STATUS_CORRUPT, jpeg.STATUS_RECORD) == (1, 2, 4)


def test_entry_points_reject_bad_arguments_on_the_host():
    """The argument checks return PMCE_ERR_ARG before anything is launched: no GPU is touched (the pointers are never followed)."""
    lib = _lib.load()
    p = C.c_void_p(4096)
    ent = lambda data=p, nbytes=100, nseg=3, nimg=2, nhuf=4, nblk=24, first=0, lanes=0: lib.pmce_jpeg_entropy(     # noqa: E731
        data, nbytes, p, first, nseg, p, nimg, p, nhuf, p, nblk, p, 1, lanes, None)
    assert ent(data=None) == -1 and "null pointer" in _lib.last_error()
    assert ent(nbytes=0) == -1 and ent(nbytes=2 ** 31 - 128) == -1 and "2^31" in _lib.last_error()
    assert ent(lanes=-1) == -1 and ent(lanes=65) == -1 and "lanes" in _lib.last_error()
    assert ent(nseg=0) == -1 and ent(nimg=0) == -1 and ent(nhuf=0) == -1 and ent(first=-1) == -1 and ent(nblk=0) == -1
    idct = lambda coef=p, first=0, n=2, mb=24, nq=2, nblk=48, pb=4096: lib.pmce_jpeg_idct(coef, p, first, n, mb, p, nq, nblk, p, pb, None)  # noqa: E731
    assert idct(coef=None) == -1 and idct(first=-1) == -1 and idct(n=0) == -1 and idct(n=65536) == -1 and idct(mb=0) == -1
    assert idct(nq=0) == -1 and idct(nblk=0) == -1 and idct(pb=0) == -1
    col = lambda planes=p, pb=4096, first=0, n=2, nseg=3, w=16, h=16: lib.pmce_jpeg_colour(planes, pb, p, first, n, p, nseg, w, h, 0, p, p, None)  # noqa: E731
    assert col(planes=None) == -1 and col(pb=0) == -1 and col(first=-1) == -1 and col(n=0) == -1 and col(nseg=0) == -1
    assert col(w=0) == -1 and col(h=16385) == -1 and "16384" in _lib.last_error()


def test_decode_argument_errors_come_before_the_gpu():
    files = [file("j0"), file("j1")]
    with pytest.raises(ValueError, match="channel_order"):
        jpeg.decode(files, channel_order="gbr")
    with pytest.raises(ValueError, match="chunk"):
        jpeg.decode(files, chunk=0)
    with pytest.raises(ValueError, match="lanes"):
        jpeg.decode(files, lanes=65)
    with pytest.raises(ValueError, match="first.jpg is 64 x 48"):
        jpeg.decode([file("j0"), file("a")], names=["first.jpg", "second.jpg"])
    with pytest.raises(ValueError, match="no files"):
        jpeg.decode([])
    with pytest.raises(ValueError, match="progressive"):
        jpeg.decode([file("j0"), file("k")])


def test_load_frames_folder_rules(tmp_path, monkeypatch):
    seen = {}

    def fake_decode(files, device=None, channel_order="bgr", names=None, chunk=32, **kw):
        jpeg.parse_all(files, names)                        # the size rule and the refusals, on the host
        seen.update(files=files, names=names, channel_order=channel_order, chunk=chunk)
        import torch
        return torch.zeros(len(files), 48, 64, 3, dtype=torch.uint8), torch.tensor([0, 0, jpeg.STATUS_TRUNCATED][:len(files)], dtype=torch.int32)

    monkeypatch.setattr(jpeg, "decode", fake_decode)
    folder = tmp_path / "frames"
    folder.mkdir()
    with pytest.raises(ValueError, match="no .jpg or .jpeg file"):
        demo.load_frames(str(folder))
    for fname, case in (("000010.jpg", "j1"), ("000002.JPG", "j0"), ("notes.txt", None), ("000003.jpeg", "j2")):
        (folder / fname).write_bytes(file(case) if case else b"hello")
    with pytest.raises(ValueError) as e:                    # the third file's status
        demo.load_frames(str(folder))
    assert "000010.jpg" in str(e.value) and "truncated" in str(e.value)
    frames, wh, names = demo.load_frames(str(folder), strict=False, chunk=7)
    assert seen["chunk"] == 7
    assert names == ["000002.JPG", "000003.jpeg", "000010.jpg"] and wh == (64, 48) and tuple(frames.shape) == (3, 48, 64, 3)
    assert seen["files"] == [file("j0"), file("j2"), file("j1")] and seen["channel_order"] == "bgr"
    assert names == sorted(names)                           # main/run_demo.py:386-390: sorted()
    (folder / "000004.jpg").write_bytes(file("a"))
    with pytest.raises(ValueError) as e:
        demo.load_frames(str(folder), strict=False)
    assert "000004.jpg" in str(e.value) and "16 x 16" in str(e.value)
    (folder / "000004.jpg").unlink()
    (folder / "000001.png").write_bytes(b"\x89PNG\r\n\x1a\n")
    with pytest.raises(ValueError) as e:
        demo.load_frames(str(folder))
    assert "PNG is not served" in str(e.value) and "000001.png" in str(e.value)


def test_run_folder_wiring(monkeypatch):
    calls = {}

    def fake_load(folder, device=None, strict=True, chunk=32):
        calls["load"] = (folder, device, strict, chunk)
        return "FRAMES", (64, 48), ["a.jpg"]

    def fake_run(model, frames, tracker, pose, extractor, img_wh, **kw):
        calls["run"] = (model, frames, tracker, pose, extractor, img_wh, kw)
        return [{"person_id": 3}]

    monkeypatch.setattr(demo, "load_frames", fake_load)
    monkeypatch.setattr(demo, "run_frames", fake_run)
    out = demo.run_folder("M", "some/folder", "T", "P", "E", strict=False, chunk=300, min_frames=5, extract_batch=64)
    assert out == [{"person_id": 3}]
    assert calls["load"] == ("some/folder", None, False, 300)
    assert calls["run"] == ("M", "FRAMES", "T", "P", "E", (64, 48), dict(min_frames=5, extract_batch=64))


def test_entropy_body_on_the_host(tmp_path):
    """scripts/jpeg_entropy_host.cpp, built with the host compiler (no sanitizer here), over the records of cases d, e and h: the
    intact streams give the restatement's coefficients, every shortened or bit-flipped stream ends with a status made of the known
    bits or a clean decode, nothing is written outside a segment's own blocks and the guards stay untouched - in the body's direct form and in the form the
    device runs."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "jpeg_entropy_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", osp.join(REPO, "pmce_amd", "csrc"), osp.join(REPO, "scripts", "jpeg_entropy_host.cpp"),
                    "-o", exe], check=True, capture_output=True)
    files = [file(n) for n in "deh"]
    coef = np.concatenate([JR.entropy_decode(f)[1] for f in files])
    rec = jpeg.dump_records(files, str(tmp_path / "records.bin"), coefficients=coef, names=list("deh"))
    assert coef.shape == (rec["rounds"][0][4], 64) and np.abs(coef).max() >= 128       # e: values of eight bits
    r = subprocess.run([exe, str(tmp_path / "records.bin"), "3000"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 2          # the body's direct form, and the device's (window and block scratch)
    for line, form in zip(lines, ("direct", "window and block scratch")):
        assert line.startswith("ok (%s): 16 segments; intact 16 runs, %d coefficients compared" % (form, coef.size)), line
        m = re.search(r"cut (\d+) runs \((\d+) flagged\); bit flips (\d+) runs", line)
        assert m and int(m.group(1)) == sum(int(s[2] - s[1]) for s in rec["segments"]) and int(m.group(2)) == int(m.group(1))
        assert int(m.group(3)) == 3000 and line.endswith("guards untouched")
    # a dump whose expected coefficients are wrong is caught (the comparison is live)
    coef[5, 0] += 1
    jpeg.dump_records(files, str(tmp_path / "wrong.bin"), coefficients=coef)
    r = subprocess.run([exe, str(tmp_path / "wrong.bin"), "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL intact" in r.stdout
