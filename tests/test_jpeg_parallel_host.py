"""The parallel entropy stage of the JPEG reader, the parts that need no GPU: its body (csrc/jpeg_parallel.hpp) emulated on the host
against the serial body on intact, shortened and damaged streams (scripts/jpeg_parallel_host.cpp), the subsequence records, the
arguments of ``jpeg.decode`` and of the C entry, and the demo's wiring."""
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
PAR = np.load(osp.join(REPO, "tests", "golden", "jpeg_parallel.npz"))


def file(name):
    return bytes(GOLD[f"file_{name}"])


def test_parallel_body_equals_the_serial_body_on_the_host(tmp_path):
    """scripts/jpeg_parallel_host.cpp, built with the host compiler (no sanitizer here), over the records of cases d, e, h, i, f, b and
    t: every segment intact, cut short at every length and with single bits flipped (3000 variants), each at S = 4, 8, 12, 64, 256 and
    one larger than the segment, with the lanes visited in three orders and in runs of 5 and of 256: coefficients and status word
    equal decode_segment<false>'s on the same bytes in every run (the program compares them and exits 1 otherwise), the intact
    streams give the restatement's coefficients, the guards stay untouched and no fixed point takes more rounds than it has lanes."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "jpeg_parallel_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", osp.join(REPO, "pmce_amd", "csrc"), osp.join(REPO, "scripts", "jpeg_parallel_host.cpp"),
                    "-o", exe], check=True, capture_output=True)
    names = list("dehifbt")
    files = [file(n) for n in names]
    coef = np.concatenate([JR.entropy_decode(f)[1] for f in files])
    rec = jpeg.dump_records(files, str(tmp_path / "records.bin"), coefficients=coef, names=names)
    assert {int(im[21]) for im in rec["images"]} == {1, 3, 4, 6}           # blocks per MCU: i, b, f and the 4:2:0 files
    r = subprocess.run([exe, str(tmp_path / "records.bin"), "3000"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 1
    line = lines[0]
    assert line.startswith("ok: 20 segments; intact 20 streams, %d coefficients compared" % coef.size), line
    m = re.search(r"cut (\d+) streams \((\d+) flagged\); bit flips (\d+) streams \((\d+) flagged\); (\d+) lanes, (\d+) subsequence decodes, "
                  r"(\d+) serial hand-offs", line)
    assert m and int(m.group(1)) == sum(int(s[2] - s[1]) for s in rec["segments"]) and int(m.group(2)) == int(m.group(1))
    assert int(m.group(3)) == 3000 and int(m.group(4)) > 0
    # lanes decoded more than once (the synchronisation ran), and runs of 5 lanes made the serial hand-off happen
    assert int(m.group(6)) > 2 * int(m.group(5)) and int(m.group(7)) > 0
    assert line.endswith("every run equals the serial body; guards untouched")
    # a dump whose expected coefficients are wrong is caught (the comparison is live)
    coef[5, 0] += 1
    jpeg.dump_records(files, str(tmp_path / "wrong.bin"), coefficients=coef)
    r = subprocess.run([exe, str(tmp_path / "wrong.bin"), "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "FAIL intact" in r.stdout


def test_decode_refuses_bad_entropy_and_subsequence_before_the_gpu():
    files = [file("j0"), file("j1")]
    for bad in ("fast", "", None, 1):
        with pytest.raises(ValueError, match="entropy") as e:
            jpeg.decode(files, entropy=bad)
        assert repr(bad) in str(e.value)
    for bad in (2, 6, -4, 130, 65540, 8.5, "64"):
        with pytest.raises(ValueError, match="subsequence") as e:
            jpeg.decode(files, entropy="parallel", subsequence=bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="subsequence"):
        jpeg.decode(files, subsequence=6)                   # checked whatever the stage
    assert jpeg.AUTO_THRESHOLD >= 4096 and jpeg.DEFAULT_SUBSEQUENCE % 4 == 0
    assert jpeg.MIN_SUBSEQUENCE <= jpeg.DEFAULT_SUBSEQUENCE <= jpeg.MAX_SUBSEQUENCE
    # every segment of the first golden file set lies below the threshold: "auto" leaves those files on the serial stage
    longest = max(int((s[1] - s[0])) for n in "abcdefghitm" for s in jpeg.parse(file(n), n).segments)
    assert longest == 2605 < jpeg.AUTO_THRESHOLD
    # ... and the scans of the second set lie above it
    for n in ("p420", "p420opt", "pgrey"):
        h = jpeg.parse(bytes(PAR[f"file_{n}"]), n)
        assert len(h.segments) == 1 and int(h.segments[0, 1] - h.segments[0, 0]) >= jpeg.AUTO_THRESHOLD


def test_subsequence_records():
    hd = jpeg.parse_all([file("d")])
    rec = jpeg.build_records(hd, 32)
    sub = jpeg.subsequence_records(rec, 128)                # d: 12 segments of 30 .. 83 bytes, each shorter than S
    lengths = rec["segments"][:, 2] - rec["segments"][:, 1]
    assert len(lengths) == 12 and lengths.max() < 128
    assert sub["offsets"].dtype == np.int32 and sub["offsets"].tolist() == [[k, k] for k in range(12)]
    assert sub["totals"] == [(12, 12, int(lengths.max()))]
    sub = jpeg.subsequence_records(rec, 4)
    n = -(-lengths // 4)
    assert sub["offsets"][:, 0].tolist() == (np.cumsum(n) - n).tolist() and sub["offsets"][:, 1].tolist() == list(range(12))
    # e: three segments of several hundred bytes
    rec = jpeg.build_records(jpeg.parse_all([file("e")]), 32)
    lengths = rec["segments"][:, 2] - rec["segments"][:, 1]
    sub = jpeg.subsequence_records(rec, 12)
    n = -(-lengths // 12)
    assert len(n) == 3 and sub["offsets"].tolist() == [[0, 0], [int(n[0]), 1], [int(n[0] + n[1]), 2]]
    assert sub["totals"] == [(int(n.sum()), 3, int(lengths.max()))]
    # t at S = 4: 652 subsequences in three runs of the synchronise stage
    rec = jpeg.build_records(jpeg.parse_all([file("t")]), 32)
    sub = jpeg.subsequence_records(rec, 4)
    assert sub["totals"] == [(652, 3, 2605)] and -(-652 // jpeg.PARALLEL_RUN) == 3
    # rounds count on their own: j0 (3 segments), j1 | j2, j3 (3) | j4, and an empty segment still has a subsequence
    files = [file(n) for n in ("j0", "j1", "j2", "j3", "j4")]
    rec = jpeg.build_records(jpeg.parse_all(files), chunk=2)
    sub = jpeg.subsequence_records(rec, 65536)
    assert sub["offsets"].tolist() == [[0, 0], [1, 1], [2, 2], [3, 3], [0, 0], [1, 1], [2, 2], [3, 3], [0, 0]]
    assert [t[:2] for t in sub["totals"]] == [(4, 4), (4, 4), (1, 1)]
    cut = file("e")[:(jpeg.parse(file("e")).scan_begin + jpeg.parse(file("e")).scan_end) // 2]
    rec = jpeg.build_records(jpeg.parse_all([cut]), 32)
    assert rec["segments"][2, 1] == rec["segments"][2, 2]
    sub = jpeg.subsequence_records(rec, 64)
    assert sub["offsets"][2, 0] - sub["offsets"][1, 0] >= 1 and sub["totals"][0][0] == sub["offsets"][2, 0] + 1
    assert jpeg.parallel_workspace_bytes(652, 3, 1) == 32 * 652 + 28 * 3 + 8


def test_new_symbols_are_prototyped_and_built():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, n_args in (("pmce_jpeg_entropy_parallel", 21), ("pmce_jpeg_parallel_run", 0), ("pmce_jpeg_parallel_stages", 0)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "jpeg_parallel.hip" in build.SOURCES and build.FILE_FLAGS["jpeg_parallel.hip"] == build.NO_PACKED_FP32
    # the constants are written once per language and agree
    assert lib.pmce_jpeg_parallel_run() == jpeg.PARALLEL_RUN and lib.pmce_jpeg_parallel_stages() == len(jpeg.PARALLEL_STAGES)
    hpp = open(osp.join(REPO, "pmce_amd", "csrc", "jpeg_parallel.hpp")).read()
    assert re.search(r"constexpr int RUN = %d;" % jpeg.PARALLEL_RUN, hpp)
    assert re.search(r"constexpr int MIN_SUBSEQUENCE = %d, MAX_SUBSEQUENCE = 1 << 16;" % jpeg.MIN_SUBSEQUENCE, hpp) and jpeg.MAX_SUBSEQUENCE == 1 << 16
    assert re.search(r"constexpr int JOIN_ROUNDS = %d;" % jpeg.PARALLEL_STAGES.count("join"), hpp)
    assert re.search(r"constexpr int SUB_BYTES = 32;", hpp) and re.search(r"constexpr int RUN_BYTES = 16 \+ 4 \* \(1 \+ JOIN_ROUNDS\);", hpp)


def test_entry_point_rejects_bad_arguments_on_the_host():
    """The argument checks return PMCE_ERR_ARG before anything is launched: no GPU is touched (the pointers are never followed)."""
    lib = _lib.load()
    p = C.c_void_p(4096)

    def ent(data=p, nbytes=100, nseg=3, nimg=2, nhuf=4, coef=p, nblk=24, first=0, S=64, off=p, nsub=5, nrun=3, ws=p, wsb=None, stage=-1):
        wsb = 32 * nsub + 28 * nrun + 8 * nseg if wsb is None else wsb
        return lib.pmce_jpeg_entropy_parallel(data, nbytes, p, first, nseg, p, nimg, p, nhuf, coef, nblk, p, 1, S, off, nsub, nrun, ws, wsb,
                                              stage, None)

    assert ent(data=None) == -1 and "null pointer" in _lib.last_error()
    assert ent(off=None) == -1 and ent(ws=None) == -1 and "null pointer" in _lib.last_error()
    assert ent(nbytes=0) == -1 and ent(nbytes=2 ** 31 - 128) == -1 and "2^31" in _lib.last_error()
    assert ent(nseg=0) == -1 and ent(nimg=0) == -1 and ent(nhuf=0) == -1 and ent(first=-1) == -1 and ent(nblk=0) == -1
    assert ent(coef=C.c_void_p(4104)) == -1 and "16-byte aligned" in _lib.last_error()
    for S in (0, 2, 6, -4, 65540):
        assert ent(S=S) == -1 and "subsequence" in _lib.last_error() and str(S) in _lib.last_error()
    assert ent(nsub=2) == -1 and ent(nrun=2) == -1 and ent(nsub=3, nrun=4) == -1 and "n_subsequences >= n_runs >= n_segments" in _lib.last_error()
    assert ent(ws=C.c_void_p(4100)) == -1 and "8-byte aligned" in _lib.last_error()
    assert ent(wsb=32 * 5 + 28 * 3 + 8 * 3 - 1) == -1 and "workspace needs 268 bytes" in _lib.last_error()
    assert ent(stage=-2) == -1 and ent(stage=6) == -1 and "stage" in _lib.last_error()


def test_load_frames_and_run_folder_pass_entropy_on(tmp_path, monkeypatch):
    seen = {}

    def fake_decode(files, device=None, channel_order="bgr", names=None, chunk=32, **kw):
        seen.update(kw=kw, chunk=chunk)
        import torch
        return torch.zeros(len(files), 48, 64, 3, dtype=torch.uint8), torch.zeros(len(files), dtype=torch.int32)

    monkeypatch.setattr(jpeg, "decode", fake_decode)
    (tmp_path / "000001.jpg").write_bytes(file("j0"))
    demo.load_frames(str(tmp_path))
    assert seen["kw"] == dict(entropy="auto")               # the default: files without restart markers get the parallel stage unasked
    demo.load_frames(str(tmp_path), entropy="parallel", chunk=5)
    assert seen["kw"] == dict(entropy="parallel") and seen["chunk"] == 5
    demo.load_frames(str(tmp_path), entropy="serial")
    assert seen["kw"] == dict(entropy="serial")

    calls = {}

    def fake_load(folder, device=None, strict=True, chunk=32, entropy="auto"):
        calls["load"] = (folder, device, strict, chunk, entropy)
        return "FRAMES", (64, 48), ["a.jpg"]

    def fake_run(model, frames, tracker, pose, extractor, img_wh, **kw):
        calls["run"] = kw
        return []

    monkeypatch.setattr(demo, "load_frames", fake_load)
    monkeypatch.setattr(demo, "run_frames", fake_run)
    demo.run_folder("M", "some/folder", "T", "P", "E", chunk=8, entropy="parallel", min_frames=5)
    assert calls["load"] == ("some/folder", None, True, 8, "parallel") and calls["run"] == dict(min_frames=5)
    demo.run_folder("M", "some/folder", "T", "P", "E", entropy="serial")
    assert calls["load"][4] == "serial"
    demo.run_folder("M", "some/folder", "T", "P", "E")
    assert calls["load"][4] == "auto" and calls["run"] == {}
