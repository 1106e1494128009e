"""Host side of the demo in frame chunks, without a GPU: the state's argument checks, the new C entries' declarations and refusals,
the pass planner's chunk tables, ``frames_per_pass``' range and the untouched wiring of the whole-video route."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from pmce_amd import demo

SORT_KW = dict(max_age=1, min_hits=3, iou_threshold=0.3, max_tracks=64, update_on_empty=0)


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def people(F=2):
    return torch.zeros(F, 3, 5, dtype=torch.float64), torch.zeros(F, dtype=torch.int32)


def test_a_state_holds_its_first_arguments():
    from pmce_amd import tracker as T
    st = T.SortState()
    assert st.n_seq == 1 and st.args is None and st.buffer is None and st.frames.tolist() == [0]
    st.bind(1, **SORT_KW)                                                             # what the first sort_tracks(..., state=st) does
    st.bind(1, **SORT_KW)
    for name, other in (("max_age", 2), ("min_hits", 0), ("iou_threshold", 0.5), ("max_tracks", 8), ("update_on_empty", True)):
        with pytest.raises(ValueError, match=rf"^{name} = "):                          # before any device work: host tensors, no GPU
            T.sort_tracks(*people(), state=st, **{name: other})
    assert st.args == SORT_KW and st.buffer is None and st.frames.tolist() == [0]
    c = st.clone()
    assert c.args == st.args and c.args is not st.args and c.n_seq == 1 and c.frames is not st.frames
    with pytest.raises(ValueError, match="max_age"):
        T.sort_tracks(*people(), state=c, max_age=3)


def test_a_state_refuses_another_number_of_sequences():
    from pmce_amd import tracker as T
    with pytest.raises(ValueError, match=r"n_seq = 1 .*the call has 2"):
        T.sort_tracks(*people(), seq_offsets=[0, 1, 2], state=T.SortState())
    with pytest.raises(ValueError, match=r"n_seq = 2 .*the call has 1"):
        T.sort_tracks(*people(), state=T.SortState(2))
    with pytest.raises(ValueError, match=r"n_seq = 2 .*the call has 3"):
        T.sort_tracks(*people(), seq_offsets=[0, 0, 2, 2], state=T.SortState(2))
    with pytest.raises(ValueError, match="SortState"):
        T.sort_tracks(*people(), state=torch.zeros(4))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_seq"):
            T.SortState(bad)
    with pytest.raises(ValueError, match="people must be"):                            # the old checks come first
        T.sort_tracks(torch.zeros(2, 3, 5), torch.zeros(2, dtype=torch.int32), state=T.SortState())


def test_the_new_symbols(lib):
    from pmce_amd import _lib
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pmce_sort_state_bytes", "pmce_sort_track_resume_f64"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", code)
    assert _lib.PROTOTYPES["pmce_sort_state_bytes"] == [] and _lib._RESTYPES["pmce_sort_state_bytes"] is C.c_size_t
    old, new = _lib.PROTOTYPES["pmce_sort_track_f64"], _lib.PROTOTYPES["pmce_sort_track_resume_f64"]
    _f, _i, _d, _s = _lib._f, _lib._i, _lib._d, _lib._s
    assert old == [_f, _f, C.POINTER(C.c_int), _f, _i, _i, _i, _i, _i, _d, _i, _i, _f, _f, _f, _s] and len(old) == 16    # as it was
    assert new == old[:-1] + [_f, _s]                                                 # the same arguments plus the state
    n = lib.pmce_sort_state_bytes()
    assert n > 0 and n % 8 == 0 and n >= (7 + 49) * 64 * 8 + (4 * 64 + 2) * 4         # x, P, four ints per slot, two counters
    for text in ("pmce_sort_state_bytes() bytes each", "double x[7][64]", "double P[7][7][64]", "int    frame_count, next_id",
                 "An all-zero record is a fresh tracker", "a slot that is not alive is stored as zeros",
                 "the same max_tracks, max_age, min_hits, iou_threshold and update_on_empty on every call of one state"):
        assert text in hdr, text


def test_the_resume_entry_rejects_bad_arguments_before_any_launch(lib):
    from pmce_amd import _lib

    def sort(people=16, pc=16, sh=None, sd=None, F=4, K=8, S=1, age=1, hits=3, thr=0.3, T=64, uoe=0, tr=16, tc=16, st=16, state=16):
        return lib.pmce_sort_track_resume_f64(people, pc, sh, sd, F, K, S, age, hits, thr, T, uoe, tr, tc, st, state, None)

    seq = (C.c_int * 3)(0, 3, 2)
    for kw, word in ((dict(state=None), "null"), (dict(state=12), "aligned"), (dict(people=None), "null"), (dict(st=None), "null"),
                     (dict(K=65), "K"), (dict(K=0), "K"), (dict(T=65), "max_tracks"), (dict(T=0), "max_tracks"),
                     (dict(thr=float("nan")), "finite"), (dict(S=2), "one sequence"), (dict(sh=seq, S=2), "host and"),
                     (dict(sh=seq, sd=16, S=2), "end at F"), (dict(age=-1), "max_age"), (dict(hits=-1), "min_hits"), (dict(F=-1), "F must be")):
        assert sort(**kw) == -1 and word in _lib.last_error() and "sort_track_resume_f64" in _lib.last_error(), (kw, _lib.last_error())
    assert sort(F=0) == 0                                                             # nothing to do: no launch, the records untouched
    assert lib.pmce_sort_track_f64(16, 16, None, None, 0, 8, 1, 1, 3, 0.3, 64, 0, 16, 16, 16, None) == 0           # today's 16 arguments
    assert lib.pmce_sort_track_f64(None, 16, None, None, 4, 8, 1, 1, 3, 0.3, 64, 0, 16, 16, 16, None) == -1
    assert _lib.last_error().startswith("sort_track_f64: null")


@pytest.mark.parametrize("F", [1, 7, 30])
@pytest.mark.parametrize("k", [1, 7, 64])
def test_plan_passes_partitions_every_tracklet(F, k):
    g = np.random.default_rng(100 * F + k)
    tracklets = [np.arange(F), np.arange(F // 3, F), np.sort(g.choice(F, size=max(1, F // 2), replace=False)), np.zeros(0, np.int64)]
    fi = np.concatenate(tracklets)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracklets])])
    plan = demo.plan_passes(fi, F, k)
    assert [p[0] for p in plan] == list(range(0, F, k)) and [p[1] for p in plan] == [min(k, F - a) for a in range(0, F, k)]
    rows = np.concatenate([p[2] for p in plan])
    assert sorted(rows.tolist()) == list(range(len(fi)))                               # every row in exactly one chunk
    for first, n, r, rel in plan:
        assert r.dtype == np.int64 and rel.dtype == np.int32 and r.shape == rel.shape
        assert (rel >= 0).all() and (rel < n).all() and np.array_equal(fi[r], first + rel)
        assert r.tolist() == sorted(r.tolist())                                       # in row order: tracklet after tracklet
        for a, b in zip(off[:-1], off[1:]):                                           # of a tracklet: exactly its frames of this chunk
            mine = r[(r >= a) & (r < b)]
            assert np.array_equal(fi[mine], [f for f in fi[a:b] if first <= f < first + n])
    with pytest.raises(ValueError, match="frame_index runs"):
        demo.plan_passes([0, F], F, k)


@pytest.mark.parametrize("bad", [0, -1, -7, 2.5, 7.0, "7", True])
def test_frames_per_pass_must_be_a_positive_whole_number(bad, tmp_path):
    for call in (lambda: demo.run_folder("M", str(tmp_path), "T", "P", "E", frames_per_pass=bad),
                 lambda: demo.render_folder("M", str(tmp_path), str(tmp_path / "out"), "T", "P", "E", "R", frames_per_pass=bad),
                 lambda: next(demo.iter_frames(str(tmp_path), bad)), lambda: demo.plan_passes([0], 1, bad)):
        with pytest.raises(ValueError, match="frames_per_pass"):
            call()
    assert not (tmp_path / "out").exists()


def test_iter_frames_has_load_frames_folder_rules(tmp_path):
    with pytest.raises(ValueError, match="no .jpg or .jpeg file"):
        next(demo.iter_frames(str(tmp_path), 4))
    (tmp_path / "000001.png").write_bytes(b"\x89PNG\r\n\x1a\n")
    with pytest.raises(ValueError, match=r"000001\.png: PNG is not served"):
        next(demo.iter_frames(str(tmp_path), 4))


def test_iter_frames_reads_one_step_at_a_time(tmp_path, monkeypatch):
    from pmce_amd import jpeg
    for name in ("b.JPG", "a.jpg", "c.jpeg", "d.jpg", "notes.txt", "e.jpg"):
        (tmp_path / name).write_bytes(name.encode())
    calls = []

    def fake_decode(files, device=None, channel_order="bgr", chunk=32, names=None, entropy="auto"):
        calls.append((list(files), device, channel_order, chunk, [osp.basename(n) for n in names], entropy))
        return torch.zeros(len(files), 4, 6, 3, dtype=torch.uint8), torch.zeros(len(files), dtype=torch.int32)

    monkeypatch.setattr(jpeg, "decode", fake_decode)
    it = demo.iter_frames(str(tmp_path), 2, device="D", chunk=9, entropy="serial")
    assert calls == []                                                                # a generator: nothing is read before the first step
    first, frames, names = next(it)
    assert (first, tuple(frames.shape), names) == (0, (2, 4, 6, 3), ["a.jpg", "b.JPG"])
    assert calls == [([b"a.jpg", b"b.JPG"], "D", "bgr", 9, ["a.jpg", "b.JPG"], "serial")]      # the step's files only
    rest = list(it)
    assert [(r[0], r[2]) for r in rest] == [(2, ["c.jpeg", "d.jpg"]), (4, ["e.jpg"])] and len(calls) == 3
    # strict: the step's status is read and the file named
    monkeypatch.setattr(jpeg, "decode", lambda files, *a, **kw: (torch.zeros(len(files), 4, 6, 3, dtype=torch.uint8),
                                                                  torch.tensor([0, jpeg.STATUS_TRUNCATED][:len(files)], dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"b\.JPG: the scan is truncated"):
        next(demo.iter_frames(str(tmp_path), 2))
    assert len(list(demo.iter_frames(str(tmp_path), 2, strict=False))) == 3


def test_without_frames_per_pass_the_wiring_is_the_old_one(monkeypatch):
    calls = {}

    def fake_load(folder, device=None, strict=True, chunk=32):
        calls["load"] = (folder, device, strict, chunk)
        return "FRAMES", (64, 48), ["a.jpg"]

    def fake_run(model, frames, tracker, pose, extractor, img_wh, **kw):
        calls["run"] = (model, frames, tracker, pose, extractor, img_wh, kw)
        return [{"person_id": 3}]

    def no_passes(*a, **kw):
        raise AssertionError("the chunked route was taken")

    monkeypatch.setattr(demo, "load_frames", fake_load)
    monkeypatch.setattr(demo, "run_frames", fake_run)
    monkeypatch.setattr(demo, "run_folder_in_passes", no_passes)
    monkeypatch.setattr(demo, "iter_frames", no_passes)
    for kw in (dict(), dict(frames_per_pass=None)):
        calls.clear()
        out = demo.run_folder("M", "some/folder", "T", "P", "E", strict=False, chunk=300, min_frames=5, extract_batch=64, **kw)
        assert out == [{"person_id": 3}]
        assert calls["load"] == ("some/folder", None, False, 300)
        assert calls["run"] == ("M", "FRAMES", "T", "P", "E", (64, 48), dict(min_frames=5, extract_batch=64))
    saved = []
    monkeypatch.setattr(demo, "render_tracklets", lambda outs, fr, wh, renderer=None, order="reference": calls.setdefault(
        "render", (outs, fr, wh, renderer, order)) and "RENDERED")
    monkeypatch.setattr(demo, "save_frames", lambda folder, fr, **kw: saved.append((folder, fr, kw)))
    for kw in (dict(), dict(frames_per_pass=None)):
        calls.clear()
        del saved[:]
        out = demo.render_folder("M", "some/folder", "out", "T", "P", "E", "R", input_folder="in", chunk=8, order="depth",
                                 encode_kwargs=dict(quality=90), min_frames=5, **kw)
        assert out == [{"person_id": 3}] and calls["load"] == ("some/folder", None, True, 8)
        assert calls["run"] == ("M", "FRAMES", "T", "P", "E", (64, 48), dict(min_frames=5))
        assert calls["render"] == ([{"person_id": 3}], "FRAMES", (64, 48), "R", "depth")
        assert saved == [("out", "RENDERED", dict(quality=90)), ("in", "FRAMES", dict(quality=90))]
