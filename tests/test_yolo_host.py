"""Host tests of the detector (pmce_amd/yolo.py, csrc/yolo.cpp): the counts that identify the published network, darknet files, state
dicts, the buffer plan checked from the table alone, the letterbox restatement against torch's own operators, argument checks.  No GPU."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import yolo_ref as YR
from conftest import REPO
from pmce_amd import yolo as Y


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def mini():
    spec = YR.mini_spec()
    return spec, YR.draw_state_dict(spec)


def test_the_spec_is_the_published_network():
    s = Y.yolov3_spec()
    L = s["layers"]
    assert len(L) == 107 and Y.darknet_conv_count(s) == 75
    assert Y.darknet_float_count(s) == 62001757 and Y.darknet_file_bytes(s) == 248007048
    assert f"{Y.flops(s, 416) / 1e9:.4g}" == "65.86"
    assert Y.num_rows(s, 416) == 10647 and Y.grids(s, 416) == [13, 26, 52]
    shapes = Y.layer_shapes(s)
    assert shapes[86] == (768, 16) and shapes[98] == (384, 8) and L[86]["layers"] == [85, 61] and L[98]["layers"] == [97, 36]
    assert [shapes[i][0] for i in (81, 93, 105)] == [255] * 3 and [L[i]["kind"] for i in (82, 94, 106)] == ["yolo"] * 3
    assert L[83] == {"kind": "route", "layers": [79]} and L[95] == {"kind": "route", "layers": [91]}
    assert shapes[36] == (256, 8) and shapes[61] == (512, 16) and shapes[74] == (1024, 32) and shapes[79] == (512, 32)
    assert [L[i]["mask"] for i in (82, 94, 106)] == [[6, 7, 8], [3, 4, 5], [0, 1, 2]] and s["anchors"][8] == (373.0, 326.0)
    assert sum(l["kind"] == "shortcut" for l in L) == 23 and Y.darknet_conv_count(Y.yolov3_spec(2)) == 75
    module_keys = [k for k in YR.Darknet(YR.mini_spec()).state_dict() if not k.endswith("num_batches_tracked")]
    assert sorted(module_keys) == sorted(Y.required_keys(YR.mini_spec()))        # the names a torch module of the structure carries


@pytest.mark.parametrize("major,minor,header", [(0, 2, 20), (0, 1, 16)])
def test_darknet_file_round_trip(tmp_path, mini, major, minor, header):
    spec, sd = mini
    path = str(tmp_path / "mini.weights")
    floats = YR.write_darknet(path, sd, spec, major=major, minor=minor)
    assert floats == Y.darknet_float_count(spec) and osp.getsize(path) == Y.darknet_file_bytes(spec, header)
    got = Y.read_darknet_weights(path, spec)
    assert sorted(got) == sorted(Y.required_keys(spec)) and all(torch.equal(got[k], sd[k]) for k in got) and len(got) == len(sd)
    back = YR.read_darknet(path, spec)
    assert all(torch.equal(back[k], sd[k]) for k in sd)


def test_darknet_file_of_the_wrong_length_is_rejected(tmp_path, mini):
    spec, sd = mini
    want = Y.darknet_float_count(spec)
    path = str(tmp_path / "short.weights")
    YR.write_darknet(path, sd, spec, drop_floats=7)
    with pytest.raises(ValueError, match=rf"holds {want - 7} floats .* stores {want}"):
        Y.read_darknet_weights(path, spec)
    path = str(tmp_path / "long.weights")
    YR.write_darknet(path, sd, spec, extra_floats=3)
    with pytest.raises(ValueError, match=rf"holds {want + 3} floats .* stores {want}"):
        Y.read_darknet_weights(path, spec)
    with pytest.raises(ValueError, match=rf"stores {Y.darknet_float_count(Y.yolov3_spec())}"):
        Y.read_darknet_weights(path, Y.yolov3_spec())


def test_state_dict_selection(mini):
    spec, sd = mini
    wrapped = {"module." + k: v.double() for k, v in sd.items()}
    wrapped["module.module_list.0.batch_norm_0.num_batches_tracked"] = torch.tensor(0)
    got = Y.select_state_dict(wrapped, spec)
    assert list(got) == list(Y.required_keys(spec)) and all(torch.equal(got[k], sd[k]) and got[k].dtype == torch.float32 for k in got)
    det = [i for i, _, _, bn, _ in Y.conv_table(spec) if not bn][0]
    broken = dict(sd)
    del broken[f"module_list.{det}.conv_{det}.bias"]
    with pytest.raises(ValueError, match=re.escape(f"'module_list.{det}.conv_{det}.bias'")):
        Y.select_state_dict(broken, spec)
    broken = dict(sd)
    broken["module_list.1.conv_1.weight"] = torch.zeros(16, 8, 1, 1)
    with pytest.raises(ValueError, match=r"'module_list\.1\.conv_1\.weight' has shape \(16, 8, 1, 1\), expected \(16, 8, 3, 3\)"):
        Y.select_state_dict(broken, spec)
    with pytest.raises(ValueError, match="mapping"):
        Y.select_state_dict([1], spec)
    folded = Y.fold_state_dict(got, spec)
    assert list(folded) == [c[0] for c in Y.conv_table(spec)] and torch.equal(folded[det][1], sd[f"module_list.{det}.conv_{det}.bias"])


def readers_from_table(spec):
    """layer -> the steps that read its map, from the cfg sections alone.  A shortcut is computed by the convolution before it, so that
    convolution's input is read at the shortcut's step; a one-source route passes its readers on to its source; the parts of a
    concatenation are read by the concatenation's readers."""
    L = spec["layers"]
    direct = {i: [] for i in range(len(L))}
    for i, l in enumerate(L):
        if l["kind"] == "convolutional" and i:
            direct[i - 1].append(i + 1 if i + 1 < len(L) and L[i + 1]["kind"] == "shortcut" else i)
        elif l["kind"] == "shortcut":
            direct[l["frm"]].append(i)
        elif l["kind"] == "upsample":
            direct[i - 1].append(i)

    def resolve(i):
        out = list(direct[i])
        for j, l in enumerate(L):
            if l["kind"] == "route" and i in l["layers"]:
                out += resolve(j)
        return out
    return {i: resolve(i) for i in range(len(L))}


@pytest.mark.parametrize("which", ["yolov3", "mini"])
def test_the_buffer_plan_never_frees_a_map_before_its_last_reader(lib, which):
    spec = Y.yolov3_spec() if which == "yolov3" else YR.mini_spec()
    L = spec["layers"]
    plan = Y.Plan(spec)
    readers = readers_from_table(spec)
    shapes = Y.layer_shapes(spec)
    produced = [i for i, l in enumerate(L) if l["kind"] in ("shortcut", "upsample") or
                (l["kind"] == "convolutional" and not (i + 1 < len(L) and L[i + 1]["kind"] in ("shortcut", "yolo")))]
    spans = {}
    for i in produced:
        p = plan.layers[i]
        assert p["buffer"] >= 0 and p["channels"] == shapes[i][0] and p["divisor"] == shapes[i][1], i
        assert p["units"] == p["pitch"] * (32 // shapes[i][1]) ** 2 and p["channel_offset"] + p["channels"] <= p["pitch"]
        assert readers[i], f"layer {i} is never read"
        assert p["last_reader"] >= max(readers[i])
        b = spans.setdefault(p["buffer"], {"lo": p["offset"], "hi": p["offset"] + p["units"], "birth": i, "death": i, "slices": []})
        assert (b["lo"], b["hi"]) == (p["offset"], p["offset"] + p["units"])
        b["birth"], b["death"] = min(b["birth"], i), max(b["death"], max(readers[i]))
        b["slices"].append((p["channel_offset"], p["channel_offset"] + p["channels"]))
    for b in spans.values():                     # the slices of a concatenation buffer do not overlap
        s = sorted(b["slices"])
        assert all(s[k][1] <= s[k + 1][0] for k in range(len(s) - 1))
    items = list(spans.values())
    for a in range(len(items)):                  # two buffers that share memory are never alive at the same step
        for c in range(a + 1, len(items)):
            x, z = items[a], items[c]
            if x["lo"] < z["hi"] and z["lo"] < x["hi"]:
                assert x["death"] < z["birth"] or z["death"] < x["birth"], (x, z)
    assert plan.total_units == max(b["hi"] for b in items)
    if which == "yolov3":
        assert readers[36] == [37, 99] and readers[61] == [62, 87] and readers[79] == [80, 84] and readers[91] == [92, 96]
        assert plan.layers[61]["pitch"] == 768 and plan.layers[61]["channel_offset"] == 256 and plan.layers[85]["channel_offset"] == 0
        assert plan.layers[36]["pitch"] == 384 and plan.layers[36]["channel_offset"] == 128
        assert plan.layers[83]["buffer"] == plan.layers[79]["buffer"] and plan.layers[105]["buffer"] == -2
        assert lib.pmce_yolo_workspace_units(None) == 0


def make_frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


LETTERBOX_CASES = [(1080, 1920, 416), (37, 53, 64), (48, 48, 32), (53, 38, 64)]


@pytest.mark.parametrize("H,W,S", LETTERBOX_CASES)
def test_letterbox_restatement_matches_torch(H, W, S):
    frame = make_frame(H, W, H + W)
    want = YR.letterbox_torch(frame, S, pad_value=0.25)
    sy, sx, pad_x, pad_y, ratio = Y.letterbox_geometry(H, W, S)
    table = Y.byte_table()
    got = torch.full((3, S, S), 0.25)
    yy, xx = np.meshgrid(sy, sx, indexing="ij")
    inside = (yy >= 0) & (xx >= 0)
    px = torch.from_numpy(frame[yy[inside], xx[inside]].astype(np.int64))
    got[:, torch.from_numpy(inside)] = table[px].T
    assert torch.equal(got, want)
    d = abs(H - W)
    assert (pad_x, pad_y) == ((d // 2, 0) if H > W else (0, d // 2)) and ratio == max(H, W) / S
    assert torch.equal(table, torch.arange(256).float().div(255))


def test_argument_checks_in_python():
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="channel_order"):
        Y.check_letterbox_args(frames, np.zeros(1, np.int64), 32, 0.0, "gbr")
    with pytest.raises(ValueError, match="uint8"):
        Y.check_letterbox_args(frames.astype(np.float32), np.zeros(1, np.int64), 32, 0.0, "rgb")
    with pytest.raises(ValueError, match="there are 2 frames"):
        Y.check_letterbox_args(frames, np.asarray([0, 2]), 32, 0.0, "rgb")
    with pytest.raises(ValueError, match="size"):
        Y.check_letterbox_args(frames, np.asarray([0]), 0, 0.0, "rgb")
    with pytest.raises(ValueError, match="pad_value"):
        Y.check_letterbox_args(frames, np.asarray([0]), 32, float("nan"), "rgb")
    assert Y.check_letterbox_args(frames, np.asarray([1, 1, 0]), 32, 0.0, "bgr")[:4] == (2, 4, 6, 3)
    for bad in (torch.zeros(1, 3, 100, 100), torch.zeros(1, 3, 64, 96), torch.zeros(1, 1, 64, 64), torch.zeros(3, 64, 64),
                torch.zeros(1, 3, 64, 64, dtype=torch.float64), torch.zeros(1, 3, 1056, 1056), np.zeros((1, 3, 64, 64), np.float32)):
        with pytest.raises(ValueError, match="multiple of 32"):
            Y.check_images(bad)
    assert Y.check_images(torch.zeros(0, 3, 96, 96)) == (0, 96)


def test_entries_are_declared_bound_and_built(lib):
    from pmce_amd import _lib, build
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    for name, n_args in (("pmce_conv2d_act_split_f16", 25), ("pmce_upsample2x_nhwc_f32", 9), ("pmce_yolo_decode_f32", 11),
                         ("pmce_letterbox_u8_f32", 13), ("pmce_yolo_create", 5), ("pmce_yolo_set_conv", 4), ("pmce_yolo_finalize_on", 2),
                         ("pmce_yolo_workspace_bytes", 3), ("pmce_yolo_forward", 15), ("pmce_yolo_layer_plan", 3)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "yolo.cpp" in build.SOURCES and osp.exists(osp.join(build.CSRC, "yolo.hip"))
    for text in ("(sigmoid(t0) + gx) * stride", "(exp(t2) * (aw / stride)) * stride", "min((int)floorf(dst * scale), L - 1)"):
        assert text in hdr


def test_c_entries_check_their_arguments(lib):
    from pmce_amd import _lib
    conv = lambda **kw: lib.pmce_conv2d_act_split_f16(*[kw.get(k, d) for k, d in (
        ("x", 16), ("sn", 64), ("sc", 1), ("sy", 16), ("sx", 4), ("n", 1), ("Cin", 4), ("H", 4), ("W", 4), ("Wp", 16), ("ws", 16), ("bias", None),
        ("R", None), ("ldr", 0), ("out", 16), ("ldo", 8), ("Cout", 8), ("KH", 1), ("KW", 1), ("stride", 1), ("pad", 0), ("act", 2), ("slope", 0.1),
        ("after", 1), ("stream", None))])
    assert conv(act=3) == -1 and "act" in _lib.last_error()
    assert conv(slope=float("nan")) == -1 and "slope" in _lib.last_error()
    assert conv(slope=1.5) == -1 and "slope" in _lib.last_error()
    assert conv(after=2) == -1 and "res_after_act" in _lib.last_error()
    assert conv(ldo=7) == -1 and "pitch" in _lib.last_error()
    assert conv(R=16, ldr=4) == -1 and "residual pitch=4" in _lib.last_error()
    assert conv(pad=1) == -1 and "pad" in _lib.last_error()
    assert conv(out=None) == -1 and "null" in _lib.last_error()
    up = lib.pmce_upsample2x_nhwc_f32
    assert up(16, 8, 16, 8, 1, 2, 2, 6, None) == -1 and "C % 4" in _lib.last_error()
    assert up(16, 8, 16, 6, 1, 2, 2, 8, None) == -1 and "pitches" in _lib.last_error()
    assert up(16, 8, 20, 16, 1, 2, 2, 8, None) == -1 and "aligned" in _lib.last_error()
    assert up(None, 8, 16, 16, 1, 2, 2, 8, None) == -1 and "null" in _lib.last_error()
    pit, gr, anc = (C.c_longlong * 3)(21, 21, 21), (C.c_int * 3)(2, 4, 8), (C.c_float * 18)(*[4.0] * 18)
    dec = lib.pmce_yolo_decode_f32
    assert dec(16, 16, 16, pit, gr, anc, 1, 0, 64, 16, None) == -1 and "nc in 1..255" in _lib.last_error()
    assert dec(16, 16, 16, pit, gr, anc, 1, 256, 64, 16, None) == -1
    assert dec(16, 16, 16, pit, gr, anc, 1, 3, 64, 16, None) == -1 and "pitch of map 0" in _lib.last_error()
    assert dec(16, 16, 16, pit, (C.c_int * 3)(2, 0, 8), anc, 1, 2, 64, 16, None) == -1 and "grid 1" in _lib.last_error()
    assert dec(16, 16, 16, pit, gr, (C.c_float * 18)(*[0.0] * 18), 1, 2, 64, 16, None) == -1 and "anchor" in _lib.last_error()
    lb = lib.pmce_letterbox_u8_f32
    fi = (C.c_int * 2)(0, 3)
    assert lb(16, 3, 4, 4, fi, 16, 2, 32, 0, 16, 0.0, 16, None) == -1 and "frame_index[1] = 3" in _lib.last_error()
    assert lb(16, 3, 4, 4, None, 16, 2, 0, 0, 16, 0.0, 16, None) == -1 and "S in 1..4096" in _lib.last_error()
    assert lb(16, 3, 4, 4, None, 16, 2, 32, 0, 16, float("nan"), 16, None) == -1 and "NaN" in _lib.last_error()


def test_network_handle_checks_its_table(lib):
    from pmce_amd import _lib
    spec = YR.mini_spec()

    def create(s):
        try:
            lib.pmce_yolo_destroy(Y._create(s))
            return ""
        except _lib.PmceError as e:
            return str(e)

    assert create(spec) == ""
    bad = dict(spec, layers=[dict(l) for l in spec["layers"]])
    bad["layers"][4]["frm"] = 0
    assert "layer 4: the shortcut's two maps differ" in create(bad)
    bad = dict(spec, layers=[dict(l) for l in spec["layers"]])
    bad["layers"][2]["filters"] = 6
    assert "layer 2" in create(bad)
    assert "three are needed" in create(dict(spec, layers=spec["layers"][:-1]))
    assert "num_classes" in create(dict(spec, num_classes=0))
    h = Y._create(spec)
    shape = (C.c_int * 4)()
    assert lib.pmce_yolo_conv_shape(h, 4, shape) == -1 and "layer 4 is not a convolution" in _lib.last_error()
    assert lib.pmce_yolo_conv_shape(h, 2, shape) == 0 and tuple(shape) == (8, 16, 1, 1)
    assert lib.pmce_yolo_set_conv(h, 4, 16, 16) == -1 and "layer 4" in _lib.last_error()
    assert lib.pmce_yolo_finalize_on(h, None) == -1 and "layer 0 was not set" in _lib.last_error()
    assert lib.pmce_yolo_workspace_bytes(h, 1, 100) == 0 and "multiple of 32" in _lib.last_error()
    assert lib.pmce_yolo_workspace_bytes(h, 0, 64) == 0 and lib.pmce_yolo_workspace_bytes(h, 1, 1056) == 0
    assert lib.pmce_yolo_workspace_bytes(h, 3, 64) == 3 * Y.Plan(spec).total_units * 4 * 4
    assert lib.pmce_yolo_forward(h, 16, 1, 1, 1, 1, 1, 64, 16, 16, 16, 16, 16, 1 << 40, None) == -1 and "not finalized" in _lib.last_error()
    lib.pmce_yolo_destroy(h)
