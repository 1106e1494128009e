"""Host tests of the convolution networks' single-product f16 mode: the CPU restatement (tests/conv_f16_ref.py) against the reference's
recordings (tests/golden/extractor.npz), the yardsticks the GPU tests divide by, the rounding rules on convolution rows, the shared
precision check and the argument checks of the new C entries.  No GPU.  Every test prints what it measures (run with -s)."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import conv_f16_ref as CR
import extractor_ref as ER
from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "extractor.npz"))


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def test_restatement_against_the_recordings(gold):
    """dev16 = the restatement's fp64 run against the reference's recorded fp64 results: what f16 operands cost by themselves.  Finite
    and > 0 for the features and every tap; printed relative to the recorded dev32 (the reference's own fp32 run against fp64)."""
    _, _, (feat, taps), _ = CR.extractor_case()
    d = float(np.abs(feat.numpy() - gold["feat64"]).max())
    print(f"features: dev16 = {d:.3e} = {d / float(gold['dev32_feat']):.0f} x the recorded dev32 ({float(gold['dev32_feat']):.2e})")
    assert np.isfinite(d) and d > 0
    for t in ER.TAPS:
        flat = taps[t].reshape(-1).numpy()
        d = float(np.abs(flat[ER.tap_index(flat.size)] - gold[t + "_64"]).max())
        print(f"{t}: dev16 = {d:.3e} = {d / float(gold['dev32_' + t]):.0f} x the recorded dev32 ({float(gold['dev32_' + t]):.2e})")
        assert np.isfinite(d) and d > 0


def guard(what, dev32r, out64):
    floor = 2.0 ** -12 * float(out64.abs().max())
    print(f"{what}: dev32r = {dev32r:.3e}, 2^-12 max |value| = {floor:.3e} ({dev32r / floor:.2f} x)")
    return dev32r > 0 and dev32r >= floor


def test_yardsticks_are_not_degenerate_extractor():
    """The GPU tests divide by dev32r, the restatement's fp32 run against its fp64 run.  Between layers the operands are rounded to f16,
    so that yardstick is made of f16 rounding flips between the two runs; dev32r >= 2^-12 x max |value| (half an f16 ulp of the largest
    value) says that the fp32 run met some.  Asserted as it stands for every tensor on the f16 grid: the four taps, the two bottleneck
    cases (on 16 images: the recorded two met too few flips).
    The features are not on the grid: they are the mean of layer4's tap over 49 pixels, so ONE flip of that tap moves a feature by 1 / 49
    of it.  Their condition is the same one carried through the mean, with the mean's own factor: dev32r(features) >= 2^-12 x max
    |layer4 tap| / 49 - asserted - next to the tap's own guard above.  (Held against the features' own largest value the same yardstick
    stands at 0.80 x the floor, with two patches and with six alike: printed.)"""
    _, _, (feat, taps), (d_feat, d_taps) = CR.extractor_case()
    for t in ER.TAPS:
        assert guard(t, d_taps[t], taps[t])
    guard("features against their own maximum (printed only)", d_feat, feat)
    assert guard("features against layer4's tap / 49", d_feat, taps["layer4"] / 49.0)
    for name in sorted(ER.BLOCK_CASES):
        _, out64, d = CR.block_case(name)
        assert guard(name, d, out64)


def row_floors(spec, maps64, S):
    """The floor of each decoded column group: what ONE half-ulp flip of a detection map (2^-12 x max |map value|, the maps' own guard)
    moves a decoded value by at the least - the flip times the smallest slope of that group's decoding over the map's range |t| <= T =
    max |map value|, the smallest over the three scales:
        xy = (sigmoid(t) + g) stride: slope sigmoid'(T) stride;   wh = exp(t) anchor: slope exp(-T) x the scale's smallest anchor side;
        conf, cls = sigmoid(t): slope sigmoid'(T)."""
    anchors = [[spec["anchors"][a] for a in l["mask"]] for l in spec["layers"] if l["kind"] == "yolo"]
    floors = {"xy": [], "wh": [], "conf_cls": []}
    for m, anc in zip(maps64, anchors):
        T = float(m.abs().max())
        flip = 2.0 ** -12 * T
        ds = float(np.exp(-T) / (1.0 + np.exp(-T)) ** 2)
        floors["xy"].append(flip * ds * S / m.shape[-1])
        floors["wh"].append(flip * float(np.exp(-T)) * min(min(a) for a in anc))
        floors["conf_cls"].append(flip * ds)
    return {g: min(v) for g, v in floors.items()}


@pytest.mark.parametrize("name", sorted(CR.YOLO_CASES))
def test_yardsticks_are_not_degenerate_detector(name):
    """The same guard, as it stands, for the three detection maps of every detector case.  The rows are decoded from the maps in fp32
    (sigmoid, exp times an anchor of up to 373 pixels) and are not on the f16 grid: a group's largest value is a box side or a grid
    offset, while its error is a map's flip carried through the decoding's slope.  Their condition is the maps' one carried through the
    decoding: dev32r(group) >= row_floors' floor - asserted per group - next to the maps' own guard.  (Held against each group's own
    largest value the yardsticks stand at 0.14 - 10.8 x the floor, the same with 5 and with 16 images: printed.)  dev16 is finite and
    > 0 throughout."""
    spec, _, images, ref = CR.yolo_case(name)
    for k, m in enumerate(ref["maps64"]):
        assert guard(f"{name} map {k}", ref["dev32r"][f"map {k}"], m)
    floors = row_floors(spec, ref["maps64"], images.shape[-1])
    for g, sl in CR.ROW_GROUPS:
        guard(f"{name} rows {g} against their own maximum (printed only)", ref["dev32r"][f"rows {g}"], ref["rows64"][..., sl])
        d = ref["dev32r"][f"rows {g}"]
        print(f"{name} rows {g}: dev32r = {d:.3e}, one map flip through the decoding = {floors[g]:.3e} ({d / floors[g]:.1f} x)")
        assert d > 0 and d >= floors[g]
    print(f"{name}: dev16 " + ", ".join(f"{k} {v:.2e}" for k, v in ref["dev16"].items()))
    assert all(v > 0 and np.isfinite(v) for v in ref["dev32r"].values()) and all(v > 0 and np.isfinite(v) for v in ref["dev16"].values())


def test_rounding_rules_on_convolution_rows():
    g = torch.Generator().manual_seed(7)
    w = torch.randn(6, 5, 3, 3, generator=g) * 0.05
    w[2] = 0
    w[3, 0, 0, 0] = 1e-10                     # far below the row's max: flushed to zero by r16 of the scaled value
    q = CR.w16(w)
    up = CR.VF.row_scale(w.reshape(6, -1))
    assert float(up[2]) == 1.0 and float(q[2].abs().max()) == 0.0
    scaled = (q.reshape(6, -1) * up)
    assert torch.equal(scaled, scaled.half().float())                    # on the f16 grid
    m = (w.reshape(6, -1) * up).abs().amax(dim=1)
    assert all(2.0 ** 14 <= float(v) < 2.0 ** 15 for i, v in enumerate(m) if i != 2)
    assert float(q[3, 0, 0, 0]) == 0.0
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 3e-5, -3e-5, 2.0 ** -14, 65519.0, 65520.0, -1e30, float("nan")])
    r = CR.r16(x)
    assert r[:8].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 0.0, 2.0 ** -14, 65504.0, float("inf")]
    assert float(r[8]) == float("-inf") and bool(torch.isnan(r[9]))
    assert torch.equal(CR.r16(x.double()).float()[:9], r[:9])
    # a convolution of grid operands is exact in both dtypes: the restatement's two runs agree to the bit before any rounding flips
    xi = torch.randint(-8, 9, (1, 5, 6, 6), generator=g).float()
    wi = torch.randint(-4, 5, (6, 5, 3, 3), generator=g).float()
    assert torch.equal(CR.conv(xi, wi, pad=1, out16=False).double(), CR.conv(xi.double(), wi, pad=1, out16=False))
    assert torch.equal(CR.conv(xi, wi, pad=1, out16=False).long(), ER.conv2d_int(xi, wi, 1, 1))


def test_bf16_is_refused_before_any_device_work(tmp_path):
    """One shared check (pmce_amd/_net.py), the same text for every class; nothing is loaded, uploaded or created."""
    from pmce_amd import _net, extractor, hmr, vitpose, yolo
    assert vitpose.check_precision is _net.check_precision and _net.check_precision("split_f16") == 0 and _net.check_precision("f16") == 1
    text = re.escape('precision must be "split_f16" or "f16" (got \'bf16\')')
    missing = str(tmp_path / "no_such_checkpoint.pth")
    calls = [lambda: extractor.FeatureExtractor({}, "cuda:0", precision="bf16"),
             lambda: extractor.FeatureExtractor.from_state_dict({}, "cuda:0", precision="bf16"),
             lambda: extractor.FeatureExtractor.from_checkpoint(missing, "cuda:0", precision="bf16"),
             lambda: yolo.YOLOv3({}, "cuda:0", precision="bf16"),
             lambda: yolo.YOLOv3.from_state_dict({}, "cuda:0", precision="bf16"),
             lambda: yolo.YOLOv3.from_darknet_weights(missing, "cuda:0", precision="bf16"),
             lambda: yolo.YOLOv3.from_checkpoint(missing, "cuda:0", precision="bf16"),
             lambda: hmr.HMR.from_state_dict({}, "cuda:0", precision="bf16"),
             lambda: hmr.HMR.from_checkpoint(missing, "cuda:0", precision="bf16")]
    for call in calls:
        with pytest.raises(ValueError, match=text):
            call()


def test_entries_are_declared_bound_and_built(lib):
    from pmce_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(osp.join(REPO, "include", "pmce_hip.h")).read(), flags=re.S)
    for name, n_args in (("pmce_conv_packed_halves", 4), ("pmce_conv_pack_f16", 8), ("pmce_conv2d_act_f16", 27), ("pmce_maxpool3x3s2_nhwc_f16", 7),
                         ("pmce_avgpool_nhwc_f16_f32", 6), ("pmce_upsample2x_nhwc_f16", 9), ("pmce_widen_f16_f32", 4),
                         ("pmce_extractor_create_precision", 2), ("pmce_extractor_precision", 1), ("pmce_extractor_workspace_bytes_for", 2),
                         ("pmce_yolo_create_precision", 6), ("pmce_yolo_precision", 1)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    # the kernel is compiled with conv.hip: its flags (no packed fp32) and the suite's device-code census cover it
    assert "conv.hip" in build.SOURCES and build.FILE_FLAGS["conv.hip"] == build.NO_PACKED_FP32
    assert '#include "conv_f16.hpp"' in open(osp.join(build.CSRC, "conv.hip")).read() and osp.exists(osp.join(build.CSRC, "conv_f16.hpp"))


def test_argument_validation_without_gpu(lib):
    from pmce_amd import _lib
    assert lib.pmce_conv_packed_halves(64, 3, 7, 7) == 64 * 192 and lib.pmce_conv_packed_halves(192, 128, 3, 3) == 192 * 1152
    assert lib.pmce_conv_packed_halves(65, 16, 1, 1) == 128 * 64 and lib.pmce_conv_packed_halves(64, 32, 3, 3) == 64 * 320
    assert lib.pmce_conv_packed_halves(0, 3, 7, 7) == 0 and "Cout" in _lib.last_error()
    assert lib.pmce_conv_pack_f16(None, 64, 3, 7, 7, 16, 16, None) == -1 and "null" in _lib.last_error()
    assert lib.pmce_conv_pack_f16(16, 64, 0, 7, 7, 16, 16, None) == -1 and "bad shape" in _lib.last_error()

    def conv(x=16, x_dtype=1, n=1, cin=32, h=4, w=4, wp=16, ws=16, res=None, ldr=0, out=16, ldo=8, out_dtype=1, cout=8, k=3, stride=1, pad=1,
             act=0, slope=0.0, after=0):
        return lib.pmce_conv2d_act_f16(x, x_dtype, h * w * cin, 1, w * cin, cin, n, cin, h, w, wp, ws, None, res, ldr, out, ldo, out_dtype, cout,
                                       k, k, stride, pad, act, slope, after, None)

    for kw in (dict(x=None), dict(wp=None), dict(ws=None), dict(out=None)):
        assert conv(**kw) == -1 and "null pointer" in _lib.last_error()
    assert conv(pad=3) == -1 and "pad" in _lib.last_error()
    assert conv(k=1, pad=1) == -1 and "pad" in _lib.last_error()
    assert conv(ldo=7) == -1 and "pitches" in _lib.last_error()
    assert conv(ldo=1 << 24) == -1 and "pitches" in _lib.last_error()
    assert conv(res=16, ldr=7) == -1 and "pitches" in _lib.last_error()
    assert conv(act=3) == -1 and "act must be" in _lib.last_error()
    assert conv(act=2, slope=1.5) == -1 and "slope" in _lib.last_error()
    assert conv(act=2, slope=float("nan")) == -1 and "slope" in _lib.last_error()
    assert conv(after=2) == -1 and "res_after_act" in _lib.last_error()
    assert conv(x_dtype=2) == -1 and "dtype codes" in _lib.last_error()
    assert conv(out_dtype=-1) == -1 and "dtype codes" in _lib.last_error()
    assert conv(n=1 << 20, h=64, w=64) == -1 and "too large" in _lib.last_error()
    assert lib.pmce_maxpool3x3s2_nhwc_f16(16, 16, 1, 4, 4, 6, None) == -1 and "C % 4" in _lib.last_error()
    assert lib.pmce_maxpool3x3s2_nhwc_f16(16, 20, 1, 4, 4, 8, None) == -1 and "aligned" in _lib.last_error()
    assert lib.pmce_avgpool_nhwc_f16_f32(None, 16, 1, 49, 8, None) == -1 and "null" in _lib.last_error()
    assert lib.pmce_avgpool_nhwc_f16_f32(16, 16, 1, 0, 8, None) == -1
    assert lib.pmce_upsample2x_nhwc_f16(16, 8, 16, 6, 1, 2, 2, 8, None) == -1 and "pitches" in _lib.last_error()
    assert lib.pmce_upsample2x_nhwc_f16(16, 8, 18, 16, 1, 2, 2, 8, None) == -1 and "aligned" in _lib.last_error()
    assert lib.pmce_widen_f16_f32(16, 16, 0, None) == -1 and "count" in _lib.last_error()
    # the handles: the mode is validated, reported, and sizes the workspace
    h = C.c_void_p()
    assert lib.pmce_extractor_create_precision(2, C.byref(h)) == -1 and "precision must be 0" in _lib.last_error()
    assert lib.pmce_extractor_precision(None) == -1
    sizes = {}
    for mode in (0, 1):
        assert lib.pmce_extractor_create_precision(mode, C.byref(h)) == 0 and lib.pmce_extractor_precision(h) == mode
        sizes[mode] = [lib.pmce_extractor_workspace_bytes_for(h, n) for n in (1, 2, 3, 64)]
        assert lib.pmce_extractor_workspace_bytes_for(h, 0) == 0
        assert lib.pmce_extractor_finalize_on(h, None) == -1 and "'conv1' was not set" in _lib.last_error()
        lib.pmce_extractor_destroy(h)
    assert sizes[0] == [lib.pmce_extractor_workspace_bytes(n) for n in (1, 2, 3, 64)]
    assert sizes[1] == [b // 2 for b in sizes[0]] and sizes[1] == sorted(sizes[1])
    assert lib.pmce_extractor_create(C.byref(h)) == 0 and lib.pmce_extractor_precision(h) == 0
    lib.pmce_extractor_destroy(h)
    from pmce_amd import yolo
    import yolo_ref as YR
    spec = YR.mini_spec()
    units = {}
    for mode in (0, 1):
        hy = yolo._create(spec, mode)
        assert lib.pmce_yolo_precision(hy) == mode
        units[mode] = (lib.pmce_yolo_workspace_units(hy), [lib.pmce_yolo_workspace_bytes(hy, n, 64) for n in (1, 2, 5)])
        lib.pmce_yolo_destroy(hy)
    assert units[0][0] == units[1][0] and units[1][1] == [b // 2 for b in units[0][1]] and units[1][1] == sorted(units[1][1])
    with pytest.raises(_lib.PmceError, match="precision must be 0"):
        yolo._create(spec, 2)
    assert lib.pmce_yolo_precision(None) == -1
