"""GPU tests of the feature extractor's single-product f16 mode (``FeatureExtractor(..., precision="f16")``) against the restatement of
its arithmetic (tests/conv_f16_ref.py) and the reference's recordings (tests/golden/extractor.npz).

Two bounds per tensor: within 4 x dev32r of the restatement's fp64 run (dev32r = the restatement's own fp32 run against it: the device
is another summation order of the same arithmetic), and within 4 x dev16 of the recordings (dev16 = the restatement's fp64 run against
them: what f16 operands cost by themselves).  tests/test_conv_f16_host.py checks on the CPU that neither yardstick is degenerate.
Invariances are to the bit.  Every test prints what it measures (run with -s)."""
import os.path as osp

import numpy as np
import pytest
import torch

import conv_f16_ref as CR
import extractor_ref as ER
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = CR.FACTOR


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def case():
    """The golden state dict, its patches (a third for the batch tests) and, BEFORE any f16 object exists, a default-mode extractor and
    its features."""
    from pmce_amd.extractor import FeatureExtractor
    sd, _, ref, d32r = CR.extractor_case()
    patches = ER.patches(3).to(DEV)
    default = FeatureExtractor.from_state_dict(sd, DEV)
    assert default.precision == "split_f16"
    before = default(patches).cpu()
    ext = FeatureExtractor.from_state_dict(sd, DEV, precision="f16")
    assert ext.precision == "f16"
    feats, taps = ext.forward(patches[:2], taps=ER.TAPS)
    torch.cuda.synchronize()
    return {"sd": sd, "patches": patches, "ref": ref, "dev32r": d32r, "default": default, "before": before, "ext": ext,
            "feats": feats.cpu(), "taps": {k: v.cpu() for k, v in taps.items()}}


def test_features_and_taps_within_both_bounds(case):
    gold = np.load(osp.join(GOLDEN, "extractor.npz"))
    (feat64, taps64), (d_feat, d_taps) = case["ref"], case["dev32r"]
    feats, taps = case["feats"], case["taps"]
    assert feats.dtype == torch.float32 and feats.shape == (2, 2048) and all(v.dtype == torch.float32 for v in taps.values())
    assert taps["layer1"].shape == (2, 256, 56, 56) and taps["layer4"].shape == (2, 2048, 7, 7)
    worst = {}
    for t in ER.TAPS:
        assert torch.equal(taps[t], taps[t].half().float()), f"{t} is not on the f16 grid"
        idx = ER.tap_index(taps[t].numel())
        got = taps[t].contiguous().reshape(-1).double().numpy()[idx]
        dev16 = float(np.abs(taps64[t].reshape(-1).numpy()[idx] - gold[t + "_64"]).max())
        worst[t] = (float((taps[t].double() - taps64[t]).abs().max()) / d_taps[t], float(np.abs(got - gold[t + "_64"]).max()) / dev16)
    dev16 = float(np.abs(feat64.numpy() - gold["feat64"]).max())
    worst["features"] = (float((feats.double() - feat64).abs().max()) / d_feat, float(np.abs(feats.double().numpy() - gold["feat64"]).max()) / dev16)
    print("(x dev32r, x dev16): " + ", ".join(f"{k} ({a:.2f}, {b:.2f})" for k, (a, b) in worst.items()))
    assert all(a <= FACTOR and b <= FACTOR for a, b in worst.values()), worst
    assert float((feats == 0).float().mean()) < 0.5


@pytest.mark.parametrize("name", sorted(ER.BLOCK_CASES))
def test_recorded_bottlenecks_through_the_operators(name):
    """conv_f16_ref.block_case: the recorded [2,64,9,7] input and 14 more images through pack_conv_f16 / conv2d_f16, every form of the
    bottleneck's epilogue; all 16 against the restatement, the recorded two against the recordings."""
    from pmce_amd import extractor as ex
    gold = np.load(osp.join(GOLDEN, "extractor.npz"))
    _, _, stride = ER.BLOCK_CASES[name]
    f = ER.fold_block(name)
    x16, out64, dev32r = CR.block_case(name)

    def conv(key, x, res=None, stride=1, pad=0, act="none"):
        w, b = f[f"{name}.{key}"]
        packed, ws = ex.pack_conv_f16(w.to(DEV))
        return ex.conv2d_f16(x, "nhwc", packed, ws, tuple(w.shape), b.to(DEV), res, stride=stride, pad=pad, act=act)

    x = x16.permute(0, 2, 3, 1).contiguous().half().to(DEV)
    y = conv("conv1", x, act="relu")
    y = conv("conv2", y, stride=stride, pad=1, act="relu")
    ds = conv("downsample.0", x, stride=stride)
    y = conv("conv3", y, res=ds, act="relu")
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert got.shape == out64.shape
    dev16 = float(np.abs(out64[:2].numpy() - gold[name + "_64"]).max())
    a = float((got - out64).abs().max()) / dev32r
    b = float(np.abs(got[:2].numpy() - gold[name + "_64"]).max()) / dev16
    print(f"{name}: {a:.2f} x dev32r ({dev32r:.2e}), {b:.2f} x dev16 ({dev16:.2e})")
    assert a <= FACTOR and b <= FACTOR


def test_a_patch_does_not_depend_on_the_batch(case):
    """Patch 0 has the same bits for n = 1, 2 (the fixture's run), 3 and through a handle with max_batch = 1."""
    from pmce_amd.extractor import FeatureExtractor
    ext, patches, want = case["ext"], case["patches"], bits(case["feats"][0])
    for n in (1, 3):
        got = ext(patches[:n]).cpu()
        assert got.shape == (n, 2048) and torch.equal(bits(got[0]), want), f"patch 0 differs at n = {n}"
    one = FeatureExtractor.from_state_dict(case["sd"], DEV, max_batch=1, precision="f16")
    got, taps = one.forward(patches, taps=("layer2",))
    assert torch.equal(bits(got[:2].cpu()), bits(case["feats"])) and torch.equal(bits(taps["layer2"][:2].cpu()), bits(case["taps"]["layer2"]))


def test_the_default_mode_keeps_its_bits_and_the_f16_mode_differs(case):
    """The default-mode handle built before any f16 object gives the same bits after f16 forwards in the same process, and so does a
    fresh default handle; the f16 features are other numbers (this fails without the feature)."""
    from pmce_amd.extractor import FeatureExtractor
    patches = case["patches"]
    f16 = case["ext"](patches).cpu()
    after = case["default"](patches).cpu()
    fresh = FeatureExtractor.from_state_dict(case["sd"], DEV)(patches).cpu()
    assert torch.equal(bits(after), bits(case["before"])) and torch.equal(bits(fresh), bits(case["before"]))
    differ = float((bits(f16) != bits(case["before"])).float().mean())
    print(f"{100 * differ:.1f} % of the f16 mode's features differ from the default's bits")
    assert differ > 0.5


def test_checkpoint_file_gives_the_same_bits(case, tmp_path):
    from pmce_amd.extractor import FeatureExtractor
    full = {"module." + k: v for k, v in case["sd"].items()}
    full.update({"module.fc1.weight": torch.zeros(4, 4), "module.bn1.num_batches_tracked": torch.tensor(7)})
    path = str(tmp_path / "spin.pth.tar")
    torch.save({"model": full, "epoch": 1}, path)
    ext = FeatureExtractor.from_checkpoint(path, DEV, precision="f16")
    assert ext.precision == "f16" and torch.equal(bits(ext(case["patches"][:2]).cpu()), bits(case["feats"]))


def test_an_overflowing_pixel_is_named_and_the_next_call_is_clean(case):
    from pmce_amd import _lib
    bad = case["patches"].clone()
    bad[1, 2, 100, 100] = 1e30                         # beyond f16's range: infinity in the stem's gather
    with pytest.raises(_lib.PmceError, match="patch 1 "):
        case["ext"](bad)
    assert torch.equal(bits(case["ext"](case["patches"][:2]).cpu()), bits(case["feats"]))


def test_hmr_runs_in_f16_mode_and_reports_it():
    from pmce_amd import hmr
    import hmr_ref as HR
    sd = HR.hmr_state_dict()
    model = hmr.HMR.from_state_dict(sd, DEV, precision="f16")
    assert model.precision == "f16" and model.extractor.precision == "f16"
    patches = ER.patches(2).to(DEV)
    feats, out = model(patches, return_features=True)
    torch.cuda.synchronize()
    assert feats.shape == (2, 2048) and bool(torch.isfinite(feats).all()) and bool(torch.isfinite(out["theta"]).all())
    assert hmr.HMR.from_state_dict(sd, DEV).precision == "split_f16"


def test_the_workspace_is_about_half(case):
    from pmce_amd import _lib
    lib = _lib.load()
    for n in (1, 64):
        a, b = lib.pmce_extractor_workspace_bytes_for(case["ext"]._h, n), lib.pmce_extractor_workspace_bytes_for(case["default"]._h, n)
        print(f"n = {n}: {a} bytes against {b}")
        assert 0 < a <= 0.55 * b
    assert case["ext"]._ws.numel() * 4 <= 0.55 * case["default"]._ws.numel() * 4
