"""Host tests of the feature extractor: the CPU restatement (tests/extractor_ref.py) against the real reference's recordings
(tests/golden/extractor.npz, made by tests/golden/make_golden_extractor.py from lib/models/spin.py), the BatchNorm folding, the state
dict handling and the argument checks of pmce_amd/extractor.py.  No GPU.

The yardstick, here as on the device: every comparison is against the reference's fp64 result, the allowed error is 4 x dev32 = four
times the largest deviation of the reference's OWN fp32 run from its fp64 run on that tensor (the project's factor for "another
summation order").  Each test prints the ratio it measures (run with -s)."""
import os.path as osp
import re

import numpy as np
import pytest
import torch

import extractor_ref as ER
from conftest import GOLDEN, REPO
from pmce_amd import extractor as EX
from pmce_amd import synth

FACTOR = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "extractor.npz"))


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(synth.extractor_spec(), ER.SEED)


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def ratio(got, want64, dev32, what):
    r = float(np.abs(np.asarray(got, np.float64) - want64).max() / dev32)
    print(f"{what}: {r:.2f} x dev32 ({dev32:.2e})")
    return r


def test_restatement_matches_the_recorded_network(gold, sd):
    with torch.no_grad():
        feat, taps = ER.forward(ER.fold_state_dict(sd), ER.patches())
    assert ratio(feat.numpy(), gold["feat64"], gold["dev32_feat"], "features") <= FACTOR
    for t in ER.TAPS:
        flat = taps[t].reshape(-1).numpy()
        assert ratio(flat[ER.tap_index(flat.size)], gold[t + "_64"], gold["dev32_" + t], t) <= FACTOR


@pytest.mark.parametrize("name", sorted(ER.BLOCK_CASES))
def test_restatement_matches_the_recorded_bottlenecks(gold, name):
    _, _, stride = ER.BLOCK_CASES[name]
    with torch.no_grad():
        out = ER.bottleneck(ER.block_input(), ER.fold_block(name), name, stride, True)
    assert out.shape == gold[name + "_64"].shape
    assert ratio(out.numpy(), gold[name + "_64"], gold["dev32_" + name], name) <= FACTOR


def test_folding_formula_against_fp64_batchnorm():
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(5, 7, 3, stride=2, padding=1, bias=False).double()
    bn = torch.nn.BatchNorm2d(7).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(7, 5, 3, 3, generator=g).float())
        bn.weight.copy_(torch.rand(7, generator=g).float() + 0.5)
        bn.bias.copy_(torch.randn(7, generator=g).float())
        bn.running_mean.copy_(torch.randn(7, generator=g).float())
        bn.running_var.copy_(torch.rand(7, generator=g).float() + 0.5)
        x = torch.randn(2, 5, 9, 8, generator=g).double()
        want = bn(conv(x))
        for fold in (ER.fold_bn, EX.fold_bn):
            w, b = fold(conv.weight.float(), bn.weight.float(), bn.bias.float(), bn.running_mean.float(), bn.running_var.float())
            assert w.dtype == torch.float32 and b.dtype == torch.float32
            got = torch.nn.functional.conv2d(x, w.double(), b.double(), stride=2, padding=1)
            # the folded values are fp32 roundings of the exact ones: 45 products of relative error 2^-24 each
            assert float((got - want).abs().max()) <= 46 * 2.0 ** -24 * float((x.abs().max() * conv.weight.abs().max() * 4))
        assert torch.equal(ER.fold_bn(conv.weight.float(), bn.weight.float(), bn.bias.float(), bn.running_mean.float(), bn.running_var.float())[0], w)


def test_spec_is_deterministic_and_has_the_reference_key_set(gold, sd):
    again = synth.make_state_dict(synth.extractor_spec(), ER.SEED)
    assert list(again) == list(sd) and all(torch.equal(again[k], sd[k]) for k in sd)
    other = synth.make_state_dict(synth.extractor_spec(), ER.SEED + 1)
    assert not torch.equal(other["conv1.weight"], sd["conv1.weight"])
    assert sorted(sd) == [str(k) for k in gold["keys"]]           # strict=True against the reference module's own keys
    assert list(EX.required_keys()) == list(sd) and all(tuple(sd[k].shape) == tuple(s) for k, s in EX.required_keys().items())
    assert sum(v.numel() for v in sd.values()) == 23561152
    assert [c[0] for c in ER.conv_list()] == [c[0] for c in EX.conv_table()] and len(EX.conv_table()) == 53
    bn3 = sd["layer2.1.bn3.weight"]
    assert 0.25 <= float(bn3.min()) and float(bn3.max()) <= 0.75 and 0.5 <= float(sd["layer2.1.bn2.weight"].min())
    w = sd["layer3.0.conv2.weight"]
    assert float(w.abs().max()) <= np.sqrt(6.0 / (256 * 9)) and float(w.abs().max()) > 0.99 * np.sqrt(6.0 / (256 * 9))


def test_state_dict_prefix_and_ignored_keys(sd):
    wrapped = {"module." + k: v for k, v in sd.items()}
    wrapped.update({"module.fc1.weight": torch.zeros(2), "module.decpose.bias": torch.zeros(1), "module.init_pose": torch.zeros(1),
                    "module.smpl.faces": torch.zeros(1), "module.bn1.num_batches_tracked": torch.tensor(0), "module.fc2.bias": torch.zeros(3)})
    got = EX.select_state_dict(wrapped)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    got = EX.select_state_dict({k: v.double() for k, v in sd.items()})
    assert all(v.dtype == torch.float32 for v in got.values())


def test_state_dict_errors_name_the_tensor(sd):
    broken = dict(sd)
    del broken["layer3.4.bn2.running_var"]
    with pytest.raises(ValueError, match=re.escape("'layer3.4.bn2.running_var'")):
        EX.select_state_dict(broken)
    broken = dict(sd)
    broken["layer2.0.downsample.0.weight"] = torch.zeros(512, 256, 3, 3)
    with pytest.raises(ValueError, match=r"'layer2\.0\.downsample\.0\.weight' has shape \(512, 256, 3, 3\), expected \(512, 256, 1, 1\)"):
        EX.select_state_dict(broken)
    with pytest.raises(ValueError, match="'conv1.weight'"):
        EX.select_state_dict({})
    with pytest.raises(ValueError, match="mapping"):
        EX.select_state_dict([1, 2])


@pytest.mark.parametrize("bad", [torch.zeros(2, 3, 224, 223), torch.zeros(2, 3, 256, 256), torch.zeros(3, 224, 224), torch.zeros(1, 1, 224, 224),
                                 torch.zeros(1, 3, 224, 224, dtype=torch.float64), np.zeros((1, 3, 224, 224), np.float32)])
def test_only_224_patches_are_accepted(bad):
    with pytest.raises(ValueError, match=r"\[n, 3, 224, 224\]"):
        EX.check_patches(bad)
    assert EX.check_patches(torch.zeros(0, 3, 224, 224)) == 0 and EX.check_patches(torch.zeros(5, 3, 224, 224)) == 5


def test_int64_convolution_oracle():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-4, 5, (2, 3, 9, 8), generator=g)
    w = torch.randint(-3, 4, (4, 3, 3, 3), generator=g)
    for stride, pad in ((1, 1), (2, 1), (2, 0)):
        want = torch.nn.functional.conv2d(x.double(), w.double(), stride=stride, padding=pad)
        assert torch.equal(ER.conv2d_int(x, w, stride, pad).double(), want)


def test_entries_are_declared_bound_and_built(lib):
    from pmce_amd import _lib, build
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    for name, n_args in (("pmce_conv_pack_split_f16", 8), ("pmce_conv2d_split_f16", 21), ("pmce_maxpool3x3s2_nhwc_f32", 7),
                         ("pmce_avgpool_nhwc_f32", 6), ("pmce_extractor_forward", 15), ("pmce_extractor_set_conv", 4)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not prototyped in include/pmce_hip.h"
        assert len(m.group(1).split(",")) == n_args == len(_lib.PROTOTYPES[name]), name
        assert hasattr(lib, name)
    assert "extractor.cpp" in build.SOURCES and osp.exists(osp.join(build.CSRC, "conv.hip"))


def test_argument_validation_without_gpu(lib):
    import ctypes as C
    from pmce_amd import _lib
    assert lib.pmce_conv_packed_floats(64, 3, 7, 7) == 64 * 160 and lib.pmce_conv_packed_floats(192, 128, 3, 3) == 192 * 1152
    assert lib.pmce_conv_packed_floats(65, 16, 1, 1) == 128 * 32 and lib.pmce_conv_packed_floats(0, 3, 7, 7) == 0
    rc = lib.pmce_conv2d_split_f16(16, 1, 1, 1, 1, 1, 3, 4, 4, 16, 16, None, None, 16, 8, 3, 3, 1, 3, 0, None)
    assert rc == -1 and "pad" in _lib.last_error()
    assert lib.pmce_maxpool3x3s2_nhwc_f32(16, 16, 1, 4, 4, 6, None) == -1 and "C % 4" in _lib.last_error()
    assert lib.pmce_extractor_workspace_bytes(0) == 0
    assert lib.pmce_extractor_workspace_bytes(2) == 2 * (3 * 112 * 112 * 64 + 2 * 56 * 56 * 128) * 4
    h = C.c_void_p()
    assert lib.pmce_extractor_create(C.byref(h)) == 0
    names = [lib.pmce_extractor_conv_name(h, i).decode() for i in range(lib.pmce_extractor_conv_count(h))]
    assert names == [c[0] for c in EX.conv_table()]
    shape = (C.c_int * 4)()
    for i, (_, _, s) in enumerate(EX.conv_table()):
        assert lib.pmce_extractor_conv_shape(h, i, shape) == 0 and tuple(shape) == tuple(s)
    assert lib.pmce_extractor_set_conv(h, b"layer9.0.conv1", 16, 16) == -1 and "layer9.0.conv1" in _lib.last_error()
    assert lib.pmce_extractor_finalize_on(h, None) == -1 and "'conv1' was not set" in _lib.last_error()
    assert lib.pmce_extractor_forward(h, 16, 1, 1, 1, 1, 16, 1, None, None, None, None, 16, 1 << 40, None) == -1
    assert "not finalized" in _lib.last_error()
    lib.pmce_extractor_destroy(h)
