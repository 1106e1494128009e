"""GPU tests of the feature extractor as a network (pmce_amd/extractor.py on csrc/extractor.cpp and csrc/conv.hip) against the real
reference's recordings (tests/golden/extractor.npz: HMR.feature_extractor of lib/models/spin.py on the synthetic state dict).

The yardstick is the reference's OWN fp32 error, as in tests/test_gpu_smpl.py: features and stage outputs must stay within 4 x dev32 of
the reference's fp64 result, dev32 = the largest deviation of its fp32 run from its fp64 run on that tensor.  The extractor is built once
per module; every test prints the ratio it measures (run with -s)."""
import os.path as osp

import numpy as np
import pytest
import torch

import extractor_ref as ER
from conftest import GOLDEN
from pmce_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(synth.extractor_spec(), ER.SEED)


@pytest.fixture(scope="module")
def ext(sd):
    from pmce_amd.extractor import FeatureExtractor
    return FeatureExtractor.from_state_dict(sd, DEV)


@pytest.fixture(scope="module")
def patches():
    return ER.patches(3).to(DEV)


@pytest.fixture(scope="module")
def first(ext, patches):
    """Features and the four stage outputs of the fixture's two patches, computed once."""
    feats, taps = ext.forward(patches[:2], taps=ER.TAPS)
    torch.cuda.synchronize()
    return feats.cpu(), {k: v.cpu() for k, v in taps.items()}


def test_features_and_stage_outputs_against_the_reference(first):
    gold = np.load(osp.join(GOLDEN, "extractor.npz"))
    feats, taps = first
    assert feats.shape == (2, 2048) and taps["layer1"].shape == (2, 256, 56, 56) and taps["layer4"].shape == (2, 2048, 7, 7)
    worst = {}
    for t in ER.TAPS:
        flat = taps[t].contiguous().reshape(-1).double().numpy()
        worst[t] = float(np.abs(flat[ER.tap_index(flat.size)] - gold[t + "_64"]).max() / gold["dev32_" + t])
    worst["features"] = float(np.abs(feats.double().numpy() - gold["feat64"]).max() / gold["dev32_feat"])
    print("x dev32: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= FACTOR for v in worst.values()), worst
    assert float((feats == 0).float().mean()) < 0.5


def test_a_patch_does_not_depend_on_the_batch(ext, patches, first):
    """Patch 0 has the same bits for n = 1, 2 (the module's first run) and 3."""
    want = bits(first[0][0])
    for n in (1, 3):
        got = ext(patches[:n]).cpu()
        assert got.shape == (n, 2048) and torch.equal(bits(got[0]), want), f"patch 0 differs at n = {n}"
        if n == 3:
            assert torch.equal(bits(got[1]), bits(first[0][1]))


def test_chunking_and_repeated_calls(sd, ext, patches):
    from pmce_amd.extractor import FeatureExtractor
    a = ext(patches).cpu()
    b = ext(patches).cpu()
    assert torch.equal(bits(a), bits(b))
    one = FeatureExtractor.from_state_dict(sd, DEV, max_batch=1)
    c, taps = one.forward(patches, taps=("layer2",))
    assert torch.equal(bits(c.cpu()), bits(a))
    d, taps64 = ext.forward(patches, taps=("layer2",))
    assert taps["layer2"].shape == (3, 512, 28, 28) and torch.equal(bits(taps["layer2"].cpu()), bits(taps64["layer2"].cpu()))
    # strided patches (a channel-last view) are read through their strides
    cl = patches.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous() and torch.equal(bits(ext(cl).cpu()), bits(a))
    assert ext(patches[:0]).shape == (0, 2048)


def test_checkpoint_file_gives_the_same_bits(sd, ext, patches, tmp_path, first):
    from pmce_amd.extractor import FeatureExtractor
    full = {"module." + k: v for k, v in sd.items()}
    full.update({"module.fc1.weight": torch.zeros(4, 4), "module.decpose.weight": torch.zeros(2, 2), "module.init_pose": torch.zeros(1, 144),
                 "module.smpl.faces": torch.zeros(3, dtype=torch.int64), "module.bn1.num_batches_tracked": torch.tensor(7)})
    path = str(tmp_path / "spin.pth.tar")
    torch.save({"model": full, "epoch": 1}, path)
    got = FeatureExtractor.from_checkpoint(path, DEV)(patches[:2]).cpu()
    assert torch.equal(bits(got), bits(first[0]))
    torch.save({"state_dict": full}, path)
    with pytest.raises(ValueError, match="'model'"):
        FeatureExtractor.from_checkpoint(path, DEV)


def test_bad_patches_and_non_finite_features(ext, patches):
    from pmce_amd import _lib
    with pytest.raises(ValueError, match=r"\[n, 3, 224, 224\]"):
        ext(torch.zeros(1, 3, 256, 256, device=DEV))
    with pytest.raises(ValueError, match="taps"):
        ext.forward(patches[:1], taps=("layer5",))
    bad = patches.clone()
    bad[1, 2, 100, 100] = float("nan")
    with pytest.raises(_lib.PmceError, match="patch 1 "):
        ext(bad)


def video(n_frames=24, H=240, W=320):
    """Frames and two tracklets of 20 and 22 frames whose keypoints span a person-sized box inside the 320 x 240 frame."""
    rng = np.random.default_rng(17)
    fr = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    out = []
    for n, first_frame in ((20, 2), (22, 0)):
        xy = rng.uniform(0, 1, (1, 17, 2)) * np.array([60.0, 120.0]) + rng.uniform(40, 100, (n, 1, 2)) + rng.normal(0, 1.0, (n, 17, 2))
        kp = np.concatenate([xy, rng.uniform(0.4, 0.95, (n, 17, 1))], -1).astype(np.float32)
        out.append((kp, np.arange(first_frame, first_frame + n)))
    return fr, out


def test_run_video_with_the_extractor(ext):
    """Frames -> meshes with the extractor as ``run_video``'s callable: bit-identical to ``run_tracklets`` fed the extractor's features of
    the patches ``crop_tracklets`` cuts, computed separately."""
    from pmce_amd import demo
    from test_gpu_demo import get_model
    model = get_model(256)
    fr, tracks = video()
    frames = torch.from_numpy(fr).to(DEV)
    outs = demo.run_video(model, frames, tracks, ext, (320, 240), seed=3)
    c = demo.crop_tracklets(frames, tracks)
    off = c["offsets"]
    assert off.tolist() == [0, 20, 42] and not bool(c["status"].any())
    feats = ext(c["patches"])
    want = demo.run_tracklets(model, [(c["keypoints"][i], feats[int(off[i]):int(off[i + 1])]) for i in range(2)], (320, 240), seed=3)
    torch.cuda.synchronize()
    assert len(outs) == 2
    for o, w in zip(outs, want):
        for key in w:
            assert torch.equal(o[key], w[key]), key
