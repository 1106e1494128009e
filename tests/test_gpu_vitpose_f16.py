"""GPU tests of ViTPose's single-product f16 mode as a network (``ViTPose(..., precision="f16")``) against tests/vitpose_f16_ref.py, the
restatement of the mode's arithmetic run on the CPU in fp64 and fp32, and against tests/vitpose_ref.py's plain fp64 run.

Heatmaps and the backbone's map must stay within 4 x dev32r of the restatement's fp64 run (dev32r: its fp32 run against its fp64 run) and
within 4 x dev16 of the plain fp64 run (dev16: the restatement's fp64 run against it - what f16 operands cost by themselves).  The three
mini networks of tests/test_gpu_vitpose.py and one of depth 4.  Every test prints the ratios it measures (run with -s)."""
import numpy as np
import pytest
import torch

import pose2d_ref as PR
import vitpose_f16_ref as FR
import vitpose_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = FR.FACTOR

NETS = {
    "hd80": dict(H=256, W=192, C=160, depth=2, heads=2, F1=32, F2=32, K=17),
    "hd64": dict(H=64, W=48, C=128, depth=1, heads=2, F1=32, F2=32, K=17),
    "hd64_80tok": dict(H=160, W=128, C=128, depth=1, heads=2, F1=32, F2=32, K=17),
    "hd64_depth4": dict(H=64, W=48, C=128, depth=4, heads=2, F1=32, F2=32, K=17),
}


def bits(t):
    return t.contiguous().view(torch.int32)


def spec_args(cfg):
    return dict(C=cfg["C"], depth=cfg["depth"], heads=cfg["heads"], F1=cfg["F1"], F2=cfg["F2"], K=cfg["K"], img_size=(cfg["H"], cfg["W"]))


@pytest.fixture(scope="module", params=list(NETS))
def net(request):
    """(cfg, state dict, the default-mode result of the first two patches BEFORE any f16 network exists, the f16 network, three patches on
    the device, its (heat, feat) of the first two) - once per network."""
    from pmce_amd.vitpose import ViTPose
    cfg = NETS[request.param]
    size = (cfg["H"], cfg["W"])
    sd = VR.state_dict(**spec_args(cfg))
    x = VR.patches(3, size).to(DEV)
    split = ViTPose.from_state_dict(sd, DEV, img_size=size)
    assert split.precision == "split_f16"
    before = split.forward(x[:2], return_features=True)
    before = (before[0].cpu(), before[1].cpu())
    vp = ViTPose.from_state_dict(sd, DEV, img_size=size, precision="f16")
    assert vp.cfg == cfg and vp.precision == "f16"
    heat, feat = vp.forward(x[:2], return_features=True)
    torch.cuda.synchronize()
    return cfg, sd, (split, before), vp, x, (heat.cpu(), feat.cpu())


def test_heatmaps_and_features_against_the_restatement(net):
    cfg, sd, _, vp, x, (heat, feat) = net
    Hp, Wp = cfg["H"] // 16, cfg["W"] // 16
    assert heat.shape == (2, cfg["K"], 4 * Hp, 4 * Wp) and feat.shape == (2, cfg["C"], Hp, Wp)
    (h64r, f64r), (dev_h, dev_f) = FR.run_both(sd, cfg, x[:2].cpu())
    (h64, f64), (d32_h, d32_f) = VR.run_both(sd, cfg, x[:2].cpu())
    dev16_h, dev16_f = float((h64r - h64).abs().max()), float((f64r - f64).abs().max())
    rh = float((heat.double() - h64r).abs().max()) / dev_h
    rf = float((feat.double() - f64r).abs().max()) / dev_f
    ph = float((heat.double() - h64).abs().max()) / dev16_h
    pf = float((feat.double() - f64).abs().max()) / dev16_f
    print(f"C={cfg['C']} N={Hp * Wp} depth={cfg['depth']}: x dev32r: heatmaps {rh:.2f} (dev32r {dev_h:.2e}), features {rf:.2f} (dev32r {dev_f:.2e}); "
          f"x dev16: heatmaps {ph:.2f} (dev16 {dev16_h:.2e} = {dev16_h / d32_h:.0f} dev32), features {pf:.2f} (dev16 {dev16_f:.2e} = "
          f"{dev16_f / d32_f:.0f} dev32)")
    assert rh <= FACTOR and rf <= FACTOR
    assert ph <= FACTOR and pf <= FACTOR
    assert float((heat.abs() > 1e-6).float().mean()) > 0.5, "the network is dead"
    assert float(h64.abs().max()) > 0.1


def test_a_patch_does_not_depend_on_the_batch(net):
    from pmce_amd.vitpose import ViTPose
    cfg, sd, _, vp, x, (heat, feat) = net
    want = bits(heat[0])
    for n in (1, 2, 3):
        got = vp(x[:n]).cpu()
        assert got.shape[0] == n and torch.equal(bits(got[0]), want), f"patch 0 differs at n = {n}"
        if n >= 2:
            assert torch.equal(bits(got[1]), bits(heat[1]))
        if n == 3:
            full = got
    one = ViTPose.from_state_dict(sd, DEV, img_size=(cfg["H"], cfg["W"]), max_batch=1, precision="f16")
    h1, f1 = one.forward(x, return_features=True)
    assert torch.equal(bits(h1.cpu()), bits(full)) and torch.equal(bits(f1[:2].cpu()), bits(feat))


def test_the_default_mode_keeps_its_bits_and_the_f16_mode_is_in_use(net):
    from pmce_amd.vitpose import ViTPose
    cfg, sd, (split, before), vp, x, (heat, feat) = net
    after = split.forward(x[:2], return_features=True)                 # the same handle, after f16 forwards in the same process
    fresh = ViTPose.from_state_dict(sd, DEV, img_size=(cfg["H"], cfg["W"])).forward(x[:2], return_features=True)
    for got in (after, fresh):
        assert torch.equal(bits(got[0].cpu()), bits(before[0])) and torch.equal(bits(got[1].cpu()), bits(before[1]))
    assert not torch.equal(bits(heat), bits(before[0])) and not torch.equal(bits(feat), bits(before[1])), "the f16 mode gives the default mode's bits"
    assert float((heat - before[0]).abs().max()) > 1e-5


def test_checkpoint_file_gives_the_f16_bits(net, tmp_path):
    from pmce_amd.vitpose import ViTPose
    cfg, sd, _, vp, x, (heat, feat) = net
    path = str(tmp_path / "vitpose.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    got = ViTPose.from_checkpoint(path, DEV, img_size=(cfg["H"], cfg["W"]), precision="f16")
    assert got.precision == "f16" and torch.equal(bits(got(x[:2]).cpu()), bits(heat))


def test_a_value_beyond_the_range_is_reported_and_the_next_call_is_clean(net):
    from pmce_amd import _lib
    cfg, sd, _, vp, x, (heat, feat) = net
    bad = x.clone()
    bad[1, 2, cfg["H"] // 2, cfg["W"] // 2] = 1e30
    with pytest.raises(_lib.PmceError, match="patch 1 "):
        vp(bad)
    assert torch.equal(bits(vp(x[:2]).cpu()), bits(heat))


def test_top_down_pose_runs_on_the_f16_network(net):
    """Wiring only: boxes of a small synthetic frame -> finite keypoints of the right shape, status 0."""
    from pmce_amd import pose2d
    cfg, sd, _, vp, x, _ = net
    frames = torch.from_numpy(PR.frames()).to(DEV)
    boxes = np.array([(40.0, 30.0, 20.0, 30.0), (41.0, 31.0, 50.0, 20.0)])
    kp, st = pose2d.TopDownPose(vp)(frames, np.array([0, 1], np.int32), boxes)
    assert kp.shape == (2, cfg["K"], 3) and st.tolist() == [0, 0] and bool(torch.isfinite(kp).all())
