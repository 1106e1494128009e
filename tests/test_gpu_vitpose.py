"""GPU tests of ViTPose as a network (pmce_amd/vitpose.py on csrc/vitpose.cpp) against tests/vitpose_ref.py, the plain torch module
of the same structure run on the CPU in fp64 and fp32.  No tensor was recorded from mmpose.

Heatmaps and the backbone's map must stay within 4 x dev32 of the module's fp64 result, dev32 = the largest deviation of its fp32 run
from its fp64 run on that tensor.  Two small networks, each built once per module: 256 x 192 patches (192 tokens) at C = 160 with two
heads of 80 and two blocks, and 64 x 48 patches (12 tokens: one partial attention tile) at C = 128 with two heads of 64 and one block.
Every test prints the ratio it measures (run with -s)."""
import pytest
import torch

import vitpose_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = VR.FACTOR

NETS = {
    "hd80": dict(H=256, W=192, C=160, depth=2, heads=2, F1=32, F2=32, K=17),
    "hd64": dict(H=64, W=48, C=128, depth=1, heads=2, F1=32, F2=32, K=17),
    "hd64_80tok": dict(H=160, W=128, C=128, depth=1, heads=2, F1=32, F2=32, K=17),     # 80 tokens: three key tiles inside the network
}


def bits(t):
    return t.contiguous().view(torch.int32)


def spec_args(cfg):
    return dict(C=cfg["C"], depth=cfg["depth"], heads=cfg["heads"], F1=cfg["F1"], F2=cfg["F2"], K=cfg["K"], img_size=(cfg["H"], cfg["W"]))


@pytest.fixture(scope="module", params=list(NETS))
def net(request):
    """(cfg, state dict, the device network, three patches on the device, (heat, feat) of the first two) - once per network."""
    from pmce_amd.vitpose import ViTPose
    cfg = NETS[request.param]
    sd = VR.state_dict(**spec_args(cfg))
    vp = ViTPose.from_state_dict(sd, DEV, img_size=(cfg["H"], cfg["W"]))
    assert vp.cfg == cfg
    x = VR.patches(3, (cfg["H"], cfg["W"])).to(DEV)
    heat, feat = vp.forward(x[:2], return_features=True)
    torch.cuda.synchronize()
    return cfg, sd, vp, x, (heat.cpu(), feat.cpu())


def test_heatmaps_and_features_against_the_reference(net):
    cfg, sd, vp, x, (heat, feat) = net
    Hp, Wp = cfg["H"] // 16, cfg["W"] // 16
    assert heat.shape == (2, cfg["K"], 4 * Hp, 4 * Wp) and feat.shape == (2, cfg["C"], Hp, Wp)
    (h64, f64), (dev_h, dev_f) = VR.run_both(sd, cfg, x[:2].cpu())
    rh = float((heat.double() - h64).abs().max()) / dev_h
    rf = float((feat.double() - f64).abs().max()) / dev_f
    print(f"C={cfg['C']} N={Hp * Wp}: x dev32: heatmaps {rh:.2f} (dev32 {dev_h:.2e}), features {rf:.2f} (dev32 {dev_f:.2e})")
    assert rh <= FACTOR and rf <= FACTOR
    assert float((heat.abs() > 1e-6).float().mean()) > 0.5, "the network is dead"
    assert float(h64.abs().max()) > 0.1


def test_a_patch_does_not_depend_on_the_batch(net):
    from pmce_amd.vitpose import ViTPose
    cfg, sd, vp, x, (heat, feat) = net
    want = bits(heat[0])
    for n in (1, 3):
        got = vp(x[:n]).cpu()
        assert got.shape[0] == n and torch.equal(bits(got[0]), want), f"patch 0 differs at n = {n}"
        if n == 3:
            assert torch.equal(bits(got[1]), bits(heat[1]))
            full = got
    one = ViTPose.from_state_dict(sd, DEV, img_size=(cfg["H"], cfg["W"]), max_batch=1)
    h1, f1 = one.forward(x, return_features=True)
    assert torch.equal(bits(h1.cpu()), bits(full)) and torch.equal(bits(f1[:2].cpu()), bits(feat))


def test_repeated_calls_and_strided_patches(net):
    cfg, sd, vp, x, (heat, feat) = net
    a, b = vp(x).cpu(), vp(x).cpu()
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a[:2]), bits(heat))
    cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # a channel-last view, read through its strides
    assert not cl.is_contiguous() and torch.equal(bits(vp(cl).cpu()), bits(a))
    assert torch.equal(bits(vp(x.cpu()).cpu()), bits(a))            # a host tensor is uploaded


def test_empty_and_bad_input(net):
    from pmce_amd import _lib
    cfg, sd, vp, x, (heat, feat) = net
    H, W, Hp, Wp = cfg["H"], cfg["W"], cfg["H"] // 16, cfg["W"] // 16
    assert vp(x[:0]).shape == (0, 17, 4 * Hp, 4 * Wp)
    h, f = vp.forward(x[:0], return_features=True)
    assert h.shape == (0, 17, 4 * Hp, 4 * Wp) and f.shape == (0, cfg["C"], Hp, Wp)
    with pytest.raises(ValueError, match=rf"\[n, 3, {H}, {W}\]"):
        vp(torch.zeros(1, 3, 224, 224, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        vp(x.double())
    bad = x.clone()
    bad[1, 2, H // 2, W // 2] = float("nan")
    with pytest.raises(_lib.PmceError, match="patch 1 "):
        vp(bad)
    assert torch.equal(bits(vp(x[:2]).cpu()), bits(heat))            # and the network still works


def test_checkpoint_file_gives_the_same_bits(net, tmp_path):
    from pmce_amd.vitpose import ViTPose
    cfg, sd, vp, x, (heat, feat) = net
    size = (cfg["H"], cfg["W"])
    full = {"module." + k: v for k, v in sd.items()}
    full.update({"module.associate_keypoint_heads.0.final_layer.weight": torch.zeros(14, 32, 1, 1),
                 "module.keypoint_head.deconv_layers.1.num_batches_tracked": torch.tensor(7)})
    path = str(tmp_path / "vitpose.pth")
    torch.save({"state_dict": full, "meta": {"epoch": 210}}, path)
    got = ViTPose.from_checkpoint(path, DEV, img_size=size)(x[:2]).cpu()
    assert torch.equal(bits(got), bits(heat))
    torch.save({"model": full}, path)
    with pytest.raises(ValueError, match="'state_dict'"):
        ViTPose.from_checkpoint(path, DEV, img_size=size)
