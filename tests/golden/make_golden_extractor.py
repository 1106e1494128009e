#!/usr/bin/env python3
"""Golden vectors for the feature extractor from the REAL reference code (build container only): HMR.feature_extractor and Bottleneck of
lib/models/spin.py on the seeded synthetic state dict (pmce_amd.synth.extractor_spec) and the seeded patches of tests/extractor_ref.py.
HMR.__init__ reads licensed SMPL files and spin.py imports torchvision, a geometry module and an SMPL wrapper at its top; the backbone
needs none of them, so the three imports are satisfied by empty stub modules and the network is made with HMR.__new__ +
torch.nn.Module.__init__ + the reference's own _make_layer calls.  Outputs only: the reference's fp64 results (``.double()`` on a deep
copy) and the largest absolute deviation of its own fp32 run from them, over the whole tensor - the yardstick of the tests.

    python tests/golden/make_golden_extractor.py /path/to/reference        (or PMCE_REFERENCE_DIR)"""
import copy
import importlib.util
import os
import os.path as osp
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = osp.dirname(osp.abspath(__file__)); REPO = osp.dirname(osp.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PMCE_REFERENCE_DIR", "")
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests"))
import extractor_ref as ER  # noqa: E402
from pmce_amd import synth  # noqa: E402


def load_spin():
    stubs = {"torchvision": {}, "torchvision.models": {}, "torchvision.models.resnet": {}, "geometry": {"rot6d_to_rotmat": None},
             "models": {}, "models.smpl_mps": {"SMPL": None}}
    for name, attrs in stubs.items():
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision.models"].resnet = sys.modules["torchvision.models.resnet"]
    spec = importlib.util.spec_from_file_location("reference_spin", osp.join(REF, "lib", "models", "spin.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_backbone(spin):
    net = spin.HMR.__new__(spin.HMR)
    nn.Module.__init__(net)
    net.inplanes = 64                                   # what _make_layer reads and advances
    net.conv1, net.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
    net.relu, net.maxpool, net.avgpool = nn.ReLU(True), nn.MaxPool2d(3, 2, 1), nn.AvgPool2d(7, 1)
    for i, (planes, blocks, stride) in enumerate(ER.LAYERS, 1):
        setattr(net, f"layer{i}", net._make_layer(spin.Bottleneck, planes, blocks, stride=stride))
    return net.eval()


def run_taps(net, x):
    taps = {}
    hooks = [getattr(net, t).register_forward_hook(lambda m, i, o, t=t: taps.__setitem__(t, o.detach().clone())) for t in ER.TAPS]
    with torch.no_grad():
        f = net.feature_extractor(x)
    for h in hooks:
        h.remove()
    return f, taps


def dev(a32, a64):
    assert torch.isfinite(a32).all() and torch.isfinite(a64).all()
    return np.float64((a32.double() - a64).abs().max())


def main():
    if not osp.isfile(osp.join(REF, "lib", "models", "spin.py")):
        raise SystemExit("give the reference checkout's directory as the first argument (or PMCE_REFERENCE_DIR)")
    spin = load_spin()
    net = make_backbone(spin)
    sd = synth.make_state_dict(synth.extractor_spec(), ER.SEED)
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
    net.load_state_dict(sd, strict=True)
    x = ER.patches()
    f32, t32 = run_taps(net, x)
    f64, t64 = run_taps(copy.deepcopy(net).double(), x.double())
    rec = {"feat64": f64.numpy(), "dev32_feat": dev(f32, f64), "seed": np.int64(ER.SEED), "patch_seed": np.int64(ER.PATCH_SEED),
           "keys": np.array(sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked")))}
    amax = float(f64.abs().max())
    for t in ER.TAPS:
        flat = t64[t].reshape(-1).numpy()
        rec[t + "_64"] = flat[ER.tap_index(flat.size)]
        rec["dev32_" + t] = dev(t32[t], t64[t])
        amax = max(amax, float(np.abs(flat).max()))
    zero = float((f64 == 0).double().mean())
    assert amax < 4096 and zero < 0.5, (amax, zero)
    # the two bottlenecks
    xb = ER.block_input()
    for name, (inplanes, planes, stride) in ER.BLOCK_CASES.items():
        ds = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes))
        blk = spin.Bottleneck(inplanes, planes, stride, ds).eval()
        bsd = {k[len(name) + 1:]: v for k, v in ER.block_state_dict(name).items()}
        for k, v in blk.state_dict().items():
            if k.endswith("num_batches_tracked"):
                bsd[k] = v
        blk.load_state_dict(bsd, strict=True)
        with torch.no_grad():
            o32 = blk(xb.clone())
            o64 = copy.deepcopy(blk).double()(xb.double())
        assert float(o64.abs().max()) < 4096
        rec[name + "_64"] = o64.numpy()
        rec["dev32_" + name] = dev(o32, o64)
    out = osp.join(HERE, "extractor.npz")
    np.savez_compressed(out, **rec)
    devs = {k: float(v) for k, v in rec.items() if k.startswith("dev32_")}
    print(f"{out}: max |activation| {amax:.1f}, zero features {100 * zero:.1f} %, {osp.getsize(out)} bytes")
    print(" ".join(f"{k} {v:.3e}" for k, v in devs.items()))
    assert osp.getsize(out) < 200 * 1024


if __name__ == "__main__":
    main()
