#!/usr/bin/env python3
"""Golden vectors for SPIN's regression head from the REAL reference code (build container only): Regressor.forward and HMR.forward of
lib/models/spin.py with the real lib/geometry.py (rot6d_to_rotmat, rotation_matrix_to_angle_axis) and spin.py's own projection, on the
seeded inputs of tests/hmr_ref.py.  spin.py imports torchvision and an SMPL wrapper at its top; torchvision is an empty stub as in
make_golden_extractor.py, the geometry module is the real one, and the networks are made with __new__ + their layers (their __init__
reads licensed SMPL files).

``self.smpl`` is a stand-in: the reference's wrapper (lib/models/smpl_mps.py) derives from smplx's SMPL, and smplx is absent here.  The
stand-in feeds the reference's OWN smplpytorch SMPL_Layer (built as make_golden_smpl.py builds it) - the same linear blend skinning on the
same model arrays: v_shaped, regressed joints, pose blend shapes, the kinematic chain, skinning.  That layer takes axis-angle, so its
pose input is geometry.rotation_matrix_to_angle_axis of the rotation matrices, computed in fp64 in both runs; every rotation of the
fixture stays below 2.5 rad (asserted), where that round trip is exact to fp64 rounding.  The extra joints are smpl_mps.py:71-83 applied to
the layer's outputs: the 24 posed joints, 21 vertices (smplx's vertex joint selector; seeded ids, its table is not available), the rows of
a seeded J_regressor_extra, indexed by the joint map - which is read from smpl_mps.py's text and compared with pmce_amd.hmr's restatement.

Outputs only: the reference's fp64 results (``.double()`` on a deep copy, torch's default dtype set to float64 for that run because
spin.py's projection creates its constants in the default dtype) and, per output, dev32 = the largest deviation of its own fp32 run.

    python tests/golden/make_golden_hmr_head.py /path/to/reference        (or PMCE_REFERENCE_DIR)"""
import ast
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
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests")); sys.path.insert(0, HERE); sys.path.insert(0, osp.join(REF, "smplpytorch"))
import extractor_ref as ER  # noqa: E402
import hmr_ref as HR  # noqa: E402
import make_golden_extractor as MGE  # noqa: E402
import make_golden_smpl as MGS  # noqa: E402
from pmce_amd import hmr  # noqa: E402


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    geometry = load_module("geometry", osp.join(REF, "lib", "geometry.py"))            # the REAL one, under the name spin.py imports
    for name in ("torchvision", "torchvision.models", "torchvision.models.resnet", "models", "models.smpl_mps"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision.models"].resnet = sys.modules["torchvision.models.resnet"]
    sys.modules["models.smpl_mps"].SMPL = None
    spin = load_module("reference_spin", osp.join(REF, "lib", "models", "spin.py"))
    spin.rotation_matrix_to_angle_axis = geometry.rotation_matrix_to_angle_axis        # spin.py calls it without importing it
    return spin, geometry


def reference_joint_map():
    """JOINT_MAP / JOINT_NAMES literals of smpl_mps.py (the module itself needs smplx)."""
    tree = ast.parse(open(osp.join(REF, "lib", "models", "smpl_mps.py")).read())
    lit = {t.targets[0].id: ast.literal_eval(t.value) for t in tree.body
           if isinstance(t, ast.Assign) and getattr(t.targets[0], "id", "") in ("JOINT_MAP", "JOINT_NAMES")}
    return lit["JOINT_NAMES"], [lit["JOINT_MAP"][n] for n in lit["JOINT_NAMES"]]


MAX_ANGLE = [0.0]       # the largest rotation angle the stand-in has seen (module-level: the runs work on deep copies of it)


class SmplStandIn(nn.Module):
    """What spin.py calls as self.smpl(betas=, body_pose=, global_orient=, pose2rot=False) -> .vertices, .joints (see the docstring)."""

    def __init__(self, layer, geometry, ids, jr_extra, joint_map):
        super().__init__()
        self.layer = layer
        self.to_angle_axis = [geometry.rotation_matrix_to_angle_axis]     # (in a list: deep copies share the function)
        self.register_buffer("J_regressor_extra", torch.tensor(jr_extra, dtype=torch.float32))
        self.ids = torch.tensor(ids, dtype=torch.long)
        self.joint_map = torch.tensor(joint_map, dtype=torch.long)

    def forward(self, betas, body_pose, global_orient, pose2rot):
        assert pose2rot is False
        R = torch.cat([global_orient, body_pose], 1)
        n = R.shape[0]
        aa = self.to_angle_axis[0](R.double().reshape(-1, 3, 3)).reshape(n, 72)
        MAX_ANGLE[0] = max(MAX_ANGLE[0], float(aa.reshape(-1, 3).norm(dim=1).max()))
        verts, jtr = self.layer(aa.to(betas.dtype), betas)
        extra = torch.einsum("bik,ji->bjk", [verts, self.J_regressor_extra])            # smplx.lbs.vertices2joints
        joints = torch.cat([jtr, verts[:, self.ids], extra], 1)[:, self.joint_map]
        return types.SimpleNamespace(vertices=verts, joints=joints)


def add_head(net, sd):
    net.fc1, net.drop1 = nn.Linear(2048 + 157, 1024), nn.Dropout()
    net.fc2, net.drop2 = nn.Linear(1024, 1024), nn.Dropout()
    net.decpose, net.decshape, net.deccam = nn.Linear(1024, 144), nn.Linear(1024, 10), nn.Linear(1024, 3)
    for k in ("init_pose", "init_shape", "init_cam"):
        net.register_buffer(k, sd[k].clone())


def both_runs(spin, net, x, **kw):
    """(fp32 outputs, fp64 outputs) of net(x): dicts of tensors, with the 6D pose the regressor hands to rot6d_to_rotmat as 'pose6d'."""
    real, seen = spin.rot6d_to_rotmat, {}

    def spy(p):
        seen["pose6d"] = p.detach().clone()
        return real(p)

    spin.rot6d_to_rotmat = spy
    outs = []
    try:
        for dt in (torch.float32, torch.float64):
            torch.set_default_dtype(dt)
            m = copy.deepcopy(net).to(dt).eval()
            with torch.no_grad():
                r = m(x.to(dt), **kw)
            feats, r = (r[0], r[1]) if isinstance(r, tuple) else (None, r)
            o = dict(r[0]); o["pose6d"] = seen["pose6d"]
            if feats is not None:
                o["features"] = feats
            outs.append(o)
    finally:
        torch.set_default_dtype(torch.float32)
        spin.rot6d_to_rotmat = real
    return outs


def dev(a32, a64):
    d = (a32.double() - a64).abs()
    d[torch.isnan(a32) & torch.isnan(a64)] = 0.0
    assert torch.isfinite(d).all()
    return d


def main():
    if not osp.isfile(osp.join(REF, "lib", "models", "spin.py")):
        raise SystemExit("give the reference checkout's directory as the first argument (or PMCE_REFERENCE_DIR)")
    spin, geometry = load_reference()
    names, jmap = reference_joint_map()
    assert tuple(names) == hmr.JOINT_NAMES and tuple(jmap) == hmr.JOINT_MAP, "pmce_amd.hmr's joint table is not smpl_mps.py's"
    sd = HR.state_dict()
    ids, jre = HR.extra_vertex_ids(), HR.extra_regressor()
    stand_in = SmplStandIn(MGS.make_layer(HR.smpl_model()), geometry, ids, jre, jmap)
    rec = {"seed": np.int64(HR.SEED), "n": np.int64(HR.N_GOLDEN), "V": np.int64(HR.V_GOLDEN)}

    # 1. the head: Regressor.forward on seeded features
    reg = spin.Regressor.__new__(spin.Regressor)
    nn.Module.__init__(reg)
    add_head(reg, sd)
    reg.smpl = stand_in
    reg.load_state_dict({k: v for k, v in sd.items()}, strict=False)
    missing = set(dict(reg.named_parameters())) - set(sd)
    assert not missing, missing
    x = torch.from_numpy(HR.features())
    o32, o64 = both_runs(spin, reg, x)
    for o in (o32, o64):
        o["state"] = torch.cat([o["pose6d"], o["theta"][:, 75:], o["theta"][:, :3]], 1)
    for k in ("theta", "rotmat", "state", "verts", "kp_3d", "kp_2d"):
        assert torch.isfinite(o64[k]).all()
        rec[k + "64"] = o64[k].numpy()
        rec["dev32_" + k] = np.float64(dev(o32[k], o64[k]).max())
    assert 0 < MAX_ANGLE[0] < HR.MAX_ANGLE, MAX_ANGLE
    head_angle = MAX_ANGLE[0]

    # 2. the two rotation functions alone, on the table of cases
    cnames, six = HR.rotation_cases()
    runs = []
    for dt in (torch.float32, torch.float64):
        R = geometry.rot6d_to_rotmat(torch.tensor(six, dtype=dt))
        runs.append((R, geometry.rotation_matrix_to_angle_axis(R.clone())))
    (R32, a32), (R64, a64) = runs
    ok = ~torch.isnan(R64).any(dim=2).any(dim=1).numpy()
    b32, b64 = HR.quaternion_branch(R32.numpy(), np.float32), HR.quaternion_branch(R64.numpy(), np.float64)
    assert np.array_equal(b32[ok], b64[ok]), (b32, b64)
    assert set(b64[ok]) == {0, 1, 2, 3}
    assert np.array_equal(torch.isnan(R32).numpy(), torch.isnan(R64).numpy()) and torch.isfinite(a32).all() and torch.isfinite(a64).all()
    rec.update(rot_names=np.array(cnames), rot_rotmat64=R64.numpy(), rot_aa64=a64.numpy(), rot_branch=b64.astype(np.int64),
               rot_dev32_rotmat=dev(R32, R64).reshape(len(cnames), -1).max(dim=1).values.numpy(),
               rot_dev32_aa=dev(a32, a64).max(dim=1).values.numpy())

    # 3. HMR.forward(return_features=True) on the extractor's patches: backbone + head
    net = MGE.make_backbone(spin)
    add_head(net, sd)
    net.smpl = stand_in
    full = HR.hmr_state_dict()
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            full[k] = v
    net.load_state_dict({k: v for k, v in full.items() if not k.startswith("smpl.")}, strict=False)
    assert not [k for k in net.state_dict() if k not in full and not k.startswith("smpl.")]
    MAX_ANGLE[0] = 0.0
    h32, h64 = both_runs(spin, net, ER.patches(), return_features=True)
    assert 0 < MAX_ANGLE[0] < HR.MAX_ANGLE, MAX_ANGLE
    for k in ("features", "theta", "verts", "kp_3d", "kp_2d"):
        assert torch.isfinite(h64[k]).all()
        if k != "features":             # (the features are the extractor fixture's)
            rec["hmr_" + k + "64"] = h64[k].numpy()
        rec["hmr_dev32_" + k] = np.float64(dev(h32[k], h64[k]).max())

    out = osp.join(HERE, "hmr_head.npz")
    np.savez_compressed(out, **rec)
    print(f"{out}: {osp.getsize(out)} bytes; largest angle {head_angle:.3f} rad (head), {MAX_ANGLE[0]:.3f} rad (HMR)")
    print(" ".join(f"{k} {float(np.max(v)):.3e}" for k, v in rec.items() if "dev32" in k))
    print("rotation cases:", " ".join(f"{n}:{b}" for n, b in zip(cnames, b64)))
    assert osp.getsize(out) < 200 * 1024


if __name__ == "__main__":
    main()
