#!/usr/bin/env python3
"""Golden vectors for the SMPL layer from the REAL reference code (build container only): smplpytorch's SMPL_Layer.forward on the seeded
synthetic model and parameter rows of tests/smpl_ref.py.  The layer's __init__ reads a licensed model file through chumpy; its forward
needs neither, so the object is made with SMPL_Layer.__new__ + torch.nn.Module.__init__ and given the seven buffers and four constants
__init__ would have set.  Outputs only: the layer's fp64 result (``.double()`` on a deep copy) and the largest absolute deviation of its
own fp32 run from it - the yardstick of the device tests.

    python tests/golden/make_golden_smpl.py /path/to/reference        (or PMCE_REFERENCE_DIR)"""
import copy
import os
import os.path as osp
import sys

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__)); REPO = osp.dirname(osp.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PMCE_REFERENCE_DIR", "")
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests")); sys.path.insert(0, osp.join(REF, "smplpytorch"))
import smpl_ref as SR  # noqa: E402


def make_layer(model, gender="neutral"):
    from smplpytorch.pytorch.smpl_layer import SMPL_Layer
    layer = SMPL_Layer.__new__(SMPL_Layer)
    torch.nn.Module.__init__(layer)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)    # noqa: E731
    layer.register_buffer("th_betas", torch.zeros(1, 10))
    layer.register_buffer("th_shapedirs", t(model["shapedirs"]))
    layer.register_buffer("th_posedirs", t(model["posedirs"]))
    layer.register_buffer("th_v_template", t(model["v_template"]).unsqueeze(0))
    layer.register_buffer("th_J_regressor", t(model["J_regressor"]))
    layer.register_buffer("th_weights", t(model["weights"]))
    layer.register_buffer("th_faces", torch.tensor(model["faces"].astype(np.int64)))
    layer.kintree_parents = [int(p) for p in model["parents"]]
    layer.num_joints = 24
    layer.center_idx = None
    layer.gender = gender
    return layer


def run(model, pose, betas, trans):
    """(verts64, joints64, dev32_verts, dev32_joints) of the real layer on float32-valued inputs."""
    layer = make_layer(model)
    with torch.no_grad():
        v32, j32 = layer(*(torch.tensor(a, dtype=torch.float32) for a in (pose, betas, trans)))
        v64, j64 = copy.deepcopy(layer).double()(*(torch.tensor(a, dtype=torch.float64) for a in (pose, betas, trans)))
    assert torch.isfinite(v32).all() and torch.isfinite(v64).all() and torch.isfinite(j32).all() and torch.isfinite(j64).all()
    return (v64.numpy(), j64.numpy(), float((v32.double() - v64).abs().max()), float((j32.double() - j64).abs().max()))


def main():
    if not osp.isdir(osp.join(REF, "smplpytorch")):
        raise SystemExit("give the reference checkout's directory as the first argument (or PMCE_REFERENCE_DIR)")
    model = SR.synthetic_model(SR.V_GOLDEN, SR.SEED)
    pose, betas, trans = SR.cases(SR.B_GOLDEN, SR.SEED)
    v64, j64, dv, dj = run(model, pose, betas, trans)
    out = osp.join(HERE, "smpl.npz")
    np.savez_compressed(out, verts64=v64, joints64=j64, dev32_verts=np.float64(dv), dev32_joints=np.float64(dj),
                        seed=np.int64(SR.SEED), V=np.int64(SR.V_GOLDEN), B=np.int64(SR.B_GOLDEN))
    print(f"{out}: verts {v64.shape} max |x| {np.abs(v64).max():.3f} m, dev32_verts {dv:.3e} m, dev32_joints {dj:.3e} m, "
          f"{osp.getsize(out)} bytes")
    if "--full" in sys.argv:        # for orientation only: the same at SMPL's size
        m = SR.synthetic_model(6890, SR.SEED)
        _, _, dv, dj = run(m, pose, betas, trans)
        print(f"V = 6890: dev32_verts {dv:.3e} m, dev32_joints {dj:.3e} m")


if __name__ == "__main__":
    main()
