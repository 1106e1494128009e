#!/usr/bin/env python3
"""Golden vectors for the camera fit from the REAL reference code (build container only): lib/models/project_net.py's
OptimzeCamLayer (imported with a stub ``core.config``) driven by torch.nn.L1Loss and torch.optim.Adam exactly as the demo's loop does
(main/run_demo.py:134-173: a new Adam per window on a project_net that persists, lr 0.1 -> 0.05 after j == 100 -> 0.001 after
j == 200), and lib/utils/demo_utils.convert_crop_cam_to_orig_img (imported with stub cv2 / pytube / utils.* modules).  Outputs only;
the windows are regenerated from pmce_amd.synth by tests/camfit_ref.py."""
import os.path as osp
import sys
import types

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__)); REPO = osp.dirname(osp.dirname(HERE)); REF = "/root/reference"
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests"))
import camfit_ref as CR  # noqa: E402


def shims():
    class AD(dict):
        __getattr__ = dict.__getitem__
    core = types.ModuleType("core"); cc = types.ModuleType("core.config"); cc.cfg = AD(); core.config = cc
    cv2 = types.ModuleType("cv2"); pyt = types.ModuleType("pytube"); pyt.YouTube = object
    sb = types.ModuleType("utils.smooth_bbox"); sb.get_smooth_bbox_params = sb.get_all_bbox_params = None
    iu = types.ModuleType("utils._img_utils"); iu.get_single_image_crop_demo = None
    sys.modules.update({"core": core, "core.config": cc, "cv2": cv2, "pytube": pyt, "utils.smooth_bbox": sb, "utils._img_utils": iu})
    ut = types.ModuleType("utils"); ut.smooth_bbox = sb; ut._img_utils = iu
    sys.modules["utils"] = ut


def load_file(name, rel):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, osp.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def demo_loop(net, joints, target, dtype, steps=300, snapshots=()):
    """optimize_cam_param's loop for ONE window on `net` (which keeps its camera from the previous call)."""
    j3d = torch.from_numpy(joints[None]).to(dtype)
    tgt = torch.from_numpy(target[None, :, :2]).to(dtype)[:, :CR.N_FIT, :]
    l1 = torch.nn.L1Loss()
    adam = torch.optim.Adam(net.parameters(), lr=0.1)
    net.train()
    snaps = []
    for j in range(steps):
        loss = l1(net(j3d), tgt)
        adam.zero_grad()
        loss.backward()
        adam.step()
        if j in (100, 200):                      # the rate changes AFTER the step at these indices
            for group in adam.param_groups:
                group["lr"] = 0.05 if j == 100 else 0.001
        if j + 1 in snapshots:
            snaps.append(net.cam_param[0].detach().numpy().copy())
    return net.cam_param[0].detach().numpy().copy(), snaps


def main():
    shims()
    torch.set_num_threads(1)
    get_model = load_file("ref_project_net", "lib/models/project_net.py").get_model     # (the packages' __init__ pull in timm etc.)
    convert_crop_cam_to_orig_img = load_file("ref_demo_utils", "lib/utils/demo_utils.py").convert_crop_cam_to_orig_img
    joints, target, init = CR.windows()
    W = joints.shape[0]

    def net_from(init_row, dtype):
        net = get_model(crop_size=CR.CROP).to(dtype)
        with torch.no_grad():
            net.cam_param.copy_(torch.from_numpy(init_row[None]).to(dtype))
        return net

    cam64 = np.zeros((W, 3)); cam32 = np.zeros((W, 3), dtype=np.float32); snaps64 = np.zeros((len(CR.SNAP_STEPS), W, 3))
    for w in range(W):
        cam64[w], sn = demo_loop(net_from(init[w], torch.float64), joints[w], target[w], torch.float64, snapshots=CR.SNAP_STEPS)
        snaps64[:, w] = np.stack(sn)
        cam32[w], _ = demo_loop(net_from(init[w], torch.float32), joints[w], target[w], torch.float32)
    net = net_from(init[0], torch.float64)                 # the demo: one project_net along the tracklet
    chain64 = np.stack([demo_loop(net, joints[w], target[w], torch.float64)[0] for w in range(CR.CHAIN_LEN)])
    # the reference-fp32's own agreement with the reference-fp64: the yardstick of the fp32 kernel test
    l64, l32 = CR.l1_loss(cam64, joints, target), CR.l1_loss(cam32, joints, target)
    share32 = float((np.abs(cam32.astype(np.float64) - cam64).max(1) <= 1e-3).mean())
    excess32 = float(((l32 - l64) / l64).max())
    assert share32 >= 0.95, f"reference fp32 within 1e-3 of its fp64 on {share32:.3f} of the windows: change the seed"
    bx = CR.boxes()
    K = bx.shape[0]
    b64 = bx.astype(np.float64)
    ocam = convert_crop_cam_to_orig_img(cam64[:K], np.stack([b64[:, 0] + b64[:, 2] / 2, b64[:, 1] + b64[:, 3] / 2, b64[:, 3]], 1),
                                        CR.IMG_WH[0], CR.IMG_WH[1])
    np.savez_compressed(osp.join(HERE, "camfit.npz"), W=W, seed=CR.SEED, cam64=cam64, cam32=cam32, snap_steps=np.array(CR.SNAP_STEPS),
                        snaps64=snaps64, chain64=chain64, share32=share32, excess32=excess32, boxes=bx, img_wh=np.array(CR.IMG_WH),
                        orig_cam=ocam)
    r = CR.fit(joints, target, init)
    print(f"reference fp32 vs fp64: share within 1e-3 {share32:.4f}, worst relative loss excess {excess32:.3e}")
    print(f"numpy restatement vs reference fp64: {np.abs(r - cam64).max():.2e}; "
          f"chain: {np.abs(CR.fit_chain(joints[:CR.CHAIN_LEN], target[:CR.CHAIN_LEN], init[0]) - chain64).max():.2e}")
    r32 = CR.fit(joints, target, init, dtype=np.float32)
    print(f"numpy fp32 restatement: share {float((np.abs(r32 - cam64).max(1) <= 1e-3).mean()):.4f}, "
          f"excess {float(((CR.l1_loss(r32, joints, target) - l64) / l64).max()):.3e}")


if __name__ == "__main__":
    main()
