#!/usr/bin/env python3
"""Golden vectors for the demo's per-window preparation from the REAL reference code (build container only).

Imported from the reference: ``get_bbox`` / ``process_bbox`` (lib/coord_utils.py), ``j2d_processing`` (lib/aug_utils.py), ``FeatureDataset``
(lib/utils/_dataset_demo.py), ``get_all_bbox_params`` (lib/utils/smooth_bbox.py) and ``prepare_rendering_results``
(lib/utils/demo_utils.py).  ``add_pelvis_and_neck`` and ``normalize_screen_coordinates`` live in main/run_demo.py, which cannot be
imported (tracker, mmpose, renderer): their two definitions are cut out of its source and executed as they stand.  ``core.config``, pytube,
torchvision and utils._img_utils are stubs.  cv2 is not installed here: its stand-in implements ONLY ``getAffineTransform``, as a float64
solve of the 3-point system (cv2 returns float64 too; its own elimination order may differ from numpy's in the last bit).

The loop below is run_demo.py:332-351 without the model, behind a real ``DataLoader(batch_size=1)`` over a ``FeatureDataset``, so that the
aliasing between ``nj2d[seq_len//2].numpy()`` and the window is the reference's and not ours: it is asserted that after j2d_processing the
window's middle row equals the returned target bit for bit while the other 15 rows and the per-frame source table are untouched.

Stored per tracklet i: bbox{i} [N,4], target{i} [N,19,2], input{i} [N,16,19,2] (float32, what ``torch.Tensor(norm_joint2d[None])`` hands
the model); the largest deviation of tests/demo_ref.py's numpy-float32 restatement from them (yard_bbox, yard_target in pixels,
yard_input); tracklet_span cases; the frame_results table."""
import ast
import os
import os.path as osp
import sys
import tempfile
import types

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__)); REPO = osp.dirname(osp.dirname(HERE)); REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests"))
import demo_ref as DR  # noqa: E402


def shims():
    class AD(dict):
        __getattr__ = dict.__getitem__
    core = types.ModuleType("core"); cc = types.ModuleType("core.config"); cc.cfg = AD(); core.config = cc
    cv2 = types.ModuleType("cv2")

    def get_affine_transform(src, dst):
        """[2,3] float64 M with M @ (x, y, 1) = (x', y') for the three point pairs."""
        a = np.concatenate([np.asarray(src, dtype=np.float64), np.ones((3, 1))], 1)
        return np.linalg.solve(a, np.asarray(dst, dtype=np.float64)).T
    cv2.getAffineTransform = get_affine_transform
    pyt = types.ModuleType("pytube"); pyt.YouTube = object
    tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms"); tvf = types.ModuleType("torchvision.transforms.functional")
    tvf.to_tensor = None; tvt.functional = tvf; tv.transforms = tvt
    iu = types.ModuleType("utils._img_utils"); iu.get_single_image_crop_demo = None
    ut = types.ModuleType("utils"); ut.__path__ = [osp.join(REF, "lib", "utils")]; ut._img_utils = iu
    sys.modules.update({"core": core, "core.config": cc, "cv2": cv2, "pytube": pyt, "torchvision": tv, "torchvision.transforms": tvt,
                        "torchvision.transforms.functional": tvf, "utils": ut, "utils._img_utils": iu})
    sys.path.insert(0, osp.join(REF, "lib"))


def run_demo_defs(*names):
    """The named top-level function definitions of main/run_demo.py, executed from its source text."""
    src = open(osp.join(REF, "main", "run_demo.py")).read()
    tree = ast.parse(src)
    ns = {"np": np, "torch": torch}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), "run_demo.py", "exec"), ns)
    return [ns[n] for n in names]


def main():
    shims()
    torch.set_num_threads(1)
    from torch.utils.data import DataLoader
    from aug_utils import j2d_processing
    from coord_utils import get_bbox, process_bbox
    from utils._dataset_demo import FeatureDataset
    from utils.smooth_bbox import get_all_bbox_params
    from utils.demo_utils import prepare_rendering_results
    add_pelvis_and_neck, normalize_screen_coordinates = run_demo_defs("add_pelvis_and_neck", "normalize_screen_coordinates")

    seq_len, virtual_crop_size = 16, 500
    out = {"seed": DR.SEED}
    yard = {"bbox": 0.0, "target": 0.0, "input": 0.0}
    for i, (n, (orig_width, orig_height)) in enumerate(DR.TRACKLETS):
        kp, _ = DR.tracklet(i)
        nj = torch.Tensor(add_pelvis_and_neck(torch.from_numpy(kp)[:, :, :2])).reshape(-1, 19, 2)       # run_demo.py:310-312
        with tempfile.TemporaryDirectory() as folder:
            for k in range(n):
                open(osp.join(folder, f"{k + 1:06d}.jpg"), "w").close()
            dataset = FeatureDataset(image_folder=folder, frames=np.arange(n), seq_len=seq_len)
        dataset.feature_list = torch.zeros(n, 4)
        dataset.joint2d_list = nj
        table_before = nj.clone()
        assert len(dataset) == n and np.array_equal(np.array(dataset.seq_list) % n, DR.window_list(n) % n)
        bboxes, targets, inputs, left_out = [], [], [], 0
        for batch in DataLoader(dataset, batch_size=1, num_workers=0):                                   # run_demo.py:332-351
            img_features, nj2d = batch
            nj2d = nj2d[0]
            before = nj2d.clone()
            bbox = get_bbox(nj2d[seq_len // 2])
            bbox1 = process_bbox(bbox, aspect_ratio=1.0, scale=1.25)
            if bbox1 is None:
                left_out += 1
                continue
            proj_target_joint_img, trans = j2d_processing(nj2d[seq_len // 2].numpy(), (virtual_crop_size, virtual_crop_size), bbox1, 0, 0, None)
            norm_joint2d = normalize_screen_coordinates(nj2d.numpy(), orig_width, orig_height)
            # the finding: the middle row now IS the target; nothing else moved
            assert np.array_equal(nj2d[seq_len // 2].numpy(), proj_target_joint_img)
            keep = [t for t in range(seq_len) if t != seq_len // 2]
            assert torch.equal(nj2d[keep], before[keep]) and not torch.equal(nj2d[seq_len // 2], before[seq_len // 2])
            assert bbox1.dtype == np.float32 and proj_target_joint_img.dtype == np.float32
            bboxes.append(np.asarray(bbox1, dtype=np.float32))
            targets.append(proj_target_joint_img)
            inputs.append(torch.Tensor(norm_joint2d[None, :, :, :])[0].numpy())                           # run_demo.py:135
        assert left_out == 0, f"tracklet {i}: process_bbox returned None for {left_out} windows"
        assert torch.equal(dataset.joint2d_list, table_before), "the per-frame source table changed"
        b, t, x = np.stack(bboxes), np.stack(targets), np.stack(inputs)
        out[f"bbox{i}"], out[f"target{i}"], out[f"input{i}"] = b, t, x
        rb, rt, rx, rv = DR.prepare(kp, (orig_width, orig_height))
        assert rv.all()
        for key, got, want in (("bbox", rb, b), ("target", rt, t), ("input", rx, x)):
            yard[key] = max(yard[key], float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
        mid = seq_len // 2
        rest = [k for k in range(seq_len) if k != mid]
        clean = DR.prepare(kp, (orig_width, orig_height), reference_mode=False)[2]
        print(f"tracklet {i}: N = {n}, {orig_width} x {orig_height}; restatement's other 15 rows vs reference "
              f"{np.abs(clean[:, rest].astype(np.float64) - x[:, rest]).max():.2e}; middle row moved by "
              f"{np.abs(clean[:, mid].astype(np.float64) - x[:, mid]).max():.2f} (normalised units)")
    # the degenerate frame: process_bbox has no box for it
    deg = torch.from_numpy(add_pelvis_and_neck(torch.from_numpy(DR.degenerate_frames(1))[:, :, :2]).astype(np.float32))
    assert process_bbox(get_bbox(deg[0]), aspect_ratio=1.0, scale=1.25) is None
    out.update({f"yard_{k}": v for k, v in yard.items()})
    print("numpy-float32 restatement vs reference: " + ", ".join(f"{k} {v:.3e}" for k, v in yard.items()))

    cases = DR.span_cases()
    names = sorted(cases)
    spans = []
    for name in names:
        _, a, b = get_all_bbox_params(cases[name], vis_thresh=0.3)
        spans.append((a, b))
    out["span_names"] = np.array(names)
    out["spans"] = np.array(spans, dtype=np.int64)
    res, num_frames = DR.render_case()
    out["render"] = DR.render_table(prepare_rendering_results(res, num_frames))
    np.savez_compressed(osp.join(HERE, "demo.npz"), **out)
    print({n: tuple(s) for n, s in zip(names, spans)})
    print("wrote", osp.join(HERE, "demo.npz"), os.path.getsize(osp.join(HERE, "demo.npz")), "bytes")


if __name__ == "__main__":
    main()
