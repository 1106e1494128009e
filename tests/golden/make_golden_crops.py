#!/usr/bin/env python3
"""Golden vectors for the demo's person crops from the REAL reference code (build container only): python make_golden_crops.py [reference].

``get_all_bbox_params`` is imported from the reference (lib/utils/smooth_bbox.py) with the shims of make_golden_demo.py.  The box lines of
``CropDataset.__init__`` (lib/utils/_dataset_demo.py:48-50) and the functions ``rotate_2d`` / ``gen_trans_from_patch_cv``
(lib/utils/_img_utils.py:45-86) sit in modules that cannot be imported here (cv2, torchvision, the occluder utilities): their statements
are cut out of the source with ``ast`` and executed as they stand.  cv2 is not installed: ``cv2.getAffineTransform`` is the float64 solve
of the 3-point system (cv2 returns float64 too; its own elimination may differ from numpy's in the last bit).  No pixel is recorded: no
OpenCV exists here to warp with.

Stored: per tracklet of tests/crops_ref.golden_tracklets() the reference's boxes over its span ``boxes_<name>`` [end - start, 4] and
``span_<name>``; for tests/crops_ref.golden_boxes() the 2 x 3 matrices ``trans`` [M,2,3] of gen_trans_from_patch_cv(inv=False).  The
inputs are regenerated from the seed by the tests, not stored."""
import ast
import os
import os.path as osp
import sys
import types

import numpy as np

HERE = osp.dirname(osp.abspath(__file__)); REPO = osp.dirname(osp.dirname(HERE)); REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REPO); sys.path.insert(0, osp.join(REPO, "tests"))
import crops_ref as CR  # noqa: E402
from make_golden_demo import shims  # noqa: E402


def definitions(path, *names):
    """The named top-level function definitions of a source file, executed from its text with numpy and the cv2 shim in scope."""
    tree = ast.parse(open(path).read())
    ns = {"np": np, "cv2": sys.modules["cv2"]}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), osp.basename(path), "exec"), ns)
    return [ns[n] for n in names]


def crop_dataset_box_lines(path):
    """The three statements of CropDataset.__init__ that make ``self.bboxes`` (and the trim indices), as a function of joints2d."""
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CropDataset")
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    branch = [n for n in init.body if isinstance(n, ast.If)][-1]
    stmts = branch.body[:3]
    text = [ast.unparse(s) for s in stmts]
    assert "get_all_bbox_params(joints2d, vis_thresh=0.3)" in text[0] and "150.0 / bboxes[:, 2:]" in text[1] and "self.bboxes" in text[2], text
    code = compile(ast.Module(stmts, []), "_dataset_demo.py", "exec")

    def run(joints2d, get_all_bbox_params):
        ns = {"np": np, "joints2d": joints2d, "get_all_bbox_params": get_all_bbox_params, "self": types.SimpleNamespace()}
        exec(code, ns)
        return ns["self"].bboxes, ns["time_pt1"], ns["time_pt2"]
    return run


def main():
    shims()
    from utils.smooth_bbox import get_all_bbox_params
    box_lines = crop_dataset_box_lines(osp.join(REF, "lib", "utils", "_dataset_demo.py"))
    _, gen_trans = definitions(osp.join(REF, "lib", "utils", "_img_utils.py"), "rotate_2d", "gen_trans_from_patch_cv")

    out = {"seed": CR.SEED}
    worst_box = 0.0
    for name, kp in CR.golden_tracklets().items():
        assert kp.dtype == np.float64 and np.array_equal(kp, kp.astype(np.float32).astype(np.float64))
        boxes, a, b = box_lines(kp, get_all_bbox_params)
        boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
        assert len(boxes) == max(b - max(a, 0), 0), (name, boxes.shape, a, b)
        out[f"boxes_{name}"], out[f"span_{name}"] = boxes, np.array([a, b], dtype=np.int64)
        mine, _, span = CR.tracklet_boxes(kp)
        assert span == (a, b), (name, span, (a, b))
        if len(boxes):
            worst_box = max(worst_box, float(np.max(np.abs(mine[a:b] - boxes) / np.abs(boxes))))
        print(f"{name}: N = {len(kp)}, span = ({a}, {b})")
    trans, worst_map = [], 0.0
    for cx, cy, w, h, scale, S in CR.golden_boxes():
        m = np.asarray(gen_trans(cx, cy, w, h, int(S), int(S), scale, 0, inv=False), dtype=np.float64)
        trans.append(m)
        mine = CR.forward_matrix((cx, cy, w, h), scale, int(S))
        worst_map = max(worst_map, CR.map_difference(mine, m))
    out["trans"] = np.stack(trans)
    print(f"oracle vs reference, largest relative difference: boxes {worst_box:.3e}, forward map {worst_map:.3e}")
    path = osp.join(HERE, "crops.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
