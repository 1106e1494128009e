"""GPU tests of the device SMPL layer (pmce_amd/smpl.py on csrc/smpl.hip) against the real SMPL_Layer's results
(tests/golden/smpl.npz) and the numpy restatement held to them (tests/smpl_ref.py, test_smpl_host.py).

The yardstick is the reference's OWN fp32 error: dev32 = the largest deviation of SMPL_Layer's fp32 run from its fp64 run on the same
rows.  The device result must stay within 4 x dev32 of the fp64 result - the factor covers another summation order over the 217-term
blend sum and the 24-term skinning sum, nothing else.  Shapes: V = 137 = two full waves and a 9-lane tail inside one 256-vertex tile;
B = 19 = one full batch tile of 16 and a tail of 3; V = 6890 = 27 vertex tiles, the last partial.

Every test prints the deviation it measures before it asserts (run with -s)."""
import ctypes as C
import os.path as osp

import numpy as np
import pytest
import torch

import smpl_ref as SR
from conftest import GOLDEN
from pmce_amd import _lib, datasets, smpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")


def make_layer(model, gender="neutral"):
    return smpl.SMPL({gender: smpl.SMPLModel.from_arrays(*(model[k] for k in MODEL_KEYS))})


def run(layer, pose, betas, trans=None, gender=None, **kw):
    with torch.cuda.device(DEV):
        v, j = layer.forward(np.asarray(pose, np.float32), np.asarray(betas, np.float32), None if trans is None else np.asarray(trans, np.float32),
                             gender, **{k: (np.asarray(a, np.float32) if isinstance(a, np.ndarray) else a) for k, a in kw.items()})
        torch.cuda.synchronize()
    return v.cpu().numpy(), j.cpu().numpy()


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "smpl.npz"))


@pytest.fixture(scope="module")
def small():
    """(model, layer, rows, device result) of the golden case, computed once."""
    model = SR.synthetic_model(SR.V_GOLDEN, SR.SEED)
    layer = make_layer(model)
    rows = SR.cases(SR.B_GOLDEN, SR.SEED)
    return model, layer, rows, run(layer, *rows)


@pytest.fixture(scope="module")
def full():
    """A synthetic model of SMPL's size whose root regressor row is supported on the first 100 vertices (the evaluator test moves the
    others), three rows, the fp64 and fp32 restatements and the device result."""
    model = SR.synthetic_model(6890, SR.SEED + 1)
    model["J_regressor"][0, 100:] = 0.0
    model["J_regressor"][0] = (model["J_regressor"][0] / model["J_regressor"][0].sum()).astype(np.float32)
    layer = make_layer(model)
    rows = SR.cases(3, SR.SEED + 1)
    v64, j64 = SR.forward(model, *rows, np.float64)
    v32, j32 = SR.forward(model, *rows, np.float32)
    return model, layer, rows, (v64, j64), (np.abs(v32 - v64).max(), np.abs(j32 - j64).max()), run(layer, *rows)


def test_golden_case(gold, small):
    _, _, _, (v, j) = small
    dv, dj = np.abs(v - gold["verts64"]).max(), np.abs(j - gold["joints64"]).max()
    print(f"V=137 B=19: verts {dv:.3e} m (reference fp32 {float(gold['dev32_verts']):.3e}), joints {dj:.3e} m ({float(gold['dev32_joints']):.3e})")
    assert np.isfinite(v).all() and np.isfinite(j).all()
    assert dv <= 4 * gold["dev32_verts"] and dj <= 4 * gold["dev32_joints"]
    # the all-zero pose row: every rotation is the identity, the vertices are v_shaped + trans
    model, _, (pose, betas, trans), _ = small
    rest = model["v_template"] + np.einsum("vck,k->vc", model["shapedirs"], betas[0]) + trans[0]
    assert np.abs(v[0] - rest).max() <= 4 * gold["dev32_verts"]


def test_single_sample(gold, small):
    _, layer, (pose, betas, trans), _ = small
    for i in (0, 6):
        v, j = run(layer, pose[i:i + 1], betas[i:i + 1], trans[i:i + 1])
        assert v.shape == (1, SR.V_GOLDEN, 3) and j.shape == (1, 24, 3)
        assert np.abs(v[0] - gold["verts64"][i]).max() <= 4 * gold["dev32_verts"]
        assert np.abs(j[0] - gold["joints64"][i]).max() <= 4 * gold["dev32_joints"]


def test_batch_invariance(small):
    _, layer, (pose, betas, trans), (v, j) = small
    B = SR.B_GOLDEN
    for i in range(B):                                   # alone
        v1, j1 = run(layer, pose[i:i + 1], betas[i:i + 1], trans[i:i + 1])
        assert np.array_equal(v1[0], v[i]) and np.array_equal(j1[0], j[i]), f"row {i} alone differs from row {i} of B = {B}"
    for i0 in list(range(0, B - 2, 3)) + [B - 3]:        # inside B = 3 (every row is covered)
        v3, j3 = run(layer, pose[i0:i0 + 3], betas[i0:i0 + 3], trans[i0:i0 + 3])
        assert np.array_equal(v3, v[i0:i0 + 3]) and np.array_equal(j3, j[i0:i0 + 3]), f"rows {i0}..{i0 + 2} in B = 3 differ"
    v17, j17 = run(layer, pose[:17], betas[:17], trans[:17])         # one full batch tile + 1
    assert np.array_equal(v17, v[:17]) and np.array_equal(j17, j[:17])


def test_two_runs_are_bit_identical(small):
    _, layer, rows, (v, j) = small
    v2, j2 = run(layer, *rows)
    assert np.array_equal(v, v2) and np.array_equal(j, j2)


def test_mixed_genders(small):
    names = ("neutral", "female", "male")
    models = {g: smpl.SMPLModel.from_arrays(*(SR.synthetic_model(SR.V_GOLDEN, SR.SEED + 10 + k)[key] for key in MODEL_KEYS))
              for k, g in enumerate(names)}
    layer = smpl.SMPL(models)
    pose, betas, trans = SR.cases(7, SR.SEED + 2)
    gender = np.array(["male", "female", "neutral", "f", "m", "neutral", "male"])
    v, j = run(layer, pose, betas, trans, gender)
    assert np.isfinite(v).all()
    single = {g: run(layer, pose, betas, trans, g) for g in names}
    for i, g in enumerate(gender):
        vs, js = single[smpl.GENDER_ALIASES[g]]
        assert np.array_equal(v[i], vs[i]) and np.array_equal(j[i], js[i]), f"row {i} ({g}) differs from the single-gender call"
    assert not np.array_equal(single["male"][0][1], single["female"][0][1])
    with pytest.raises(_lib.PmceError):
        run(smpl.SMPL({"male": models["male"]}), pose, betas, trans, gender)


def test_full_size(full):
    _, _, _, (v64, j64), (d32v, d32j), (v, j) = full
    dv, dj = np.abs(v - v64).max(), np.abs(j - j64).max()
    print(f"V=6890 B=3: verts {dv:.3e} m (fp32 restatement {d32v:.3e}), joints {dj:.3e} m ({d32j:.3e})")
    assert dv <= 4 * d32v and dj <= 4 * d32j


def test_output_transform_and_gt_mesh(gold, small):
    model, layer, (pose, betas, trans), _ = small
    rng = np.random.default_rng(3)
    # a root near the body's own, as the datasets' h36m root joint is: the target is root-relative
    root = (gold["joints64"][:, 0] * 1000 + rng.normal(0, 50, (SR.B_GOLDEN, 3))).astype(np.float32)
    want_v, want_j = SR.pw3d_targets(model, pose, betas, trans, root.astype(np.float64))
    v, j = run(layer, pose, betas, trans, scale=1000.0, offset=root)
    dv, dj = np.abs(v - want_v).max(), np.abs(j - want_j).max()
    print(f"scale 1000 + offset: verts {dv:.3e} mm, joints {dj:.3e} mm")
    assert dv <= 4 * gold["dev32_verts"] * 1000 and dj <= 4 * gold["dev32_joints"] * 1000
    # FrameTable.gt_mesh on a hand-built five-frame table: the same numbers, in metres
    n = 5
    z = lambda *s: np.zeros(s, np.float32)    # noqa: E731
    jc = z(n, 17, 3)
    jc[:, 0] = root[:n]
    table = datasets.FrameTable(name="five frames", img_paths=np.array([f"0/s/image_{i:05d}.jpg" for i in range(n)]), vid_names=np.array(["s0"] * n),
                                img_shapes=np.full((n, 2), 1000, np.int32), keypoints=z(n, 17, 3), features=z(n, 4), joints_cam_h36m=jc,
                                joints_cam_coco=z(n, 19, 3), gt_joints_img_coco=z(n, 17, 3),
                                smpl={"pose": pose[:n].astype(np.float32), "shape": betas[:n].astype(np.float32), "trans": trans[:n].astype(np.float32),
                                      "gender": np.array(["neutral"] * n)})
    idx = np.array([3, 0, 4])
    gm = table.gt_mesh(layer, idx, DEV)
    assert gm.is_cuda and tuple(gm.shape) == (3, SR.V_GOLDEN, 3)
    assert torch.equal(gm, torch.from_numpy(v[idx]).to(DEV) / 1000.0)
    # back in metres: one more fp32 rounding, at most an ulp of a coordinate below 4 m (2^-21 m)
    assert np.abs(gm.cpu().numpy().astype(np.float64) - want_v[idx] / 1000).max() <= 4 * gold["dev32_verts"] + 2.0 ** -21
    gm2 = table.gt_mesh(layer, idx, DEV, root_mm=np.zeros((3, 3)))
    assert np.abs(gm2.cpu().numpy().astype(np.float64) - gold["verts64"][idx]).max() <= 4 * gold["dev32_verts"] + 2.0 ** -21


def test_camera_form(small):
    model, layer, _, _ = small
    B = 5
    pose, betas, trans = SR.cases(B, SR.SEED + 3)
    betas[1, 3] = 3.5                                   # the whole row of betas counts as 0 (Human36M/dataset.py:365)
    pose[2, :3] = 0.0                                   # a zero root pose (row 0 is all zeros anyway)
    cam_R = SR.random_rotations(B, 4)
    rng = np.random.default_rng(6)
    cam_t = (rng.normal(0, 500, (B, 3)) + np.array([0, 0, 4000.0])).astype(np.float32).astype(np.float64)
    v64, j64 = SR.h36m_camera_form(model, pose, betas, trans, cam_R, cam_t, np.float64)
    v32, j32 = SR.h36m_camera_form(model, pose, betas, trans, cam_R, cam_t, np.float32)
    bv, bj = 4 * np.abs(v32 - v64).max(), 4 * np.abs(j32 - j64).max()
    v, j = run(layer, pose, betas, trans, cam_R=cam_R, cam_t=cam_t, scale=1000.0)
    dv, dj = np.abs(v - v64).max(), np.abs(j - j64).max()
    print(f"camera form: verts {dv:.3e} mm (bound {bv:.3e}), joints {dj:.3e} mm (bound {bj:.3e})")
    assert np.isfinite(v).all() and dv <= bv and dj <= bj
    # the zero-root rows against cam_R composed directly: no axis-angle round trip at all
    zb = betas.copy()
    zb[1] = 0.0
    for i in (0, 2):
        vi, ji = SR.forward(model, pose[i:i + 1], zb[i:i + 1], None, np.float64, root_rot=cam_R[i:i + 1])
        tr = cam_R[i] @ trans[i] + cam_t[i] / 1000 - ji[0, 0] + cam_R[i] @ ji[0, 0]
        assert np.abs(v[i] - (vi[0] + tr) * 1000).max() <= bv and np.abs(j[i] - (ji[0] + tr) * 1000).max() <= bj
    # the row with |beta| > 3 is the row with zero betas
    v0, _ = run(layer, pose, zb, trans, cam_R=cam_R, cam_t=cam_t, scale=1000.0)
    assert np.array_equal(v0, v)
    # ... and a Human3.6M table feeds the same form
    z = lambda *s: np.zeros(s, np.float32)    # noqa: E731
    jc = z(B, 17, 3)
    jc[:, 0] = j64[:, 0].astype(np.float32)
    table = datasets.FrameTable(name="h36m rows", img_paths=np.array([f"s_{i:02d}.jpg" for i in range(B)]), vid_names=np.array(["s"] * B),
                                img_shapes=np.full((B, 2), 1000, np.int32), keypoints=z(B, 17, 3), features=z(B, 4), joints_cam_h36m=jc,
                                joints_cam_coco=z(B, 0, 3), gt_joints_img_coco=z(B, 17, 3),
                                smpl={"pose": pose.astype(np.float32), "shape": betas.astype(np.float32), "trans": trans.astype(np.float32),
                                      "gender": np.array(["neutral"] * B)},
                                cam_idxs=np.full(B, 4), extras={"cam_Rs": cam_R.astype(np.float32), "cam_ts": cam_t.astype(np.float32)})
    gm = table.gt_mesh(layer, np.arange(B), DEV).cpu().numpy()
    # (root-relative coordinates below 4 m, rounded once more on the way back to metres: 2^-21 m = 4.8e-4 mm)
    assert np.abs(gm.astype(np.float64) * 1000.0 - (v64 - jc[:, :1].astype(np.float64))).max() <= bv + 1e-3


def test_evaluator_hookup(full):
    from pmce_amd.eval import Evaluator
    _, layer, _, _, _, (v, _) = full
    ev = Evaluator(DEV, root_regressor_row=layer.root_regressor_row())
    gt = torch.from_numpy(v).to(DEV)
    mv = ev.per_sample(gt, gt)[0].cpu().numpy()
    assert np.array_equal(mv, np.zeros(3, np.float32))
    # 3 mm along x on every vertex the root row does not touch: the root stays, so the error is 3 mm on 6790 of 6890 vertices.
    # fp32 coordinates of a few metres carry half an ulp of 2^-22 m = 1.2e-4 mm each; 1e-3 mm is several of those.
    pred = gt.clone()
    pred[:, 100:, 0] += 0.003
    mv = ev.per_sample(pred, gt)[0].cpu().numpy()
    assert np.abs(mv - 3.0 * 6790 / 6890).max() < 1e-3, mv


def test_non_finite_row_stays_in_its_row(small):
    _, layer, (pose, betas, trans), (v, j) = small
    bad = pose.copy()
    bad[4] = np.nan
    vb, jb = run(layer, bad, betas, trans)
    keep = np.arange(SR.B_GOLDEN) != 4
    assert np.array_equal(vb[keep], v[keep]) and np.array_equal(jb[keep], j[keep])
    # (the root joint's position is the rest joint + trans: it does not depend on the pose and stays finite, as in the reference)
    assert not np.isfinite(vb[4]).any() and not np.isfinite(jb[4, 1:]).any()


def test_invalid_arguments_launch_nothing(small):
    from pmce_amd import ops
    _, layer, (pose, betas, trans), _ = small
    lib = _lib.load()
    m = layer.models["neutral"]
    dev = torch.device(DEV)
    B, V = 2, SR.V_GOLDEN
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:B], np.float32)).to(dev)    # noqa: E731
    p, b = t(pose), t(betas)
    verts = torch.full((B, V, 3), 7.0, device=dev)
    joints = torch.full((B, 24, 3), 7.0, device=dev)
    ws = torch.empty(ops.smpl_workspace_bytes(B), device=dev, dtype=torch.uint8)
    vt, dirs, wts, jt, jsd = m.to(dev)
    P = _lib.ptr

    def call(V_=V, parents=m.parents):
        par = np.ascontiguousarray(parents, np.int32)
        with torch.cuda.device(dev):
            return lib.pmce_smpl_forward(P(vt), P(dirs), P(wts), P(jt), P(jsd), par.ctypes.data_as(C.POINTER(C.c_int)), 24, P(p), P(b), None, None,
                                         None, None, B, 1.0, None, P(verts), P(joints), C.c_void_p(ws.data_ptr()), ws.numel(), B, V_,
                                         _lib.current_stream())

    assert call(V_=0) == -1 and "V must be" in _lib.last_error()
    bad = m.parents.copy()
    bad[9] = 9
    assert call(parents=bad) == -1 and "parent of joint 9" in _lib.last_error()
    with pytest.raises(_lib.PmceError):                      # a model of another size than the output
        ops.smpl_forward(m, p, b, None, None, None, None, 1.0, None, torch.empty(B, V + 1, 3, device=dev), joints, ws)
    with pytest.raises(_lib.PmceError):
        run(layer, pose[:, :71], betas)
    torch.cuda.synchronize()
    assert bool((verts == 7.0).all()) and bool((joints == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((verts == 7.0).any())
