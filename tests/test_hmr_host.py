"""CPU-only tests of the HMR head's host side (pmce_amd/hmr.py: the fold of the iterated regressor, state dicts, the joint table, the C
entry points' argument checks) and of the oracle the GPU tests lean on (tests/hmr_ref.py, held to the real reference functions' results
in tests/golden/hmr_head.npz)."""
import ctypes as C
import os.path as osp
import re

import numpy as np
import pytest
import torch

import hmr_ref as HR
import smpl_ref as SR
from conftest import GOLDEN, REPO
from pmce_amd import _lib, hmr


@pytest.fixture(scope="module")
def gold():
    g = np.load(osp.join(GOLDEN, "hmr_head.npz"))
    assert int(g["seed"]) == HR.SEED and g["theta64"].shape == (HR.N_GOLDEN, 85) and g["verts64"].shape == (HR.N_GOLDEN, HR.V_GOLDEN, 3)
    return g


@pytest.fixture(scope="module")
def sd():
    return HR.state_dict()


def test_restatement_against_the_reference_head(gold, sd):
    out = HR.forward(sd, HR.features(), HR.smpl_model(), HR.extra_vertex_ids(), HR.extra_regressor())
    for k in ("state", "rotmat", "theta", "verts", "kp_3d", "kp_2d"):
        d = np.abs(out[k] - gold[k + "64"]).max()
        print(f"fp64 restatement, {k}: {d:.2e}")
        assert out[k].shape == gold[k + "64"].shape and d < 1e-12, k
    assert out["kp_3d"].shape == (HR.N_GOLDEN, 49, 3) and out["kp_2d"].shape == (HR.N_GOLDEN, 49, 2)


def test_restatement_against_the_reference_rotation_functions(gold):
    names, six = HR.rotation_cases()
    assert list(gold["rot_names"]) == names
    R = HR.rot6d_to_rotmat(six)
    aa = HR.rotmat_to_angle_axis(R)
    assert np.array_equal(np.isnan(R), np.isnan(gold["rot_rotmat64"]))
    assert np.nanmax(np.abs(R - gold["rot_rotmat64"])) < 1e-12 and np.abs(aa - gold["rot_aa64"]).max() < 1e-12
    assert np.array_equal(HR.quaternion_branch(np.nan_to_num(R)), HR.quaternion_branch(np.nan_to_num(gold["rot_rotmat64"])))
    assert set(gold["rot_branch"][:-1]) == {0, 1, 2, 3}
    # the degenerate inputs: what the reference makes of them
    i = names.index
    assert np.array_equal(R[i("a1_zero")], np.diag([0.0, 1.0, 0.0])) and np.allclose(aa[i("a1_zero")], (0, np.pi, 0), atol=1e-15)
    assert np.array_equal(R[i("a2_parallel")], np.diag([1.0, 0.0, 0.0])) and np.allclose(aa[i("a2_parallel")], (np.pi, 0, 0), atol=1e-15)
    assert np.array_equal(R[i("both_zero")], np.zeros((3, 3)))
    assert np.isnan(R[i("nan")]).all() and np.array_equal(aa[i("nan")], np.zeros(3))
    assert np.allclose(aa[i("pi_about_x")], (np.pi, 0, 0), atol=1e-15) and np.allclose(aa[i("identity")], 0, atol=0)


@pytest.mark.parametrize("n_iter", [1, 3, 5])
def test_fold_equals_the_iteration(sd, n_iter):
    D, bD = HR.dec_stack(sd)
    Q, P, c = hmr.fold_regressor(sd["fc1.weight"], sd["fc1.bias"], sd["fc2.weight"], sd["fc2.bias"], D, bD, n_iter)
    assert Q.shape == (157, 2048) and P.shape == (157, 157) and c.shape == (157,) and Q.dtype == np.float64
    xf = HR.features(7).astype(np.float64)
    s0 = HR.initial_state(sd, 7)
    want = HR.iterate(sd, xf, n_iter)
    got = s0 @ P.T + xf @ Q.T + c
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"n_iter = {n_iter}: fold vs iteration {rel:.2e} relative")
    assert rel < 1e-12
    # a per-sample initial state
    rng = np.random.default_rng(3)
    init = s0 + rng.normal(0, 0.3, s0.shape)
    want = HR.iterate(sd, xf, n_iter, init)
    got = init @ P.T + xf @ Q.T + c
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-12


def test_fold_rejects_other_iteration_counts(sd):
    D, bD = HR.dec_stack(sd)
    args = (sd["fc1.weight"], sd["fc1.bias"], sd["fc2.weight"], sd["fc2.bias"], D, bD)
    for bad in (0, 17, -1, 2.0, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="n_iter"):
            hmr.fold_regressor(*args, bad)
    with pytest.raises(ValueError, match="dec_w"):
        hmr.fold_regressor(*args[:4], D[:-1], bD, 3)


def test_state_dict_errors_name_the_tensor(sd):
    t = hmr.select_head_state_dict({"module." + k: v for k, v in sd.items()})
    assert list(t) == list(hmr.HEAD_KEYS) and all(v.dtype == torch.float64 for v in t.values())
    for name in hmr.HEAD_KEYS:
        with pytest.raises(ValueError, match=re.escape(f"'{name}'")):
            hmr.select_head_state_dict({k: v for k, v in sd.items() if k != name})
    bad = dict(sd)
    bad["init_pose"] = sd["init_pose"].reshape(144)
    with pytest.raises(ValueError, match="'init_pose' has shape"):
        hmr.select_head_state_dict(bad)
    bad = dict(sd)
    bad["fc1.weight"] = sd["fc1.weight"][:, :2048]
    with pytest.raises(ValueError, match="'fc1.weight' has shape"):
        hmr.select_head_state_dict(bad)
    with pytest.raises(ValueError):
        hmr.select_head_state_dict([1, 2])


def test_no_training_mode():
    for cls in (hmr.RegressorHead, hmr.HMR):
        obj = cls.__new__(cls)
        with pytest.raises(NotImplementedError):
            obj.train()
        assert obj.train(False) is obj and obj.eval() is obj


def test_joint_table():
    ids, jre = HR.extra_vertex_ids(), HR.extra_regressor()
    sel, (indptr, indices, data) = hmr.spin_joint_table(ids, jre)
    assert sel.dtype == np.int32 and sel.shape == (49,) and indptr.shape == (50,) and indices.dtype == np.int32 and data.dtype == np.float32
    # against the dense form of smpl_mps.py:71-83 on random points
    rng = np.random.default_rng(0)
    joints, verts = rng.normal(size=(2, 24, 3)), rng.normal(size=(2, HR.V_GOLDEN, 3))
    want = HR.joints49(joints, verts, ids, jre)
    got = np.empty_like(want)
    for k in range(49):
        if sel[k] >= 0:
            assert indptr[k] == indptr[k + 1]
            got[:, k] = joints[:, sel[k]]
        else:
            cols, w = indices[indptr[k]:indptr[k + 1]], data[indptr[k]:indptr[k + 1]].astype(np.float64)
            got[:, k] = np.einsum("e,bec->bc", w, verts[:, cols])
    assert np.abs(got - want).max() < 1e-12
    assert hmr.JOINT_NAMES[8] == "OP MidHip" and sel[8] == 0 and hmr.JOINT_NAMES[27] == "Right Hip" and sel[27] == -1
    with pytest.raises(ValueError, match="21"):
        hmr.spin_joint_table(ids[:20], jre)
    bad = ids.copy()
    bad[5] = HR.V_GOLDEN
    with pytest.raises(ValueError, match=f"{HR.V_GOLDEN}"):
        hmr.spin_joint_table(bad, jre)
    bad[5] = -1
    with pytest.raises(ValueError):
        hmr.spin_joint_table(bad, jre)
    with pytest.raises(ValueError):
        hmr.spin_joint_table(ids.astype(np.float64), jre)
    with pytest.raises(ValueError, match="J_regressor_extra"):
        hmr.spin_joint_table(ids, jre[:8])


def test_symbols_exported_and_prototyped():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("pmce_hmr_head_f32", "pmce_hmr_joints_f32", "pmce_smpl_forward_rotmat", "pmce_hmr_head_batch_tile"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not prototyped in include/pmce_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.pmce_hmr_head_batch_tile() == 16


def test_argument_checks_run_before_any_launch():
    """The entry points validate on the host and return before they touch the device: these calls pass made-up pointers."""
    lib = _lib.load()
    p = C.c_void_p(4096)

    def head(feat=p, q=p, cst=p, pt=None, init=None, n=2, theta=p):
        return lib.pmce_hmr_head_f32(feat, q, cst, pt, init, n, p, p, theta, None)

    assert head(n=0) == -1 and "n must be" in _lib.last_error()
    assert head(feat=None) == -1 and "null" in _lib.last_error()
    assert head(q=None) == -1 and head(cst=None) == -1 and head(theta=None) == -1
    assert head(pt=p) == -1 and "go together" in _lib.last_error()
    assert head(init=p) == -1 and "go together" in _lib.last_error()

    def joints(n=2, K=49, V=137, sel=p, cam=p, stride=85, kp=p):
        return lib.pmce_hmr_joints_f32(p, p, sel, p, p, p, cam, stride, n, K, V, kp, p, None)

    assert joints(n=0) == -1 and "n must be" in _lib.last_error()
    assert joints(K=0) == -1 and "K must be" in _lib.last_error()
    assert joints(K=257) == -1 and "K must be" in _lib.last_error()
    assert joints(V=0) == -1 and joints(stride=2) == -1
    assert joints(sel=None) == -1 and "null" in _lib.last_error()
    assert joints(cam=None) == -1 and joints(kp=None) == -1

    par = (C.c_int * 24)(*([0] + list(SR.PARENTS[1:])))

    def rot(V=137, B=2, n=2, nj=24, rotmats=p, stride=157, idx=None, ws_bytes=1 << 20):
        return lib.pmce_smpl_forward_rotmat(p, p, p, p, p, par, nj, rotmats, p, stride, None, idx, n, 1.0, None, p, p, p, ws_bytes, B, V, None)

    assert rot(V=0) == -1 and "V must be" in _lib.last_error()
    assert rot(nj=23) == -1 and "24 joints" in _lib.last_error()
    assert rot(rotmats=None) == -1 and "smpl_forward_rotmat: null" in _lib.last_error()
    assert rot(stride=9) == -1 and "betas_stride" in _lib.last_error()
    assert rot(n=1) == -1 and rot(idx=p, n=3) == -1
    assert rot(ws_bytes=16) == -3 and "workspace" in _lib.last_error()


def test_source_is_built_without_packed_fp32():
    from pmce_amd import build as B
    assert "hmr_head.hip" in B.SOURCES and B.FILE_FLAGS["hmr_head.hip"] == B.NO_PACKED_FP32
