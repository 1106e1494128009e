"""GPU tests of SPIN's regression head (pmce_amd/hmr.py on csrc/hmr_head.hip, smpl.SMPL.forward_rotmat on csrc/smpl.hip) against the
real reference functions' results (tests/golden/hmr_head.npz, made by tests/golden/make_golden_hmr_head.py).

The yardstick is the reference's OWN fp32 error: dev32 = the largest deviation of its fp32 run from its fp64 run on the same inputs, per
output.  The device result must stay within 4 x dev32 of the fp64 record - the factor is the project's (test_gpu_smpl.py): it covers
another summation order (here: one folded 2048-term product instead of three rounds of two 1024-wide layers), nothing else.  Where a
dev32 is 0 (exact cases of the rotation table) the floor is 2^-22, two ulps of a number below 1.  Shapes: n = 19 = one batch tile of 16
and a tail of 3; n = 17 = the tile + 1; V = 137 as in the SMPL tests.

Every test prints the deviation it measures before it asserts (run with -s)."""
import os.path as osp

import numpy as np
import pytest
import torch

import extractor_ref as ER
import hmr_ref as HR
from conftest import GOLDEN
from pmce_amd import _lib, hmr, ops, smpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -22
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")


def tol(dev32):
    return 4 * float(dev32) if float(dev32) > 0 else FLOOR


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def gold():
    return np.load(osp.join(GOLDEN, "hmr_head.npz"))


@pytest.fixture(scope="module")
def layer():
    model = HR.smpl_model()
    return smpl.SMPL({"neutral": smpl.SMPLModel.from_arrays(*(model[k] for k in MODEL_KEYS))})


@pytest.fixture(scope="module")
def head():
    h = hmr.RegressorHead.from_state_dict(HR.state_dict(), DEV)
    return h.set_joint_table(*hmr.spin_joint_table(HR.extra_vertex_ids(), HR.extra_regressor()))


@pytest.fixture(scope="module")
def feats():
    return torch.from_numpy(HR.features()).to(DEV)


@pytest.fixture(scope="module")
def out19(head, layer, feats):
    """The head + SMPL + joints on the fixture's 19 rows, computed once (host arrays)."""
    return host(head(feats, layer))


def check(name, got, want, dev32):
    d = np.abs(got.astype(np.float64) - want).max()
    print(f"{name}: {d:.3e} (reference fp32 {float(dev32):.3e}, bound {tol(dev32):.3e})")
    assert got.shape == want.shape and np.isfinite(got).all(), name
    assert d <= tol(dev32), name


def test_head_against_the_fixture(gold, out19):
    for k in ("theta", "rotmat", "state"):
        check(k, out19[k], gold[k + "64"], gold["dev32_" + k])
    assert np.array_equal(out19["pred_cam"], out19["theta"][:, :3]) and np.array_equal(out19["theta"][:, :3], out19["state"][:, 154:])
    assert np.array_equal(out19["theta"][:, 75:], out19["state"][:, 144:154])


def test_batch_invariance(gold, head, feats, out19):
    tile = _lib.load().pmce_hmr_head_batch_tile()
    assert tile + 1 < HR.N_GOLDEN
    for n in (1, 5, tile + 1, HR.N_GOLDEN):
        o = host(head(feats[:n].clone()))
        for k in ("state", "rotmat", "theta"):
            assert np.array_equal(o[k], out19[k][:n]), f"{k}: rows 0..{n - 1} of n = {n} differ from the same rows of n = {HR.N_GOLDEN}"
    # wherever the sample sits: row 18 (the tail tile's third) moved to the front
    o = host(head(feats.flip(0).contiguous()))
    for k in ("state", "rotmat", "theta"):
        assert np.array_equal(o[k][::-1], out19[k]), k
    # two runs give the same bits
    o = host(head(feats))
    assert all(np.array_equal(o[k], out19[k]) for k in ("state", "rotmat", "theta"))


def test_per_sample_initial_state(gold, head, feats, out19):
    sd = HR.state_dict()
    n = HR.N_GOLDEN
    o = host(head(feats, init_pose=sd["init_pose"].expand(n, -1), init_shape=sd["init_shape"], init_cam=sd["init_cam"].expand(n, -1)))
    for k in ("theta", "rotmat", "state"):
        check("per-sample init, " + k, o[k], gold[k + "64"], gold["dev32_" + k])
    # only one of the three given, and a state that differs per sample: against the fp64 iteration
    rng = np.random.default_rng(5)
    cam = (sd["init_cam"].numpy() + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    o = host(head(feats, init_cam=torch.from_numpy(cam)))
    init = HR.initial_state(sd, n)
    init[:, 154:] = cam
    want = HR.iterate(sd, HR.features(), 3, init)
    check("per-sample camera, state", o["state"], want, gold["dev32_state"])
    with pytest.raises(ValueError, match="init_pose"):
        head(feats, init_pose=sd["init_pose"].expand(3, -1))


def test_rotation_cases(gold):
    """The rotation stage alone: with Q = 0, P = I, c = 0 the affine map returns the initial state to the bit, so chosen 6D vectors reach
    rot6d_to_rotmat and rotation_matrix_to_angle_axis as they are.  Every joint of sample c holds case c."""
    names, six = HR.rotation_cases()
    assert list(gold["rot_names"]) == names
    C = len(names)
    rng = np.random.default_rng(2)
    init = np.concatenate([np.tile(six.astype(np.float32), (1, 24)), rng.normal(0, 1, (C, 13)).astype(np.float32)], 1)
    pmi_t = np.zeros((157, 160), np.float32)                           # P = I: the entry takes P - I
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)    # noqa: E731
    state, rotmat, theta = torch.empty(C, 157, device=DEV), torch.empty(C, 24, 3, 3, device=DEV), torch.empty(C, 85, device=DEV)
    ops.hmr_head(d(rng.random((C, 2048), dtype=np.float32)), d(np.zeros((2048, 160), np.float32)), d(np.zeros(157, np.float32)), d(pmi_t),
                 d(init), state, rotmat, theta)
    torch.cuda.synchronize()
    state, rotmat, theta = state.cpu().numpy(), rotmat.cpu().numpy(), theta.cpu().numpy()
    nan = names.index("nan")
    ok = np.arange(C) != nan
    assert np.array_equal(state[ok], init[ok]), "Q = 0, P = I, c = 0 must return the initial state to the bit"
    assert np.isnan(state[nan]).all()                                  # (0 x NaN: the whole sample)
    assert np.array_equal(theta[ok, :3], init[ok, 154:]) and np.array_equal(theta[ok, 75:], init[ok, 144:154])
    aa = theta[:, 3:75].reshape(C, 24, 3)
    for c, name in enumerate(names):
        Rw, aw = gold["rot_rotmat64"][c], gold["rot_aa64"][c]
        assert np.array_equal(rotmat[c], np.broadcast_to(rotmat[c, 0], (24, 3, 3)), equal_nan=True), f"{name}: the joints differ"
        assert np.array_equal(aa[c], np.broadcast_to(aa[c, 0], (24, 3))), f"{name}: the joints differ"
        assert np.array_equal(np.isnan(rotmat[c, 0]), np.isnan(Rw)), name
        dR = np.nanmax(np.abs(rotmat[c, 0] - Rw)) if not np.isnan(Rw).all() else 0.0
        da = np.abs(aa[c, 0] - aw).max()
        bR, ba = 4 * gold["rot_dev32_rotmat"][c] + FLOOR, 4 * gold["rot_dev32_aa"][c] + FLOOR
        print(f"{name} (case {int(gold['rot_branch'][c])}): rotmat {dR:.3e} (bound {bR:.3e}), angle-axis {da:.3e} (bound {ba:.3e})")
        assert np.isfinite(aa[c]).all() and dR <= bR and da <= ba, name
    assert np.array_equal(aa[nan], np.zeros((24, 3))), "NaN -> 0 (geometry.py:112)"
    assert np.array_equal(rotmat[names.index("a1_zero"), 0], np.diag([0, 1, 0]).astype(np.float32))
    assert np.array_equal(rotmat[names.index("a2_parallel"), 0], np.diag([1, 0, 0]).astype(np.float32))
    assert np.array_equal(rotmat[names.index("both_zero"), 0], np.zeros((3, 3), np.float32))


def test_smpl_from_rotation_matrices(gold, layer):
    n = HR.N_GOLDEN
    R = torch.from_numpy(gold["rotmat64"].astype(np.float32)).to(DEV)
    state = torch.from_numpy(gold["state64"].astype(np.float32)).to(DEV)
    betas = state[:, 144:154]                                           # a view with a row stride of 157, read in place
    v, j = layer.forward_rotmat(R, betas)
    torch.cuda.synchronize()
    vh, jh = v.cpu().numpy(), j.cpu().numpy()
    check("verts from the record's matrices", vh, gold["verts64"], gold["dev32_verts"])
    assert np.isfinite(jh).all() and jh.shape == (n, 24, 3)
    v2, j2 = layer.forward_rotmat(R, betas.contiguous())
    assert torch.equal(v2, v) and torch.equal(j2, j), "the strided and the contiguous shape rows differ"
    # the posed joints: the fixture's kp_3d holds joint JOINT_MAP[k] < 24 at k
    for k, i in enumerate(hmr.JOINT_MAP):
        if i < 24:
            assert np.abs(jh[:, i] - gold["kp_3d64"][:, k]).max() <= tol(gold["dev32_kp_3d"])
    # a subset in place, and one sample alone: the same bits as in the batch
    idx = torch.tensor([2, 5, 18], dtype=torch.int32, device=DEV)
    vs, js = layer.forward_rotmat(R, betas, sample_index=idx)
    assert torch.equal(vs[idx.long()], v[idx.long()]) and torch.equal(js[idx.long()], j[idx.long()])
    for i in (0, 6, 18):
        v1, j1 = layer.forward_rotmat(R[i:i + 1], betas[i:i + 1])
        assert torch.equal(v1[0], v[i]) and torch.equal(j1[0], j[i]), f"row {i} alone differs from row {i} of B = {n}"
    # translation, scale and offset as in forward
    t = torch.from_numpy(np.random.default_rng(1).normal(0, 0.5, (n, 3)).astype(np.float32)).to(DEV)
    vt, _ = layer.forward_rotmat(R, betas, t, scale=1000.0, offset=t)
    assert (vt.cpu().numpy() - ((vh.astype(np.float64) + t.cpu().numpy()[:, None]) * 1000 - t.cpu().numpy()[:, None])).__abs__().max() < 1e-3
    with pytest.raises(_lib.PmceError):
        layer.forward_rotmat(R.reshape(n, 216), betas)
    with pytest.raises(_lib.PmceError):
        layer.forward_rotmat(R, betas[:3])


def test_mesh_and_joints_against_the_fixture(gold, out19):
    for k in ("verts", "kp_3d", "kp_2d"):
        check(k, out19[k], gold[k + "64"], gold["dev32_" + k])


def test_hmr_end_to_end(gold, layer):
    """Backbone + head on the extractor fixture's patches against the reference's HMR.forward(return_features=True)."""
    model = hmr.HMR.from_state_dict(HR.hmr_state_dict(), DEV, smpl=layer)
    model.head.set_joint_table(*hmr.spin_joint_table(HR.extra_vertex_ids(), HR.extra_regressor()))
    x = ER.patches().to(DEV)
    feats, out = model(x, return_features=True)
    o = host(out)
    assert feats.shape == (ER.B_GOLDEN, 2048) and torch.equal(feats, model.feature_extractor(x))
    for k in ("theta", "verts", "kp_3d", "kp_2d"):
        check("HMR " + k, o[k], gold["hmr_" + k + "64"], gold["hmr_dev32_" + k])
    assert set(model(x)) == set(out)
    with pytest.raises(NotImplementedError):
        model.train()
