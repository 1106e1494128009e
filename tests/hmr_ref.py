"""Helper of the HMR head's tests (not a test module): the seeded inputs of the fixture tests/golden/hmr_head.npz and a plain numpy fp64
restatement of the reference's head - the iterated regressor (lib/models/spin.py:169-180, 252-263, eval mode), rot6d_to_rotmat and
rotation_matrix_to_angle_axis (lib/geometry.py:346-360, 84-249), the 49 joints (lib/models/smpl_mps.py:65-83) and the weak-perspective
projection (spin.py:309-353).  tests/golden/make_golden_hmr_head.py drives the REAL reference functions on the same inputs;
test_hmr_host.py holds this restatement to those records."""
import numpy as np

import smpl_ref as SR
from pmce_amd import hmr, synth

SEED = 31
N_GOLDEN = 19
V_GOLDEN = SR.V_GOLDEN            # 137
MAX_ANGLE = 2.5                   # every rotation of the fixture stays below it (the stand-in's axis-angle round trip)


HMR_FEATURE_GAIN = 2.0 ** -7      # the end-to-end case: the synthetic backbone's features have an rms near 80 (synth.hmr_head_state_dict)


def state_dict(seed=SEED, feature_gain=1.0):
    return synth.hmr_head_state_dict(seed, feature_gain=feature_gain)


def hmr_state_dict():
    """The end-to-end case's state dict: the extractor fixture's backbone and this fixture's head behind it."""
    import extractor_ref as ER
    sd = synth.make_state_dict(synth.extractor_spec(), ER.SEED)
    sd.update(state_dict(feature_gain=HMR_FEATURE_GAIN))
    return sd


def features(n=N_GOLDEN, seed=SEED):
    """[n,2048] float32, non-negative and sparse-ish like average-pooled ReLU features; row i does not depend on n."""
    f = synth.uniform_pm1("hmr.features", n * 2048, seed)
    return np.maximum(np.float32(1.5) * f - np.float32(0.3), np.float32(0.0)).reshape(n, 2048)


def smpl_model(seed=SEED):
    return SR.synthetic_model(V_GOLDEN, seed)


def extra_regressor(V=V_GOLDEN, seed=SEED):
    """A seeded J_regressor_extra [9,V]: sparse non-negative rows that sum to 1, float32 values."""
    rng = np.random.default_rng(seed + 1)
    jr = rng.random((9, V)) ** 6
    jr[jr < 0.05 * jr.max(axis=1, keepdims=True)] = 0.0
    return (jr / jr.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def extra_vertex_ids(V=V_GOLDEN, seed=SEED):
    """21 seeded vertex ids (a stand-in for smplx's table, which is not available offline)."""
    return np.random.default_rng(seed + 2).choice(V, size=21, replace=False).astype(np.int64)


def rotation(axis, angle):
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def to_6d(R):
    """The 6D vector whose reshape(3, 2) holds R's first two columns (element 2 r + c = R[r][c])."""
    return np.asarray(R, dtype=np.float64)[:, :2].reshape(6)


# name -> 6D vector (float32 values).  Branch = which of rotation_matrix_to_quaternion's four cases the matrix takes.
def rotation_cases():
    c = [("identity", to_6d(np.eye(3))),
         ("pi_about_x", np.array([1, 0, 0, -1, 0, 0], dtype=np.float64)),          # diag(1, -1, -1): R22 < eps, R00 > R11
         ("pi_about_y", np.array([-1, 0, 0, 1, 0, 0], dtype=np.float64)),          # diag(-1, 1, -1): R22 < eps, R00 <= R11
         ("pi_about_z", np.array([-1, 0, 0, -1, 0, 0], dtype=np.float64)),         # diag(-1, -1, 1): R22 >= eps, R00 < -R11
         ("generic", to_6d(rotation((0.3, -0.5, 0.8), 0.9))),                      # positive trace: the fourth case
         ("wide_x", to_6d(rotation((0.9, 0.3, 0.2), 2.8))),
         ("wide_y", to_6d(rotation((0.2, 0.9, -0.3), 2.8))),
         ("wide_z", to_6d(rotation((-0.3, 0.2, 0.9), 2.8))),
         ("near_pi", to_6d(rotation((1.0, 2.0, 3.0), np.pi - 1e-3))),
         ("tiny", to_6d(rotation((1.0, 2.0, 3.0), 1e-4))),
         ("scaled", 3.0 * to_6d(rotation((0.5, 0.5, -0.7), 1.3)) + np.array([0, 0.4, 0, -0.2, 0, 0.1])),   # not orthonormal: Gram-Schmidt works
         ("a1_zero", np.array([0, 0, 0, 1, 0, 0], dtype=np.float64)),              # a1 = 0, a2 = (0, 1, 0)
         ("a2_parallel", np.array([2, 3, 0, 0, 0, 0], dtype=np.float64)),          # a1 = (2, 0, 0), a2 = (3, 0, 0): the residual is exactly 0
         ("both_zero", np.zeros(6)),
         ("nan", np.array([np.nan, 0, 0, 1, 0, 0], dtype=np.float64))]             # NaN matrix, angle-axis 0 (geometry.py:112)
    names = [n for n, _ in c]
    return names, np.stack([v for _, v in c]).astype(np.float32).astype(np.float64)


def quaternion_branch(R, dtype=np.float64):
    """0..3: the case rotation_matrix_to_quaternion selects for each matrix [N,3,3] when the tests run in `dtype`."""
    R = np.asarray(R, dtype=dtype)
    d2, d01, d0n1 = R[:, 2, 2] < dtype(1e-6), R[:, 0, 0] > R[:, 1, 1], R[:, 0, 0] < -R[:, 1, 1]
    return np.where(d2, np.where(d01, 0, 1), np.where(d0n1, 2, 3))


def rot6d_to_rotmat(x):
    """geometry.py:346-360 on [N,6] -> [N,3,3]."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    with np.errstate(invalid="ignore"):
        b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(axis=1, keepdims=True)), 1e-6)
        u = a2 - (b1 * a2).sum(axis=1, keepdims=True) * b1
        b2 = u / np.maximum(np.sqrt((u * u).sum(axis=1, keepdims=True)), 1e-6)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-1)


def rotmat_to_angle_axis(R):
    """geometry.py:84-249 on [N,3,3] -> [N,3]: the four-case quaternion on the transpose the reference takes, then the angle-axis with
    k = 2 where sin^2 is 0 and NaN -> 0."""
    R = np.asarray(R, dtype=np.float64)
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = (R[:, i, j] for i in range(3) for j in range(3))
    t0, t1, t2, t3 = 1 + R00 - R11 - R22, 1 - R00 + R11 - R22, 1 - R00 - R11 + R22, 1 + R00 + R11 + R22
    q = [np.stack([R21 - R12, t0, R10 + R01, R02 + R20], -1), np.stack([R02 - R20, R10 + R01, t1, R21 + R12], -1),
         np.stack([R10 - R01, R02 + R20, R21 + R12, t2], -1), np.stack([t3, R21 - R12, R02 - R20, R10 - R01], -1)]
    with np.errstate(invalid="ignore", divide="ignore"):
        br = quaternion_branch(R)
        quat = np.choose(br[:, None], q)
        t = np.choose(br, [t0, t1, t2, t3])
        quat = quat / np.sqrt(t)[:, None] * 0.5
        s2 = quat[:, 1] ** 2 + quat[:, 2] ** 2 + quat[:, 3] ** 2
        s, c = np.sqrt(s2), quat[:, 0]
        two_theta = 2.0 * np.where(c < 0, np.arctan2(-s, -c), np.arctan2(s, c))
        k = np.where(s2 > 0, two_theta / s, 2.0)
        aa = quat[:, 1:] * k[:, None]
    aa[np.isnan(aa)] = 0.0
    return aa


def dec_stack(sd):
    f64 = lambda k: np.asarray(sd[k], dtype=np.float64)    # noqa: E731
    return (np.concatenate([f64("decpose.weight"), f64("decshape.weight"), f64("deccam.weight")], 0),
            np.concatenate([f64("decpose.bias"), f64("decshape.bias"), f64("deccam.bias")], 0))


def initial_state(sd, n):
    s0 = np.concatenate([np.asarray(sd[k], dtype=np.float64) for k in ("init_pose", "init_shape", "init_cam")], 1)
    return np.repeat(s0, n, axis=0)


def iterate(sd, xf, n_iter=3, init=None):
    """The iterated regressor in fp64: [n,2048] -> state [n,157] = (6D pose, shape, camera)."""
    f64 = lambda k: np.asarray(sd[k], dtype=np.float64)    # noqa: E731
    xf = np.asarray(xf, dtype=np.float64)
    D, bD = dec_stack(sd)
    s = initial_state(sd, xf.shape[0]) if init is None else np.asarray(init, dtype=np.float64)
    for _ in range(n_iter):
        xc = np.concatenate([xf, s], 1) @ f64("fc1.weight").T + f64("fc1.bias")
        xc = xc @ f64("fc2.weight").T + f64("fc2.bias")
        s = xc @ D.T + bD + s
    return s


def joints49(posed_joints, verts, ids, jr_extra):
    """smpl_mps.py:71-83: [24 posed joints | the 21 vertices `ids` | J_regressor_extra verts] indexed by the joint map."""
    j54 = np.concatenate([posed_joints, verts[:, ids], np.einsum("jv,bvc->bjc", jr_extra, verts)], 1)
    return j54[:, list(hmr.JOINT_MAP)]


def projection(kp_3d, cam):
    """spin.py:309-353 in closed form -> [n,K,2]."""
    t = np.stack([cam[:, 1], cam[:, 2], 2 * 5000.0 / (224.0 * cam[:, 0] + 1e-9)], -1)
    p = kp_3d + t[:, None]
    return 5000.0 * (p[:, :, :2] / p[:, :, 2:]) / 112.0


def forward(sd, xf, model=None, ids=None, jr_extra=None, n_iter=3, init=None):
    """The whole head in fp64 -> dict(state, rotmat, theta[, verts, kp_3d, kp_2d]).  The SMPL layer is fed the angle-axis of the matrices,
    as the fixture's stand-in for smplx feeds smplpytorch's layer."""
    s = iterate(sd, xf, n_iter, init)
    n = s.shape[0]
    R = rot6d_to_rotmat(s[:, :144].reshape(-1, 6))
    aa = rotmat_to_angle_axis(R).reshape(n, 72)
    out = {"state": s, "rotmat": R.reshape(n, 24, 3, 3), "theta": np.concatenate([s[:, 154:], aa, s[:, 144:154]], 1)}
    if model is not None:
        verts, joints = SR.forward(model, aa, s[:, 144:154], None, np.float64)
        out["verts"] = verts
        if ids is not None:
            out["kp_3d"] = joints49(joints, verts, ids, jr_extra)
            out["kp_2d"] = projection(out["kp_3d"], s[:, 154:])
    return out
