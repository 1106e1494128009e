"""Helper of the SMPL tests (not a test module): seeded synthetic SMPL-shaped models and parameter rows, and a plain numpy restatement
of the reference's layer (smplpytorch/pytorch/smpl_layer.py:65-158 on rodrigues_layer.py:13-52) in a chosen dtype, of the 3DPW output
transform (data/PW3D/dataset.py:86,240) and of the Human3.6M world -> camera form (data/Human36M/dataset.py:354-398, with the
``transforms3d`` axis-angle round trip written out).  tests/golden/make_golden_smpl.py drives the REAL SMPL_Layer on the same model and
rows; test_smpl_host.py holds this restatement to those results."""
import numpy as np

V_GOLDEN, B_GOLDEN, SEED = 137, 19, 11
PARENTS = (2 ** 32 - 1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)   # SMPL's kintree_table[0]


def synthetic_model(V, seed):
    """A random model of SMPL's shapes, float64 arrays holding float32 VALUES (an fp32 and an fp64 run read the same numbers)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)    # noqa: E731
    w = rng.random((V, 24)) ** 8
    w[w < 0.02 * w.max(axis=1, keepdims=True)] = 0.0
    w = f32(w / w.sum(axis=1, keepdims=True))
    jr = rng.random((24, V)) ** 6
    return {"v_template": f32(rng.normal(0, 0.4, (V, 3))), "shapedirs": f32(rng.normal(0, 0.01, (V, 3, 10))),
            "posedirs": f32(rng.normal(0, 0.005, (V, 3, 207))), "weights": w, "J_regressor": f32(jr / jr.sum(axis=1, keepdims=True)),
            "parents": np.array(PARENTS, dtype=np.int64), "faces": rng.integers(0, V, size=(2 * V, 3)).astype(np.int32)}


def cases(B, seed):
    """pose[B,72] ~ N(0, 0.6), betas[B,10] ~ N(0, 1), trans[B,3] ~ N(0, 0.5) (float32 values), with the edge rows that fit into B:
    0: all-zero pose; 1: pose ~ N(0, 1e-6); 2: root rotation (3.1, 0, 0) with joint 1 at (0, 3.14159, 0); 3: pose ~ N(0, 2);
    4: zero betas; 5: zero trans."""
    rng = np.random.default_rng(seed)
    pose = rng.normal(0, 0.6, (B, 72))
    betas = rng.normal(0, 1.0, (B, 10))
    trans = rng.normal(0, 0.5, (B, 3))
    tiny, wide = rng.normal(0, 1e-6, 72), rng.normal(0, 2.0, 72)
    if B > 0:
        pose[0] = 0.0
    if B > 1:
        pose[1] = tiny
    if B > 2:
        pose[2, :3] = (3.1, 0.0, 0.0)
        pose[2, 3:6] = (0.0, 3.14159, 0.0)
    if B > 3:
        pose[3] = wide
    if B > 4:
        betas[4] = 0.0
    if B > 5:
        trans[5] = 0.0
    f32 = lambda a: a.astype(np.float32).astype(np.float64)    # noqa: E731
    return f32(pose), f32(betas), f32(trans)


def rodrigues(axisang, dtype=np.float64):
    """batch_rodrigues + quat2mat (rodrigues_layer.py:13-52) on [N,3] -> [N,3,3], every operation in `dtype`."""
    a = np.asarray(axisang, dtype=dtype)
    norm = np.sqrt(((a + dtype(1e-8)) ** 2).sum(axis=1, dtype=dtype))[:, None]
    axis = a / norm
    half = norm * dtype(0.5)
    q = np.concatenate([np.cos(half), np.sin(half) * axis], axis=1).astype(dtype)
    q = q / np.sqrt((q ** 2).sum(axis=1, dtype=dtype))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return np.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                     2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], axis=1).reshape(-1, 3, 3).astype(dtype)


def forward(model, pose, betas, trans=None, dtype=np.float64, root_rot=None):
    """SMPL_Layer.forward (center_idx = None) -> (verts[B,V,3], joints[B,24,3]) in `dtype`.  root_rot [B,3,3] replaces the root joint's
    rotation matrix (what a changed root pose amounts to)."""
    c = lambda a: np.asarray(a, dtype=dtype)    # noqa: E731
    pose, betas = c(pose), c(betas)
    B = pose.shape[0]
    vt, sd, pd, wts, jr = (c(model[k]) for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor"))
    parents = [int(p) for p in model["parents"]]
    R = rodrigues(pose.reshape(-1, 3), dtype).reshape(B, 24, 3, 3)
    if root_rot is not None:
        R[:, 0] = c(root_rot)
    pose_map = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(B, 207)
    v_shaped = vt[None] + np.einsum("vck,bk->bvc", sd, betas).astype(dtype)
    J = np.einsum("jv,bvc->bjc", jr, v_shaped).astype(dtype)
    v_posed = v_shaped + np.einsum("vck,bk->bvc", pd, pose_map).astype(dtype)
    G = np.zeros((B, 24, 4, 4), dtype=dtype)
    G[:, :, 3, 3] = 1
    G[:, 0, :3, :3], G[:, 0, :3, 3] = R[:, 0], J[:, 0]
    for i in range(1, 24):
        L = np.zeros((B, 4, 4), dtype=dtype)
        L[:, 3, 3] = 1
        L[:, :3, :3], L[:, :3, 3] = R[:, i], J[:, i] - J[:, parents[i]]
        G[:, i] = np.matmul(G[:, parents[i]], L)
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], J).astype(dtype)
    T = np.einsum("bjrc,vj->bvrc", A, wts).astype(dtype)
    vh = np.concatenate([v_posed, np.ones((B, vt.shape[0], 1), dtype=dtype)], axis=2)
    verts = np.einsum("bvrc,bvc->bvr", T, vh).astype(dtype)[:, :, :3]
    joints = G[:, :, :3, 3].copy()
    if trans is not None:
        verts = verts + c(trans)[:, None]
        joints = joints + c(trans)[:, None]
    return verts, joints


def pw3d_targets(model, pose, betas, trans, root_mm, dtype=np.float64):
    """data/PW3D/dataset.py:86,240: (mesh * 1000 - root, joints * 1000 - root), mm."""
    v, j = forward(model, pose, betas, trans, dtype)
    r = np.asarray(root_mm, dtype=dtype)[:, None]
    return v * dtype(1000) - r, j * dtype(1000) - r


def axangle2mat(axis, angle):
    """transforms3d.axangles.axangle2mat (normalises the axis)."""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = np.cos(angle), np.sin(angle)
    C = 1 - c
    return np.array([[x * x * C + c, x * y * C - z * s, z * x * C + y * s], [x * y * C + z * s, y * y * C + c, y * z * C - x * s],
                     [z * x * C - y * s, y * z * C + x * s, z * z * C + c]])


def mat2axangle(M):
    """transforms3d.axangles.mat2axangle: the unit eigenvector of eigenvalue 1, the angle from the trace and one off-diagonal entry."""
    M = np.asarray(M, dtype=np.float64)
    L, W = np.linalg.eig(M.T)
    i = np.where(np.abs(L - 1.0) < 1e-5)[0]
    d = np.real(W[:, i[-1]]).squeeze()
    cosa = (np.trace(M) - 1.0) / 2.0
    if abs(d[2]) > 1e-8:
        sina = (M[1, 0] + (cosa - 1.0) * d[0] * d[1]) / d[2]
    elif abs(d[1]) > 1e-8:
        sina = (M[0, 2] + (cosa - 1.0) * d[0] * d[2]) / d[1]
    else:
        sina = (M[2, 1] + (cosa - 1.0) * d[1] * d[2]) / d[0]
    return d, np.arctan2(sina, cosa)


def h36m_camera_form(model, pose, betas, trans, cam_R, cam_t, dtype=np.float64, zero_root="cam_R"):
    """Human36M.get_smpl_coord (data/Human36M/dataset.py:354-398), sample by sample -> (mesh, joints) in mm, camera coordinates.  In fp64
    the root pose goes through the reference's axis-angle round trip; in another dtype the matrices are composed directly.  A zero root
    pose is 0 / 0 in the reference; zero_root='cam_R' composes cam_R with the identity instead."""
    pose, betas, trans, cam_R, cam_t = (np.asarray(a, dtype=np.float64) for a in (pose, betas, trans, cam_R, cam_t))
    B = pose.shape[0]
    betas = betas.copy()
    betas[(np.abs(betas) > 3).any(axis=1)] = 0.0
    pose = pose.copy()
    root_rot = None
    if dtype == np.float64:
        for b in range(B):
            angle = np.linalg.norm(pose[b, :3])
            if angle == 0 and zero_root == "cam_R":
                m = cam_R[b]
            else:
                m = cam_R[b] @ axangle2mat(pose[b, :3] / angle, angle)
            axis, ang = mat2axangle(m)
            pose[b, :3] = axis * ang
    else:
        root_rot = np.matmul(cam_R.astype(dtype), rodrigues(pose[:, :3], dtype))
    v, j = forward(model, pose, betas, None, dtype, root_rot=root_rot)
    R, t = cam_R.astype(dtype), cam_t.astype(dtype)
    tr = np.einsum("brc,bc->br", R, trans.astype(dtype)) + t / dtype(1000)
    j0 = j[:, 0]
    tr = tr - j0 + np.einsum("brc,bc->br", R, j0)
    return ((v + tr[:, None]) * dtype(1000)).astype(dtype), ((j + tr[:, None]) * dtype(1000)).astype(dtype)


def random_rotations(n, seed):
    """n proper rotations (QR of a Gaussian matrix, determinant fixed to +1), float32 values."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out).astype(np.float32).astype(np.float64)
