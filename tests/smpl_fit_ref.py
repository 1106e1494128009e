"""Helper of the SMPL fitting tests (not a test module): a plain numpy restatement of ``SMPL.fit`` (csrc/smpl_fit.hip), sample by sample.

The algorithm is this project's (the reference has no inverse of its SMPL layer).  It rests on the layer being LINEAR in the global
rotations G_j (G_0 = R_0, G_j = G_parent(j) R_j): with x = T + S beta + P vec(R_1..23 - I), J = J_T + J_S beta, b_c = J_c - J_parent(c) and
the subtree weights W[v][c] = sum of w[v][k] over the subtree of c,

    v_v = trans + J_0 + sum_j G_j m_vj,      m_vj = w_vj (x_v - J_j) + sum_{c child of j} W_vc b_c

(`linear_forward`; it takes the skinning weights of a vertex to sum to one).  One sweep: Gauss-Seidel over the joints in index order, each
an orthogonal Procrustes problem on the current residual with the pose map held fixed; then the pose map is refreshed and (beta, trans) are
the least-squares solution of the 13-unknown affine problem, solved as a correction of the current values through its normal equations.

The model is the PACKED one (``pmce_amd.smpl.pack_tables`` + ``subtree_weights``): the numbers the kernels read.  `dtype` is the precision
of everything per vertex; the 3 x 3 sums, their SVD, the 13 x 13 system and its Cholesky factorisation are fp64 whatever `dtype`, as in the
kernel - so the float32 run differs from the kernel only in the order of its operations, and its distance from the float64 run is the
yardstick of the device tests."""
import numpy as np

from pmce_amd import smpl as smpl_mod

STATUS_DEGENERATE_JOINT, STATUS_SINGULAR_SHAPE, STATUS_NONFINITE = 1, 2, 4
DEGENERATE_RATIO = 1e-6


def tables(model, dtype=np.float32):
    """A ``smpl_ref.synthetic_model`` dict (or any dict of SMPL's arrays) -> the packed tables as float64 arrays holding `dtype` values
    (float32: the numbers the kernels read), vertex-major: T [V,3], S [V,3,10], P [V,3,207], w [V,24], W [V,24], JT [24,3], JS [24,3,10],
    parents, children."""
    vt, dirs, wt, jt, js = smpl_mod.pack_tables(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor")),
                                                dtype=dtype)
    par = [int(p) for p in model["parents"]]
    par[0] = -1
    W = smpl_mod.subtree_weights(wt.T, par, dtype=dtype)
    d = lambda a: np.asarray(a, dtype=np.float64)    # noqa: E731
    return {"T": d(vt.T), "S": d(dirs[:10].transpose(2, 1, 0)), "P": d(dirs[10:217].transpose(2, 1, 0)), "w": d(wt.T), "W": d(W.T),
            "JT": d(jt), "JS": d(js), "parents": par, "children": [[c for c in range(1, 24) if par[c] == j] for j in range(24)]}


def _cast(tab, dtype):
    return {k: (np.asarray(v, dtype=dtype) if isinstance(v, np.ndarray) else v) for k, v in tab.items()}


def local_rotations(tab, G):
    """R_0 = G_0, R_j = G_parent(j)^T G_j."""
    R = G.copy()
    for j in range(1, 24):
        R[j] = G[tab["parents"][j]].T @ G[j]
    return R


def global_rotations(tab, R):
    G = R.copy()
    for j in range(1, 24):
        G[j] = G[tab["parents"][j]] @ R[j]
    return G


def posed_template(tab, R, beta):
    pm = (R[1:] - np.eye(3, dtype=R.dtype)).reshape(207)
    return tab["T"] + tab["S"] @ beta + tab["P"] @ pm


def joint_term(tab, j, x, J):
    """m_vj [V,3]."""
    m = tab["w"][:, j, None] * (x - J[j])
    for c in tab["children"][j]:
        m = m + tab["W"][:, c, None] * (J[c] - J[j])
    return m


def linear_forward(tab, G, beta, trans, dtype=np.float64):
    """The layer's vertices from GLOBAL rotations by the linear form."""
    t = _cast(tab, dtype)
    G, beta, trans = (np.asarray(a, dtype=dtype) for a in (G, beta, trans))
    x = posed_template(t, local_rotations(t, G), beta)
    J = t["JT"] + t["JS"] @ beta
    return _verts(t, G, x, J, trans)


def _verts(t, G, x, J, trans):
    v = np.broadcast_to(trans + J[0], x.shape).copy()
    for j in range(24):
        v = v + joint_term(t, j, x, J) @ G[j].T
    return v


def _shape_jacobian(t, G):
    """M [V,3,10] with v_v = a_v + M_v beta + trans at fixed G and fixed pose map."""
    JS = t["JS"]
    M = np.broadcast_to(JS[0], (t["T"].shape[0], 3, 10)).copy()
    for j in range(24):
        M = M + t["w"][:, j, None, None] * np.einsum("rc,vck->vrk", G[j], t["S"] - JS[j])
        for c in t["children"][j]:
            M = M + t["W"][:, c, None, None] * (G[j] @ (JS[c] - JS[j]))
    return M


def procrustes(C):
    """C (fp64) -> (U diag(1, 1, det(U V^T)) V^T or None where the rule calls the joint degenerate, sigma_2 / sigma_1)."""
    if not np.isfinite(C).all():
        return None, np.nan
    U, s, Vt = np.linalg.svd(C)
    if s[0] == 0:
        return None, 0.0
    ratio = s[1] / s[0]
    if s[1] <= DEGENERATE_RATIO * s[0]:
        return None, ratio
    d = np.linalg.det(U @ Vt)
    return U @ np.diag([1.0, 1.0, 1.0 if d > 0 else -1.0]) @ Vt, ratio


def fit_one(tab, y, n_sweeps, fit_shape=True, init=None, betas=None, dtype=np.float64):
    """One mesh y [V,3] -> dict(rotmats [24,3,3] local, G, betas, trans, residual, status, history [n_sweeps], ratios [n_sweeps,24])."""
    t = _cast(tab, dtype)
    V = t["T"].shape[0]
    y = np.asarray(y, dtype=dtype)
    eye = np.broadcast_to(np.eye(3, dtype=dtype), (24, 3, 3)).copy()
    if not np.isfinite(y).all():
        return {"rotmats": eye, "G": eye, "betas": np.zeros(10, dtype), "trans": np.zeros(3, dtype), "residual": dtype(np.inf),
                "status": STATUS_NONFINITE, "history": np.full(n_sweeps, np.inf, dtype), "ratios": np.full((n_sweeps, 24), np.nan)}
    if init is not None:
        G = global_rotations(t, np.asarray(init[0], dtype=dtype))
        beta, trans = np.asarray(init[1], dtype=dtype).copy(), np.asarray(init[2], dtype=dtype).copy()
    else:
        G, beta = eye.copy(), np.zeros(10, dtype)
        trans = (y.mean(axis=0, dtype=np.float64) - t["T"].mean(axis=0, dtype=np.float64)).astype(dtype)
    if betas is not None:
        beta = np.asarray(betas, dtype=dtype).copy()
    status, history, ratios = 0, [], np.zeros((n_sweeps, 24))
    for sweep in range(n_sweeps):
        # 1: the residual at the current state
        x = posed_template(t, local_rotations(t, G), beta)
        J = t["JT"] + t["JS"] @ beta
        e = y - _verts(t, G, x, J, trans)
        # 2: the joints, in index order
        for j in range(24):
            m = joint_term(t, j, x, J)
            r = e + m @ G[j].T
            C = r.astype(np.float64).T @ m.astype(np.float64)
            Gn, ratios[sweep, j] = procrustes(C)
            if Gn is None:
                status |= STATUS_DEGENERATE_JOINT
            else:
                G[j] = Gn.astype(dtype)
            e = r - m @ G[j].T
        # 3: the pose map of the new rotations, then (beta, trans)
        R = local_rotations(t, G)
        x = posed_template(t, R, beta)
        e = y - _verts(t, G, x, J, trans)
        if fit_shape:
            M = _shape_jacobian(t, G).astype(np.float64)
            A = np.concatenate([M, np.broadcast_to(np.eye(3), (V, 3, 3))], axis=2).reshape(3 * V, 13)
            N, rhs = A.T @ A, A.T @ e.astype(np.float64).reshape(3 * V)
            try:
                if not (np.isfinite(N).all() and np.isfinite(rhs).all()):
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(N)
                d = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
                beta, trans = (beta + d[:10]).astype(dtype), (trans + d[10:]).astype(dtype)
            except np.linalg.LinAlgError:
                status |= STATUS_SINGULAR_SHAPE
        else:
            trans = (trans + e.mean(axis=0, dtype=np.float64)).astype(dtype)
        # 4: the distance at the new state
        x = posed_template(t, R, beta)
        J = t["JT"] + t["JS"] @ beta
        e = y - _verts(t, G, x, J, trans)
        history.append(np.sqrt((e * e).sum(axis=1)).mean(dtype=np.float64))
    return {"rotmats": local_rotations(t, G), "G": G, "betas": beta, "trans": trans, "residual": dtype(history[-1]), "status": status,
            "history": np.array(history, dtype=dtype), "ratios": ratios}


def fit(tab, verts, n_sweeps=10, fit_shape=True, init=None, betas=None, dtype=np.float64):
    """``SMPL.fit`` on verts [B,V,3] -> dict of stacked arrays (keys as `fit_one`); `min_ratio` is the smallest sigma_2 / sigma_1 met over
    all rows, sweeps and joints, exact zeros (a joint that moves no vertex) left out."""
    rows = [fit_one(tab, verts[b], n_sweeps, fit_shape, None if init is None else tuple(a[b] for a in init),
                    None if betas is None else betas[b], dtype) for b in range(len(verts))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    rt = out["ratios"][np.isfinite(out["ratios"]) & (out["ratios"] > 0)]
    out["min_ratio"] = float(rt.min()) if rt.size else 0.0
    return out
