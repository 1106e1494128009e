"""CPU-only tests of SMPL fitting's host side: the linear form the algorithm rests on, the subtree-weight table, the numpy restatement
(tests/smpl_fit_ref.py) that the device tests measure against - does it converge as the design says -, the C entry points' declarations
and argument checks, and ``save_results(smpl=True)``."""
import ctypes as C
import os.path as osp
import pickle
import re

import numpy as np
import pytest

import smpl_fit_ref as F
import smpl_ref as SR
from conftest import REPO
from pmce_amd import _lib, demo, smpl


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_linear_form_is_the_layer():
    """v = trans + J_0 + sum_j G_j m_vj against the reference's layer, fp64, unrounded tables.  The form takes a vertex's weights to
    sum to ONE (the root joint's position enters once); the synthetic model's are normalised and then rounded to fp32, so they are
    renormalised in fp64 here, and with the rounded ones the two differ by (sum w - 1) J_0, which is asserted as well."""
    model = SR.synthetic_model(SR.V_GOLDEN, SR.SEED)
    pose, betas, trans = SR.cases(19, 11)
    R = SR.rodrigues(pose.reshape(-1, 3)).reshape(19, 24, 3, 3)
    exact = dict(model, weights=model["weights"] / model["weights"].sum(axis=1, keepdims=True))
    for m, slack in ((exact, 0.0), (model, None)):
        tab = F.tables(m, dtype=np.float64)
        want, _ = SR.forward(m, pose, betas, trans)
        got = np.stack([F.linear_forward(tab, F.global_rotations(tab, R[b]), betas[b], trans[b]) for b in range(19)])
        if slack is None:
            j0 = np.abs(tab["JT"][0] + np.einsum("ck,bk->bc", tab["JS"][0], betas)).max()
            slack = np.abs(m["weights"].sum(axis=1) - 1).max() * j0
        d = np.abs(got - want).max()
        print(f"linear form vs layer: {d:.2e} (allowed {slack + 1e-12:.2e})")
        assert d <= slack + 1e-12      # values of order 1, sums of 217 and 24 terms in fp64


def test_subtree_weights_against_a_tree_walk():
    model = SR.synthetic_model(SR.V_GOLDEN, SR.SEED)
    par = [int(p) for p in model["parents"]]
    w = model["weights"]

    def below(c):
        out = [c]
        for k in range(1, 24):
            if par[k] == c:
                out += below(k)
        return out

    want = np.stack([w[:, below(c)].sum(axis=1) for c in range(24)])
    got = smpl.subtree_weights(w, par, dtype=np.float64)
    assert got.shape == (24, SR.V_GOLDEN) and np.abs(got - want).max() < 1e-15
    assert np.abs(got[0] - w.sum(axis=1)).max() < 1e-15 and np.array_equal(got[23], w[:, 23])
    m = smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents")))
    assert m.subtree_weights_t.dtype == np.float32 and m.subtree_weights_t.shape == m.weights_t.shape
    assert np.array_equal(m.subtree_weights_t, want.astype(np.float32))


@pytest.fixture(scope="module")
def v600():
    model = SR.synthetic_model(600, 11)
    pose, betas, trans = SR.cases(12, 5)
    pose[3] *= 0.4
    verts, _ = SR.forward(model, pose, betas, trans)
    return F.tables(model), (pose, betas, trans), verts.astype(np.float32)


def test_restatement_converges(v600):
    tab, _, y = v600
    out = F.fit(tab, y, 12)
    h = out["history"]
    print("residual after sweeps 1, 6, 12 (max over rows):", h[:, 0].max(), h[:, 5].max(), h[:, 11].max(), "min sigma2/sigma1", out["min_ratio"])
    assert (out["status"] == 0).all()
    assert (np.diff(h, axis=1) <= 0).all(), "a sweep raised the residual"
    assert h[:, -1].max() <= 2e-4
    # the residual reported is the layer's distance at the returned parameters
    v = np.stack([F.linear_forward(tab, out["G"][b], out["betas"][b], out["trans"][b]) for b in range(len(y))])
    assert np.abs(np.sqrt(((y - v) ** 2).sum(-1)).mean(-1) - out["residual"]).max() < 1e-12


def test_zero_weight_joints_are_kept():
    """Joints 22 and 23 move no vertex: sigma_1 == 0, their (global) rotations stay what they were - the identity -, the bit is set, and
    the other joints converge.  The meshes are posed with those two global rotations at the identity, so the exact fit is in reach; a
    fit whose other joints stalled would leave the residual at the first sweep's order, so one decade below it is asked for."""
    model = SR.synthetic_model(SR.V_GOLDEN, SR.SEED)
    w = model["weights"].copy()
    w[:, 22:] = 0.0
    model["weights"] = (w / w.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    tab = F.tables(model)
    pose, betas, trans = SR.cases(6, 7)
    R = SR.rodrigues(pose.reshape(-1, 3)).reshape(6, 24, 3, 3)
    ys = []
    for b in range(6):
        G = F.global_rotations(tab, R[b])
        G[22:] = np.eye(3)
        ys.append(F.linear_forward(tab, G, betas[b], trans[b]))
    out = F.fit(tab, np.stack(ys).astype(np.float32), 12)
    assert (out["status"] == F.STATUS_DEGENERATE_JOINT).all()
    assert np.array_equal(out["G"][:, 22:], np.broadcast_to(np.eye(3), (6, 2, 3, 3)))
    assert (out["ratios"][:, :, 22:] == 0).all() and (out["ratios"][:, :, :22] > 1e-6).all()
    h = out["history"]
    print("zero-weight joints: residual after sweep 1", h[:, 0], "after 12", h[:, -1])
    assert (np.diff(h, axis=1) <= 0).all() and (h[:, -1] <= 0.1 * h[:, 0]).all()


def test_fixed_shape(v600):
    tab, (_, betas, _), y = v600
    true = betas.astype(np.float32)
    out = F.fit(tab, y[:4], 12, fit_shape=False, betas=true[:4])
    print("fit_shape=False, true betas: residual", out["history"][:, -1])
    assert np.array_equal(out["betas"], true[:4].astype(np.float64))
    assert (np.diff(out["history"], axis=1) <= 0).all() and out["history"][:, -1].max() <= 2e-4
    wrong = np.roll(true[:4], 1, axis=0)
    out = F.fit(tab, y[:4], 4, fit_shape=False, betas=wrong)
    assert np.array_equal(out["betas"], wrong.astype(np.float64)) and np.isfinite(out["residual"]).all()


def test_nonfinite_row_in_the_restatement(v600):
    tab, _, y = v600
    bad = y[:2].copy()
    bad[1, 17, 2] = np.nan
    out = F.fit(tab, bad, 2)
    assert out["status"][1] == F.STATUS_NONFINITE and np.isinf(out["residual"][1]) and out["status"][0] == 0
    assert np.array_equal(out["rotmats"][1], np.broadcast_to(np.eye(3), (24, 3, 3))) and not out["betas"][1].any() and not out["trans"][1].any()


def test_entries_are_declared_bound_and_refuse(lib):
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pmce_smpl_fit_workspace_bytes", "pmce_smpl_fit", "pmce_smpl_fit_max_verts"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not prototyped in include/pmce_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    for name, bit in (("DEGENERATE_JOINT", 1), ("SINGULAR_SHAPE", 2), ("NONFINITE", 4)):
        assert re.search(r"#define PMCE_SMPL_FIT_%s %d\b" % (name, bit), code)
        assert getattr(smpl, "STATUS_" + name) == bit == getattr(F, "STATUS_" + name)
    vmax = lib.pmce_smpl_fit_max_verts()
    assert 6890 <= vmax and 12 * vmax <= 160 * 1024          # e of SMPL's mesh fits; e never exceeds a CU's LDS
    assert lib.pmce_smpl_fit_workspace_bytes(2, 6890) >= 2 * 6890 * 12 and lib.pmce_smpl_fit_workspace_bytes(19, 137) % 16 == 0
    assert lib.pmce_smpl_fit_workspace_bytes(0, 10) == 0 and "B must be" in _lib.last_error()
    assert lib.pmce_smpl_fit_workspace_bytes(1, vmax + 1) == 0 and str(vmax) in _lib.last_error()

    par = (C.c_int * 24)(*([0] + [int(p) for p in SR.PARENTS[1:]]))
    p = C.c_void_p(16)           # never dereferenced: every call below is refused before a launch

    def fit(V=137, B=2, n=2, sweeps=3, nj=24, verts=p, idx=None, ws=p, ws_bytes=1 << 20, parents=par):
        return lib.pmce_smpl_fit(p, p, p, p, p, p, parents, nj, verts, None, None, None, idx, n, sweeps, 1, p, p, p, p, p, p, None, ws,
                                 ws_bytes, B, V, None)

    assert fit(V=vmax + 1) == -1 and "LDS" in _lib.last_error() and str(vmax) in _lib.last_error()
    assert fit(V=0) == -1 and fit(B=0, n=0) == -1
    assert fit(sweeps=0) == -1 and "n_sweeps" in _lib.last_error()
    assert fit(nj=23) == -1 and "24 joints" in _lib.last_error()
    assert fit(verts=None) == -1 and "null pointer" in _lib.last_error()
    assert fit(n=1) == -1 and "n must equal B" in _lib.last_error()
    assert fit(idx=p, n=3) == -1 and "1..B" in _lib.last_error()
    assert fit(ws_bytes=100) == -3 and "workspace" in _lib.last_error()
    assert fit(ws=C.c_void_p(8)) == -1 and "aligned" in _lib.last_error()
    bad = (C.c_int * 24)(*([0] * 5 + [7] + [0] * 18))
    assert fit(parents=bad) == -1 and "parent of joint 5" in _lib.last_error()


def test_layer_refuses_bad_arguments():
    model = SR.synthetic_model(40, 3)
    layer = smpl.SMPL({"neutral": smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights",
                                                                                   "J_regressor", "parents")))})
    with pytest.raises(_lib.PmceError, match="float32 device tensor"):
        layer.fit(np.zeros((2, 40, 3), np.float32))


def test_save_results_with_smpl_keys(tmp_path):
    rng = np.random.default_rng(0)
    outs = [{"person_id": 7 + i, "pred_cam": rng.random((n, 3)), "mesh": rng.random((n, 5, 3)), "bboxes": rng.random((n, 4)),
             "frame_ids": np.arange(n), "smpl_pose": rng.random((n, 72)), "smpl_betas": rng.random((n, 10)), "smpl_trans": rng.random((n, 3)),
             "smpl_residual": rng.random(n), "smpl_status": np.zeros(n, np.int32)} for i, n in enumerate((3, 2))]
    plain = demo.save_results(tmp_path / "a.pkl", outs)
    assert set(plain[7]) == {"pred_cam", "mesh", "bboxes", "frame_ids"}
    data = demo.save_results(tmp_path / "b.pkl", outs, smpl=True)
    with open(tmp_path / "b.pkl", "rb") as fh:
        back = pickle.load(fh)
    assert set(back) == {7, 8}
    assert set(back[8]) == {"pred_cam", "mesh", "bboxes", "frame_ids", "pose", "betas", "trans", "smpl_residual", "smpl_status"}
    assert np.array_equal(back[8]["pose"], outs[1]["smpl_pose"]) and np.array_equal(back[7]["betas"], outs[0]["smpl_betas"])
    assert np.array_equal(data[7]["trans"], outs[0]["smpl_trans"])
    with pytest.raises(KeyError):
        demo.save_results(tmp_path / "c.pkl", [{k: v for k, v in outs[0].items() if k != "smpl_pose"}], smpl=True)
    with pytest.raises(ValueError):
        demo.save_results(tmp_path / "d.pkl", outs, smpl=1)
