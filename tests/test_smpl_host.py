"""CPU-only tests of the SMPL layer's host side (pmce_amd/smpl.py: packing, model files, the C entry points' argument checks) and of
the oracle the GPU tests measure against (tests/smpl_ref.py, held to the real SMPL_Layer's results in tests/golden/smpl.npz)."""
import ctypes as C
import os.path as osp
import pickle
import re

import numpy as np
import pytest

import smpl_ref as SR
from conftest import GOLDEN, REPO
from pmce_amd import _lib, smpl


@pytest.fixture(scope="module")
def gold():
    g = np.load(osp.join(GOLDEN, "smpl.npz"))
    assert int(g["seed"]) == SR.SEED and g["verts64"].shape == (SR.B_GOLDEN, SR.V_GOLDEN, 3)
    return g


@pytest.fixture(scope="module")
def model():
    return SR.synthetic_model(SR.V_GOLDEN, SR.SEED)


def test_oracle_against_the_reference_layer(gold, model):
    pose, betas, trans = SR.cases(SR.B_GOLDEN, SR.SEED)
    v, j = SR.forward(model, pose, betas, trans, np.float64)
    dv, dj = np.abs(v - gold["verts64"]).max(), np.abs(j - gold["joints64"]).max()
    print(f"fp64 restatement: verts {dv:.2e}, joints {dj:.2e}")
    assert dv < 1e-12 and dj < 1e-12
    v, j = SR.forward(model, pose, betas, trans, np.float32)
    assert v.dtype == np.float32 and j.dtype == np.float32
    dv, dj = np.abs(v - gold["verts64"]).max(), np.abs(j - gold["joints64"]).max()
    print(f"fp32 restatement: verts {dv:.2e} (reference's own {float(gold['dev32_verts']):.2e}), joints {dj:.2e} ({float(gold['dev32_joints']):.2e})")
    assert dv <= 4 * gold["dev32_verts"] and dj <= 4 * gold["dev32_joints"]


def test_rodrigues_against_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(5)
    a = rng.normal(0, 0.6, (500, 3))             # |a| >> 1e-8: the epsilon inside the norm moves the angle by about 1e-8 rad
    a = a[np.linalg.norm(a, axis=1) > 0.05]
    got = SR.rodrigues(a, np.float64)
    assert np.abs(got - Rotation.from_rotvec(a).as_matrix()).max() < 1e-7
    for dt in (np.float64, np.float32):
        z = SR.rodrigues(np.zeros((2, 3)), dt)
        assert z.dtype == dt and np.array_equal(z, np.stack([np.eye(3, dtype=dt)] * 2))


def test_packing_round_trips(model):
    rng = np.random.default_rng(9)
    t64 = smpl.pack_tables(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor")), dtype=np.float64)
    t32 = smpl.pack_tables(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor")))
    for a, b in zip(t64, t32):
        assert b.dtype == np.float32 and b.flags.c_contiguous and np.array_equal(a.astype(np.float32), b)
    vt_t, dirs, w_t, jt, jsd = t64
    V = SR.V_GOLDEN
    assert dirs.shape == (smpl.K_PAD, 3, V) and not dirs[217:].any()
    assert np.array_equal(vt_t.T, model["v_template"]) and np.array_equal(w_t.T, model["weights"])
    assert np.array_equal(dirs[:10].transpose(2, 1, 0), model["shapedirs"]) and np.array_equal(dirs[10:217].transpose(2, 1, 0), model["posedirs"])
    betas = rng.normal(0, 1, (6, 10))
    v_shaped = model["v_template"][None] + np.einsum("vck,bk->bvc", model["shapedirs"], betas)
    want = np.einsum("jv,bvc->bjc", model["J_regressor"], v_shaped)
    # ... from the transposed directions
    v_shaped_t = vt_t[None] + np.einsum("kcv,bk->bcv", dirs[:10], betas)
    assert np.abs(np.einsum("jv,bcv->bjc", model["J_regressor"], v_shaped_t) - want).max() < 1e-12
    # ... and from the precomputed joint tables: a 10-term sum per sample
    assert np.abs(jt[None] + np.einsum("jck,bk->bjc", jsd, betas) - want).max() < 1e-12
    m = smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")))
    assert m.parents.dtype == np.int32 and m.parents[0] == -1 and list(m.parents[1:]) == list(SR.PARENTS[1:])
    assert m.n_verts == V and np.array_equal(m.faces, model["faces"])
    layer = smpl.SMPL({"neutral": m})
    assert np.array_equal(layer.root_regressor_row(), model["J_regressor"][0].astype(np.float32)) and layer.faces is m.faces
    bad = list(SR.PARENTS)
    bad[5] = 5
    with pytest.raises(_lib.PmceError):
        smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor")), bad)
    with pytest.raises(_lib.PmceError):
        smpl.pack_tables(model["v_template"], model["shapedirs"][:, :, :9], model["posedirs"], model["weights"], model["J_regressor"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a.v_template_t, a.dirs_t, a.weights_t, a.j_template, a.j_shapedirs, a.parents, a.faces),
                                                    (b.v_template_t, b.dirs_t, b.weights_t, b.j_template, b.j_shapedirs, b.parents, b.faces)))


def test_load_model(model, tmp_path):
    import scipy.sparse
    want = smpl.SMPLModel.from_arrays(*(model[k] for k in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")))
    kt = np.stack([np.array(SR.PARENTS, dtype=np.uint32), np.arange(24, dtype=np.uint32)])
    d = {"v_template": model["v_template"], "shapedirs": model["shapedirs"], "posedirs": model["posedirs"], "weights": model["weights"],
         "J_regressor": model["J_regressor"], "kintree_table": kt, "f": model["faces"]}
    stem = smpl.MODEL_FILES["female"]
    np.savez(tmp_path / (stem + ".npz"), **d)
    assert _same(smpl.load_model(str(tmp_path / (stem + ".npz"))), want)
    d["J_regressor"] = scipy.sparse.csc_matrix(model["J_regressor"])         # as the official files hold it
    with open(tmp_path / (smpl.MODEL_FILES["male"] + ".pkl"), "wb") as fh:
        pickle.dump(d, fh, protocol=2)
    assert _same(smpl.load_model(str(tmp_path / (smpl.MODEL_FILES["male"] + ".pkl"))), want)
    layer = smpl.SMPL.from_dir(str(tmp_path))
    assert sorted(layer.models) == ["female", "male"] and layer.n_verts == SR.V_GOLDEN and layer.default_gender == "female"
    # a pickle that names a class of a module that is not importable (what the official files do with chumpy)
    bad = tmp_path / "needs_module.pkl"
    bad.write_bytes(b"cpmce_no_such_module.ch\nCh\n.")
    with pytest.raises(_lib.PmceError) as e:
        smpl.load_model(str(bad))
    assert "from_arrays" in str(e.value) and "v_template" in str(e.value) and "chumpy" in str(e.value)
    with pytest.raises(_lib.PmceError):
        smpl.SMPL.from_dir(str(tmp_path / "nothing_here"))
    np.savez(tmp_path / "short.npz", v_template=model["v_template"])
    with pytest.raises(_lib.PmceError):
        smpl.load_model(str(tmp_path / "short.npz"))


def test_symbols_exported_and_prototyped():
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("pmce_smpl_workspace_bytes", "pmce_smpl_forward"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not prototyped in include/pmce_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)


def test_workspace_grows_with_the_batch():
    lib = _lib.load()
    sizes = [lib.pmce_smpl_workspace_bytes(b) for b in (1, 2, 3, 16, 17, 19, 256, 4096)]
    assert sizes[0] >= (24 * 12 + 217 + 3) * 4 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert lib.pmce_smpl_workspace_bytes(0) == 0 and "B must be" in _lib.last_error()


def test_argument_checks_run_before_any_launch():
    """The entry point validates on the host and returns before it touches the device: these calls pass made-up pointers."""
    lib = _lib.load()
    p = C.c_void_p(4096)
    par = (C.c_int * 24)(*([0] + list(SR.PARENTS[1:])))

    def call(V=137, B=2, n=2, parents=par, nj=24, pose=p, cam_R=None, cam_t=None, idx=None, ws=p, ws_bytes=1 << 20, vt=p):
        return lib.pmce_smpl_forward(vt, p, p, p, p, parents, nj, pose, p, p, cam_R, cam_t, idx, n, 1.0, None, p, p, ws, ws_bytes, B, V, None)

    assert call(V=0) == -1 and "V must be" in _lib.last_error()
    assert call(nj=23) == -1 and "24 joints" in _lib.last_error()
    bad = (C.c_int * 24)(*par)
    bad[7] = 7
    assert call(parents=bad) == -1 and "parent of joint 7" in _lib.last_error()
    bad[7] = -1
    assert call(parents=bad) == -1
    assert call(pose=None) == -1 and "null" in _lib.last_error()
    assert call(vt=None) == -1 and "null" in _lib.last_error()
    assert call(cam_R=p) == -1 and "go together" in _lib.last_error()
    assert call(n=1) == -1 and call(idx=p, n=3) == -1
    assert call(ws_bytes=16) == -3 and "workspace" in _lib.last_error()


def test_source_is_built_without_packed_fp32():
    from pmce_amd import build as B
    assert "smpl.hip" in B.SOURCES and B.FILE_FLAGS["smpl.hip"] == B.NO_PACKED_FP32
