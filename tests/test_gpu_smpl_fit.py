"""GPU tests of SMPL fitting (``smpl.SMPL.fit`` on csrc/smpl_fit.hip) against its numpy restatement (tests/smpl_fit_ref.py, held to the
design's claims in test_smpl_fit_host.py).

The yardstick is the restatement's OWN fp32 error: dev32 = the largest deviation of its float32 run from its float64 run on the same
meshes (per-vertex arithmetic in float32; the 3 x 3 sums, SVD, normal equations and Cholesky in fp64 in both, as in the kernel).  Every
compared quantity of the device result must stay within 4 x dev32 of the float64 run: the factor covers another order of the same
operations, nothing else.  Quantities: the vertices of ``forward_rotmat`` at the result, rotmats, betas, trans, residual, history.

Shapes: V = 137 (two waves and a tail; most of the 1024 lanes own no vertex) with B = 19 and B = 1; V = 1030 (six lanes own two
vertices) with B = 3; V = 6890 (SMPL's size: the LDS and workspace sizes that matter) with B = 2 and three sweeps; V = 40 (less than a
wave).  For each the restatement's smallest sigma_2 / sigma_1 is asserted to be at least 1e-3: no Procrustes step of a test is near
the degenerate rule, where a rounding could flip the branch.  (V = 40, seed 11 meets it - 0.029 -, so that shape gets the full
comparison.)

Every test prints the figures it measures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import smpl_fit_ref as F
import smpl_ref as SR
from pmce_amd import demo, smpl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_KEYS = ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "parents", "faces")
EPS32 = float(np.finfo(np.float32).eps)
QUANTITIES = ("verts", "rotmats", "betas", "trans", "residual", "history")


def make_model(model):
    return smpl.SMPLModel.from_arrays(*(model[k] for k in MODEL_KEYS))


def dev_fit(layer, y, **kw):
    """-> dict of numpy arrays, the fitted body's vertices included."""
    with torch.cuda.device(DEV):
        yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(DEV)
        kw = {k: (tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in v) if k == "init" else
                  torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        gender = kw.pop("gender", None)
        rot, pose, betas, trans, res, status, hist = layer.fit(yt, gender, return_history=True, **kw)
        verts, _ = layer.forward_rotmat(rot, betas, trans, gender)
        torch.cuda.synchronize()
    return {"rotmats": rot.cpu().numpy(), "pose": pose.cpu().numpy(), "betas": betas.cpu().numpy(), "trans": trans.cpu().numpy(),
            "residual": res.cpu().numpy(), "status": status.cpu().numpy(), "history": hist.cpu().numpy(), "verts": verts.cpu().numpy()}


def ref_fit(tab, y, n_sweeps, **kw):
    """The restatement in both precisions, with the fitted bodies' vertices -> (fp64 run, fp32 run)."""
    runs = []
    for dt in (np.float64, np.float32):
        o = F.fit(tab, y, n_sweeps, dtype=dt, **kw)
        o["verts"] = np.stack([F.linear_forward(tab, o["G"][b], o["betas"][b], o["trans"][b], dtype=dt) for b in range(len(y))])
        runs.append(o)
    return runs


def yardstick(name, got, r64, r32, quantities=QUANTITIES, factor=4.0):
    worst = 0.0
    for q in quantities:
        dev32 = float(np.abs(r32[q].astype(np.float64) - r64[q]).max())
        d = float(np.abs(got[q].astype(np.float64) - r64[q]).max())
        print(f"{name}: {q:9s} device {d:.3e}, restatement fp32 {dev32:.3e}, ratio {d / dev32 if dev32 else float('inf' if d else 0):.2f}")
        worst = max(worst, d / dev32 if dev32 else (np.inf if d else 0.0))
    for q in quantities:
        dev32 = float(np.abs(r32[q].astype(np.float64) - r64[q]).max())
        assert np.abs(got[q].astype(np.float64) - r64[q]).max() <= factor * dev32, f"{name}: {q}"
    return worst


def conditions(name, r64):
    print(f"{name}: smallest sigma_2 / sigma_1 of the restatement {r64['min_ratio']:.3e}, last residuals {r64['history'][:, -1].max():.3e}")
    assert r64["min_ratio"] >= 1e-3 and (r64["status"] == 0).all()


SHAPES = {"v137": (137, 19, 6, 11), "v1030": (1030, 3, 4, 12), "v6890": (6890, 2, 3, 13), "v40": (40, 5, 6, 11)}
_CACHE = {}


def case(name):
    """(model dict, tables, layer, (pose, betas, trans), y fp32, fp64 run, fp32 run, device run) of a shape, computed once."""
    if name not in _CACHE:
        V, B, sweeps, seed = SHAPES[name]
        model = SR.synthetic_model(V, seed)
        tab = F.tables(model)
        layer = smpl.SMPL({"neutral": make_model(model)})
        rows = SR.cases(B, seed)
        if name == "v6890":                # (the first two rows are the zero and the tiny pose: take the one near pi and a plain one)
            rows = tuple(a[[2, 5]] for a in SR.cases(6, seed))
        y = SR.forward(model, *rows)[0].astype(np.float32)
        r64, r32 = ref_fit(tab, y, sweeps)
        _CACHE[name] = (model, tab, layer, rows, y, r64, r32, dev_fit(layer, y, n_sweeps=sweeps))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_inputs(name):
    _, _, _, _, y, r64, r32, got = case(name)
    conditions(name, r64)
    assert (got["status"] == 0).all() and all(np.isfinite(got[q]).all() for q in QUANTITIES)
    yardstick(name, got, r64, r32)
    assert (np.diff(got["history"], axis=1) <= 0).all(), "a sweep raised the residual"
    assert np.array_equal(got["history"][:, -1], got["residual"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_residual_is_the_layers_distance(name):
    """`residual` against the mean distance of ``forward_rotmat(rotmats, betas, trans)`` to the input.  Both are fp32 evaluations of the
    same body: a vertex goes through a chain of at most nine rotation products and a skinning sum on either side, some 13 roundings of
    relative size eps each on coordinates of at most max |y|, independent between the two - 16 eps max |y| bounds their difference,
    and a mean of distances moves by no more than its terms."""
    _, _, _, _, y, _, _, got = case(name)
    dist = np.sqrt(((got["verts"].astype(np.float64) - y) ** 2).sum(-1)).mean(-1)
    tol = 16 * EPS32 * float(np.abs(y).max())
    print(f"{name}: residual vs forward_rotmat's distance {np.abs(dist - got['residual']).max():.3e} (allowed {tol:.3e})")
    assert np.abs(dist - got["residual"]).max() <= tol


def test_noisy_inputs():
    model, tab, layer, rows, y, _, _, _ = case("v137")
    yn = (y[:6] + np.random.default_rng(5).normal(0, 0.01, y[:6].shape)).astype(np.float32)
    r64, r32 = ref_fit(tab, yn, 6)
    conditions("noise", r64)
    got = dev_fit(layer, yn, n_sweeps=6)
    yardstick("1 cm noise", got, r64, r32)
    assert (np.diff(got["history"], axis=1) <= 0).all()


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(a[q][rows_a], b[q][rows_b]) for q in ("rotmats", "pose", "betas", "trans", "residual", "status", "history"))


def test_batch_invariance():
    _, _, layer, _, y, _, _, got = case("v137")
    for b in (0, 7, 18):
        assert same_bits(dev_fit(layer, y[b:b + 1], n_sweeps=6), got, slice(None), slice(b, b + 1)), f"row {b} alone"
    perm = np.random.default_rng(1).permutation(len(y))
    assert same_bits(dev_fit(layer, y[perm], n_sweeps=6), got, slice(None), perm), "another order"
    _, _, layer, _, y, _, _, got = case("v1030")
    assert same_bits(dev_fit(layer, y[2:3], n_sweeps=4), got, slice(None), slice(2, 3))


def test_mixed_genders():
    ma, mb = SR.synthetic_model(137, 21), SR.synthetic_model(137, 22)
    layer = smpl.SMPL({"female": make_model(ma), "male": make_model(mb)})
    rows = SR.cases(7, 21)
    gender = np.array(["f", "m", "m", "f", "m", "f", "f"])
    y = np.where((gender == "f")[:, None, None], SR.forward(ma, *rows)[0], SR.forward(mb, *rows)[0]).astype(np.float32)
    mixed = dev_fit(layer, y, n_sweeps=4, gender=list(gender))
    for g in ("f", "m"):
        idx = np.nonzero(gender == g)[0]
        assert same_bits(dev_fit(layer, y[idx], n_sweeps=4, gender=g), mixed, slice(None), idx), g
    assert (mixed["status"] == 0).all() and (np.diff(mixed["history"], axis=1) <= 0).all()


def test_warm_start_from_the_truth():
    """One sweep from the true parameters: the residual is at the restatement's fp32 floor (the yardstick on residual and history),
    and the parameters have not left the truth by more than the restatement's fp32 run does."""
    model, tab, layer, (pose, betas, trans), y, _, _, _ = case("v137")
    R = SR.rodrigues(pose.reshape(-1, 3)).reshape(len(y), 24, 3, 3).astype(np.float32)
    init = (R, betas.astype(np.float32), trans.astype(np.float32))
    r64, r32 = ref_fit(tab, y, 1, init=init)
    conditions("warm start", r64)
    got = dev_fit(layer, y, n_sweeps=1, init=init)
    print("warm start: residual device", got["residual"].max(), "restatement fp32", r32["residual"].max(), "fp64", r64["residual"].max())
    yardstick("warm start", got, r64, r32)


def test_fixed_shape_keeps_betas():
    _, tab, layer, (_, betas, _), y, _, _, _ = case("v137")
    fixed = betas.astype(np.float32)
    fixed[4] = -0.0                        # (row 4 has zero betas: a negative zero stays one)
    got = dev_fit(layer, y, n_sweeps=4, fit_shape=False, betas=fixed)
    assert got["betas"].tobytes() == fixed.tobytes()
    r64, r32 = ref_fit(tab, y, 4, fit_shape=False, betas=fixed)
    yardstick("fit_shape=False", got, r64, r32)
    assert (np.diff(got["history"], axis=1) <= 0).all()


def test_nonfinite_row():
    _, _, layer, _, y, _, _, got = case("v137")
    bad = y.copy()
    bad[3, 100, 1] = np.nan
    bad[11, 0, 0] = np.inf
    out = dev_fit(layer, bad, n_sweeps=6)
    for b in (3, 11):
        assert out["status"][b] == smpl.STATUS_NONFINITE and out["residual"][b] == np.inf and (out["history"][b] == np.inf).all()
        assert np.array_equal(out["rotmats"][b], np.broadcast_to(np.eye(3, dtype=np.float32), (24, 3, 3)))
        assert not out["betas"][b].any() and not out["trans"][b].any() and not out["pose"][b].any()
    keep = np.array([b for b in range(len(y)) if b not in (3, 11)])
    assert same_bits(out, got, keep, keep)


def test_zero_weight_joints_set_the_bit():
    model = SR.synthetic_model(137, 11)
    w = model["weights"].copy()
    w[:, 22:] = 0.0
    model["weights"] = (w / w.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    tab = F.tables(model)
    layer = smpl.SMPL({"neutral": make_model(model)})
    pose, betas, trans = SR.cases(6, 7)
    R = SR.rodrigues(pose.reshape(-1, 3)).reshape(6, 24, 3, 3)
    ys = []
    for b in range(6):
        G = F.global_rotations(tab, R[b])
        G[22:] = np.eye(3)
        ys.append(F.linear_forward(tab, G, betas[b], trans[b]))
    y = np.stack(ys).astype(np.float32)
    r64, r32 = ref_fit(tab, y, 6)
    assert (r64["status"] == F.STATUS_DEGENERATE_JOINT).all() and r64["min_ratio"] >= 1e-3
    got = dev_fit(layer, y, n_sweeps=6)
    assert (got["status"] == smpl.STATUS_DEGENERATE_JOINT).all()
    yardstick("zero-weight joints", got, r64, r32)
    G = np.stack([F.global_rotations(tab, got["rotmats"][b].astype(np.float64)) for b in range(6)])
    print("zero-weight joints: global rotations 22, 23 from the identity by", np.abs(G[:, 22:] - np.eye(3)).max())
    assert np.abs(G[:, 22:] - np.eye(3)).max() <= 16 * EPS32    # (kept exactly; the local form and its product back round)
    assert (np.diff(got["history"], axis=1) <= 0).all()


@pytest.mark.parametrize("name", ["v137", "v40"])
def test_pose_is_the_axis_angle_of_rotmats(name):
    """Matrices are compared, not axis-angles (row 2 sits near pi, where the vector's sign is arbitrary).  The rule runs in fp32 on a
    matrix that is orthogonal to a few eps: a square root, an arc tangent, a division and some ten sums, each of relative size eps and
    magnified by at most the angle (< 4) - 64 eps bounds what comes back through Rodrigues' formula."""
    _, _, _, _, _, _, _, got = case(name)
    back = SR.rodrigues(got["pose"].astype(np.float64).reshape(-1, 3)).reshape(got["rotmats"].shape)
    angle = np.linalg.norm(got["pose"].reshape(-1, 3), axis=1)
    d = np.abs(back - got["rotmats"]).max()
    print(f"{name}: Rodrigues(pose) vs rotmats {d:.3e}, largest angle {angle.max():.4f}")
    assert d <= 64 * EPS32 and angle.max() > 3.0


def test_fit_tracklets():
    _, tab, layer, _, y, _, _, got = case("v137")
    yt = torch.from_numpy(y).to(DEV)
    cuts = [(0, 8), (8, 13), (13, 19)]

    def dicts():
        return [{"mesh": yt[a:b].clone(), "person_id": 3 + i} for i, (a, b) in enumerate(cuts)]

    outs = demo.fit_tracklets(dicts(), layer, n_sweeps=6)
    torch.cuda.synchronize()
    for o, (a, b) in zip(outs, cuts):
        assert set(demo.SMPL_KEYS) <= set(o)
        assert np.array_equal(o["smpl_pose"].cpu().numpy(), got["pose"][a:b]) and np.array_equal(o["smpl_betas"].cpu().numpy(), got["betas"][a:b])
        assert np.array_equal(o["smpl_trans"].cpu().numpy(), got["trans"][a:b]) and np.array_equal(o["smpl_residual"].cpu().numpy(), got["residual"][a:b])
        assert o["smpl_status"].dtype == torch.int32 and not o["smpl_status"].any()
    by_id = demo.fit_tracklets({7: dicts()[0]}, layer, gender="neutral", n_sweeps=6)
    assert np.array_equal(by_id[7]["smpl_pose"].cpu().numpy(), got["pose"][:8])

    outs = demo.fit_tracklets(dicts(), layer, shape="tracklet", n_sweeps=6)
    torch.cuda.synchronize()
    for o, (a, b) in zip(outs, cuts):
        mean = torch.from_numpy(got["betas"][a:b]).to(DEV).mean(0)
        sb = o["smpl_betas"]
        # (a sum of b - a terms in another order: each partial sum rounds once, none exceeds (b - a) max |beta|)
        assert (sb == sb[0]).all() and float((sb[0] - mean).abs().max()) <= (b - a) * EPS32 * float(np.abs(got["betas"][a:b]).max())
        assert sb.shape == (b - a, 10) and o["smpl_pose"].shape == (b - a, 72) and torch.isfinite(o["smpl_residual"]).all()
    # the second pass is the layer's own fixed-shape fit, warm-started from the first
    sb = torch.cat([o["smpl_betas"] for o in outs])
    with torch.cuda.device(DEV):
        first = layer.fit(yt, n_sweeps=6)
        again = layer.fit(yt, n_sweeps=6, fit_shape=False, init=(first[0], first[2], first[3]), betas=sb)
        torch.cuda.synchronize()
    assert torch.equal(torch.cat([o["smpl_pose"] for o in outs]), again[1]) and torch.equal(torch.cat([o["smpl_residual"] for o in outs]), again[4])
    with pytest.raises(ValueError):
        demo.fit_tracklets(dicts(), layer, shape="video")
