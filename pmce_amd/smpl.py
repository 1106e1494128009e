"""The SMPL layer on the device (csrc/smpl.hip): ground-truth meshes from the datasets' SMPL fits, batched.

Restates ``smplpytorch``'s ``SMPL_Layer.forward`` (smplpytorch/pytorch/smpl_layer.py:65-158, ``center_idx=None``) with the reference's
output transforms fused: ``mesh * 1000 - root`` of data/PW3D/dataset.py:86,240 and the world -> camera form of
data/Human36M/dataset.py:354-398.  The SMPL model files are licensed and not shipped: the caller supplies them at run time, as
``smpl_mean_vertices.npy`` is.

    smpl = SMPL.from_dir("/data/smpl")                        # basicModel_{neutral,f,m}_lbs_10_207_0_v1.0.0.pkl (or .npz)
    verts, joints = smpl.forward(pose, shape, trans, gender)  # [B, 6890, 3], [B, 24, 3] metres, on the current stream
    gt = table.gt_mesh(smpl, idx, device)                     # datasets.FrameTable: root-relative targets of frames idx
    render.Renderer(smpl.faces, (1920, 1080))

A model is given as arrays (``SMPLModel.from_arrays``), as an ``.npz`` holding the same names, or as a pickle of plain numpy / scipy
objects; the official pickles hold ``chumpy`` objects and need that package to be importable (no unpickler for them is restated here).
"""
from __future__ import annotations

import os.path as osp
import pickle

import numpy as np

from ._lib import PmceError

N_JOINTS, N_SHAPE, N_POSE = 24, 10, 207
K_PAD = 220                                  # the 217 blend rows padded to a multiple of four (csrc/smpl.hip)
# bits of ``SMPL.fit``'s status (include/pmce_hip.h, PMCE_SMPL_FIT_*)
STATUS_DEGENERATE_JOINT, STATUS_SINGULAR_SHAPE, STATUS_NONFINITE = 1, 2, 4
NPZ_NAMES = ("v_template", "shapedirs", "posedirs", "weights", "J_regressor", "kintree_table", "f")
# the reference's three files (smplpytorch/pytorch/smpl_layer.py:30-35)
MODEL_FILES = {"neutral": "basicModel_neutral_lbs_10_207_0_v1.0.0", "female": "basicModel_f_lbs_10_207_0_v1.0.0",
               "male": "basicModel_m_lbs_10_207_0_v1.0.0"}
GENDER_ALIASES = {"n": "neutral", "neutral": "neutral", "f": "female", "female": "female", "m": "male", "male": "male"}


def _dense(a, dtype=np.float64):
    if hasattr(a, "toarray"):                # scipy sparse
        a = a.toarray()
    if hasattr(a, "r") and not isinstance(a, np.ndarray):     # a chumpy object (only reachable when chumpy is importable)
        a = a.r
    return np.asarray(a, dtype=dtype)


def pack_tables(v_template, shapedirs, posedirs, weights, J_regressor, dtype=np.float32):
    """The load-time packing, on the host: (v_template_t [3,V], dirs_t [220,3,V], weights_t [24,V], j_template [24,3],
    j_shapedirs [24,3,10]).  The blend directions are transposed so that a wave's loads are contiguous; the joint regressor is applied
    to the template and to the shape directions in fp64, so that a sample's rest joints are a 10-term sum.  Everything is computed in
    fp64 and rounded once to `dtype` (float32: what the kernels read)."""
    vt, sd, pd, w, jr = (_dense(a) for a in (v_template, shapedirs, posedirs, weights, J_regressor))
    V = vt.shape[0]
    if vt.shape != (V, 3) or V < 1:
        raise PmceError(f"v_template must be [V >= 1, 3] (got {vt.shape})")
    for name, a, shape in (("shapedirs", sd, (V, 3, N_SHAPE)), ("posedirs", pd, (V, 3, N_POSE)), ("weights", w, (V, N_JOINTS)),
                           ("J_regressor", jr, (N_JOINTS, V))):
        if a.shape != shape:
            raise PmceError(f"{name} must be {shape} (got {a.shape})")
    dirs = np.zeros((K_PAD, 3, V), dtype=dtype)
    dirs[:N_SHAPE] = sd.transpose(2, 1, 0)
    dirs[N_SHAPE:N_SHAPE + N_POSE] = pd.transpose(2, 1, 0)
    c = lambda a: np.ascontiguousarray(a, dtype=dtype)    # noqa: E731
    return c(vt.T), dirs, c(w.T), c(jr @ vt), c(np.einsum("jv,vck->jck", jr, sd))


def subtree_weights(weights, parents, dtype=np.float32):
    """[24, V]: row c holds, per vertex, the sum of the skinning weights of c and of every joint below it in the tree - what the whole
    subtree of c moves a vertex by (``SMPL.fit``'s linear form).  `weights` [V,24]; `parents`: entry i > 0 in [0, i).  Summed in fp64,
    children into parents from the last joint up, rounded once to `dtype`; laid out like ``weights_t``."""
    W = _dense(weights).T.copy()
    for k in range(N_JOINTS - 1, 0, -1):
        W[int(parents[k])] += W[k]
    return np.ascontiguousarray(W, dtype=dtype)


class SMPLModel:
    """One gender's model, packed for the kernels (host arrays; ``.to(device)`` uploads them once per device)."""

    def __init__(self, tables, parents, faces, root_row, subtree_weights_t=None):
        self.v_template_t, self.dirs_t, self.weights_t, self.j_template, self.j_shapedirs = tables
        # (from the packed weights when not given: the same numbers the kernels skin with)
        self.subtree_weights_t = subtree_weights_t if subtree_weights_t is not None else subtree_weights(self.weights_t.T, parents)
        self.parents = parents
        self.faces = faces
        self._root_row = root_row
        self.n_verts = int(self.v_template_t.shape[1])
        self._dev = {}
        self._dev_subtree = {}

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, weights, J_regressor, parents, faces=None):
        """v_template [V,3], shapedirs [V,3,10], posedirs [V,3,207], weights [V,24], J_regressor [24,V] dense or scipy-sparse, parents:
        the kintree's first row (24 entries; the root's may be 2**32 - 1), faces int [F,3] or None."""
        par = np.asarray(parents).astype(np.int64).reshape(-1)
        if par.shape != (N_JOINTS,):
            raise PmceError(f"parents must hold {N_JOINTS} entries (got {par.shape})")
        for i in range(1, N_JOINTS):
            if not 0 <= par[i] < i:
                raise PmceError(f"the parent of joint {i} must be in [0, {i}) (got {par[i]})")
        par = par.copy()
        par[0] = -1
        f = None
        if faces is not None:
            f = np.asarray(faces)
            if f.ndim != 2 or f.shape[1] != 3:
                raise PmceError(f"faces must be [F, 3] (got {f.shape})")
            f = np.ascontiguousarray(f.astype(np.int32))
        root_row = _dense(J_regressor)[0].astype(np.float32)
        tables = pack_tables(v_template, shapedirs, posedirs, weights, J_regressor)
        return cls(tables, par.astype(np.int32), f, root_row, subtree_weights(tables[2].T, par))

    def to(self, device):
        """The model's tables on `device` (cached)."""
        import torch
        dev = torch.device(device)
        if dev not in self._dev:
            self._dev[dev] = tuple(torch.from_numpy(a).to(dev) for a in (self.v_template_t, self.dirs_t, self.weights_t, self.j_template,
                                                                        self.j_shapedirs))
        return self._dev[dev]

    def subtree_to(self, device):
        """``subtree_weights_t`` on `device` (cached; uploaded only for a model that ``SMPL.fit`` is called on)."""
        import torch
        dev = torch.device(device)
        if dev not in self._dev_subtree:
            self._dev_subtree[dev] = torch.from_numpy(self.subtree_weights_t).to(dev)
        return self._dev_subtree[dev]


def _from_mapping(d, where):
    missing = [k for k in NPZ_NAMES[:6] if k not in d]
    if missing:
        raise PmceError(f"{where}: no entry named {', '.join(missing)} (expected {', '.join(NPZ_NAMES)}; 'f' is optional)")
    kt = np.asarray(d["kintree_table"])
    return SMPLModel.from_arrays(d["v_template"], d["shapedirs"], d["posedirs"], d["weights"], d["J_regressor"],
                                 kt[0] if kt.ndim == 2 else kt, d["f"] if "f" in d else None)


def load_model(path: str) -> SMPLModel:
    """An ``.npz`` with the entries v_template, shapedirs, posedirs, weights, J_regressor (dense), kintree_table ([2,24] or its first row)
    and optionally f - or a ``.pkl`` that unpickles (encoding 'latin1') to a dict of plain numpy / scipy objects under the same names.
    The official SMPL pickles hold chumpy objects: they load when ``chumpy`` is importable, and raise a PmceError otherwise."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            return _from_mapping({k: z[k] for k in z.files}, path)
    try:
        with open(path, "rb") as fh:
            d = pickle.load(fh, encoding="latin1")
    except (ModuleNotFoundError, ImportError, AttributeError) as e:
        raise PmceError(f"{path}: the pickle needs a module that is not importable here ({e}); the official SMPL files hold chumpy "
                        f"objects.  Install chumpy, or supply the model as plain arrays: SMPLModel.from_arrays(...), or an .npz with the "
                        f"entries {', '.join(NPZ_NAMES)}") from e
    if not isinstance(d, dict):
        raise PmceError(f"{path}: expected a pickled dict (got {type(d).__name__})")
    return _from_mapping(d, path)


def upload_async(a, dev):
    """A host array on `dev` without stalling the host: staged in pinned memory (torch's caching host allocator keeps the block until the
    copy has run) and copied asynchronously on the current stream.  A pageable copy would make the host wait for everything already
    queued on the stream - inside a pipeline with batches in flight that serialises submission with execution."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def _gender_name(g):
    g = str(g).lower()
    if g not in GENDER_ALIASES:
        raise PmceError(f"unknown gender {g!r} (expected one of {sorted(set(GENDER_ALIASES.values()))})")
    return GENDER_ALIASES[g]


class SMPL:
    """The layer: ``models`` maps 'neutral' / 'female' / 'male' (or n / f / m) to SMPLModel objects with the same vertex count."""

    def __init__(self, models: dict):
        if not models:
            raise PmceError("SMPL needs at least one model")
        self.models = {_gender_name(k): m for k, m in models.items()}
        nv = {m.n_verts for m in self.models.values()}
        if len(nv) != 1:
            raise PmceError(f"the models have different vertex counts: {sorted(nv)}")
        self.n_verts = nv.pop()
        self.default_gender = "neutral" if "neutral" in self.models else next(iter(self.models))

    @classmethod
    def from_dir(cls, directory: str):
        """Every one of the reference's three files found under `directory`, as ``.npz`` (preferred) or ``.pkl``."""
        models = {}
        for gender, stem in MODEL_FILES.items():
            for ext in (".npz", ".pkl"):
                p = osp.join(directory, stem + ext)
                if osp.exists(p):
                    models[gender] = load_model(p)
                    break
        if not models:
            raise PmceError(f"no SMPL model under {directory}: expected " + ", ".join(s + ".pkl|.npz" for s in MODEL_FILES.values()))
        return cls(models)

    @property
    def faces(self):
        for m in self.models.values():
            if m.faces is not None:
                return m.faces
        raise PmceError("the SMPL models were given without faces")

    def root_regressor_row(self, gender=None):
        """[V] float32: the joint regressor's root row, what ``Evaluator(root_regressor_row=...)`` aligns the mesh with.  ONE row serves
        an evaluation, whatever genders its batches mix (the reference's ``self.joint_regressor_smpl`` is the neutral layer's, lib/smpl.py):
        `gender` names the model it is taken from, default the neutral one if loaded, else the first."""
        return self.models[_gender_name(gender or self.default_gender)]._root_row

    def forward(self, pose, shape, trans=None, gender=None, *, cam_R=None, cam_t=None, scale=1.0, offset=None):
        """pose [B,72] axis-angle, shape [B,10], trans [B,3] or None -> (verts [B,V,3], joints [B,24,3]) fp32 on the device, on the
        stream that is current on the inputs' device: ``(layer output + trans) * scale - offset[b]``.  Inputs are device tensors or
        numpy arrays (uploaded to the device of the first device tensor among them, else to the current device).  gender: one name, or one per sample; a mixed batch is one launch pair per gender present, each on its own rows.
        cam_R [B,3,3] + cam_t [B,3] (mm) select the world -> camera form of data/Human36M/dataset.py:354-398: root rotation
        cam_R . R_0, shape set to 0 where any |beta| > 3, translation cam_R trans + cam_t / 1000 - J_0 + cam_R J_0.  Where the reference
        divides 0 by 0 for a zero root pose (:370, NaN), the root rotation here is cam_R itself."""
        import torch
        dev = None
        for a in (pose, shape, trans, cam_R, cam_t, offset):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                dev = a.device
                break
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())

        def on_dev(a, shape_tail, name):
            if a is None:
                return None
            t = a if isinstance(a, torch.Tensor) else upload_async(np.asarray(a, dtype=np.float32), dev)
            t = t.to(device=dev, dtype=torch.float32).contiguous()
            if t.dim() < 1 or tuple(t.shape[1:]) != shape_tail:
                raise PmceError(f"{name} must be [B, {', '.join(map(str, shape_tail))}] (got {tuple(t.shape)})")
            return t

        if len(pose) < 1:
            raise PmceError("an empty batch")
        with torch.cuda.device(dev):          # allocations, uploads and the stream the kernels go to: all on the inputs' device
            return self._forward_on(dev, on_dev, pose, shape, trans, gender, cam_R, cam_t, scale, offset)

    def _gender_groups(self, gender, B, dev):
        """[(model name, int32 device index of its rows or None for all rows)]: one launch pair per gender present."""
        if gender is None or isinstance(gender, str):
            groups = [(_gender_name(gender or self.default_gender), None)]
        else:
            names = np.array([_gender_name(g) for g in np.asarray(gender).reshape(-1)])
            if names.shape[0] != B:
                raise PmceError(f"gender holds {names.shape[0]} entries, pose {B} rows")
            present = [g for g in MODEL_FILES if np.any(names == g)]
            groups = [(present[0], None)] if len(present) == 1 else [
                (g, upload_async(np.nonzero(names == g)[0].astype(np.int32), dev)) for g in present]
        for g, _ in groups:
            if g not in self.models:
                raise PmceError(f"no {g} model loaded (have: {sorted(self.models)})")
        return groups

    def _forward_on(self, dev, on_dev, pose, shape, trans, gender, cam_R, cam_t, scale, offset):
        import torch
        from . import ops
        pose = on_dev(pose.reshape(len(pose), -1) if hasattr(pose, "reshape") else pose, (72,), "pose")
        B = pose.shape[0]
        shape, trans = on_dev(shape, (N_SHAPE,), "shape"), on_dev(trans, (3,), "trans")
        cam_R, cam_t, offset = on_dev(cam_R, (3, 3), "cam_R"), on_dev(cam_t, (3,), "cam_t"), on_dev(offset, (3,), "offset")
        for name, t in (("shape", shape), ("trans", trans), ("cam_R", cam_R), ("cam_t", cam_t), ("offset", offset)):
            if t is not None and t.shape[0] != B:
                raise PmceError(f"{name} holds {t.shape[0]} rows, pose {B}")
        if (cam_R is None) != (cam_t is None):
            raise PmceError("cam_R and cam_t go together")
        groups = self._gender_groups(gender, B, dev)
        verts = torch.empty(B, self.n_verts, 3, device=dev, dtype=torch.float32)
        joints = torch.empty(B, N_JOINTS, 3, device=dev, dtype=torch.float32)
        ws = torch.empty(ops.smpl_workspace_bytes(B), device=dev, dtype=torch.uint8)
        for g, index in groups:
            ops.smpl_forward(self.models[g], pose, shape, trans, cam_R, cam_t, index, float(scale), offset, verts, joints, ws)
        return verts, joints

    def forward_rotmat(self, rotmats, shape, trans=None, gender=None, *, scale=1.0, offset=None, sample_index=None):
        """The layer on rotation matrices (smplx's ``pose2rot=False``, what SPIN's head calls: lib/models/spin.py:184-189): rotmats
        [B,24,3,3] fp32 device tensor, used as they are (pose map = R[1:] - I); shape [B,10] fp32 on the same device - a row-strided view
        such as ``state[:, 144:154]`` is read in place -; trans, gender, scale and offset as in ``forward``; there is no camera form.
        sample_index (int32 device tensor, one gender only): only these rows are computed, the others of the result are left unwritten.
        -> (verts [B,V,3], joints [B,24,3])."""
        import torch
        from . import ops
        if not isinstance(rotmats, torch.Tensor) or not rotmats.is_cuda or rotmats.dtype != torch.float32 or \
                tuple(rotmats.shape[1:]) != (N_JOINTS, 3, 3) or rotmats.shape[0] < 1:
            raise PmceError(f"rotmats must be a float32 device tensor [B >= 1, {N_JOINTS}, 3, 3] (got {getattr(rotmats, 'dtype', None)} "
                            f"{tuple(getattr(rotmats, 'shape', ()))})")
        dev, B = rotmats.device, rotmats.shape[0]
        rotmats = rotmats.contiguous()
        if not isinstance(shape, torch.Tensor) or shape.device != dev or shape.dtype != torch.float32 or tuple(shape.shape) != (B, N_SHAPE):
            raise PmceError(f"shape must be a float32 tensor [{B}, {N_SHAPE}] on {dev} (got {tuple(getattr(shape, 'shape', ()))})")
        if shape.stride(1) != 1 or shape.stride(0) < N_SHAPE:
            shape = shape.contiguous()
        with torch.cuda.device(dev):
            def on_dev(a, name):
                if a is None:
                    return None
                t = a if isinstance(a, torch.Tensor) else upload_async(np.asarray(a, dtype=np.float32), dev)
                t = t.to(device=dev, dtype=torch.float32).contiguous()
                if tuple(t.shape) != (B, 3):
                    raise PmceError(f"{name} must be [{B}, 3] (got {tuple(t.shape)})")
                return t
            trans, offset = on_dev(trans, "trans"), on_dev(offset, "offset")
            groups = self._gender_groups(gender, B, dev)
            if sample_index is not None:
                if len(groups) != 1 or sample_index.dtype != torch.int32 or sample_index.device != dev or sample_index.dim() != 1:
                    raise PmceError("sample_index must be a 1-d int32 tensor on the inputs' device, with one gender for all rows")
                groups = [(groups[0][0], sample_index.contiguous())]
            verts = torch.empty(B, self.n_verts, 3, device=dev, dtype=torch.float32)
            joints = torch.empty(B, N_JOINTS, 3, device=dev, dtype=torch.float32)
            ws = torch.empty(ops.smpl_workspace_bytes(B), device=dev, dtype=torch.uint8)
            for g, index in groups:
                ops.smpl_forward_rotmat(self.models[g], rotmats, shape, trans, index, float(scale), offset, verts, joints, ws)
        return verts, joints

    def fit(self, verts, gender=None, n_sweeps=10, fit_shape=True, init=None, betas=None, return_history=False):
        """The layer's inverse (csrc/smpl_fit.hip): verts [B,V,3] fp32 on the device, meshes of SMPL's topology in metres ->
        (rotmats [B,24,3,3] local, pose [B,72] their axis-angle form, betas [B,10], trans [B,3], residual [B], status [B] int32), and
        history [B,n_sweeps] last with return_history=True.  ``forward_rotmat(rotmats, betas, trans)`` is the fitted body, residual its
        mean vertex distance to `verts` (history: the same after every sweep), status a set of ``STATUS_*`` bits (0: nothing to report).
        One launch per gender present on the current stream, no host wait; a row's result does not depend on the batch.

        A sweep updates the 24 global rotations one after the other, each by a closed-form Procrustes step on the current residual,
        then solves shape and translation by least squares; the residual does not rise from sweep to sweep on SMPL-shaped inputs.
        n_sweeps=10 is PROVISIONAL: on the synthetic models of the tests 12 cold-start sweeps bring an exact SMPL mesh below 0.1 mm, and no
        real SMPL body has been fitted (the model files are licensed and were not at hand).
        init=(rotmats, betas, trans) warm-starts, e.g. from the previous frame; without it the start is the rest pose at the mesh's mean.
        fit_shape=False keeps the shape at what it starts as - `betas` [B,10] if given, else init's, else zeros - and fits pose and
        translation only; `betas` with fit_shape=True is the shape's starting point.  gender as in ``forward``.
        A row with a non-finite vertex returns (identity, 0, 0, 0, +inf, STATUS_NONFINITE)."""
        import torch
        from . import ops
        if not isinstance(verts, torch.Tensor) or not verts.is_cuda or verts.dtype != torch.float32 or verts.dim() != 3 or \
                verts.shape[0] < 1 or tuple(verts.shape[1:]) != (self.n_verts, 3):
            raise PmceError(f"verts must be a float32 device tensor [B >= 1, {self.n_verts}, 3] (got {getattr(verts, 'dtype', None)} "
                            f"{tuple(getattr(verts, 'shape', ()))})")
        if int(n_sweeps) < 1:
            raise PmceError(f"n_sweeps must be >= 1 (got {n_sweeps})")
        dev, B = verts.device, verts.shape[0]
        verts = verts.contiguous()

        def start(a, tail, name):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor) or a.device != dev or a.dtype != torch.float32 or tuple(a.shape) != (B,) + tail:
                raise PmceError(f"{name} must be a float32 tensor {[B, *tail]} on {dev} (got {tuple(getattr(a, 'shape', ()))})")
            return a.contiguous()

        if init is not None and len(init) != 3:
            raise PmceError("init must be (rotmats, betas, trans)")
        r0, b0, t0 = init if init is not None else (None, None, None)
        r0, b0, t0 = start(r0, (N_JOINTS, 3, 3), "init rotmats"), start(b0, (N_SHAPE,), "init betas"), start(t0, (3,), "init trans")
        if betas is not None:
            b0 = start(betas, (N_SHAPE,), "betas")
        with torch.cuda.device(dev):
            groups = self._gender_groups(gender, B, dev)
            f32 = dict(device=dev, dtype=torch.float32)
            rotmats, pose = torch.empty(B, N_JOINTS, 3, 3, **f32), torch.empty(B, 3 * N_JOINTS, **f32)
            out_betas, trans, residual = torch.empty(B, N_SHAPE, **f32), torch.empty(B, 3, **f32), torch.empty(B, **f32)
            status = torch.empty(B, device=dev, dtype=torch.int32)
            history = torch.empty(B, int(n_sweeps), **f32) if return_history else None
            ws = torch.empty(ops.smpl_fit_workspace_bytes(B, self.n_verts), device=dev, dtype=torch.uint8)
            for g, index in groups:
                ops.smpl_fit(self.models[g], verts, r0, b0, t0, index, int(n_sweeps), bool(fit_shape), rotmats, pose, out_betas, trans,
                             residual, status, history, ws)
        out = (rotmats, pose, out_betas, trans, residual, status)
        return out + (history,) if return_history else out

    __call__ = forward
