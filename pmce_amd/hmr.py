"""SPIN's regression head on the GPU (csrc/hmr_head.hip): the rest of the reference's HMR after the backbone (lib/models/spin.py:145-208,
the same head as Regressor.forward :211-293) - features [n,2048] -> SMPL pose, shape, camera, and with an SMPL layer the mesh and joints.

    model = HMR.from_checkpoint("spin_model_checkpoint.pth.tar", device, smpl=smpl_layer)      # torch.load(path)['model']
    out = model(patches)                                  # {'theta', 'rotmat', 'pred_cam', 'verts', ...}: ONE dict, see RegressorHead
    feats, out = model(patches, return_features=True)
    head = RegressorHead.from_state_dict(sd, device)      # the head alone, on features from anywhere
    head.set_joint_table(*spin_joint_table(extra_vertex_ids, J_regressor_extra, n_verts))      # -> 'kp_3d' [n,49,3], 'kp_2d' [n,49,2]
    out = head(features, smpl_layer)

In eval mode both dropouts are the identity and nothing non-linear sits between fc1, fc2 and the decoders, so the n_iter iterations are
one affine map of the initial state (``fold_regressor``, fp64 on the host, rounded to fp32 once): the device applies a 157 x 2048 matrix
instead of three rounds of fc1 and fc2.  There is no CPU fallback and no training mode.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import _lib, ops
from ._net import check_precision, clean_state_dict, take_tensors
from .extractor import FEAT_DIM, FeatureExtractor

NPOSE, NSHAPE, NCAM = 144, 10, 3
NSTATE = NPOSE + NSHAPE + NCAM          # 157: the order of fc1's columns 2048..
STATE_PAD = 160                         # a row of the transposed operands (csrc/hmr_head.hip)
HIDDEN = 1024
N_JOINTS = 24
HEAD_KEYS = OrderedDict([("fc1.weight", (HIDDEN, FEAT_DIM + NSTATE)), ("fc1.bias", (HIDDEN,)), ("fc2.weight", (HIDDEN, HIDDEN)),
                         ("fc2.bias", (HIDDEN,)), ("decpose.weight", (NPOSE, HIDDEN)), ("decpose.bias", (NPOSE,)),
                         ("decshape.weight", (NSHAPE, HIDDEN)), ("decshape.bias", (NSHAPE,)), ("deccam.weight", (NCAM, HIDDEN)),
                         ("deccam.bias", (NCAM,)), ("init_pose", (1, NPOSE)), ("init_shape", (1, NSHAPE)), ("init_cam", (1, NCAM))])

# lib/models/smpl_mps.py:14-53, restated: the 49 output joints as indices into [24 posed SMPL joints | smplx's 21 extra vertex joints |
# the 9 rows of J_regressor_extra].  Names in the reference's order: 25 OpenPose joints, then the 24 "ground-truth" joints.
JOINT_NAMES = ("OP Nose", "OP Neck", "OP RShoulder", "OP RElbow", "OP RWrist", "OP LShoulder", "OP LElbow", "OP LWrist", "OP MidHip",
               "OP RHip", "OP RKnee", "OP RAnkle", "OP LHip", "OP LKnee", "OP LAnkle", "OP REye", "OP LEye", "OP REar", "OP LEar",
               "OP LBigToe", "OP LSmallToe", "OP LHeel", "OP RBigToe", "OP RSmallToe", "OP RHeel", "Right Ankle", "Right Knee",
               "Right Hip", "Left Hip", "Left Knee", "Left Ankle", "Right Wrist", "Right Elbow", "Right Shoulder", "Left Shoulder",
               "Left Elbow", "Left Wrist", "Neck (LSP)", "Top of Head (LSP)", "Pelvis (MPII)", "Thorax (MPII)", "Spine (H36M)",
               "Jaw (H36M)", "Head (H36M)", "Nose", "Left Eye", "Right Eye", "Left Ear", "Right Ear")
JOINT_MAP = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 8, 5, 45, 46, 4, 7, 21, 19, 17,
             16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27)
N_EXTRA_VERTS, N_EXTRA_ROWS = 21, 9
assert len(JOINT_NAMES) == len(JOINT_MAP) == 49


def fold_regressor(fc1_w, fc1_b, fc2_w, fc2_b, dec_w, dec_b, n_iter=3):
    """The iterated regressor as one affine map, in fp64.  With W1 = [W1f | W1s] (2048 | 157 columns) and D, bD the stacked rows of
    decpose, decshape, deccam, one iteration is  s' = (I + Ms) s + Mf xf + c  with Mf = D W2 W1f, Ms = D W2 W1s, c = D (W2 b1 + b2) + bD,
    and n_iter of them are  s_n = P s_0 + Q xf + c_n:  P = (I + Ms)^n, Q = sum_{k<n} (I + Ms)^k Mf, c_n = sum_{k<n} (I + Ms)^k c.
    -> (Q [157,2048], P [157,157], c_n [157]) float64 numpy arrays.  n_iter: a whole number in 1..16."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 1 <= int(n_iter) <= 16:
        raise ValueError(f"n_iter must be a whole number in 1..16 (got {n_iter!r})")
    f64 = lambda a: (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64))   # noqa: E731
    W1, b1, W2, b2, D, bD = (f64(a) for a in (fc1_w, fc1_b, fc2_w, fc2_b, dec_w, dec_b))
    for name, a, shape in (("fc1_w", W1, (HIDDEN, FEAT_DIM + NSTATE)), ("fc1_b", b1, (HIDDEN,)), ("fc2_w", W2, (HIDDEN, HIDDEN)),
                           ("fc2_b", b2, (HIDDEN,)), ("dec_w", D, (NSTATE, HIDDEN)), ("dec_b", bD, (NSTATE,))):
        if a.shape != shape:
            raise ValueError(f"{name} must be {shape} (got {a.shape})")
    DW2 = D @ W2
    Mf, Ms = DW2 @ W1[:, :FEAT_DIM], DW2 @ W1[:, FEAT_DIM:]
    c = D @ (W2 @ b1 + b2) + bD
    A = np.eye(NSTATE) + Ms
    Q, cn, P = np.zeros_like(Mf), np.zeros_like(c), np.eye(NSTATE)
    for _ in range(int(n_iter)):            # Horner: X <- A X + M, so that X = sum_k A^k M
        Q, cn, P = A @ Q + Mf, A @ cn + c, A @ P
    return Q, P, cn


def select_head_state_dict(sd):
    """The head's thirteen tensors of a state dict (an optional ``module.`` prefix stripped) as fp64 CPU tensors.  A missing or
    mis-shaped tensor raises a ValueError that names it."""
    return take_tensors(clean_state_dict(sd), HEAD_KEYS, torch.float64)


def spin_joint_table(extra_vertex_ids, J_regressor_extra, n_verts=None):
    """The reference's 49 joints (lib/models/smpl_mps.py:14-53, 65-83) as a table for the device: -> (sel int32 [49], (indptr, indices,
    data)).  Output joint k has map index i = JOINT_MAP[k]: i < 24 is posed SMPL joint i (sel[k] = i); 24 <= i < 45 is the vertex
    extra_vertex_ids[i - 24] (sel[k] = -1, CSR row k = that vertex with weight 1); 45 <= i < 54 is row i - 45 of J_regressor_extra
    (sel[k] = -1, CSR row k = the row's non-zeros).
    extra_vertex_ids: the 21 vertex ids smplx's SMPL appends to its joints (nose, eyes, ears, toes, heels, finger tips: smplx's
    ``vertex_ids['smplx' / 'smpl']`` through ``VertexJointSelector``) - the caller's argument, like the licensed model files: they are
    smplx's table and are not restated here.  J_regressor_extra: [9, V].  n_verts: V, default J_regressor_extra's width."""
    ids = np.asarray(extra_vertex_ids)
    if ids.shape != (N_EXTRA_VERTS,) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"extra_vertex_ids must hold {N_EXTRA_VERTS} whole numbers (got shape {ids.shape}, {ids.dtype})")
    jr = np.asarray(J_regressor_extra, dtype=np.float64)
    if jr.ndim != 2 or jr.shape[0] != N_EXTRA_ROWS:
        raise ValueError(f"J_regressor_extra must be [{N_EXTRA_ROWS}, V] (got {jr.shape})")
    V = jr.shape[1] if n_verts is None else int(n_verts)
    if jr.shape[1] != V:
        raise ValueError(f"J_regressor_extra has {jr.shape[1]} columns, the model {V} vertices")
    if ids.min() < 0 or ids.max() >= V:
        bad = int(ids[(ids < 0) | (ids >= V)][0])
        raise ValueError(f"extra vertex id {bad} is outside [0, {V})")
    sel = np.full(len(JOINT_MAP), -1, dtype=np.int32)
    indptr, indices, data = [0], [], []
    for k, i in enumerate(JOINT_MAP):
        if i < N_JOINTS:
            sel[k] = i
        elif i < N_JOINTS + N_EXTRA_VERTS:
            indices.append(int(ids[i - N_JOINTS]))
            data.append(1.0)
        else:
            row = jr[i - N_JOINTS - N_EXTRA_VERTS]
            nz = np.nonzero(row)[0]
            indices.extend(nz.tolist())
            data.extend(row[nz].tolist())
        indptr.append(len(indices))
    return sel, (np.asarray(indptr, np.int32), np.asarray(indices, np.int32), np.asarray(data, np.float32))


def _no_train(self, mode=True):
    if mode:
        raise NotImplementedError("inference only: there is no training mode (dropout, BatchNorm statistics) on the device")
    return self


class RegressorHead:
    """The folded head on one device.  ``head(features, smpl_layer=None, gender=None, init_pose=None, init_shape=None, init_cam=None)``
    returns ONE dict of fp32 device tensors - the reference returns a list holding one such dict (spin.py:198-203, 286-292):
        'theta'    [n,85]        (camera 3, axis-angle pose 72, shape 10)
        'rotmat'   [n,24,3,3]
        'pred_cam' [n,3]         (a view of theta)
        'state'    [n,157]       (6D pose 144, shape 10, camera 3: what the iterations end on, before rot6d_to_rotmat)
        'verts'    [n,V,3]       with an SMPL layer (pmce_amd.smpl.SMPL)
        'kp_3d'    [n,49,3], 'kp_2d' [n,49,2]   with an SMPL layer and a joint table (``set_joint_table``)
    init_*: per-sample initial parameters, [n,.] or [1,.], the reference's arguments; those left None take the checkpoint's mean
    parameters.  With none given, P s_0 + c_n is one constant and only Q is applied."""

    def __init__(self, tensors, device, n_iter=3):
        t = tensors
        dec_w = torch.cat([t["decpose.weight"], t["decshape.weight"], t["deccam.weight"]], 0)
        dec_b = torch.cat([t["decpose.bias"], t["decshape.bias"], t["deccam.bias"]], 0)
        Q, P, cn = fold_regressor(t["fc1.weight"], t["fc1.bias"], t["fc2.weight"], t["fc2.bias"], dec_w, dec_b, n_iter)
        self.n_iter = int(n_iter)
        self.device = torch.device(device)
        s0 = torch.cat([t["init_pose"], t["init_shape"], t["init_cam"]], 1).double().numpy().reshape(NSTATE)
        pad = lambda a: np.ascontiguousarray(np.pad(a.T, ((0, 0), (0, STATE_PAD - NSTATE))), dtype=np.float32)    # noqa: E731
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)                # noqa: E731
        # (P - I, in fp64 before the rounding: the kernel adds the initial state itself, csrc/hmr_head.hip)
        self.q_t, self.pmi_t = up(pad(Q)), up(pad(P - np.eye(NSTATE)))
        self.c_n, self.const = up(cn), up(P @ s0 + cn)
        self.init_state = up(s0.reshape(1, NSTATE))
        self.joint_table = None

    train = _no_train

    def eval(self):
        return self

    @classmethod
    def from_state_dict(cls, sd, device="cuda", n_iter=3):
        return cls(select_head_state_dict(sd), device, n_iter)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", n_iter=3):
        """``torch.load(path)['model']``, as main/run_demo.py:250-251 reads the SPIN checkpoint."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not hasattr(ckpt, "keys") or "model" not in ckpt:
            raise ValueError(f"{path}: the checkpoint has no 'model' entry")
        return cls.from_state_dict(ckpt["model"], device, n_iter)

    def set_joint_table(self, sel, csr):
        """The joints 'kp_3d' / 'kp_2d' are made of (``spin_joint_table``'s result); uploaded once."""
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        indptr, indices, data = csr
        indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        if sel.ndim != 1 or not 1 <= sel.shape[0] <= 256 or len(indptr) != sel.shape[0] + 1 or sel.max() >= N_JOINTS:
            raise ValueError("the joint table needs sel [K], K in 1..256, with entries < 24 and a CSR matrix of K rows")
        if indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != len(indices) or len(data) != len(indices) or \
                (len(indices) and indices.min() < 0):
            raise ValueError("the joint table's CSR matrix is malformed (indptr must rise from 0 to len(indices), columns >= 0)")
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)    # noqa: E731
        # (a table without a single CSR entry still hands the kernel valid pointers)
        self.joint_table = (dev(sel, np.int32), dev(indptr, np.int32), dev(indices if len(indices) else [0], np.int32),
                            dev(data if len(data) else [0.0], np.float32), int(np.max(indices)) if len(indices) else 0)
        return self

    def _initial_states(self, n, init_pose, init_shape, init_cam):
        if init_pose is None and init_shape is None and init_cam is None:
            return None
        parts = []
        for name, a, lo, width in (("init_pose", init_pose, 0, NPOSE), ("init_shape", init_shape, NPOSE, NSHAPE),
                                   ("init_cam", init_cam, NPOSE + NSHAPE, NCAM)):
            if a is None:
                a = self.init_state[:, lo:lo + width]
            a = torch.as_tensor(a).to(device=self.device, dtype=torch.float32)
            if a.dim() != 2 or a.shape[1] != width or a.shape[0] not in (1, n):
                raise ValueError(f"{name} must be [{n}, {width}] or [1, {width}] (got {tuple(a.shape)})")
            parts.append(a.expand(n, -1))
        return torch.cat(parts, 1).contiguous()

    @torch.no_grad()
    def forward(self, features, smpl_layer=None, gender=None, init_pose=None, init_shape=None, init_cam=None):
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or \
                features.shape[1] != FEAT_DIM or features.shape[0] < 1:
            raise ValueError(f"features must be a float32 tensor [n >= 1, {FEAT_DIM}] (got {getattr(features, 'dtype', type(features).__name__)} "
                             f"{tuple(getattr(features, 'shape', ()))})")
        x = features.to(self.device).contiguous()
        n = x.shape[0]
        with torch.cuda.device(self.device):
            init = self._initial_states(n, init_pose, init_shape, init_cam)
            state = torch.empty(n, NSTATE, device=self.device, dtype=torch.float32)
            rotmat = torch.empty(n, N_JOINTS, 3, 3, device=self.device, dtype=torch.float32)
            theta = torch.empty(n, 3 + 3 * N_JOINTS + NSHAPE, device=self.device, dtype=torch.float32)
            if init is None:
                ops.hmr_head(x, self.q_t, self.const, None, None, state, rotmat, theta)
            else:
                ops.hmr_head(x, self.q_t, self.c_n, self.pmi_t, init, state, rotmat, theta)
            out = {"theta": theta, "rotmat": rotmat, "pred_cam": theta[:, :NCAM], "state": state}
            if smpl_layer is not None:
                verts, joints = smpl_layer.forward_rotmat(rotmat, state[:, NPOSE:NPOSE + NSHAPE], None, gender)
                out["verts"] = verts
                if self.joint_table is not None:
                    sel, indptr, indices, data, max_col = self.joint_table
                    if max_col >= verts.shape[1]:
                        raise _lib.PmceError(f"the joint table reads vertex {max_col}, the SMPL layer has {verts.shape[1]}")
                    K = sel.shape[0]
                    kp_3d = torch.empty(n, K, 3, device=self.device, dtype=torch.float32)
                    kp_2d = torch.empty(n, K, 2, device=self.device, dtype=torch.float32)
                    ops.hmr_joints(joints, verts, sel, indptr, indices, data, theta, theta.shape[1], kp_3d, kp_2d)
                    out["kp_3d"], out["kp_2d"] = kp_3d, kp_2d
        return out

    __call__ = forward


class HMR:
    """``FeatureExtractor`` + ``RegressorHead``: the reference's ``hmr(...)`` as a whole.  ``model(patches, init_pose=None, init_shape=None,
    init_cam=None, return_features=False, gender=None)`` follows HMR.forward (spin.py:145-208) and returns the head's dict, or
    (features, dict) with return_features - the reference returns ``[dict]``.  ``model.feature_extractor(patches)`` is the backbone alone.
    smpl: a pmce_amd.smpl.SMPL layer (the model files are the caller's), or None: then the dict has no 'verts'."""

    def __init__(self, extractor, head, smpl=None):
        self.extractor, self.head, self.smpl = extractor, head, smpl
        self.device = head.device

    train = _no_train

    def eval(self):
        return self

    @classmethod
    def from_state_dict(cls, sd, device="cuda", smpl=None, n_iter=3, **extractor_kw):
        """``extractor_kw`` go to the backbone: ``precision="split_f16"`` (default) or ``"f16"`` (extractor.py), ``max_batch``, ``check_finite``."""
        check_precision(extractor_kw.get("precision", "split_f16"))         # before any device work
        return cls(FeatureExtractor.from_state_dict(sd, device, **extractor_kw), RegressorHead.from_state_dict(sd, device, n_iter), smpl)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", smpl=None, n_iter=3, **extractor_kw):
        """``torch.load(path)['model']``, as main/run_demo.py:250-251 reads the SPIN checkpoint."""
        check_precision(extractor_kw.get("precision", "split_f16"))
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not hasattr(ckpt, "keys") or "model" not in ckpt:
            raise ValueError(f"{path}: the checkpoint has no 'model' entry")
        return cls.from_state_dict(ckpt["model"], device, smpl, n_iter, **extractor_kw)

    @property
    def precision(self):
        """The backbone's mode ("split_f16" or "f16"); the head is fp32 in both."""
        return self.extractor.precision

    def feature_extractor(self, patches):
        return self.extractor(patches)

    def forward(self, patches, init_pose=None, init_shape=None, init_cam=None, return_features=False, gender=None):
        feats = self.extractor(patches)
        out = self.head(feats, self.smpl, gender, init_pose, init_shape, init_cam)
        return (feats, out) if return_features else out

    __call__ = forward
