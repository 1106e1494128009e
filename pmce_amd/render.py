"""The demo's mesh overlays on the GPU (csrc/render.hip): what ``demo/renderer.py`` and the loop at ``main/run_demo.py:375-446`` of the
reference draw with pyrender, as a batched HIP rasteriser - every person of every frame in a handful of launches.

    r = render.Renderer(faces, img_wh=(1920, 1080))                    # faces [F,3] from the caller (SMPL's are licensed, not here)
    out = r.render(images[F,H,W,3] uint8, verts[N,V,3], cams[N,4], frame_index[N])
    out, aux = r.render(..., return_aux=True)                          # aux: face_id, depth, status, xy_fixed

A job is one person in one frame.  DESIGN.md section 8 says which parts of the picture are pinned to the reference's program text
(projection, flip, visibility, compositing, person order, lights, material constants), which to the rules of the API it renders through
(pixel centres, top-left fill, GL_LESS, the clip volume, back-face culling) and which are this project's (the shading formula inside a
covered pixel).  There is no fallback: without the library's kernels a call raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import PmceError

MAX_DIM = 8192                      # csrc/render.hip MAX_DIM
MAX_LIGHTS = 8
SUBPIXEL = 256                      # xy_fixed units per pixel
GUARD_PX = 1 << 14
STATUS_NONFINITE = 1                # status bit: a non-finite vertex, camera or rotation - the job drew nothing
STATUS_GUARD = 2                    # status bit: a triangle was dropped at the guard band
ORDERS = ("reference", "depth")
DEMO_COLOR = (1.0, 0.6059142480254321, 0.5)          # the demo's mesh colour; applied to the image's channels in storage order
DEMO_EMISSIVE, DEMO_AMBIENT, DEMO_INTENSITY = 0.1, 0.3, 1.2   # renderer.py:94, :51, :54
_S = math.sqrt(0.5)
# unit vectors towards the two lights in the model's frame: rotation_matrix(-45 deg, x) and rotation_matrix(45 deg, y) (renderer.py:56-59)
# acting on a light that shines along its node's -z, then through the flip
DEMO_LIGHTS = ((0.0, -_S, -_S), (_S, 0.0, -_S))
DEFAULT_KEY_BYTES = 256 << 20       # the key buffer a Renderer allocates for itself: frames are chunked to fit


def vertex_face_csr(faces, n_verts: int):
    """faces int[F,3] -> (offsets int32[V+1], face_ids int32[3F]): per vertex its incident faces, ascending face index (a face that names a
    vertex twice is listed twice).  The order of a list is the order the vertex normal is summed in."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise PmceError(f"faces must be an integer array [F, 3] (got {f.dtype} {tuple(f.shape)})")
    flat = f.reshape(-1).astype(np.int64)
    if flat.size and (flat.min() < 0 or flat.max() >= n_verts):
        raise PmceError(f"faces index vertices {int(flat.min())}..{int(flat.max())}, the mesh has {n_verts}")
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_verts))]).astype(np.int32)
    return offsets, (order // 3).astype(np.int32)


def schedule_layers(frame_index, n_frames: int, draw_order=None):
    """The launch schedule of a call: job j belongs to frame ``frame_index[j]``; the jobs of a frame are drawn in the order given (or in
    the order of the permutation ``draw_order``), the l-th of them in layer l.  -> (sched int32[N]: job ids layer by layer, ascending
    frames inside a layer; layer_offsets int32[L+1])."""
    fi = np.asarray(frame_index)
    if fi.ndim != 1 or (fi.size and not np.issubdtype(fi.dtype, np.integer)):
        raise PmceError(f"frame_index must be a 1-D integer array (got {fi.dtype} {tuple(fi.shape)})")
    fi = fi.astype(np.int64)
    if fi.size and (fi.min() < 0 or fi.max() >= n_frames):
        raise PmceError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {n_frames} frames")
    n = fi.size
    order = np.arange(n) if draw_order is None else np.asarray(draw_order, dtype=np.int64)
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        raise PmceError("draw_order must be a permutation of the jobs")
    by_frame = order[np.argsort(fi[order], kind="stable")]          # frames ascending, draw order inside a frame
    f_sorted = fi[by_frame]
    start = np.concatenate([[True], f_sorted[1:] != f_sorted[:-1]]) if n else np.zeros(0, bool)
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    layer = np.arange(n) - first                                    # rank of the job inside its frame
    sched = by_frame[np.argsort(layer, kind="stable")]              # layers ascending, frames ascending inside
    n_layers = int(layer.max()) + 1 if n else 0
    offsets = np.concatenate([[0], np.cumsum(np.bincount(layer, minlength=n_layers))]).astype(np.int32)
    return sched.astype(np.int32), offsets


def axis_rotation(angle_deg, axis):
    """The rotation by ``angle_deg`` degrees about ``axis`` -> fp64 [3,3]: cos I + (1 - cos) n n^T + sin [n]x with n = axis / |axis|, the
    formula behind trimesh's ``rotation_matrix``, which the reference's renderer turns its side view with (demo/renderer.py:76-78:
    angle 270 about (0, 1, 0)).  Every entry is those three terms summed in that order.  Cast to fp32 it is a ``Renderer.render``
    ``rotation`` - which acts on the flipped mesh, as the reference's does."""
    a = np.asarray(axis, dtype=np.float64)
    if a.shape != (3,) or not np.isfinite(a).all() or not math.isfinite(float(angle_deg)):
        raise PmceError(f"axis_rotation takes a finite angle and an axis of three finite numbers (got {angle_deg!r}, {axis!r})")
    length = math.sqrt(float(a[0]) * float(a[0]) + float(a[1]) * float(a[1]) + float(a[2]) * float(a[2]))
    if length == 0.0:
        raise PmceError("axis_rotation: the axis has no direction")
    n = [float(v) / length for v in a]
    c, s = math.cos(math.radians(float(angle_deg))), math.sin(math.radians(float(angle_deg)))
    cross = ((0.0, -n[2], n[1]), (n[2], 0.0, -n[0]), (-n[1], n[0], 0.0))
    return np.array([[c * (1.0 if i == j else 0.0) + (1.0 - c) * n[i] * n[j] + s * cross[i][j] for j in range(3)] for i in range(3)],
                    dtype=np.float64)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class Renderer:
    """faces int[F,3] (the caller's), img_wh = (width, height).  color: base colour per stored channel; emissive, ambient, intensity and
    lights ([K <= 8, 3] unit vectors towards the light, model frame) default to the demo's.  The faces and the vertex -> face table are
    built here and uploaded once per device."""

    def __init__(self, faces, img_wh, color=DEMO_COLOR, emissive=DEMO_EMISSIVE, ambient=DEMO_AMBIENT, intensity=DEMO_INTENSITY,
                 lights=DEMO_LIGHTS, cull_backfaces: bool = True, n_verts=None, key_bytes: int = DEFAULT_KEY_BYTES):
        f = _host(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
            raise PmceError(f"faces must be an integer array [F >= 1, 3] (got {f.dtype} {tuple(f.shape)})")
        if f.min() < 0:
            raise PmceError("faces hold a negative vertex index")
        if len(img_wh) != 2 or int(img_wh[0]) != img_wh[0] or int(img_wh[1]) != img_wh[1]:
            raise PmceError(f"img_wh must be (width, height) in whole pixels (got {img_wh!r})")
        self.width, self.height = int(img_wh[0]), int(img_wh[1])
        if not (1 <= self.width <= MAX_DIM and 1 <= self.height <= MAX_DIM):
            raise PmceError(f"width and height must be in 1..{MAX_DIM} (got {self.width} x {self.height})")
        col = np.asarray(color, dtype=np.float64)
        lt = np.asarray(lights, dtype=np.float64).reshape(-1, 3) if np.size(lights) else np.zeros((0, 3))
        if col.shape != (3,) or np.asarray(lights).ndim not in (1, 2) or np.size(lights) % 3:
            raise PmceError("color takes three numbers, lights [K, 3]")
        if len(lt) > MAX_LIGHTS:
            raise PmceError(f"at most {MAX_LIGHTS} lights (got {len(lt)})")
        if not (np.isfinite(col).all() and np.isfinite(lt).all() and all(math.isfinite(float(v)) for v in (emissive, ambient, intensity))):
            raise PmceError("material and lights must be finite")
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        self.min_verts = int(f.max()) + 1
        self.material = np.array([*col, float(emissive), float(ambient), float(intensity)], dtype=np.float32)
        self.lights = np.ascontiguousarray(lt, dtype=np.float32)
        self.cull_backfaces = bool(cull_backfaces)
        self.key_bytes = int(key_bytes)
        self._csr = {}        # n_verts -> (offsets, face ids) on the host
        self._dev = {}        # (device, n_verts) -> (faces, offsets, face ids) on the device
        self._ws = None
        if n_verts is not None:
            self.csr(int(n_verts))

    def csr(self, n_verts: int):
        if n_verts not in self._csr:
            self._csr[n_verts] = vertex_face_csr(self.faces, n_verts)
        return self._csr[n_verts]

    def _tables(self, dev, n_verts):
        key = (str(dev), n_verts)
        if key not in self._dev:
            off, ids = self.csr(n_verts)
            self._dev[key] = tuple(torch.from_numpy(a).to(dev) for a in (self.faces, off, ids))
        return self._dev[key]

    def workspace_bytes(self, n_jobs: int, n_verts: int, chunk_frames: int = 1) -> int:
        """Bytes of workspace for ``chunk_frames`` frames per chunk (1 = the least a call accepts)."""
        from . import ops
        return ops.render_workspace_bytes(n_jobs, n_verts, self.width, self.height, chunk_frames)

    def _workspace(self, dev, n_jobs, n_verts, n_frames):
        per_frame = self.width * self.height * 8
        need = self.workspace_bytes(n_jobs, n_verts, max(1, min(n_frames, self.key_bytes // per_frame)))
        if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, device=dev, dtype=torch.uint8)
        return self._ws

    def check_args(self, images, verts, cams, frame_index=None, rotation=None, order="reference"):
        """Shapes, dtypes and ranges of a ``render`` call, without touching the GPU -> (F, N, V, frame_index on the host)."""
        if order not in ORDERS:
            raise PmceError(f"order must be one of {ORDERS} (got {order!r})")
        if getattr(images, "ndim", 0) != 4 or images.shape[-1] != 3 or str(images.dtype).split(".")[-1] != "uint8":
            raise PmceError(f"images must be uint8 [F, H, W, 3] (got {getattr(images, 'dtype', None)} {tuple(getattr(images, 'shape', ()))})")
        F, H, W = (int(s) for s in images.shape[:3])
        if (W, H) != (self.width, self.height):
            raise PmceError(f"images are {W} x {H}, the renderer was made for {self.width} x {self.height}")
        if getattr(verts, "ndim", 0) != 3 or verts.shape[-1] != 3 or not _is_float(verts):
            raise PmceError(f"verts must be floating point [N, V, 3] (got {getattr(verts, 'dtype', None)} {tuple(getattr(verts, 'shape', ()))})")
        N, V = int(verts.shape[0]), int(verts.shape[1])
        if V < self.min_verts:
            raise PmceError(f"faces index vertex {self.min_verts - 1}, verts have {V} per mesh")
        if tuple(getattr(cams, "shape", ())) != (N, 4) or not _is_float(cams):
            raise PmceError(f"cams must be floating point [N = {N}, 4] (got {getattr(cams, 'dtype', None)} {tuple(getattr(cams, 'shape', ()))})")
        if rotation is not None and (tuple(rotation.shape) not in ((3, 3), (N, 3, 3)) or not _is_float(rotation)):
            raise PmceError(f"rotation must be floating point [3, 3] or [N = {N}, 3, 3] (got {tuple(rotation.shape)})")
        if frame_index is None:
            if N != F:
                raise PmceError(f"without frame_index job i belongs to frame i: N = {N} jobs for F = {F} frames")
            fi = np.arange(N, dtype=np.int32)
        else:
            fi = _host(frame_index)
            if fi.shape != (N,) or not np.issubdtype(fi.dtype, np.integer):
                raise PmceError(f"frame_index must be an integer array [N = {N}] (got {fi.dtype} {tuple(fi.shape)})")
            if N and (fi.min() < 0 or fi.max() >= F):
                raise PmceError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {F} frames")
            fi = np.ascontiguousarray(fi, dtype=np.int32)
        return F, N, V, fi

    @torch.no_grad()
    def render(self, images, verts, cams, frame_index=None, rotation=None, order: str = "reference", inplace: bool = False,
               return_aux: bool = False, draw_order=None, workspace=None):
        """images uint8 [F,H,W,3] (device tensor; a host array is uploaded and the result returned on the host), verts [N,V,3] metres,
        cams [N,4] = (sx, sy, tx, ty), frame_index [N] (default: job i in frame i), rotation [3,3] or [N,3,3] (acts on the reference's
        flipped mesh).  The jobs of one frame are drawn in the order given (``draw_order``: a permutation of the jobs to draw them in
        instead); order "reference": each paints over the previous ones whatever the depth, "depth": the nearest wins across persons.
        -> images (a copy unless ``inplace``), and with ``return_aux`` a dict: face_id int32 [F,H,W] (-1 = nothing drawn; with several
        persons the face of the one that shows), depth fp32 [F,H,W] (inf = nothing drawn), status int32 [N], xy_fixed int32 [N,V,2].
        ``workspace``: a uint8 device tensor of at least ``workspace_bytes(N, V)`` bytes; default: the renderer's own."""
        F, N, V, fi = self.check_args(images, verts, cams, frame_index, rotation, order)
        sched, offsets = schedule_layers(fi, F, draw_order)
        on_host = not isinstance(images, torch.Tensor) or not images.is_cuda
        if on_host:
            if inplace:
                raise PmceError("inplace=True needs the images on the device")
            dev = verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.device("cuda", torch.cuda.current_device())
            img = torch.as_tensor(np.ascontiguousarray(_host(images))).to(dev)
        else:
            dev = images.device
            if inplace and not images.is_contiguous():
                raise PmceError("inplace=True needs contiguous images")
            img = images if inplace else images.clone(memory_format=torch.contiguous_format)
        f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        vt, cm = f32(verts), f32(cams)
        rot = None
        if rotation is not None:
            rot = f32(rotation)
            rot = (rot.expand(N, 3, 3) if rot.dim() == 2 else rot).contiguous()
        status = torch.empty(N, device=dev, dtype=torch.int32)
        aux = None
        if return_aux:
            aux = {"face_id": torch.full((F, self.height, self.width), -1, device=dev, dtype=torch.int32),
                   "depth": torch.full((F, self.height, self.width), float("inf"), device=dev, dtype=torch.float32),
                   "status": status, "xy_fixed": torch.empty(N, V, 2, device=dev, dtype=torch.int32)}
        if N:
            from . import ops
            faces_d, off_d, ids_d = self._tables(dev, V)
            if workspace is None:
                workspace = self._workspace(dev, N, V, F)
            elif not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
                raise PmceError("workspace must be a contiguous uint8 tensor on the device")
            ops.render_meshes(img, vt, cm, rot, faces_d, off_d, ids_d, fi, torch.from_numpy(fi).to(dev), sched,
                              torch.from_numpy(sched).to(dev), offsets, self.material, self.lights, self.cull_backfaces,
                              order == "depth", status, aux["xy_fixed"] if aux else None, aux["face_id"] if aux else None,
                              aux["depth"] if aux else None, workspace)
        out = img.cpu().numpy() if on_host else img
        return (out, aux) if return_aux else out


def _is_float(x):
    return "float" in str(getattr(x, "dtype", ""))
