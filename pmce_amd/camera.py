"""The demo's weak-perspective camera fit on the GPU (csrc/camfit.hip), batched over windows.

Replaces ``optimize_cam_param`` (reference main/run_demo.py:134-173: 300 Adam steps through autograd per window on the three
numbers of lib/models/project_net.py's ``OptimzeCamLayer``) and ``convert_crop_cam_to_orig_img`` (run_demo.py:49-67).  The
targets (``get_bbox`` / ``process_bbox`` / ``j2d_processing``) are prepared on the device by ``pmce_amd.demo.demo_targets``;
``demo.run_tracklet`` runs targets, forward and this fit for a whole tracklet.  A caller with targets of its own passes them here.

    cam, loss = fit_camera(joints3d_m, target2d)                          # W independent windows
    cam, loss = fit_camera(joints3d_m, target2d, chain=True)              # one tracklet: each window starts from the previous result
    cam, loss, orig_cam = fit_camera(..., bbox=boxes_xywh, img_wh=(1920, 1080))
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

BETAS = (0.9, 0.999)
MAX_FIT = 32
DEMO_STEPS = 300
DEMO_LRS = (0.1, 0.05, 0.001)      # run_demo.py:141,162,165
DEMO_LR_SWITCH = (100, 200)        # the rate changes AFTER the step at these loop indices (run_demo.py:160-165)
DEMO_CROP = 500                    # virtual_crop_size, run_demo.py:236
_DTYPES = {"f32": torch.float32, "f64": torch.float64}


def step_table(steps: int = DEMO_STEPS, lrs=DEMO_LRS, lr_switch=DEMO_LR_SWITCH) -> np.ndarray:
    """float64 [steps, 2]: (lr_t / (1 - beta1^t), sqrt(1 - beta2^t)) for t = 1..steps, in Python double exactly as
    torch.optim.Adam's single-tensor step computes them.  Loop index j = t - 1 runs at lrs[0] while j <= lr_switch[0], at lrs[1]
    while j <= lr_switch[1], at lrs[2] afterwards."""
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps must be >= 1 (got {steps})")
    if len(lrs) != 3 or len(lr_switch) != 2 or not lr_switch[0] <= lr_switch[1]:
        raise ValueError("lrs takes three rates and lr_switch two ascending loop indices")
    tab = np.empty((steps, 2), dtype=np.float64)
    for t in range(1, steps + 1):
        j = t - 1
        lr = float(lrs[0] if j <= lr_switch[0] else lrs[1] if j <= lr_switch[1] else lrs[2])
        tab[j, 0] = lr / (1 - BETAS[0] ** t)
        tab[j, 1] = (1 - BETAS[1] ** t) ** 0.5
    return tab


def check_seq_offsets(seq_offsets, W: int) -> np.ndarray:
    """int32 [S + 1], monotone, first 0, last W - or ValueError."""
    s = np.asarray(seq_offsets)
    if s.ndim != 1 or s.size < 2 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("seq_offsets must be a 1-D integer table of S + 1 >= 2 entries")
    if int(s[0]) != 0 or int(s[-1]) != W:
        raise ValueError(f"seq_offsets must start at 0 and end at W = {W} (got {int(s[0])} .. {int(s[-1])})")
    if np.any(np.diff(s.astype(np.int64)) < 0):
        raise ValueError("seq_offsets must be monotone")
    return np.ascontiguousarray(s, dtype=np.int32)


def resolve_chains(W: int, seq_offsets=None, chain: bool = False):
    """The sequence table of a call: ``seq_offsets`` checked, or [0, W] for ``chain=True`` (one chain over all windows: the demo),
    or None (every window on its own)."""
    if seq_offsets is not None:
        return check_seq_offsets(seq_offsets, W)
    return np.array([0, W], dtype=np.int32) if chain else None


def default_init(S: int, seed: int = 0, device="cpu") -> torch.Tensor:
    """[S, 3] uniform [0, 1) from a seeded generator of ``device``: what ``nn.Parameter(torch.rand((1, 3)))`` (project_net.py:11) draws.
    (Drawn on the device the fit runs on, so that the default costs no host-to-device copy.)"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.rand((S, 3), generator=g, device=device)


_TABLES = {}
_SEQ_TABLES = {}


def _device_seq(seq: np.ndarray, dev):
    """The sequence table on the device.  Uploaded once per distinct table: a copy from pageable host memory makes the host wait for
    the stream, which a call of fit_camera must not do in steady state."""
    key = (str(dev), seq.tobytes())
    if key not in _SEQ_TABLES:
        if len(_SEQ_TABLES) > 64:
            _SEQ_TABLES.clear()
        _SEQ_TABLES[key] = torch.from_numpy(seq).to(dev)
    return _SEQ_TABLES[key]


def _device_table(steps, lrs, lr_switch, dtype, dev):
    key = (int(steps), tuple(float(x) for x in lrs), tuple(int(x) for x in lr_switch), dtype, str(dev))
    if key not in _TABLES:
        if len(_TABLES) > 32:
            _TABLES.clear()
        _TABLES[key] = torch.from_numpy(step_table(steps, lrs, lr_switch)).to(dtype).to(dev)
    return _TABLES[key]


@torch.no_grad()
def fit_camera(joints3d, target2d, init=None, seq_offsets=None, chain: bool = False, steps: int = DEMO_STEPS, precision: str = "f32",
               scale: float = 1.0, crop_size: float = DEMO_CROP, bbox=None, img_wh=None, lrs=DEMO_LRS, lr_switch=DEMO_LR_SWITCH,
               seed: int = 0):
    """joints3d[W, n_fit, 3] (x ``scale`` = metres in the demo), target2d[W, n_target >= n_fit, >= 2] (pixels of the virtual crop; the
    first two columns and the first n_fit rows are used) -> (cam[W, 3], loss[W]) and, with ``bbox[W, 4]`` (x, y, w, h) and
    ``img_wh = (width, height)``, also orig_cam[W, 4] = (sx, sy, tx, ty).

    Chains: ``seq_offsets`` (host int table [S + 1]) makes windows seq_offsets[s] .. seq_offsets[s + 1] - 1 one chain - the first starts
    from ``init[s]``, each later one from its predecessor's camera; ``chain=True`` alone is one chain over all windows (the demo's
    tracklet); otherwise every window starts from its own ``init`` row.  ``init`` [S, 3] defaults to uniform [0, 1) drawn on the device
    from ``seed``.
    precision "f32" (default: the reference's dtype, the shorter serial chain) or "f64" (follows the reference's fp64 run to rounding);
    outputs have that dtype.  Runs on the current stream; the host does not wait for the GPU (the step table and a sequence table are
    uploaded the first time they are seen and kept)."""
    if precision not in _DTYPES:
        raise ValueError(f"precision must be 'f32' or 'f64' (got {precision!r})")
    dt = _DTYPES[precision]
    if joints3d.dim() != 3 or joints3d.shape[-1] != 3:
        raise ValueError(f"joints3d must be [W, n_fit, 3] (got {tuple(joints3d.shape)})")
    W, n_fit = int(joints3d.shape[0]), int(joints3d.shape[1])
    if not 1 <= n_fit <= MAX_FIT:
        raise ValueError(f"n_fit (rows of joints3d) must be in 1..{MAX_FIT} (got {n_fit})")
    if target2d.dim() != 3 or target2d.shape[0] != W or target2d.shape[1] < n_fit or target2d.shape[2] < 2:
        raise ValueError(f"target2d must be [W = {W}, >= {n_fit}, >= 2] (got {tuple(target2d.shape)})")
    if (bbox is None) != (img_wh is None):
        raise ValueError("bbox and img_wh go together")
    seq = resolve_chains(W, seq_offsets, chain)
    S = W if seq is None else len(seq) - 1
    if int(steps) < 1:
        raise ValueError(f"steps must be >= 1 (got {steps})")
    dev = joints3d.device
    cam = torch.empty(W, 3, device=dev, dtype=dt)
    loss = torch.empty(W, device=dev, dtype=dt)
    orig = torch.empty(W, 4, device=dev, dtype=dt) if bbox is not None else None
    if W == 0:
        return (cam, loss) if orig is None else (cam, loss, orig)
    if init is None:
        init = default_init(S, seed, dev)
    init = torch.as_tensor(init).to(device=dev, dtype=dt).contiguous()
    if tuple(init.shape) != (S, 3):
        raise ValueError(f"init must be [S = {S}, 3] (got {tuple(init.shape)})")
    j = joints3d.to(dt).contiguous()
    t = target2d[..., :2].to(dt).contiguous()
    tab = _device_table(steps, lrs, lr_switch, dt, dev)
    seq_dev = None if seq is None else _device_seq(seq, dev)
    seq_host = None if seq is None else seq.ctypes.data_as(C.POINTER(C.c_int))
    bb = None
    iw = ih = 0.0
    if bbox is not None:
        bb = torch.as_tensor(bbox).to(device=dev, dtype=dt).contiguous()
        if tuple(bb.shape) != (W, 4):
            raise ValueError(f"bbox must be [W = {W}, 4] (got {tuple(bb.shape)})")
        iw, ih = float(img_wh[0]), float(img_wh[1])
    lib = _lib.load()
    fn = lib.pmce_camfit_f32 if precision == "f32" else lib.pmce_camfit_f64
    _lib.check(fn(_lib.ptr(j), _lib.ptr(t), _lib.ptr(init), seq_host, _lib.ptr(seq_dev), _lib.ptr(tab), _lib.ptr(cam), _lib.ptr(loss),
                  _lib.ptr(bb), _lib.ptr(orig), W, S, n_fit, int(t.shape[1]), int(steps), float(scale), float(crop_size), iw, ih,
                  _lib.current_stream()), f"pmce_camfit_{precision}")
    return (cam, loss) if orig is None else (cam, loss, orig)


def fit_camera_stream(stream_outputs, target2d, **fit_kwargs):
    """Fit a whole streamed tracklet as ONE chain: ``stream_outputs`` is what ``streaming.stream_forward(..., with_joints=True)`` /
    ``stream_forward_cached(..., with_joints=True)`` returned - (cam_mesh, cam_pose, pose3d, pred_joints_mm), one row per window - and
    ``target2d`` [W, >= rows, >= 2] the windows' 2D targets.  The regressed joints are millimetres, the demo fits metres: scale = 1e-3
    unless given.  Returns what :func:`fit_camera` returns."""
    if len(stream_outputs) < 4 or stream_outputs[3] is None:
        raise _lib.PmceError("fit_camera_stream needs the outputs of stream_forward*(..., with_joints=True)")
    fit_kwargs.setdefault("scale", 1e-3)
    if fit_kwargs.get("seq_offsets") is None:
        fit_kwargs.setdefault("chain", True)
    return fit_camera(stream_outputs[3], target2d, **fit_kwargs)
