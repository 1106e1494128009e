"""The reference demo's per-person stretch (main/run_demo.py:323-367) on the GPU: a tracklet's per-frame keypoints and image features
in, what the demo saves per person out - ``pred_cam``, ``mesh``, ``bboxes`` (``frame_ids`` are the caller's).

    model.set_j_regressor(assets.load_j_regressor("coco"))
    out = demo.run_tracklet(model, keypoints[N,17,>=2], features[N,2048], img_wh=(1920, 1080))
    outs = demo.run_tracklets(model, [(kp_a, feat_a), (kp_b, feat_b)], img_wh=(1920, 1080))     # batches filled across people
    video = demo.render_tracklets(outs, frames_u8, (1920, 1080), frame_ids=ids, renderer=render.Renderer(faces, (1920, 1080)))
    outs = demo.run_video(model, frames_u8, [(kp_a[N,17,3], ids_a), (kp_b, ids_b)], extractor, img_wh=(1920, 1080))   # crops included
    tracklets = demo.pose_tracklets(frames_u8, [(boxes_a[N,4], ids_a), (boxes_b, ids_b)], pose2d.TopDownPose(vitpose_net))   # boxes -> run_video's tracklets
                                     # (vitpose_net in either precision, vitpose.ViTPose(..., precision="split_f16" | "f16"): no change here;
                                     #  likewise the extractor and the tracker's detector built with precision="f16": taken as they are)
    boxes, person_ids = demo.track_video(frames_u8, tracker.Tracker(yolo_net))                  # frames -> pose_tracklets' tracklets
    outs = demo.run_frames(model, frames_u8, tracker.Tracker(yolo_net), pose, extractor, img_wh=(1920, 1080))   # the demo up to rendering
    frames_u8, (w, h), names = demo.load_frames("video_frames/")                               # a folder of .jpg files, decoded on the device
    outs = demo.run_folder(model, "video_frames/", tracker.Tracker(yolo_net), pose, extractor)  # load_frames, then run_frames
    names = demo.save_frames("out_frames/", video)                                             # %06d.jpg, encoded on the device
    outs = demo.render_folder(model, "video_frames/", "out_frames/", trk, pose, extractor, renderer, input_folder="in_frames/")   # folder in, folders out
    outs = demo.render_folder(model, "video_frames/", "out_frames/", trk, pose, extractor, renderer, frames_per_pass=128)        # any length: 128 frames on the device at a time
    for first, frames_u8, names in demo.iter_frames("video_frames/", 128): ...                 # load_frames in steps
    wide = demo.render_tracklets(outs, frames_u8, (1920, 1080), renderer=r, plain=True, sideview=True)   # --render_plain, --sideview: [F,H,2W,3]
    outs = demo.run_frames(model, frames_u8, trk, pose, extractor, img_wh=(1920, 1080), keep_inputs=True)   # + 'track_boxes', 'keypoints'
    debug, status = demo.draw_tracklets(outs, frames_u8)                                       # the tracker's boxes and ids, the 2D skeletons
    outs = demo.render_folder(model, "video_frames/", "out_frames/", trk, pose, extractor, renderer, sideview=True, plain=True,
                              debug_folder="debug_frames/", obj_folder="out/", pkl_path="out/pmce_output.pkl")   # the demo's output switches
    demo.save_results("out/pmce_output.pkl", outs); demo.save_meshes("out/", outs, faces)      # --save_pkl, --save_obj

Per frame k the demo builds one window (``streaming.demo_window_list``), prepares the fit target from the window's middle frame
(csrc/demo_prep.hip: add_pelvis_and_neck, get_bbox, process_bbox, j2d_processing), runs the model on the window and fits the
weak-perspective camera, one ``project_net`` persisting along the tracklet (``camera.fit_camera`` chains).

The middle-frame override.  run_demo.py:343 hands ``nj2d[seq_len//2].numpy()`` - a view that shares memory with the window - to
j2d_processing, which writes the 500-px crop coordinates back in place (lib/aug_utils.py:57-59); only then is the window
screen-normalised (:344).  Frame 8 of every window therefore enters the model as the normalisation of its crop coordinates, the other
15 frames as what they are.  ``middle_frame="reference"`` (default) reproduces that, ``"clean"`` feeds every frame its plain
normalisation.  Frame reuse survives it: every frame is the middle of exactly one window of the demo's list, so a second per-frame token
table ("as middle frame") serves row 8 of every window (``streaming.precompute_mid_frames``, pmce_stream_forward_mid).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import _lib, camera, staging, streaming
from .config import FEAT_DIM, SEQLEN

BOX_SCALE = 1.25                   # process_bbox(bbox, aspect_ratio=1.0, scale=1.25), run_demo.py:342
CROP = camera.DEMO_CROP            # virtual_crop_size, run_demo.py:236
MIDDLE_FRAME = ("reference", "clean")


def demo_windows_device(lengths, device) -> torch.Tensor:
    """``streaming.demo_window_list`` of each tracklet, offset into the concatenated frame table, built ON the device (int32 [sum N, 2]):
    window k is the one frame k is the middle of.  No upload, so the host never waits for the stream."""
    h = SEQLEN // 2
    parts, off = [], 0
    for n in lengths:
        k = torch.arange(n, device=device, dtype=torch.int32)
        single = (k < h) | (k > n - h)                       # the first 8 and the last 7 frames: one frame repeated
        parts.append(torch.stack([torch.where(single, k, k - h), torch.where(single, k, k + (h - 1))], 1) + off)
        off += n
    return torch.cat(parts).contiguous()


def demo_targets(keypoints: torch.Tensor, windows, img_wh, crop_size: float = CROP, box_scale: float = BOX_SCALE,
                 joints_name=staging.COCO_JOINTS):
    """keypoints[L, J0, >=2] pixels (GPU) + windows int[W,2] (host table, or int32 tensor on the GPU) ->
    (bbox[W,4] (x, y, w, h), target2d[W,J0+2,2] crop pixels, mid_pose2d[W,J0+2,2], valid int32[W]) of every window's middle frame:
    pmce_demo_targets_f32.  ``valid`` is 0 where the reference's process_bbox returns None; that window's rows are NaN."""
    lib = _lib.load()
    kp = keypoints.to(torch.float32).contiguous()
    L, J0, D = kp.shape
    dev = kp.device
    w = windows.contiguous() if streaming._device_table(windows) else \
        torch.as_tensor(streaming.validate_windows(windows, L), device=dev).contiguous()
    W = w.shape[0]
    bbox = torch.empty(W, 4, device=dev, dtype=torch.float32)
    target = torch.empty(W, J0 + 2, 2, device=dev, dtype=torch.float32)
    mid = torch.empty(W, J0 + 2, 2, device=dev, dtype=torch.float32)
    valid = torch.empty(W, device=dev, dtype=torch.int32)
    if W == 0:
        return bbox, target, mid, valid
    idx = [joints_name.index(n) for n in ('L_Hip', 'R_Hip', 'L_Shoulder', 'R_Shoulder')]
    _lib.check(lib.pmce_demo_targets_f32(_lib.ptr(kp), D, _lib.ptr(w), _lib.ptr(bbox), _lib.ptr(target), _lib.ptr(mid), _lib.ptr(valid),
                                         W, L, J0, SEQLEN // 2, float(img_wh[0]), float(img_wh[1]), float(crop_size), float(box_scale),
                                         *idx, _lib.current_stream()), "demo_targets")
    return bbox, target, mid, valid


def override_middle(pose_windows: torch.Tensor, mid_pose2d: torch.Tensor) -> torch.Tensor:
    """In place: row SEQLEN // 2 of every assembled window pose_windows[W,16,J,2] := mid_pose2d[W,J,2] (pmce_demo_override_mid_f32)."""
    W, T, J, _ = pose_windows.shape
    if tuple(mid_pose2d.shape) != (W, J, 2) or pose_windows.dtype != torch.float32 or mid_pose2d.dtype != torch.float32:
        raise ValueError(f"override_middle: float32 [W,16,J,2] and [W,J,2] expected (got {tuple(pose_windows.shape)}, {tuple(mid_pose2d.shape)})")
    if W:
        _lib.check(_lib.load().pmce_demo_override_mid_f32(_lib.ptr(pose_windows), _lib.ptr(mid_pose2d.contiguous()), W, T, J, T // 2,
                                                          _lib.current_stream()), "demo_override_mid")
    return pose_windows


def _as_device(x, dev, what):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what} must be floating point (got {t.dtype})")
    return t.to(device=dev, dtype=torch.float32, non_blocking=True)


@torch.no_grad()
def run_tracklets(model, tracklets, img_wh, chain_across: bool = False, middle_frame: str = "reference", reuse: bool = True,
                  batch: int = 256, init=None, seed: int = 0, precision: str = "f32", check: bool = True):
    """``run_tracklet`` for several tracklets [(keypoints[N_i,17,>=2], features[N_i,2048]), ...] of one video (one ``img_wh``) at once:
    the per-frame tables are concatenated and the window tables offset, so that batches of ``batch`` windows are filled across people;
    each tracklet is its own camera chain (``init`` [S,3], default seeded uniform) - or, with ``chain_across=True``, all tracklets in
    order are ONE chain (``init`` [1,3]), which is what the reference's single persistent project_net does between persons.
    Returns one dict per tracklet (views of the shared result tensors)."""
    if middle_frame not in MIDDLE_FRAME:
        raise ValueError(f"middle_frame must be one of {MIDDLE_FRAME} (got {middle_frame!r})")
    if len(tracklets) == 0:
        return []
    if len(img_wh) != 2 or not (float(img_wh[0]) > 0 and float(img_wh[1]) > 0):
        raise ValueError(f"img_wh must be (width, height), both positive (got {img_wh!r})")
    if float(img_wh[0]) != int(img_wh[0]) or float(img_wh[1]) != int(img_wh[1]):
        raise ValueError(f"img_wh must be whole pixels (got {img_wh!r})")
    if int(batch) < 1:
        raise ValueError(f"batch must be >= 1 (got {batch})")
    if getattr(model, "_j_regressor", None) is None:
        raise _lib.PmceError("demo.run_tracklet needs a joint regressor: model.set_j_regressor(assets.load_j_regressor('coco')) first")
    J0 = model.num_joint - 2
    lengths = []
    for i, (kp, feat) in enumerate(tracklets):
        if kp.ndim != 3 or kp.shape[1] != J0 or kp.shape[2] < 2:
            raise ValueError(f"tracklet {i}: keypoints must be [N, {J0}, >= 2] for this model of {model.num_joint} joints (got {tuple(kp.shape)})")
        n = int(kp.shape[0])
        if feat.ndim != 2 or tuple(feat.shape) != (n, FEAT_DIM):
            raise ValueError(f"tracklet {i}: features must be [N = {n}, {FEAT_DIM}] (got {tuple(feat.shape)})")
        if n < SEQLEN:
            raise ValueError(f"tracklet {i}: the demo's window list needs at least {SEQLEN} frames (got {n})")
        lengths.append(n)
    eng = model._ensure_packed()
    dev = eng.device
    kps = [_as_device(kp, dev, "keypoints")[..., :2] for kp, _ in tracklets]
    feats = [_as_device(feat, dev, "features") for _, feat in tracklets]
    kp_all = (kps[0] if len(kps) == 1 else torch.cat(kps)).contiguous()
    feat_all = (feats[0] if len(feats) == 1 else torch.cat(feats)).contiguous()
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    N = int(offsets[-1])

    win = demo_windows_device(lengths, dev)                                  # window k <-> frame k
    bbox, target, mid, valid = demo_targets(kp_all, win, img_wh)
    shapes = torch.cat([torch.full((N, 1), int(img_wh[1]), device=dev, dtype=torch.int32),           # (height, width), filled on
                        torch.full((N, 1), int(img_wh[0]), device=dev, dtype=torch.int32)], 1)       # the device: no upload
    pose_fr = staging.prepare_pose2d(kp_all, shapes)
    override = middle_frame == "reference"
    if reuse:
        cache = streaming.precompute_frames(model, pose_fr, feat_all)
        if override:
            cache = streaming.precompute_mid_frames(model, cache, mid, feat_all)   # window k <-> frame k: mid is ordered by frame
        mesh, _, _, joints = streaming.stream_forward_cached(model, cache, windows=win, batch=batch, with_joints=True)
    else:
        ms, js = [], []
        for lo in range(0, N, batch):
            p, f = streaming.assemble_windows(pose_fr, feat_all, win[lo:lo + batch])
            if override:
                override_middle(p, mid[lo:lo + batch])
            o = model.forward_with_joints(p, f)
            ms.append(o[0])
            js.append(o[3])
        mesh, joints = torch.cat(ms), torch.cat(js)
    seq = np.array([0, N], dtype=np.int32) if chain_across else offsets
    cam, loss, orig = camera.fit_camera(joints, target, init=init, seq_offsets=seq, precision=precision, scale=1e-3, bbox=bbox,
                                        img_wh=img_wh, seed=seed)
    if check:
        bad = np.nonzero(valid.cpu().numpy() == 0)[0]                        # the one host wait
        if bad.size:
            t = int(np.searchsorted(offsets, bad[0], side="right") - 1)
            raise ValueError(f"tracklet {t}, frame {int(bad[0] - offsets[t])}: the keypoints span no box (the reference's process_bbox "
                             f"returns None there and the demo stops); {bad.size} such frame(s) in all - check=False keeps them as NaN")
    outs = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        outs.append({"mesh": mesh[a:b], "pred_cam": cam[a:b], "bboxes": bbox[a:b], "orig_cam": orig[a:b], "loss": loss[a:b],
                     "joints_mm": joints[a:b], "target2d": target[a:b]})
    return outs


@torch.no_grad()
def run_tracklet(model, keypoints, features, img_wh, middle_frame: str = "reference", reuse: bool = True, batch: int = 256, init=None,
                 seed: int = 0, precision: str = "f32", check: bool = True):
    """One person's tracklet: keypoints[N,17,>=2] (pixels, COCO order; further columns such as the score are ignored) and
    features[N,2048] (numpy or torch, any device) -> one row per frame:

        mesh[N,6890,3] m, pred_cam[N,3] (s, tx, ty of the 500-px crop), bboxes[N,4] (x, y, w, h), orig_cam[N,4] (sx, sy, tx, ty in the
        image), loss[N], joints_mm[N,rows,3] (the regressed joints the camera was fitted to), target2d[N,19,2] (crop pixels)

    middle_frame: "reference" reproduces the demo's overwrite of every window's middle frame (module docstring), "clean" does not.
    reuse: True serves the windows from per-frame tables (``streaming.stream_forward_cached``), False assembles every window and runs
    ``model.forward_with_joints`` on it.  The camera is one chain along the tracklet from ``init`` [1,3] (default: seeded uniform), in
    ``precision`` "f32" or "f64" (the fit only).  Fewer than 16 frames raise ValueError, a model without regressor PmceError.
    Everything is enqueued on the current stream without a host wait (with ``reuse=False`` under the model's default "rerun" overflow
    policy ``forward_with_joints`` itself waits per batch: ``model.set_overflow_policy("report")`` removes that); with ``check=True`` the
    per-window ``valid`` flags are read back once at the end, and a frame on which the reference would have stopped (process_bbox
    returning None) raises ValueError naming it.  With ``check=False`` its rows are NaN."""
    return run_tracklets(model, [(keypoints, features)], img_wh, middle_frame=middle_frame, reuse=reuse, batch=batch, init=init,
                         seed=seed, precision=precision, check=check)[0]


def tracklet_span(joints2d, vis_thresh: float = 0.3):
    """(start, end) - first usable frame and one past the last - by which the reference's CropDataset trims a tracklet before anything
    else (lib/utils/_dataset_demo.py:48-54): the two indices ``get_all_bbox_params`` returns (lib/utils/smooth_bbox.py:62-103).  A frame
    is usable when it has a keypoint with score > vis_thresh and those keypoints span at least half a pixel (:49-56); ``None`` entries
    are unusable.  joints2d: sequence of [K,3] (x, y, score).  No usable frame gives (-1, 0)."""
    if len(joints2d) == 0:
        raise ValueError("tracklet_span: empty tracklet")
    ok = np.zeros(len(joints2d), dtype=bool)
    for i, kp in enumerate(joints2d):
        if kp is None:
            continue
        kp = np.asarray(kp)
        vis = kp[:, 2] > vis_thresh
        if vis.any():
            ok[i] = np.linalg.norm(kp[vis, :2].max(0) - kp[vis, :2].min(0)) >= 0.5
    hit = np.nonzero(ok)[0]
    return (int(hit[0]), int(hit[-1]) + 1) if hit.size else (-1, 0)


@torch.no_grad()
def crop_tracklets(frames, tracklets, scale: float = 1.1, size: int = 224, channel_order: str = "rgb", vis_thresh: float = 0.3,
                   return_raw: bool = False):
    """The reference's ``CropDataset`` for every person of a video (main/run_demo.py:289-321 up to the feature extractor), on the device:
    frames uint8 [F,H,W,3], tracklets = [(keypoints[N_i,17,3] (x, y, score), frame_ids[N_i]), ...] ->

        {'patches': fp32 [sum n_i,3,size,size] (all persons, tracklet after tracklet), 'status': int32 [sum n_i], 'offsets': the
         tracklets' row ranges in them (host, int64 [T+1]), 'keypoints': [fp32 [n_i,17,3] on the device, ...], 'frame_ids': [int64
         [n_i] on the host, ...], 'spans': [(start, end), ...], 'boxes': [fp64 [n_i,4] on the device, ...][, 'raw': uint8
         [sum n_i,size,size,3]]}

    The boxes are computed per tracklet (``crops.tracklet_boxes``); every tracklet is then trimmed to its span - the reference's
    ``[time_pt1:time_pt2]``, and the one host read of this function - and ONE ``crops.crop_patches`` launch cuts all persons' patches.
    A tracklet without a usable frame keeps no row."""
    from . import crops
    crops.check_patch_args(frames, np.zeros(0, np.int32), np.zeros((0, 4)), scale, size, channel_order)
    ids = _tracklet_frame_ids(tracklets, int(frames.shape[0]))
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        frames = torch.as_tensor(np.ascontiguousarray(frames)).to(torch.device("cuda", torch.cuda.current_device()))
    res = _trim_tracklets(tracklets, ids, frames.device, vis_thresh)
    out = crops.crop_patches(frames, res.pop("frame_index"), res.pop("rows"), scale=scale, size=size, channel_order=channel_order,
                             return_raw=return_raw)
    res.update(patches=out[0], status=out[-1])
    if return_raw:
        res["raw"] = out[1]
    return res


def _tracklet_frame_ids(tracklets, F):
    """``crop_tracklets``' checks of [(keypoints[N_i,17,3], frame_ids[N_i]), ...] against a video of F frames -> the ids as int64 arrays."""
    from . import crops
    ids = []
    for i, (kp, fid) in enumerate(tracklets):
        crops.check_keypoints(kp)
        fid = np.asarray(fid.cpu() if isinstance(fid, torch.Tensor) else fid)
        if fid.shape != (len(kp),) or not np.issubdtype(fid.dtype, np.integer):
            raise ValueError(f"tracklet {i}: frame_ids must be an integer array [N = {len(kp)}] (got {fid.dtype} {fid.shape})")
        if fid.size and (fid.min() < 0 or fid.max() >= F):
            raise ValueError(f"tracklet {i}: frame_ids run {int(fid.min())}..{int(fid.max())}, there are {F} frames")
        ids.append(fid.astype(np.int64))
    return ids


def _trim_tracklets(tracklets, ids, dev, vis_thresh):
    """``crop_tracklets`` up to the cut, which needs no frame: the boxes over whole tracklets (``crops.tracklet_boxes`` interpolates over
    unusable frames wherever they lie), the spans - the one host read - and every tracklet trimmed to its span -> ``crop_tracklets``'
    dict without 'patches' and 'status', plus the cut's job table: 'frame_index' (host, int32 [sum n_i]) and 'rows' (the boxes, fp64
    [sum n_i, 4] on the device)."""
    from . import crops
    kps = [torch.as_tensor(kp).to(device=dev, dtype=torch.float32) for kp, _ in tracklets]
    results = [crops.tracklet_boxes(kp, vis_thresh) for kp in kps]
    spans = torch.stack([r[2] for r in results]).cpu().numpy() if results else np.zeros((0, 2), np.int64)     # the one host wait
    spans = [(int(a), int(b)) for a, b in spans]
    cut = [slice(max(a, 0), b) for a, b in spans]
    boxes = [r[0][c] for r, c in zip(results, cut)]
    kps = [k[c] for k, c in zip(kps, cut)]
    ids = [f[c] for f, c in zip(ids, cut)]
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in ids])]).astype(np.int64)
    fi = np.concatenate(ids).astype(np.int32) if ids else np.zeros(0, np.int32)
    bx = torch.cat(boxes) if boxes else torch.zeros(0, 4, device=dev, dtype=torch.float64)
    return {"offsets": offsets, "keypoints": kps, "frame_ids": ids, "spans": spans, "boxes": boxes, "frame_index": fi, "rows": bx}


@torch.no_grad()
def pose_tracklets(frames, tracklets, pose):
    """The reference's 2D pose stage for every person of a video (main/run_demo.py:264-286), on the device: frames uint8 [F,H,W,3],
    tracklets = [(boxes[N_i,4] as the tracker gives them - ``pose.box_format`` -, frame_ids[N_i]), ...], ``pose`` a
    ``pose2d.TopDownPose`` -> [(keypoints fp32 [N_i,K,3] = (x, y, score) on the device, frame_ids int64 [N_i] on the host), ...]: what
    ``run_video`` takes as its tracklets.  All persons go through ONE ``pose`` call (its chunks are filled across persons); there is no
    host wait here.  A job the warp refused (a box that is not finite, or empty) has the keypoints (0, 0, 0): an unusable frame to
    ``crops.tracklet_boxes``."""
    F = int(frames.shape[0]) if getattr(frames, "ndim", 0) == 4 else -1
    ids, boxes = [], []
    for i, (bx, fid) in enumerate(tracklets):
        bs = tuple(getattr(bx, "shape", ()))
        if len(bs) != 2 or bs[1] != 4 or "float" not in str(getattr(bx, "dtype", "")):
            raise ValueError(f"tracklet {i}: boxes must be floating point [N, 4] (got {getattr(bx, 'dtype', None)} {bs})")
        fid = np.asarray(fid.cpu() if isinstance(fid, torch.Tensor) else fid)
        if fid.shape != (bs[0],) or not np.issubdtype(fid.dtype, np.integer):
            raise ValueError(f"tracklet {i}: frame_ids must be an integer array [N = {bs[0]}] (got {fid.dtype} {fid.shape})")
        if F >= 0 and fid.size and (fid.min() < 0 or fid.max() >= F):
            raise ValueError(f"tracklet {i}: frame_ids run {int(fid.min())}..{int(fid.max())}, there are {F} frames")
        ids.append(fid.astype(np.int64))
        boxes.append(torch.as_tensor(bx).to(torch.float64))
    if not ids:
        return []
    if len({b.device for b in boxes}) > 1:
        raise ValueError("the tracklets' boxes must all be on one device")
    kp, _ = pose(frames, np.concatenate(ids).astype(np.int32), torch.cat(boxes))
    off = np.concatenate([[0], np.cumsum([len(f) for f in ids])])
    return [(kp[int(off[i]):int(off[i + 1])], ids[i]) for i in range(len(ids))]


@torch.no_grad()
def track_video(frames, tracker, min_frames: int = 25):
    """The reference's tracking stage (main/run_demo.py:199-215) on the device: frames uint8 [F,H,W,3], ``tracker`` a
    ``tracker.Tracker`` -> ([(boxes fp64 [N_i,4] = (cx, cy, s, s) on the device, frame_ids int64 [N_i] on the host), ...], person ids):
    ``pose_tracklets``' tracklets, without the persons seen in fewer than ``min_frames`` frames (MIN_NUM_FRAMES)."""
    return tracker(frames, min_frames=min_frames)


@torch.no_grad()
def run_frames(model, frames, tracker, pose, extractor, img_wh, min_frames: int = 25, keep_inputs: bool = False, **run_video_kwargs):
    """The whole demo up to rendering: ``track_video``, then ``pose_tracklets``, then ``run_video`` -> ``run_video``'s dicts, each with
    'person_id' (the tracker's id) added.  ``tracker``'s boxes are (cx, cy, w, h): ``pose.box_format`` must be "cxcywh".
    ``keep_inputs``: every dict also carries what the mesh stage was given, row-aligned with 'frame_ids' (trimmed by the same span):
    'track_boxes' fp64 [N_i,4], the tracker's (cx, cy, s, s), and 'keypoints' fp32 [N_i,17,3] as ``pose_tracklets`` returned them -
    ``draw_tracklets``' input."""
    if getattr(pose, "box_format", "cxcywh") != "cxcywh":
        raise ValueError(f"run_frames: the tracker's boxes are cxcywh, pose.box_format is {pose.box_format!r}")
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        frames = torch.as_tensor(np.ascontiguousarray(frames)).to(torch.device("cuda", torch.cuda.current_device()))     # one upload for all stages
    boxes, ids = track_video(frames, tracker, min_frames=min_frames)
    if keep_inputs:
        run_video_kwargs = dict(run_video_kwargs, track_boxes=[b for b, _ in boxes])
    outs = run_video(model, frames, pose_tracklets(frames, boxes, pose), extractor, img_wh, **run_video_kwargs)
    for o, pid in zip(outs, ids):
        o["person_id"] = pid
    return outs


def load_frames(folder, device=None, strict: bool = True, chunk: int = 32, entropy: str = "auto"):
    """The frames of a folder of JPEG files, as the reference's demo first sees its video (lib/utils/demo_utils.py:101-121 has ffmpeg
    write ``%06d.jpg``) -> (frames uint8 [F, H, W, 3] on the device, channels B, G, R as ``cv2.imread`` leaves them, (width, height),
    the file names in frame order).  The files ending in .jpg or .jpeg (any letter case) are taken, sorted by name as
    main/run_demo.py:386-390 sorts them, and decoded by ``jpeg.decode`` (csrc/jpeg.hip): no host decode, one upload of the files' bytes.
    A .png in the folder is a ValueError (PNG is not served), as are an empty folder, files of unequal size and every file
    ``jpeg.parse`` refuses.  ``strict``: make the one host read of the decoder's status and raise, naming the first file whose
    scan was truncated or corrupt; without it such a frame is returned as far as it decoded.  An Exif orientation tag is not read
    (``cv2.imread`` would rotate such a file; ffmpeg's frames carry none).  ``chunk``: images per round of the decoder (``jpeg.decode``; 9.4 MB of
    workspace per 1080p image).  ``entropy``: ``jpeg.decode``'s - "auto" gives files without restart markers, which is what ffmpeg
    writes, the entropy stage with many lanes per scan; "serial" and "parallel" force one stage.  The same frames either way."""
    names = _frame_names(folder)
    frames = _decode_files(folder, names, device, strict, chunk, entropy)
    return frames, (int(frames.shape[2]), int(frames.shape[1])), names


def _frame_names(folder):
    """The JPEG files of ``folder`` in frame order (sorted by name); a .png and an empty folder are ValueErrors."""
    import os
    entries = sorted(os.listdir(folder))
    png = [x for x in entries if x.lower().endswith(".png")]
    if png:
        raise ValueError(f"{os.path.join(folder, png[0])}: PNG is not served, only JPEG files (.jpg, .jpeg)")
    names = [x for x in entries if x.lower().endswith((".jpg", ".jpeg"))]
    if not names:
        raise ValueError(f"{folder}: no .jpg or .jpeg file")
    return names


def _decode_files(folder, names, device, strict, chunk, entropy):
    """Read ``names`` of ``folder`` from disk and decode them by one ``jpeg.decode`` call -> frames uint8 [n, H, W, 3]; ``strict`` as
    ``load_frames`` has it."""
    import os
    from . import jpeg
    files = []
    for x in names:
        with open(os.path.join(folder, x), "rb") as fh:
            files.append(fh.read())
    frames, status = jpeg.decode(files, device, channel_order="bgr", chunk=chunk, names=[os.path.join(folder, x) for x in names],
                                 entropy=entropy)
    if strict:
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if len(bad):
            what = " and ".join(w for bit, w in ((jpeg.STATUS_TRUNCATED, "truncated"), (jpeg.STATUS_CORRUPT, "corrupt"),
                                                (jpeg.STATUS_RECORD, "not decodable")) if st[bad[0]] & bit)
            raise ValueError(f"{os.path.join(folder, names[int(bad[0])])}: the scan is {what} (status {int(st[bad[0]])})")
    return frames


def check_frames_per_pass(frames_per_pass) -> int:
    if isinstance(frames_per_pass, bool) or not isinstance(frames_per_pass, (int, np.integer)) or int(frames_per_pass) < 1:
        raise ValueError(f"frames_per_pass must be a whole number >= 1 (got {frames_per_pass!r})")
    return int(frames_per_pass)


def iter_frames(folder, frames_per_pass, device=None, strict: bool = True, chunk: int = 32, entropy: str = "auto"):
    """``load_frames`` in steps, for a video that does not fit on the device: a generator of (first_index, frames uint8 [n, H, W, 3],
    names) over the folder's files in frame order, ``frames_per_pass`` files per step (the last step has the rest).  Per step the files
    are read from disk, uploaded and decoded, so the host holds one step's files and the device one step's frames; the caller drops a
    chunk before it asks for the next.  The folder's rules are ``load_frames``' own; all steps must have one size - a file of another
    size is a ValueError naming it.  The chunks in a row are the frames ``load_frames`` returns, to the bit."""
    import os
    from . import jpeg
    k = check_frames_per_pass(frames_per_pass)
    names = _frame_names(folder)
    shape = None
    for first in range(0, len(names), k):
        part = names[first:first + k]
        frames = _decode_files(folder, part, device, strict, chunk, entropy)
        if shape is None:
            shape = tuple(frames.shape[1:])
        elif tuple(frames.shape[1:]) != shape:
            for x in part:                                   # the error path only: parse again to name the file
                with open(os.path.join(folder, x), "rb") as fh:
                    hd = jpeg.parse(fh.read(), os.path.join(folder, x))
                if (hd.height, hd.width) != shape[:2]:
                    raise ValueError(f"{hd.name}: {hd.width} x {hd.height}, but {os.path.join(folder, names[0])} is {shape[1]} x {shape[0]}: "
                                     f"all files of one folder must have one size")
        yield first, frames, part
        del frames                       # before the next step decodes: one chunk at a time, if the caller dropped its own name too


def plan_passes(frame_index, num_frames: int, frames_per_pass: int):
    """The chunk table of a pass, on the host: frame_index int [N] (the frame of every job row, any order), a video of ``num_frames``
    frames cut every ``frames_per_pass`` -> [(first, n, rows int64 [m], relative int32 [m]), ...], one entry per chunk in frame order:
    the rows whose frame lies in first..first + n - 1, in row order, and their frame counted from ``first``.  Every row is in exactly
    one chunk."""
    k = check_frames_per_pass(frames_per_pass)
    fi = np.asarray(frame_index, dtype=np.int64).reshape(-1)
    if fi.size and (fi.min() < 0 or fi.max() >= num_frames):
        raise ValueError(f"frame_index runs {int(fi.min())}..{int(fi.max())}, there are {num_frames} frames")
    order = np.argsort(fi // k, kind="stable")
    cuts = np.searchsorted((fi // k)[order], np.arange(-(-int(num_frames) // k) + 1))
    return [(c * k, min(k, int(num_frames) - c * k), order[cuts[c]:cuts[c + 1]], (fi[order[cuts[c]:cuts[c + 1]]] - c * k).astype(np.int32))
            for c in range(len(cuts) - 1)]


def run_folder(model, folder, tracker, pose, extractor, device=None, strict: bool = True, chunk: int = 32, entropy=None,
               frames_per_pass=None, **run_frames_kwargs):
    """``load_frames`` then ``run_frames``, with ``img_wh`` taken from the files -> ``run_frames``' dicts.  ``entropy``: passed to
    ``load_frames``; None leaves it at ``load_frames``' default ("auto").  ``frames_per_pass``: serve a video of any length - only that
    many frames are on the device at a time (``run_folder_in_passes``); the same results, to the bit."""
    if frames_per_pass is not None:
        return run_folder_in_passes(model, folder, tracker, pose, extractor, frames_per_pass, device=device, strict=strict, chunk=chunk,
                                    entropy=entropy, **run_frames_kwargs)[0]
    frames, img_wh, _ = load_frames(folder, device=device, strict=strict, chunk=chunk, **({} if entropy is None else dict(entropy=entropy)))
    return run_frames(model, frames, tracker, pose, extractor, img_wh, **run_frames_kwargs)


@torch.no_grad()
def run_folder_in_passes(model, folder, tracker, pose, extractor, frames_per_pass, device=None, strict: bool = True, chunk: int = 32,
                         entropy=None, min_frames: int = 25, extract_batch: int = 256, crop_scale: float = 1.1, crop_size: int = 224,
                         channel_order: str = "rgb", vis_thresh: float = 0.3, keep_inputs: bool = False, **run_tracklets_kwargs):
    """``run_folder`` for a video of any length: two passes over ``iter_frames``, ``frames_per_pass`` frames on the device at a time ->
    (``run_frames``' dicts, img_wh, a function that starts another pass over the folder).

    Pass A, per chunk: ``tracker.stream().feed(frames, report=True)`` - the resumed SORT - and ``pose`` on the reported boxes while the
    chunk is there; the keypoints (204 B per reported row) are kept.  Then the stream's ``records(min_frames)``, the kept tracklets'
    keypoints gathered in record order, and ``crop_tracklets``' boxes and spans over WHOLE tracklets, which interpolate across chunk
    borders as they do across any frame.  Pass B, per chunk: ``crops.crop_patches`` for the tracklet rows whose frame is in the chunk
    (``plan_passes``) and ``extractor`` on them, the features scattered to their rows.  Then ``run_tracklets`` as ``run_video`` calls it.

    What stays on the device is per person and frame, not per frame: ``run_tracklets``' results (82,680 B of mesh per row), keypoints,
    features (8 KB per row) and the tracker's tables (2.5 KB per frame) - about 1/75 of a 1080p frame per person and frame.  The model
    stage itself is not chunked.  The results equal ``run_folder``'s to the bit if every stage is batch-invariant - it sees other batches
    here: ``pose`` the rows of a chunk (of every reported person, also those ``min_frames`` drops later), ``extractor`` the rows of a
    chunk.  The project's ``YOLOv3``, ``TopDownPose`` and ``FeatureExtractor`` are; a caller's torch module need not be.
    ``keep_inputs``: as ``run_frames``' - 'track_boxes' and 'keypoints' in every dict."""
    k = check_frames_per_pass(frames_per_pass)
    if getattr(pose, "box_format", "cxcywh") != "cxcywh":
        raise ValueError(f"run_frames: the tracker's boxes are cxcywh, pose.box_format is {pose.box_format!r}")
    if int(extract_batch) < 1:
        raise ValueError(f"extract_batch must be >= 1 (got {extract_batch})")
    from . import crops

    def frames_of():
        return iter_frames(folder, k, device=device, strict=strict, chunk=chunk, **({} if entropy is None else dict(entropy=entropy)))

    # pass A
    stream, kp_parts, row_of, F, img_wh, at = tracker.stream(), [], {}, 0, None, 0
    for first, frames, _ in frames_of():
        _, _, boxes, rel, pids = stream.feed(frames, report=True)
        if len(rel):
            kp_parts.append(pose(frames, rel, boxes)[0])
        for f, pid in zip(rel.tolist(), pids.tolist()):
            row_of[(first + f, pid)] = at
            at += 1
        F, img_wh = first + int(frames.shape[0]), (int(frames.shape[2]), int(frames.shape[1]))
        dev = frames.device
        del frames
    recs, ids = stream.records(min_frames)
    if not recs:
        return [], img_wh, frames_of
    kp_all = torch.cat(kp_parts)
    tracklets = []
    for (_, fid), pid in zip(recs, ids):
        rows = torch.from_numpy(np.asarray([row_of[(int(f), pid)] for f in fid], np.int64)).to(dev)
        tracklets.append((kp_all[rows], fid))
    del kp_all, kp_parts
    crops.check_patch_args(torch.zeros(0, img_wh[1], img_wh[0], 3, dtype=torch.uint8), np.zeros(0, np.int32), np.zeros((0, 4)), crop_scale,
                           crop_size, channel_order)
    c = _trim_tracklets(tracklets, _tracklet_frame_ids(tracklets, F), dev, vis_thresh)
    _refuse_short(c["offsets"])          # before pass B: no extractor work for a video that is refused
    fi, bx = c.pop("frame_index"), c.pop("rows")
    # pass B
    feats = torch.empty(len(fi), FEAT_DIM, device=dev, dtype=torch.float32)
    plan = plan_passes(fi, F, k)
    for (first, frames, _), (p_first, n, rows, rel) in zip(frames_of(), plan):
        if (first, int(frames.shape[0])) != (p_first, n):
            raise ValueError(f"{folder}: the files changed between two passes (chunk {p_first}: {frames.shape[0]} frames, {n} before)")
        if len(rows):
            rows_dev = torch.from_numpy(rows).to(dev)
            patches = crops.crop_patches(frames, rel, bx[rows_dev], scale=crop_scale, size=crop_size, channel_order=channel_order)[0]
            feats[rows_dev] = torch.cat(_extract(extractor, patches, extract_batch)).to(torch.float32)
        del frames
    outs = _lift_tracklets(model, c, feats, img_wh, run_tracklets_kwargs, [b for b, _ in recs] if keep_inputs else None)
    for o, pid in zip(outs, ids):
        o["person_id"] = pid
    return outs, img_wh, frames_of


def save_frames(folder, frames, first: int = 0, names=None, **encode_kwargs):
    """Write frames uint8 [F, H, W, 3] (device, B, G, R as every stage here holds them) into ``folder`` as JPEG files, encoded on the
    device by ``jpeg.encode`` (csrc/jpeg_encode.hip): what main/run_demo.py:424-426 does with ``cv2.imwrite`` per frame.  The files are
    named ``%06d.jpg`` counting from ``first``, as the reference names them, or by ``names`` (one per frame).  ``encode_kwargs`` go to
    ``jpeg.encode`` (quality 95, 4:2:0 and no restart markers by default: ``cv2.imwrite``'s).  Only the files' bytes cross to the host.
    A frame that did not fit ``capacity`` raises ``jpeg.files``' ValueError before anything is written.  -> the file names."""
    import os
    from . import jpeg
    F = int(frames.shape[0])
    names = [f"{int(first) + i:06d}.jpg" for i in range(F)] if names is None else [str(x) for x in names]
    if len(names) != F:
        raise ValueError(f"save_frames: {F} frames but {len(names)} names")
    blobs = jpeg.files(*jpeg.encode(frames, **encode_kwargs))
    os.makedirs(folder, exist_ok=True)
    for name, blob in zip(names, blobs):
        with open(os.path.join(folder, name), "wb") as fh:
            fh.write(blob)
    return names


def render_folder(model, folder, out_folder, tracker, pose, extractor, renderer, input_folder=None, device=None, strict: bool = True,
                  chunk: int = 32, entropy=None, order: str = "reference", encode_kwargs=None, frames_per_pass=None, sideview: bool = False,
                  plain: bool = False, debug_folder=None, obj_folder=None, pkl_path=None, overlay_kwargs=None, **run_frames_kwargs):
    """Folder in, folder out: ``load_frames``, ``run_frames``, ``render_tracklets`` and ``save_frames`` - the frames are decoded, drawn on
    and encoded on the device.  The overlaid frames go to ``out_folder``; ``input_folder``, if given, receives the input frames again, as
    main/run_demo.py:424-426 writes both folders for ffmpeg.  Both are named ``%06d.jpg`` from 0.  ``renderer``: a ``render.Renderer``
    or the mesh's face array; ``encode_kwargs``: a dict for ``jpeg.encode``.  -> ``run_frames``' dicts.  ``frames_per_pass``: as
    ``run_folder``'s, with a third pass over the folder that draws and writes chunk by chunk; the same files, to the byte.

    The reference's output switches: ``sideview`` (--sideview: the written frames are 2W wide, ``render_tracklets``' side view on the
    right) and ``plain`` (--render_plain: the meshes on black; ``input_folder`` still gets the untouched frames); ``obj_folder``
    (--save_obj, ``save_meshes``: needs ``renderer``'s faces) and ``pkl_path`` (--save_pkl, ``save_results``).  ``debug_folder`` (what
    --display is for): ``draw_tracklets`` on the input frames - the tracker's boxes and ids, the 2D skeletons - named ``%06d.jpg``; it
    turns ``keep_inputs`` on, so the dicts carry 'track_boxes' and 'keypoints'; ``overlay_kwargs``: a dict for ``overlay.draw``.  The
    three picture folders must differ: their files have the same names."""
    import os
    from . import render as R
    sideview, plain = _flag(sideview, "sideview"), _flag(plain, "plain")
    named = [(n, os.path.abspath(os.fspath(f))) for n, f in (("out_folder", out_folder), ("input_folder", input_folder),
                                                              ("debug_folder", debug_folder)) if f is not None]
    for i, (n, f) in enumerate(named):
        for m, g in named[:i]:
            if f == g:
                raise ValueError(f"{n} and {m} are the same folder ({f}): both write %06d.jpg files, one would replace the other's")
    if overlay_kwargs is not None and debug_folder is None:
        raise ValueError("overlay_kwargs are for the debug frames: give debug_folder= too")
    if obj_folder is not None and renderer is None:
        raise ValueError("obj_folder needs the mesh's faces: give renderer= (a render.Renderer, or the face array)")
    views = {k: v for k, v in (("plain", plain), ("sideview", sideview)) if v}           # without the switches: the call it was
    if debug_folder is not None:
        run_frames_kwargs = dict(run_frames_kwargs, keep_inputs=True)
    okw, kw = dict(overlay_kwargs or {}), dict(encode_kwargs or {})
    faces = None if obj_folder is None else (renderer.faces if isinstance(renderer, R.Renderer) else R._host(renderer))
    if frames_per_pass is not None:
        outs, img_wh, frames_of = run_folder_in_passes(model, folder, tracker, pose, extractor, frames_per_pass, device=device,
                                                       strict=strict, chunk=chunk, entropy=entropy, **run_frames_kwargs)
        if renderer is not None and not isinstance(renderer, R.Renderer):
            renderer = R.Renderer(renderer, img_wh)          # once, not per chunk
        keys = ("mesh", "orig_cam", "bboxes") + (("track_boxes", "keypoints") if debug_folder is not None else ())
        extras = debug_folder is not None or obj_folder is not None      # the debug frames and the .obj files name person and frame
        # pass C: the rows of a tracklet are in frame order, so a chunk's rows are one slice of each
        for first, frames, _ in frames_of():
            if input_folder is not None:
                save_frames(input_folder, frames, first=first, **kw)         # before the chunk is drawn on
            part, ids = [], []
            for o in outs:
                a, b = np.searchsorted(o["frame_ids"], [first, first + int(frames.shape[0])])
                part.append({k: o[k][a:b] for k in keys})
                if extras:
                    part[-1].update(person_id=o["person_id"], frame_ids=o["frame_ids"][a:b])
                ids.append(o["frame_ids"][a:b] - first)
            if debug_folder is not None:                                     # on a copy, before the meshes are drawn in place
                save_frames(debug_folder, draw_tracklets(part, frames, frame_ids=ids, **okw)[0], first=first, **kw)
            if obj_folder is not None:
                save_meshes(obj_folder, part, faces)
            if sum(len(i) for i in ids) or renderer is None:         # (no renderer: render_tracklets' own error)
                frames = render_tracklets(part, frames, img_wh, frame_ids=ids, renderer=renderer, order=order,
                                          **(dict(views) if sideview else dict(views, inplace=True)))
            elif views:
                frames = _empty_views(frames, plain, sideview)
            save_frames(out_folder, frames, first=first, **kw)
            del frames
        if pkl_path is not None:
            save_results(pkl_path, outs)
        return outs
    frames, img_wh, _ = load_frames(folder, device=device, strict=strict, chunk=chunk, **({} if entropy is None else dict(entropy=entropy)))
    outs = run_frames(model, frames, tracker, pose, extractor, img_wh, **run_frames_kwargs)
    rendered = render_tracklets(outs, frames, img_wh, renderer=renderer, order=order, **views)
    save_frames(out_folder, rendered, **kw)
    del rendered
    if input_folder is not None:
        save_frames(input_folder, frames, **kw)
    if debug_folder is not None:
        save_frames(debug_folder, draw_tracklets(outs, frames, **okw)[0], **kw)
    if obj_folder is not None:
        save_meshes(obj_folder, outs, faces)
    if pkl_path is not None:
        save_results(pkl_path, outs)
    return outs


def _flag(v, name):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False (got {v!r})")
    return bool(v)


def _empty_views(frames, plain, sideview):
    """What ``render_tracklets(plain=, sideview=)`` returns for frames without a person."""
    zeros = torch.zeros_like(frames) if isinstance(frames, torch.Tensor) else np.zeros_like(frames)
    left = zeros if plain else frames
    if not sideview:
        return left
    return torch.cat([left, zeros], 2) if isinstance(frames, torch.Tensor) else np.concatenate([left, zeros], 2)


def _person_ids(results):
    """-> (keys, person ids) of ``run_frames``' list, or of a dict by person id."""
    keys = list(results.keys()) if isinstance(results, dict) else list(range(len(results)))
    return keys, [int(results[k].get("person_id", k)) for k in keys]


SMPL_KEYS = ("smpl_pose", "smpl_betas", "smpl_trans", "smpl_residual", "smpl_status")


@torch.no_grad()
def fit_tracklets(outs, layer, gender=None, shape: str = "frame", n_sweeps: int = 10):
    """SMPL parameters for the meshes of ``run_frames``' dicts (a list, or a dict by person id; 'mesh' [N_i,V,3] device tensors in metres,
    V the vertex count of `layer`, a ``smpl.SMPL``): adds 'smpl_pose' [N_i,72] axis-angle, 'smpl_betas' [N_i,10], 'smpl_trans' [N_i,3],
    'smpl_residual' [N_i] (mean vertex distance of the fitted body to the mesh, metres) and 'smpl_status' [N_i] (``smpl.STATUS_*`` bits)
    to every dict, from ONE ``layer.fit`` call over all rows of all tracklets.  gender: one name for all rows, or one per tracklet.
    shape='frame': every row has its own betas.  shape='tracklet': a person has one body - the rows are fitted free, each tracklet's
    betas are averaged on the device, and the rows are fitted again with the shape fixed at that mean, warm-started from the first
    pass; 'smpl_betas' then repeats the mean.  -> outs."""
    if shape not in ("frame", "tracklet"):
        raise ValueError(f"shape must be 'frame' or 'tracklet' (got {shape!r})")
    keys = list(outs.keys()) if isinstance(outs, dict) else list(range(len(outs)))
    if not keys:
        return outs
    meshes = [outs[k]["mesh"] for k in keys]
    for k, m in zip(keys, meshes):
        if not isinstance(m, torch.Tensor) or not m.is_cuda:
            raise ValueError(f"tracklet {k!r}: 'mesh' must be a device tensor")
    lengths = [int(m.shape[0]) for m in meshes]
    verts = torch.cat([m.to(torch.float32) for m in meshes], 0)
    if gender is not None and not isinstance(gender, str):
        if len(gender) != len(keys):
            raise ValueError(f"gender holds {len(gender)} entries for {len(keys)} tracklets")
        gender = [g for g, n in zip(gender, lengths) for _ in range(n)]
    if verts.shape[0] == 0:
        fitted = None
    else:
        rotmats, pose, betas, trans, residual, status = layer.fit(verts, gender, n_sweeps=n_sweeps)
        if shape == "tracklet":
            owner = torch.repeat_interleave(torch.arange(len(keys), device=verts.device),
                                            torch.tensor(lengths, device=verts.device), output_size=verts.shape[0])
            mean = torch.zeros(len(keys), betas.shape[1], device=verts.device, dtype=torch.float32).index_add_(0, owner, betas)
            mean = mean / torch.tensor(lengths, device=verts.device, dtype=torch.float32).clamp(min=1)[:, None]
            first = status
            rotmats, pose, betas, trans, residual, status = layer.fit(verts, gender, n_sweeps=n_sweeps, fit_shape=False,
                                                                      init=(rotmats, betas, trans), betas=mean[owner].contiguous())
            status = status | first
        fitted = (pose, betas, trans, residual, status)
    a = 0
    for k, n in zip(keys, lengths):
        for name, t in zip(SMPL_KEYS, fitted if fitted is not None else [None] * len(SMPL_KEYS)):
            outs[k][name] = t[a:a + n] if t is not None else torch.empty(0)
        a += n
    return outs


def save_results(pkl_path, outs, smpl: bool = False):
    """--save_pkl (main/run_demo.py:360-373): ``run_frames``' dicts (a list, or a dict by person id) -> a pickle of {person_id:
    {'pred_cam' [N,3], 'mesh' [N,6890,3], 'bboxes' [N,4], 'frame_ids' [N]}} as numpy arrays - the reference's keys.  Written with the
    standard ``pickle`` module; the reference writes with joblib, and reading this file with ``joblib.load`` has not been checked.
    smpl=True (not in the reference; the dicts have been through ``fit_tracklets``) adds 'pose' [N,72], 'betas' [N,10], 'trans' [N,3],
    'smpl_residual' [N] and 'smpl_status' [N].  -> the dict written."""
    import os
    import pickle
    keys, pids = _person_ids(outs)
    if len(set(pids)) != len(pids):
        raise ValueError(f"save_results: person ids repeat ({pids})")
    names = {name: name for name in ("pred_cam", "mesh", "bboxes", "frame_ids")}
    if _flag(smpl, "smpl"):
        names.update({"smpl_pose": "pose", "smpl_betas": "betas", "smpl_trans": "trans", "smpl_residual": "smpl_residual",
                      "smpl_status": "smpl_status"})
    data = {}
    for k, pid in zip(keys, pids):
        o = outs[k]
        data[pid] = {out: np.asarray(o[name].detach().cpu().numpy() if isinstance(o[name], torch.Tensor) else o[name])
                     for name, out in names.items()}
    folder = os.path.dirname(os.path.abspath(os.fspath(pkl_path)))
    os.makedirs(folder, exist_ok=True)
    with open(pkl_path, "wb") as fh:
        pickle.dump(data, fh, protocol=pickle.HIGHEST_PROTOCOL)
    return data


def save_meshes(obj_folder, outs, faces):
    """--save_obj (main/run_demo.py:407-411): per person and frame ``obj_folder/meshes/{person_id:04d}/{frame:06d}.obj``.  The
    reference exports inside its renderer after the flip by Rx(180 deg) and before the side view's rotation (demo/renderer.py:65-74),
    so the vertices written are (x, -y, -z) of 'mesh'.  The file is ``v x y z`` lines with %.8f, then ``f a b c`` lines, 1-based - this
    project's layout (trimesh, the reference's exporter, is not at hand: its text will differ in formatting).  The one place where the
    meshes cross to the host.  -> the files' paths."""
    import os
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be an integer array [F, 3] (got {f.dtype} {f.shape})")
    tail = "".join(f"f {a} {b} {c}\n" for a, b, c in (f.astype(np.int64) + 1).tolist())
    keys, pids = _person_ids(outs)
    paths = []
    for k, pid in zip(keys, pids):
        o = outs[k]
        mesh = o["mesh"].detach().cpu().numpy() if isinstance(o["mesh"], torch.Tensor) else np.asarray(o["mesh"])
        fid = o["frame_ids"] if "frame_ids" in o else np.arange(len(mesh))
        if len(fid) != len(mesh):
            raise ValueError(f"person {pid}: {len(fid)} frame ids for {len(mesh)} rows")
        if f.size and f.max() >= mesh.shape[1]:
            raise ValueError(f"faces index vertex {int(f.max())}, the meshes have {mesh.shape[1]}")
        folder = os.path.join(obj_folder, "meshes", f"{pid:04d}")
        if len(fid):
            os.makedirs(folder, exist_ok=True)
        flipped = mesh.astype(np.float64) * np.array([1.0, -1.0, -1.0])
        for verts, frame in zip(flipped, fid):
            paths.append(os.path.join(folder, f"{int(frame):06d}.obj"))
            with open(paths[-1], "w") as fh:
                fh.write("".join("v %.8f %.8f %.8f\n" % tuple(v) for v in verts.tolist()) + tail)
    return paths


@torch.no_grad()
def draw_tracklets(results, frames, frame_ids=None, inplace: bool = False, **overlay_kwargs):
    """The debug view of ``run_frames(keep_inputs=True)``' dicts (a list, or a dict by person id): per row the tracker's box
    ('track_boxes'), the person's id ('person_id') and the 2D keypoints ('keypoints') drawn on frames uint8 [F,H,W,3] (device) by ONE
    ``overlay.draw`` call over the concatenated rows.  frame_ids: as ``render_tracklets``'.  The persons of a frame are drawn in
    ``tracklet_draw_order``'s order - the boxes' top edges are read back once for it, as ``render_tracklets`` does.
    -> (the frames - a copy unless ``inplace`` -, status int32 [sum N_i] in the rows' own order: ``overlay.STATUS_*``)."""
    from . import overlay
    keys, pids = _person_ids(results)
    for k in keys:
        if "track_boxes" not in results[k] or "keypoints" not in results[k]:
            raise ValueError(f"draw_tracklets: tracklet {k!r} has no 'track_boxes' / 'keypoints': run the demo with keep_inputs=True")
    if not keys or not sum(len(results[k]["keypoints"]) for k in keys):
        return (frames if inplace else frames.clone()), torch.zeros(0, dtype=torch.int32, device=frames.device)
    ids = []
    for k in keys:
        d = results[k]
        fid = frame_ids[k] if frame_ids is not None else d.get("frame_ids", np.arange(len(d["keypoints"])))
        if len(fid) != len(d["keypoints"]) or len(fid) != len(d["track_boxes"]):
            raise ValueError(f"tracklet {k!r}: {len(fid)} frame ids for {len(d['keypoints'])} keypoint rows, {len(d['track_boxes'])} boxes")
        ids.append(np.asarray(fid.cpu() if isinstance(fid, torch.Tensor) else fid))
    dev = frames.device
    cat = lambda name: torch.cat([torch.as_tensor(results[k][name]).to(dev) for k in keys])  # noqa: E731
    tops = cat("bboxes")[:, 1].cpu().numpy()
    frame_index, order = tracklet_draw_order([tops], ids)
    person = np.concatenate([np.full(len(f), pid, np.int64) for f, pid in zip(ids, pids)])
    order_dev = torch.from_numpy(order).to(dev)
    out, st = overlay.draw(frames, frame_index[order], boxes=cat("track_boxes")[order_dev], ids=person[order],
                           keypoints=cat("keypoints")[order_dev], inplace=inplace, **{"box_format": "cxcywh", **overlay_kwargs})
    status = torch.empty_like(st)
    status[order_dev] = st
    return out, status


@torch.no_grad()
def run_video(model, frames, tracklets, extractor, img_wh, extract_batch: int = 256, crop_scale: float = 1.1, crop_size: int = 224,
              channel_order: str = "rgb", vis_thresh: float = 0.3, track_boxes=None, **run_tracklets_kwargs):
    """Frames to what the demo saves: ``crop_tracklets``, then ``extractor(patches[k:k + extract_batch])`` -> [n, 2048] (the caller's
    callable on device tensors: the reference's is a torch ResNet, main/run_demo.py:248-259,314-321), then ``run_tracklets`` on the
    trimmed keypoints and those features.  -> ``run_tracklets``' dicts, each with 'frame_ids' (host, int64: the frames its rows belong
    to) added, ready for ``render_tracklets``.  A tracklet shorter than 16 frames after trimming raises ``run_tracklets``' ValueError.
    ``track_boxes``: per tracklet the tracker's boxes [N_i,4] (``run_frames``' ``keep_inputs``) - the dicts then also carry them and
    the keypoints, both trimmed as the rows are."""
    if int(extract_batch) < 1:
        raise ValueError(f"extract_batch must be >= 1 (got {extract_batch})")
    if len(tracklets) == 0:
        return []
    c = crop_tracklets(frames, tracklets, scale=crop_scale, size=crop_size, channel_order=channel_order, vis_thresh=vis_thresh)
    _refuse_short(c["offsets"])          # before the extractor runs
    return _lift_tracklets(model, c, torch.cat(_extract(extractor, c["patches"], extract_batch)), img_wh, run_tracklets_kwargs, track_boxes)


def _refuse_short(off):
    """``run_tracklets``' own error for a tracklet shorter than a window after trimming, from the row ranges alone."""
    short = [i for i in range(len(off) - 1) if off[i + 1] - off[i] < SEQLEN]
    if short:
        raise ValueError(f"tracklet {short[0]}: the demo's window list needs at least {SEQLEN} frames (got {int(off[short[0] + 1] - off[short[0]])})")


def _extract(extractor, patches, extract_batch):
    """``extractor`` on batches of ``extract_batch`` patches -> the list of its results, each checked to be [n, 2048]."""
    feats = []
    for k in range(0, patches.shape[0], int(extract_batch)):
        f = extractor(patches[k:k + int(extract_batch)])
        if f.ndim != 2 or f.shape[0] != min(int(extract_batch), patches.shape[0] - k) or f.shape[1] != FEAT_DIM:
            raise ValueError(f"the extractor must return [n, {FEAT_DIM}] (got {tuple(f.shape)})")
        feats.append(f)
    return feats


def _lift_tracklets(model, c, feats, img_wh, run_tracklets_kwargs, track_boxes=None):
    """``run_tracklets`` on the trimmed keypoints of ``c`` (``crop_tracklets``' dict) and features [sum n_i, 2048], 'frame_ids' added -
    and, with the tracker's untrimmed ``track_boxes`` per tracklet, 'track_boxes' (trimmed by the tracklet's span) and 'keypoints'."""
    if track_boxes is not None and len(track_boxes) != len(c["keypoints"]):
        raise ValueError(f"track_boxes: {len(track_boxes)} entries for {len(c['keypoints'])} tracklets")
    off = c["offsets"]
    outs = run_tracklets(model, [(c["keypoints"][i], feats[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)], img_wh,
                         **run_tracklets_kwargs)
    for o, fid in zip(outs, c["frame_ids"]):
        o["frame_ids"] = fid
    if track_boxes is not None:
        for o, bx, kp, (a, b) in zip(outs, track_boxes, c["keypoints"], c["spans"]):
            o["track_boxes"] = torch.as_tensor(bx).to(device=kp.device, dtype=torch.float64)[max(a, 0):b]
            o["keypoints"] = kp
    return outs


def frame_results(results: dict, frame_ids, num_frames: int):
    """Per-frame view of per-person results, as ``prepare_rendering_results`` builds it (lib/utils/demo_utils.py:164-182):
    results {person_id: {'mesh', 'pred_cam', 'bboxes'[, 'frame_ids']}} (host arrays, one row per frame of the tracklet) and frame_ids
    {person_id: ids} (None: every entry carries its own 'frame_ids', as the demo's pickle does) -> list of ``num_frames`` OrderedDicts
    {person_id: {'verts', 'cam', 'bbox'}}, the persons of a frame ordered by ``bbox[1]`` ascending (the reference's sort key)."""
    frames = [{} for _ in range(num_frames)]
    for pid, data in results.items():
        ids = frame_ids[pid] if frame_ids is not None and pid in frame_ids else data["frame_ids"]
        if len(ids) != len(data["mesh"]):
            raise ValueError(f"person {pid!r}: {len(ids)} frame ids for {len(data['mesh'])} rows")
        for idx, fid in enumerate(ids):
            frames[int(fid)][pid] = {"verts": data["mesh"][idx], "cam": data["pred_cam"][idx], "bbox": data["bboxes"][idx]}
    out = []
    for fd in frames:
        keys = list(fd.keys())
        order = np.argsort([fd[k]["bbox"][1] for k in keys]) if keys else []
        out.append(OrderedDict((keys[i], fd[keys[i]]) for i in order))
    return out


def tracklet_draw_order(bbox_tops, frame_ids):
    """The order ``frame_results`` draws in, as job tables: bbox_tops[i] = bbox[:, 1] and frame_ids[i] of tracklet i (host arrays) ->
    (frame_index int32[N], draw_order int64[N]) over the concatenated rows: inside a frame ``bbox[1]`` ascending, ties in tracklet order."""
    fi = np.concatenate([np.asarray(f, dtype=np.int64) for f in frame_ids]) if len(frame_ids) else np.zeros(0, np.int64)
    top = np.concatenate([np.asarray(t, dtype=np.float64) for t in bbox_tops]) if len(bbox_tops) else np.zeros(0)
    if fi.shape != top.shape:
        raise ValueError(f"{fi.size} frame ids for {top.size} rows")
    by_top = np.argsort(top, kind="stable")
    return fi.astype(np.int32), by_top[np.argsort(fi[by_top], kind="stable")]


@torch.no_grad()
def render_tracklets(results, frames, img_wh, frame_ids=None, renderer=None, order: str = "reference", inplace: bool = False,
                     plain: bool = False, sideview: bool = False):
    """The demo's overlay video (main/run_demo.py:375-446) from ``run_tracklets``' outputs: results = list (or dict by person id) of dicts
    with 'mesh' [N_i,V,3], 'orig_cam' [N_i,4], 'bboxes' [N_i,4]; frames uint8 [F,H,W,3]; frame_ids = per tracklet the frame of each row
    (same container as results; None: the entry's own 'frame_ids', or rows 0..N_i-1).  renderer: a ``render.Renderer`` for ``img_wh``, or
    a face array to make one from.  The persons of a frame are drawn in ``frame_results``' order (``bbox[1]`` ascending, ties in tracklet
    order), each over the previous one (order "reference") or depth-tested against them ("depth").  Meshes, cameras and frames stay on
    the device; the boxes' top edges (one number per row) are read back once to build the schedule.  -> the overlaid frames.
    ``plain`` (--render_plain, run_demo.py:396-397): the meshes are drawn on black instead of on the frames.  ``sideview`` (--sideview,
    :399-422): -> uint8 [F,H,2W,3]; the left half is what the call returns without it, the right half the same jobs in the same order,
    turned by ``render.axis_rotation(270, (0, 1, 0))`` and drawn on black (whether or not ``plain`` is set, as in the reference)."""
    from . import render as R
    plain, sideview = _flag(plain, "plain"), _flag(sideview, "sideview")
    if sideview and inplace:
        raise ValueError("render_tracklets: inplace=True cannot be combined with sideview=True - the result is twice as wide as the "
                         "frames, so it cannot be written into them")
    if renderer is None:
        raise _lib.PmceError("render_tracklets needs renderer=: a render.Renderer, or the mesh's face array (SMPL's faces are not shipped)")
    if not isinstance(renderer, R.Renderer):
        renderer = R.Renderer(renderer, img_wh)
    if (renderer.width, renderer.height) != (int(img_wh[0]), int(img_wh[1])):
        raise _lib.PmceError(f"the renderer was made for {renderer.width} x {renderer.height}, img_wh is {tuple(img_wh)}")
    keys = list(results.keys()) if isinstance(results, dict) else list(range(len(results)))
    if not keys:
        if plain or sideview:
            if plain and inplace:
                frames[...] = 0
                return frames
            return _empty_views(frames, plain, sideview)
        return frames if inplace else (frames.clone() if isinstance(frames, torch.Tensor) else np.array(frames))
    ids = []
    for k in keys:
        d = results[k]
        fid = frame_ids[k] if frame_ids is not None else d.get("frame_ids", np.arange(len(d["mesh"])))
        if len(fid) != len(d["mesh"]):
            raise ValueError(f"tracklet {k!r}: {len(fid)} frame ids for {len(d['mesh'])} rows")
        ids.append(R._host(fid))
    cat = lambda name: torch.cat([torch.as_tensor(results[k][name]) for k in keys])  # noqa: E731
    tops = cat("bboxes")[:, 1].cpu().numpy()
    frame_index, draw = tracklet_draw_order([tops], ids)
    if not (plain or sideview):
        return renderer.render(frames, cat("mesh"), cat("orig_cam"), frame_index=frame_index, order=order, inplace=inplace, draw_order=draw)
    mesh, cams = cat("mesh"), cat("orig_cam")
    on_device = isinstance(frames, torch.Tensor) and frames.is_cuda

    def black():
        return torch.zeros(frames.shape, dtype=torch.uint8, device=frames.device) if on_device else np.zeros(tuple(frames.shape), np.uint8)

    if plain and inplace:
        frames[...] = 0
        base, into = frames, True
    else:
        base, into = (black(), on_device) if plain else (frames, False)       # a canvas of our own is drawn on in place
    left = renderer.render(base, mesh, cams, frame_index=frame_index, order=order, inplace=into, draw_order=draw)
    if not sideview:
        return left
    side = torch.from_numpy(R.axis_rotation(270, (0, 1, 0)).astype(np.float32))
    right = renderer.render(black(), mesh, cams, frame_index=frame_index, rotation=side, order=order, inplace=on_device, draw_order=draw)
    return torch.cat([left, right], 2) if isinstance(left, torch.Tensor) else np.concatenate([left, right], 2)
