"""GPU tests of the demo's 2D pose stage around the network (pmce_amd/pose2d.py on csrc/pose2d.hip) against tests/pose2d_ref.py, the
numpy restatement of the specification in include/pmce_hip.h.  No value was recorded from mmpose or OpenCV.

The warp is integer arithmetic after its map and must agree to the bit: bytes, normalised patches, the centre and scale record, the
status.  Of the decoding, the averaged heatmap, its first maximum and the score are exact and must agree to the bit; the refined
coordinates must stay within FACTOR = 4 x dev32 of the restatement's fp64 run, dev32 = the largest deviation of the restatement's own
fp32 run from its fp64 run on the same set (asserted > 0).  Every such test prints the ratio it measures (run with -s).

Measured on an MI355X, the largest ratio of each group: blobs 1.69 x (heatmap coordinates) and 1.29 x (image keypoints), corners and
edges 1.00 x, the pipeline 2.30 x on the 256 x 192 network and 1.00 x on the 64 x 48 one."""
import numpy as np
import pytest
import torch

import pose2d_ref as PR
import vitpose_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = PR.FACTOR
PERM17 = PR.flip_perm(PR.COCO_FLIP_PAIRS, 17)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """A device (or host) tensor and a numpy array, to the bit."""
    a = a.detach().cpu().contiguous().numpy()
    b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    return np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# the warp
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    f = PR.frames()
    return f, torch.from_numpy(f).to(DEV)


def rows_of(fmt, size):
    rows = PR.warp_boxes(size=size)
    boxes = np.array([PR.to_xywh(b) if fmt == "xywh" else b for _, b in rows], np.float64)
    fi = np.arange(len(rows), dtype=np.int32) % 2
    return [n for n, _ in rows], boxes, fi


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("fmt", ["cxcywh", "xywh"])
@pytest.mark.parametrize("size", [(256, 192), (64, 48), (27, 19)], ids=["256x192", "64x48", "27x19"])
def test_warp_is_the_restatement_to_the_bit(frames, size, fmt, order):
    """Inside, across each border, wholly outside, the three aspects, a 3 px box, four times the frame; 27 x 19 takes the path of a
    width that is no multiple of four.  The mirror rows are flip(3) of the plain rows."""
    from pmce_amd import pose2d
    host, dev = frames
    names, boxes, fi = rows_of(fmt, size)
    N = len(names)
    want_f32, want_u8, want_cs, want_st = PR.pose_patches(host, fi, boxes, size, fmt, 1.25, order, mirror=True)
    assert want_st.tolist() == [0] * N and not want_u8[names.index("outside")].any()
    assert all(want_u8[i].any() for i, n in enumerate(names) if n != "outside")
    patch, raw, cs, st = pose2d.pose_patches(dev, fi, torch.from_numpy(boxes).to(DEV), size, fmt, 1.25, order, mirror=True, return_raw=True)
    assert patch.shape == (2 * N, 3) + size and raw.shape == (2 * N,) + size + (3,) and raw.dtype == torch.uint8
    assert same(st, want_st) and same(cs, want_cs)
    bad = [names[i % N] for i in range(2 * N) if not np.array_equal(raw[i].cpu().numpy(), want_u8[i])]
    assert not bad, f"raw bytes differ for {bad}"
    assert same(patch, want_f32)
    assert torch.equal(bits(patch[N:]), bits(patch[:N].flip(3))) and torch.equal(raw[N:], raw[:N].flip(2))
    # without the mirror and without the bytes: the same plain rows; a host frame array and host boxes are uploaded
    p2, cs2, st2 = pose2d.pose_patches(host, fi, boxes, size, fmt, 1.25, order)
    assert p2.shape == (N, 3) + size and torch.equal(bits(p2), bits(patch[:N])) and torch.equal(bits(cs2), bits(cs)) and torch.equal(st2, st)


def test_warp_status_codes(frames):
    from pmce_amd import pose2d
    host, dev = frames
    boxes = np.array([(40.0, 30.0, 20.0, 30.0), (40.0, 30.0, 0.0, 30.0), (40.0, 30.0, 20.0, -1.0), (np.nan, 30.0, 20.0, 30.0),
                      (40.0, np.inf, 20.0, 30.0), (40.0, 30.0, 1e9, 30.0), (3e6, 30.0, 20.0, 30.0), (40.0, 30.0, 20.0, 30.0),
                      (41.0, 31.0, 20.0, 30.0)])
    fi = np.array([0, 0, 0, 0, 0, 0, 0, 2, 1], np.int32)           # job 7 names a frame that does not exist: a device table is trusted
    want_f32, want_u8, want_cs, want_st = PR.pose_patches(host, fi, boxes, (64, 48), mirror=True)
    assert want_st.tolist() == [0, 1, 1, 1, 1, 2, 2, 3, 0]
    with pytest.raises(ValueError):
        pose2d.pose_patches(dev, fi, boxes, (64, 48))               # the host table is validated
    patch, raw, cs, st = pose2d.pose_patches(dev, torch.from_numpy(fi).to(DEV), boxes, (64, 48), mirror=True, return_raw=True)
    assert same(st, want_st) and same(cs, want_cs) and same(raw, want_u8) and same(patch, want_f32)
    assert not raw[1:8].any() and raw[0].any() and raw[8].any()


def test_warp_does_not_depend_on_the_batch(frames):
    from pmce_amd import pose2d
    host, dev = frames
    names, boxes, fi = rows_of("cxcywh", (64, 48))
    seven = pose2d.pose_patches(dev, fi[:7], boxes[:7], (64, 48), mirror=True, return_raw=True)
    for j in (0, 6):
        one = pose2d.pose_patches(dev, fi[j:j + 1], boxes[j:j + 1], (64, 48), mirror=True, return_raw=True)
        assert torch.equal(bits(one[0][0]), bits(seven[0][j])) and torch.equal(bits(one[0][1]), bits(seven[0][7 + j]))
        assert torch.equal(one[1][0], seven[1][j]) and torch.equal(bits(one[2][0]), bits(seven[2][j]))
    again = pose2d.pose_patches(dev, fi[:7], boxes[:7], (64, 48), mirror=True, return_raw=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(seven, again))
    empty = pose2d.pose_patches(dev, fi[:0], boxes[:0], (64, 48), mirror=True, return_raw=True)
    assert [tuple(t.shape) for t in empty] == [(0, 3, 64, 48), (0, 64, 48, 3), (0, 4), (0,)]


# ------------------------------------------------------------------------------------------------------------------------------------
# decoding, on given heatmaps
# ------------------------------------------------------------------------------------------------------------------------------------
_blob_sets = {}


def blob_set(Hh, Wh, K, n=3):
    """(heat, flipped, centre_scale) as numpy - seeded, made once."""
    key = (Hh, Wh, K, n)
    if key not in _blob_sets:
        _blob_sets[key] = (PR.blobs(n, K, Hh, Wh)[0], PR.blobs(n, K, Hh, Wh, seed=PR.SEED + 7)[0], PR.centre_scales(n))
    return _blob_sets[key]


def nhwc_view(a):
    """The network's layout: NHWC storage behind an NCHW view."""
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(DEV).permute(0, 3, 1, 2)


def ratios(got_kp, got_xy, ref, label):
    """-> the two ratios (heatmap coordinates, image keypoints) of a device result to dev32; prints them."""
    (kp64, xy64, _), (kp32, xy32, _) = ref
    dev_xy = float(np.abs(xy32.astype(np.float64) - xy64).max())
    dev_kp = float(np.abs(kp32[..., :2].astype(np.float64) - kp64[..., :2]).max())
    assert dev_xy > 0 and dev_kp > 0, "the bound is vacuous"
    r_xy = float(np.abs(got_xy.cpu().numpy().astype(np.float64) - xy64).max()) / dev_xy
    r_kp = float(np.abs(got_kp[..., :2].cpu().numpy().astype(np.float64) - kp64[..., :2]).max()) / dev_kp
    print(f"{label}: x dev32: heatmap coordinates {r_xy:.2f} (dev32 {dev_xy:.2e} px), image keypoints {r_kp:.2f} (dev32 {dev_kp:.2e} px)")
    return r_xy, r_kp


# one keypoint has no pairs: its flipped set goes through the identity permutation
@pytest.mark.parametrize("K,flip", [(17, "plain"), (17, "coco"), (17, "identity"), (1, "plain"), (1, "identity")])
@pytest.mark.parametrize("hw", [(64, 48), (16, 12), (6, 6)], ids=["64x48", "16x12", "6x6"])
def test_decode_blobs(hw, K, flip):
    from pmce_amd import pose2d
    heat, flipped, cs = blob_set(*hw, K)
    pairs = PR.COCO_FLIP_PAIRS if flip == "coco" else ()
    perm = PR.flip_perm(pairs, K)
    hf = None if flip == "plain" else flipped
    ref = [PR.decode(heat, cs, hf, perm, dtype=d) for d in (np.float64, np.float32)]
    csd = torch.from_numpy(cs).to(DEV)
    outs = []
    for lay in (nhwc_view, lambda a: torch.from_numpy(a).to(DEV)):
        h = lay(heat)
        f = None if hf is None else lay(hf)
        outs.append(pose2d.decode_heatmaps(h, csd, f, pairs, return_heatmap_coords=True))
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b)), "the layout changes the result"
    kp, xy, arg = outs[0]
    assert kp.shape == (3, K, 3) and xy.shape == (3, K, 2) and arg.shape == (3, K, 2)
    assert same(arg, ref[1][2]) and same(kp[..., 2], ref[1][0][..., 2]), "argmax and score are exact"
    r_xy, r_kp = ratios(kp, xy, ref, f"{hw[0]} x {hw[1]}, K = {K}, {flip}")
    assert r_xy <= FACTOR and r_kp <= FACTOR


def exact_maps(Hh=12, Wh=9):
    """Heatmaps [1,K,Hh,Wh] (+ a flipped set) whose outcome is known: name -> channel."""
    y, x = np.mgrid[0:Hh, 0:Wh].astype(np.float64)
    spots = [(0, 0), (Wh - 1, 0), (0, Hh - 1), (Wh - 1, Hh - 1), (4, 0), (4, Hh - 1), (0, 5), (Wh - 1, 5)]       # corners, then edges
    maps = [0.9 * np.exp(-((x - px) ** 2 + (y - py) ** 2) / 8.0) + 0.01 for px, py in spots]
    tie = np.full((Hh, Wh), 0.1)
    tie[7, 2] = tie[3, 6] = 0.7                              # two equal maxima: (6, 3) comes first
    flat = np.full((Hh, Wh), 0.25)
    neg = np.full((Hh, Wh), -0.25)
    neg[5, 5] = -0.125
    zero = np.zeros((Hh, Wh))
    big = np.full((Hh, Wh), 60.0)
    big[4, 3] = 80.0                                         # the blur stays above 50: the log map is flat, the offset exactly 0
    tiny = np.full((Hh, Wh), 1e-5)
    tiny[8, 7] = 2e-5                                        # the blur stays below 0.001
    maps += [tie, flat, neg, zero, big, tiny]
    want = spots + [(6, 3), (0, 0), (-1, -1), (-1, -1), (3, 4), (7, 8)]
    return np.stack(maps)[None].astype(np.float32), want


def test_decode_exact_cases():
    from pmce_amd import pose2d
    heat, want = exact_maps()
    K = heat.shape[1]
    cs = PR.centre_scales(1)
    csd = torch.from_numpy(cs).to(DEV)
    ref64, ref32 = (PR.decode(heat, cs, dtype=d) for d in (np.float64, np.float32))
    assert ref32[2][0].tolist() == [list(w) for w in want]
    kp, xy, arg = pose2d.decode_heatmaps(nhwc_view(heat), csd, return_heatmap_coords=True)
    assert arg[0].tolist() == [list(w) for w in want] and same(kp[..., 2], ref32[0][..., 2])
    # corners and edges: refined like any other peak
    r_xy, r_kp = ratios(kp[:, :8], xy[:, :8], [tuple(a[:, :8] for a in r) for r in (ref64, ref32)], "corners and edges")
    assert r_xy <= FACTOR and r_kp <= FACTOR
    # the tie, the constant map, maxima <= 0, values beyond the clip: the log map is flat or unused there, every step exact
    for k in range(9, K):
        assert xy[0, k].tolist() == [float(v) for v in want[k]], k
    assert same(xy[:, 9:], ref32[1][:, 9:]) and same(kp[:, 9:], ref32[0][:, 9:])
    r_xy, r_kp = ratios(kp[:, 8:9], xy[:, 8:9], [tuple(a[:, 8:9] for a in r) for r in (ref64, ref32)], "two equal maxima")
    assert r_xy <= FACTOR and r_kp <= FACTOR
    # a tie that only the flip average makes, channels 1 and 2 swapped: the plain set alone would pick (6, 5), the average is
    # f32(0.4 + 0.8) / 2 at (2, 3) and f32(0.8 + 0.4) / 2 at (6, 5), and the first of the two wins
    h = np.full((1, 3, 12, 9), 0.05, np.float32)
    hf = np.full((1, 3, 12, 9), 0.05, np.float32)
    h[0, 1, 3, 2], h[0, 1, 5, 6] = 0.4, 0.8
    hf[0, 2, 3, 9 - 1 - 2], hf[0, 2, 5, 9 - 1 - 6] = 0.8, 0.4
    r32 = PR.decode(h, cs, hf, [0, 2, 1])
    assert PR.decode(h, cs)[2][0, 1].tolist() == [6, 5] and r32[2][0, 1].tolist() == [2, 3]
    kp, xy, arg = pose2d.decode_heatmaps(nhwc_view(h), csd, nhwc_view(hf), ((1, 2),), return_heatmap_coords=True)
    assert same(arg, r32[2]) and same(kp[..., 2], r32[0][..., 2])
    assert float(kp[0, 1, 2]) == float(np.float32(np.float32(0.4) + np.float32(0.8)) * np.float32(0.5))


def test_decode_batch_and_repeats():
    from pmce_amd import pose2d
    heat, flipped, cs = (np.concatenate([a, a[:2]]) for a in blob_set(16, 12, 17))
    h, f, csd = nhwc_view(heat), nhwc_view(flipped), torch.from_numpy(cs).to(DEV)
    five = pose2d.decode_heatmaps(h, csd, f, return_heatmap_coords=True)
    again = pose2d.decode_heatmaps(h, csd, f, return_heatmap_coords=True)
    one = pose2d.decode_heatmaps(h[2:3], csd[2:3], f[2:3], return_heatmap_coords=True)
    for a, b, c in zip(five, again, one):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a[2:3]), bits(c)) and torch.equal(bits(a[:2]), bits(a[3:]))
    assert torch.equal(bits(pose2d.decode_heatmaps(h, csd, f)), bits(five[0]))
    # a status marks images whose warp was refused
    st = torch.tensor([0, 1, 0, 3, 0], dtype=torch.int32, device=DEV)
    kp = pose2d.decode_heatmaps(h, csd, f, status=st)
    assert not kp[1].any() and not kp[3].any() and torch.equal(bits(kp[[0, 2, 4]]), bits(five[0][[0, 2, 4]]))
    empty = pose2d.decode_heatmaps(h[:0], csd[:0], f[:0], return_heatmap_coords=True)
    assert [tuple(t.shape) for t in empty] == [(0, 17, 3), (0, 17, 2), (0, 17, 2)] and pose2d.decode_heatmaps(h[:0], csd[:0]).shape == (0, 17, 3)


def test_decode_argument_errors():
    from pmce_amd import pose2d
    h = torch.zeros(2, 17, 16, 12, device=DEV)
    cs = torch.ones(2, 4, device=DEV)
    bad = [dict(heat=h.double()), dict(heat=h[0]), dict(heat=torch.zeros(2, 65, 16, 12, device=DEV)), dict(heat=h[:, :, :5]), dict(heat=h[..., :5]),
           dict(heat=h.cpu()), dict(heat_flipped=h[:1]), dict(heat_flipped=h[:, :16]), dict(heat_flipped=h.cpu()), dict(centre_scale=cs[:1]),
           dict(centre_scale=cs.double()), dict(centre_scale=cs[:, :3]), dict(kernel=9), dict(heat_flipped=h, flip_pairs=((1, 17),)),
           dict(heat_flipped=h, flip_pairs=((1, 2), (2, 3))), dict(status=torch.zeros(2, device=DEV)), dict(status=torch.zeros(3, dtype=torch.int32, device=DEV))]
    for kw in bad:
        args = dict(heat=h, centre_scale=cs)
        args.update(kw)
        with pytest.raises(ValueError):
            pose2d.decode_heatmaps(**args)
    kp = pose2d.decode_heatmaps(h, cs, h)                      # and the call still works: an all-zero map has no keypoint
    assert kp.shape == (2, 17, 3) and not kp[..., 2].any()


# ------------------------------------------------------------------------------------------------------------------------------------
# the pipeline, on two small networks
# ------------------------------------------------------------------------------------------------------------------------------------
NETS = {
    "hd80": dict(H=256, W=192, C=160, depth=2, heads=2, F1=32, F2=32, K=17),
    "hd64": dict(H=64, W=48, C=128, depth=1, heads=2, F1=32, F2=32, K=17),
}
JOBS = np.array([(40.0, 30.0, 20.0, 30.0), (2.0, 30.0, 20.0, 26.0), (41.0, 31.0, 50.0, 20.0), (40.0, 30.0, 0.0, 30.0), (33.3, 27.7, 13.0, 35.0),
                 (60.0, 20.0, 25.0, 33.0)])
JOB_FRAMES = np.array([0, 1, 1, 0, 0, 1], np.int32)


@pytest.fixture(scope="module", params=list(NETS))
def pipe(request, frames):
    """(cfg, the network, TopDownPose's keypoints and status, the three stages by hand) - once per network."""
    from pmce_amd import pose2d
    from pmce_amd.vitpose import ViTPose
    cfg = NETS[request.param]
    size = (cfg["H"], cfg["W"])
    sd = VR.state_dict(C=cfg["C"], depth=cfg["depth"], heads=cfg["heads"], F1=cfg["F1"], F2=cfg["F2"], K=cfg["K"], img_size=size)
    net = ViTPose.from_state_dict(sd, DEV, img_size=size)
    host, dev = frames
    kp, st = pose2d.TopDownPose(net)(dev, JOB_FRAMES, JOBS)
    patches, cs, st2 = pose2d.pose_patches(dev, JOB_FRAMES, JOBS, size, mirror=True)
    heat = net(patches)
    torch.cuda.synchronize()
    return cfg, net, (kp, st), (patches, cs, st2, heat)


def test_pipeline_is_its_three_stages(pipe, frames):
    from pmce_amd import pose2d
    cfg, net, (kp, st), (patches, cs, st2, heat) = pipe
    m = len(JOBS)
    size = (cfg["H"], cfg["W"])
    want_f32, _, want_cs, want_st = PR.pose_patches(frames[0], JOB_FRAMES, JOBS, size, mirror=True)
    assert same(patches, want_f32) and same(cs, want_cs) and same(st2, want_st) and same(st, want_st) and want_st.tolist() == [0, 0, 0, 1, 0, 0]
    assert heat.shape == (2 * m, 17, size[0] // 4, size[1] // 4) and not heat.is_contiguous()
    by_hand = pose2d.decode_heatmaps(heat[:m], cs, heat[m:], status=st2)
    assert kp.shape == (m, 17, 3) and torch.equal(bits(kp), bits(by_hand))
    # against the restatement run on the device's own heatmaps
    h, hf = heat[:m].cpu().numpy(), heat[m:].cpu().numpy()
    ref = [PR.decode(h, want_cs, hf, PERM17, dtype=d, status=want_st) for d in (np.float64, np.float32)]
    _, xy, arg = pose2d.decode_heatmaps(heat[:m], cs, heat[m:], return_heatmap_coords=True)
    assert same(arg, ref[1][2]) and same(kp[..., 2], ref[1][0][..., 2])
    r_xy, r_kp = ratios(kp, xy, ref, f"pipeline {size[0]} x {size[1]}")
    assert r_xy <= FACTOR and r_kp <= FACTOR
    assert float(kp[..., 2].abs().max()) > 0


def test_pipeline_flip_test_status_and_chunks(pipe, frames):
    from pmce_amd import pose2d
    cfg, net, (kp, st), (patches, cs, st2, heat) = pipe
    host, dev = frames
    m = len(JOBS)
    plain, st_p = pose2d.TopDownPose(net, flip_test=False)(dev, JOB_FRAMES, JOBS)
    assert torch.equal(bits(plain), bits(pose2d.decode_heatmaps(heat[:m], cs, status=st2))) and not torch.equal(bits(plain), bits(kp))
    # the refused job is (0, 0, 0) and leaves its neighbours alone
    assert st.tolist() == [0, 0, 0, 1, 0, 0] and not kp[3].any() and kp[[0, 1, 2, 4, 5]][..., 2].ne(0).any(dim=1).all()
    keep = [0, 1, 2, 4, 5]
    kp5, st5 = pose2d.TopDownPose(net)(dev, JOB_FRAMES[keep], JOBS[keep])
    assert st5.tolist() == [0] * 5 and torch.equal(bits(kp5), bits(kp[keep]))
    # chunks, a device frame table, and no jobs
    kp2, st2b = pose2d.TopDownPose(net, chunk=4)(dev, torch.from_numpy(JOB_FRAMES).to(DEV), torch.from_numpy(JOBS).to(DEV))
    assert torch.equal(bits(kp2), bits(kp)) and torch.equal(st2b, st)
    kp0, st0 = pose2d.TopDownPose(net)(dev, JOB_FRAMES[:0], JOBS[:0])
    assert kp0.shape == (0, 17, 3) and st0.shape == (0,)


def test_pose_tracklets_split_one_joint_call(pipe, frames):
    from pmce_amd import demo, pose2d
    cfg, net, (kp, st), _ = pipe
    host, dev = frames
    pose = pose2d.TopDownPose(net)
    calls = []

    def counted(*a):
        calls.append(1)
        return pose(*a)

    counted.box_format = pose.box_format
    out = demo.pose_tracklets(dev, [(JOBS[:2], JOB_FRAMES[:2]), (JOBS[2:2], JOB_FRAMES[2:2]), (torch.from_numpy(JOBS[2:]), torch.from_numpy(JOB_FRAMES[2:]))],
                              counted)
    assert len(calls) == 1 and [len(k) for k, _ in out] == [2, 0, 4]
    assert torch.equal(bits(torch.cat([k for k, _ in out])), bits(kp))
    assert all(f.dtype == np.int64 for _, f in out) and np.array_equal(np.concatenate([f for _, f in out]), JOB_FRAMES)
