"""The JPEG reader on the GPU (csrc/jpeg.hip) against Pillow's recorded pixels (tests/golden/jpeg.npz) and the numpy restatement
(tests/jpeg_ref.py).  Every comparison is exact: bytes of pixels, int16 coefficients, status words."""
import os.path as osp

import numpy as np
import pytest
import torch

import jpeg_ref as JR
from pmce_amd import demo, jpeg

pytestmark = pytest.mark.gpu

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = np.load(osp.join(REPO, "tests", "golden", "jpeg.npz"))
J = ["j0", "j1", "j2", "j3", "j4"]
# Case t (40 x 300, 4:2:0) is the one that spans the kernels' own tiles: a workgroup of the colour stage covers 256 pixels x 4 rows
# (t: 2 x 10 of them, the second one partial in x), a workgroup of the inverse DCT 256 blocks (t has 19 x 3 MCUs x 6 = 342: two
# workgroups, the second partial).  m and m2 have chroma planes of two columns, which libjpeg replicates instead of filtering.
SINGLE = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "t", "m", "m2"]


def dev():
    return torch.device("cuda:0")


def file(name):
    return bytes(GOLD[f"file_{name}"])


def golden_rgb(name):
    px = GOLD[f"pixels_{name}"]
    return np.repeat(px[..., None], 3, axis=2) if px.ndim == 2 else px


def cut_to_half_its_scan(data):
    h = jpeg.parse(data)
    return data[:(h.scan_begin + h.scan_end) // 2]


@pytest.mark.parametrize("name", SINGLE)
def test_decode_equals_pillow_to_the_bit(name):
    want = golden_rgb(name)
    frames, status = jpeg.decode([file(name)], dev())
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (1,) + want.shape and status.dtype == torch.int32
    assert int(status.cpu()[0]) == 0
    assert int((frames[0].cpu().numpy() != want[..., ::-1]).sum()) == 0                 # B, G, R: cv2.imread's order
    rgb, status = jpeg.decode([file(name)], dev(), channel_order="rgb")
    assert int(status.cpu()[0]) == 0 and int((rgb[0].cpu().numpy() != want).sum()) == 0


def test_video_equals_pillow_to_the_bit():
    want = np.stack([golden_rgb(n) for n in J])
    frames, status = jpeg.decode([file(n) for n in J], dev())
    assert status.cpu().tolist() == [0] * 5 and int((frames.cpu().numpy() != want[..., ::-1]).sum()) == 0
    rgb, status = jpeg.decode([file(n) for n in J], dev(), channel_order="rgb")
    assert status.cpu().tolist() == [0] * 5 and int((rgb.cpu().numpy() != want).sum()) == 0


@pytest.mark.parametrize("name", ["d", "e", "h"])
def test_entropy_stage_equals_the_restatement(name):
    _, want, st = JR.entropy_decode(file(name))
    frames, status, coef = jpeg.decode([file(name)], dev(), return_coefficients=True)
    assert st == 0 and int(status.cpu()[0]) == 0
    assert coef.dtype == torch.int16 and tuple(coef.shape) == want.shape
    assert int((coef.cpu().numpy() != want).sum()) == 0


def test_tables_in_global_memory_give_the_same_bits():
    """The entropy stage reads the Huffman tables from LDS when the batch has at most 16 distinct ones and from global memory otherwise;
    ``lds_tables=False`` takes the second form on the same files: h (custom tables), d (a lane per MCU) and the video."""
    for names in (["h"], ["d"], J):
        files = [file(n) for n in names]
        a, sa, ca = jpeg.decode(files, dev(), return_coefficients=True)
        b, sb, cb = jpeg.decode(files, dev(), return_coefficients=True, lds_tables=False)
        assert sb.cpu().tolist() == [0] * len(files) == sa.cpu().tolist()
        assert torch.equal(a, b) and torch.equal(ca, cb)
        assert np.array_equal(b.cpu().numpy(), np.stack([golden_rgb(n) for n in names])[..., ::-1])


@pytest.mark.parametrize("lanes", [2, 5, 64])
def test_several_lanes_per_wavefront(lanes):
    """The entropy stage gives a wavefront more than one segment only when a round has more than 4096 of them; ``lanes=`` forces it
    on small rounds.  d has 12 segments (a lane per MCU) and, with e (3 segments, stuffed bytes) and h (1, custom tables), a batch
    the restatement covers: 5 lanes leave the last wavefront with 2 (d) lanes, 64 put a whole image into one partial wavefront,
    2 split the video's 9 segments 2 + 2 + 2 + 2 + 1.  Coefficients against the restatement, pixels against Pillow."""
    for names in (["d"], ["e"], ["h"], J):
        files = [file(n) for n in names]
        frames, status, coef = jpeg.decode(files, dev(), return_coefficients=True, lanes=lanes)
        assert status.cpu().tolist() == [0] * len(files)
        want = np.concatenate([JR.entropy_decode(f)[1] for f in files])
        assert int((coef.cpu().numpy() != want).sum()) == 0
        assert np.array_equal(frames.cpu().numpy(), np.stack([golden_rgb(n) for n in names])[..., ::-1])
    frames, status, coef = jpeg.decode([file("d")], dev(), return_coefficients=True, lanes=lanes, lds_tables=False)
    assert int(status.cpu()[0]) == 0 and int((coef.cpu().numpy() != JR.entropy_decode(file("d"))[1]).sum()) == 0
    # a damaged stream beside intact ones in ONE wavefront: its neighbours keep their bits
    e = file("e")
    frames, status = jpeg.decode([e, cut_to_half_its_scan(e), e], dev(), lanes=lanes)
    st = status.cpu().tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0
    assert np.array_equal(frames[0].cpu().numpy(), golden_rgb("e")[..., ::-1]) and torch.equal(frames[0], frames[2])


def test_a_round_of_more_than_4096_segments():
    """The launcher's own choice of two lanes per wavefront: 1366 copies of j0 (3 segments each) and one j1 (1) are 4099 segments in one
    round - 2050 wavefronts, the last one with a single lane."""
    files = [file("j0")] * 1366 + [file("j1")]
    hdrs = jpeg.parse_all(files[-2:])
    assert 1366 * len(hdrs[0].segments) + len(hdrs[1].segments) == 4099
    frames, status, coef = jpeg.decode(files, dev(), chunk=len(files), return_coefficients=True)
    assert int(status.count_nonzero().cpu()) == 0
    c0, c1 = (torch.from_numpy(JR.entropy_decode(file(n))[1]).to(dev()) for n in ("j0", "j1"))
    assert torch.equal(coef[:-len(c1)].view(1366, *c0.shape), c0.expand(1366, *c0.shape)) and torch.equal(coef[-len(c1):], c1)
    w0, w1 = (torch.from_numpy(np.ascontiguousarray(golden_rgb(n)[..., ::-1])).to(dev()) for n in ("j0", "j1"))
    assert torch.equal(frames[:-1], w0.expand(1366, *w0.shape)) and torch.equal(frames[-1], w1)


def test_same_bits_alone_in_a_batch_and_across_rounds():
    files = [file(n) for n in J]
    want = np.stack([golden_rgb(n) for n in J])[..., ::-1]
    batch, _ = jpeg.decode(files, dev())
    batch = batch.cpu().numpy()
    for i, f in enumerate(files):
        alone, st = jpeg.decode([f], dev())
        assert int(st.cpu()[0]) == 0 and np.array_equal(alone[0].cpu().numpy(), batch[i])
    # 70 frames, 32 per round: three rounds, every image in other wavefronts and workspace places than in the batch of five (rounds this
    # small give every segment lane 0 of a wavefront of its own: several lanes per wavefront are test_several_lanes_per_wavefront's)
    many, st = jpeg.decode(files * 14, dev(), chunk=32)
    assert st.cpu().tolist() == [0] * 70
    many = many.cpu().numpy()
    assert all(np.array_equal(many[k], want[k % 5]) for k in range(70))
    # a round of one image, and two runs of the same call
    again, _ = jpeg.decode(files * 14, dev(), chunk=32)
    ones, _ = jpeg.decode(files, dev(), chunk=1)
    assert np.array_equal(again.cpu().numpy(), many) and np.array_equal(ones.cpu().numpy(), batch) and np.array_equal(batch, want)


def test_out_is_filled_in_place():
    files = [file(n) for n in J]
    out = torch.full((5, 48, 64, 3), 7, device=dev(), dtype=torch.uint8)
    frames, status = jpeg.decode(files, out=out)
    assert frames.data_ptr() == out.data_ptr() and status.device == out.device
    assert np.array_equal(out.cpu().numpy(), np.stack([golden_rgb(n) for n in J])[..., ::-1])
    with pytest.raises(ValueError):
        jpeg.decode(files, out=torch.empty(5, 48, 64, 3, device=dev(), dtype=torch.float32))
    with pytest.raises(ValueError):
        jpeg.decode(files, out=torch.empty(4, 48, 64, 3, device=dev(), dtype=torch.uint8))


def test_damaged_file_in_a_batch(tmp_path):
    """The error path: a file cut to half its scan between two intact ones.  Its status is nonzero, and only its; the neighbours are
    bit-equal to the golden pixels.  Safe by construction: the entropy body is the one scripts/jpeg_entropy_host.cpp runs over every
    shortened length of every segment between guard regions (tests/test_jpeg_host.py), and the later stages read only the workspace.
    A call takes files of ONE size, so case e (40 x 48), cut, stands between copies of itself; between j0 and j1 (48 x 64) stands j3,
    which like e has a restart interval per MCU row, cut the same way."""
    e, e_cut = file("e"), cut_to_half_its_scan(file("e"))
    frames, status = jpeg.decode([e, e_cut, e], dev())
    st = status.cpu().tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0 and st[1] & jpeg.STATUS_TRUNCATED
    want = golden_rgb("e")[..., ::-1]
    assert np.array_equal(frames[0].cpu().numpy(), want) and np.array_equal(frames[2].cpu().numpy(), want)
    # what was decoded before the cut is there: the first MCU row (its restart interval is whole)
    assert np.array_equal(frames[1, :8].cpu().numpy(), want[:8])

    files = [file("j0"), cut_to_half_its_scan(file("j3")), file("j1")]
    frames, status = jpeg.decode(files, dev())
    st = status.cpu().tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0
    assert np.array_equal(frames[0].cpu().numpy(), golden_rgb("j0")[..., ::-1])
    assert np.array_equal(frames[2].cpu().numpy(), golden_rgb("j1")[..., ::-1])
    for fname, data in zip(("000001.jpg", "000002.jpg", "000003.jpg"), files):
        (tmp_path / fname).write_bytes(data)
    with pytest.raises(ValueError) as err:
        demo.load_frames(str(tmp_path), device=dev())
    assert "000002.jpg" in str(err.value) and "truncated" in str(err.value)
    loose, wh, names = demo.load_frames(str(tmp_path), device=dev(), strict=False)
    assert names == ["000001.jpg", "000002.jpg", "000003.jpg"] and wh == (64, 48)
    assert np.array_equal(loose.cpu().numpy(), frames.cpu().numpy())


def test_load_frames_gives_the_videos_frames(tmp_path):
    for k, n in enumerate(J):
        (tmp_path / f"{k + 1:06d}.jpg").write_bytes(file(n))
    frames, wh, names = demo.load_frames(str(tmp_path), device=dev())
    assert wh == (64, 48) and names == [f"{k + 1:06d}.jpg" for k in range(5)] and frames.is_cuda and frames.dtype == torch.uint8
    assert np.array_equal(frames.cpu().numpy(), np.stack([golden_rgb(n) for n in J])[..., ::-1])
