"""The JPEG reader's parallel entropy stage on the GPU (csrc/jpeg_parallel.hip) against Pillow's recorded pixels
(tests/golden/jpeg.npz, jpeg_parallel.npz), the numpy restatement (tests/jpeg_ref.py) and the serial stage.  Every comparison is exact:
bytes of pixels, int16 coefficients, status words.  With a subsequence of 4 or 12 bytes the small golden files reach every structure
of the stage: t is 652 subsequences in three runs, e carries 22 stuffed bytes, h has codes longer than the lookahead, i, b and f have
1, 3 and 4 blocks per MCU, m and m2 fewer subsequences than a wavefront, d, j0 and j3 restart intervals (d's shorter than the default
subsequence)."""
import os.path as osp

import numpy as np
import pytest
import torch

import jpeg_ref as JR
from pmce_amd import _lib, demo, jpeg

pytestmark = pytest.mark.gpu

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLD = dict(np.load(osp.join(REPO, "tests", "golden", "jpeg.npz")))
GOLD.update(np.load(osp.join(REPO, "tests", "golden", "jpeg_parallel.npz")))
J = ["j0", "j1", "j2", "j3", "j4"]
SINGLE = ["a", "b", "c", "d", "e", "f", "g", "h", "i", "t", "m", "m2"]
LONG = ["p420", "p420opt", "pgrey"]
SIZES = [4, 12, 64, 0]
_restated = {}


def dev():
    return torch.device("cuda:0")


def file(name):
    return bytes(GOLD[f"file_{name}"])


def golden_rgb(name):
    px = GOLD[f"pixels_{name}"]
    return np.repeat(px[..., None], 3, axis=2) if px.ndim == 2 else px


def restated(name):
    """(coefficients, status) of the numpy restatement, computed once per file."""
    if name not in _restated:
        _, coef, st = JR.entropy_decode(file(name))
        _restated[name] = (coef, st)
    return _restated[name]


def cut_to_half_its_scan(data):
    h = jpeg.parse(data)
    return data[:(h.scan_begin + h.scan_end) // 2]


@pytest.mark.parametrize("name", SINGLE)
def test_parallel_decode_equals_pillow_to_the_bit(name):
    want = golden_rgb(name)
    for S in SIZES:
        frames, status = jpeg.decode([file(name)], dev(), entropy="parallel", subsequence=S)
        assert int(status.cpu()[0]) == 0, S
        assert int((frames[0].cpu().numpy() != want[..., ::-1]).sum()) == 0, S
        rgb, status = jpeg.decode([file(name)], dev(), channel_order="rgb", entropy="parallel", subsequence=S)
        assert int(status.cpu()[0]) == 0 and int((rgb[0].cpu().numpy() != want).sum()) == 0, S


def test_parallel_video_equals_pillow_to_the_bit():
    want = np.stack([golden_rgb(n) for n in J])
    for S in SIZES:
        frames, status = jpeg.decode([file(n) for n in J], dev(), entropy="parallel", subsequence=S)
        assert status.cpu().tolist() == [0] * 5 and int((frames.cpu().numpy() != want[..., ::-1]).sum()) == 0, S
        rgb, status = jpeg.decode([file(n) for n in J], dev(), channel_order="rgb", entropy="parallel", subsequence=S)
        assert status.cpu().tolist() == [0] * 5 and int((rgb.cpu().numpy() != want).sum()) == 0, S


def test_t_spans_three_workgroups_of_the_synchronise_stage():
    run = _lib.load().pmce_jpeg_parallel_run()
    assert run == jpeg.PARALLEL_RUN
    sub = jpeg.subsequence_records(jpeg.build_records(jpeg.parse_all([file("t")]), 32), 4)
    n_sub, n_runs, longest = sub["totals"][0]
    assert (n_sub, longest) == (652, 2605) and n_runs == -(-n_sub // run) >= 3           # two guessed borders between runs


@pytest.mark.parametrize("name", ["d", "e", "h", "t"])
def test_parallel_coefficients_equal_the_restatement(name):
    want, st = restated(name)
    assert st == 0
    for S in (4, 0):
        frames, status, coef = jpeg.decode([file(name)], dev(), return_coefficients=True, entropy="parallel", subsequence=S)
        assert int(status.cpu()[0]) == 0 and coef.dtype == torch.int16 and tuple(coef.shape) == want.shape
        assert int((coef.cpu().numpy() != want).sum()) == 0, S


def test_same_bits_whatever_the_stage_the_batch_and_the_round():
    files = [file(n) for n in J]
    want = np.stack([golden_rgb(n) for n in J])[..., ::-1]
    serial, ss, cs = jpeg.decode(files, dev(), return_coefficients=True, entropy="serial")
    for S in (4, 12, 0):
        batch, sb, cb = jpeg.decode(files, dev(), return_coefficients=True, entropy="parallel", subsequence=S)
        assert torch.equal(batch, serial) and torch.equal(sb, ss) and torch.equal(cb, cs), S
        no_lds, sn, cn = jpeg.decode(files, dev(), return_coefficients=True, entropy="parallel", subsequence=S, lds_tables=False)
        assert torch.equal(no_lds, serial) and torch.equal(sn, ss) and torch.equal(cn, cs), S
        for i, f in enumerate(files):
            alone, st = jpeg.decode([f], dev(), entropy="parallel", subsequence=S)
            assert int(st.cpu()[0]) == 0 and torch.equal(alone[0], serial[i]), (S, i)
        # 70 frames, 32 per round: three rounds through one workspace
        many, st = jpeg.decode(files * 14, dev(), chunk=32, entropy="parallel", subsequence=S)
        assert st.cpu().tolist() == [0] * 70
        many = many.cpu().numpy()
        assert all(np.array_equal(many[k], want[k % 5]) for k in range(70)), S
        again, _ = jpeg.decode(files * 14, dev(), chunk=32, entropy="parallel", subsequence=S)
        ones, _ = jpeg.decode(files, dev(), chunk=1, entropy="parallel", subsequence=S)
        assert np.array_equal(again.cpu().numpy(), many) and torch.equal(ones, serial), S
    assert np.array_equal(serial.cpu().numpy(), want)
    # h (custom tables with long codes) and t with the tables in global memory
    for name in ("h", "t"):
        a, sa, ca = jpeg.decode([file(name)], dev(), return_coefficients=True, entropy="serial")
        b, sb, cb = jpeg.decode([file(name)], dev(), return_coefficients=True, entropy="parallel", subsequence=4, lds_tables=False)
        assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(ca, cb)


def test_parallel_out_is_filled_in_place():
    files = [file(n) for n in J]
    out = torch.full((5, 48, 64, 3), 7, device=dev(), dtype=torch.uint8)
    frames, status = jpeg.decode(files, out=out, entropy="parallel", subsequence=12)
    assert frames.data_ptr() == out.data_ptr() and status.device == out.device and status.cpu().tolist() == [0] * 5
    assert np.array_equal(out.cpu().numpy(), np.stack([golden_rgb(n) for n in J])[..., ::-1])


@pytest.mark.parametrize("name", ["e", "t"])
def test_a_file_cut_to_half_its_scan_between_intact_copies(name):
    """Safe by construction: the body is the one scripts/jpeg_parallel_host.cpp runs over every shortened length of these segments
    between guard regions and compares with the serial body (tests/test_jpeg_parallel_host.py)."""
    whole, cut = file(name), cut_to_half_its_scan(file(name))
    want = golden_rgb(name)[..., ::-1]
    s_frames, s_status, s_coef = jpeg.decode([whole, cut, whole], dev(), return_coefficients=True, entropy="serial")
    for S in (4, 12, 0):
        frames, status, coef = jpeg.decode([whole, cut, whole], dev(), return_coefficients=True, entropy="parallel", subsequence=S)
        st = status.cpu().tolist()
        assert st[0] == 0 and st[2] == 0 and st[1] & jpeg.STATUS_TRUNCATED and st == s_status.cpu().tolist(), S
        assert torch.equal(coef, s_coef) and torch.equal(frames, s_frames), S
        assert np.array_equal(frames[0].cpu().numpy(), want) and np.array_equal(frames[2].cpu().numpy(), want), S


def test_a_marker_in_the_middle_of_a_scan(tmp_path):
    e = file("e")
    h = jpeg.parse(e)
    at = int(h.segments[1, 0] + h.segments[1, 1]) // 2      # the middle of the second restart interval
    bad = e[:at] + b"\xff\xd9" + e[at + 2:]
    _, want, want_status = JR.entropy_decode(bad)
    assert want_status != 0
    s_frames, s_status, s_coef = jpeg.decode([e, bad, e], dev(), return_coefficients=True, entropy="serial")
    n = want.shape[0]

    def equals_the_restatement(got):
        """Up to and including the block in which the error shows, the coefficients are the restatement's.  Behind it the two differ by
        their definitions: the device stops a segment after that block (csrc/jpeg_entropy.hpp) where the restatement, which looks at
        its status after every MCU, finishes the MCU on zero bits; and of the third interval, which the marker left empty, the device
        decodes one block on zero bits where the restatement decodes none."""
        bpm = h.blocks_per_mcu
        second, third = 3 * bpm, 6 * bpm                     # the first blocks of the second and the third restart interval
        last = second + int(np.flatnonzero(got[second:third].any(axis=1)).max())
        return (second < last < third - 1 and np.array_equal(got[:last + 1], want[:last + 1]) and not got[last + 1:third].any()
                and not got[third + 1:].any() and not want[third:].any())

    assert equals_the_restatement(s_coef[n:2 * n].cpu().numpy()) and int(s_status.cpu()[1]) == want_status
    for S in (4, 12, 0):
        frames, status, coef = jpeg.decode([e, bad, e], dev(), return_coefficients=True, entropy="parallel", subsequence=S)
        assert status.cpu().tolist() == [0, want_status, 0], S
        assert torch.equal(coef, s_coef) and torch.equal(frames, s_frames), S
        assert equals_the_restatement(coef[n:2 * n].cpu().numpy()), S
        assert np.array_equal(frames[0].cpu().numpy(), golden_rgb("e")[..., ::-1]) and torch.equal(frames[0], frames[2]), S
    for fname, data in zip(("000001.jpg", "000002.jpg", "000003.jpg"), (e, cut_to_half_its_scan(e), e)):
        (tmp_path / fname).write_bytes(data)
    with pytest.raises(ValueError) as err:
        demo.load_frames(str(tmp_path), device=dev(), strict=True, entropy="parallel")
    assert "000002.jpg" in str(err.value) and "truncated" in str(err.value)


def stages(timings):
    return [name for name, _, _ in timings]


def test_auto_takes_the_parallel_stage_from_the_threshold_on():
    parallel = ["entropy_" + s for s in jpeg.PARALLEL_STAGES] + ["idct", "colour"]
    assert len(parallel) == _lib.load().pmce_jpeg_parallel_stages() + 2
    t = []
    jpeg.decode([file("t")], dev(), timings=t)              # 2,605 bytes: below the threshold
    assert stages(t) == ["entropy", "idct", "colour"]
    for name in LONG:
        data = file(name)
        h = jpeg.parse(data)
        assert int(h.segments[0, 1] - h.segments[0, 0]) >= jpeg.AUTO_THRESHOLD
        want = golden_rgb(name)[..., ::-1]
        results = {}
        for mode in jpeg.ENTROPY_MODES:
            t = []
            frames, status, coef = jpeg.decode([data], dev(), timings=t, entropy=mode, return_coefficients=True)
            assert stages(t) == (["entropy", "idct", "colour"] if mode == "serial" else parallel), mode
            assert int(status.cpu()[0]) == 0 and np.array_equal(frames[0].cpu().numpy(), want), (name, mode)
            results[mode] = coef
        assert torch.equal(results["auto"], results["serial"]) and torch.equal(results["parallel"], results["serial"])
        frames, status = jpeg.decode([data], dev())          # and without timings: one call for all launches
        assert int(status.cpu()[0]) == 0 and np.array_equal(frames[0].cpu().numpy(), want)
    # two rounds, each with its own launches
    files = [file("p420"), file("p420opt")]
    t = []
    frames, status = jpeg.decode(files, dev(), timings=t, chunk=1)
    assert stages(t) == parallel * 2 and status.cpu().tolist() == [0, 0]
    assert np.array_equal(frames.cpu().numpy(), np.stack([golden_rgb(n) for n in ("p420", "p420opt")])[..., ::-1])
