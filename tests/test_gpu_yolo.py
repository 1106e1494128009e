"""GPU tests of the detector as a network (pmce_amd/yolo.py on csrc/yolo.cpp) against the plain torch module of tests/yolo_ref.py run on
the CPU in fp32 and fp64: a mini spec of the same layer kinds (S = 64, grids 2 / 4 / 8, nc = 2; body convolutions with Cin = 24 and 12,
both concatenations, residual stages of two blocks) at n = 1, 3, 5, and the full yolov3 spec at S = 96 (grids 3 / 6 / 12), n = 2, with
drawn weights.  The rule: max |device - ref64| <= 4 x dev32, dev32 = max |ref32 - ref64|, per raw map and per group of decoded columns
(printed; run with -s).  Invariances are to the bit."""
import numpy as np
import pytest
import torch

import yolo_ref as YR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0


def Y():
    from pmce_amd import yolo
    return yolo


def bits(t):
    return t.contiguous().view(torch.int32)


def judge(got, ref32, ref64, what):
    dev32 = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    print(f"{what}: {err / dev32 if dev32 else float('inf'):.2f} x dev32 ({dev32:.2e}), max |ref| {float(ref64.abs().max()):.3g}")
    assert dev32 > 0
    assert err <= FACTOR * dev32


def judge_all(rows, maps, ref, n, nc, what):
    (maps32, rows32), (maps64, rows64) = ref
    for k in range(3):
        judge(maps[k].cpu(), maps32[k][:n], maps64[k][:n], f"{what} n={n} map {k}")
    rows = rows.cpu()
    for name, sl in (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf_cls", slice(4, 5 + nc))):
        judge(rows[..., sl], rows32[:n, :, sl], rows64[:n, :, sl], f"{what} n={n} rows {name}")


def reference(spec, sd, images):
    with torch.no_grad():
        return YR.make_module(spec, sd)(images), YR.make_module(spec, sd, torch.float64)(images.double())


@pytest.fixture(scope="module")
def mini():
    spec = YR.mini_spec()
    sd = YR.draw_state_dict(spec)
    images = YR.draw_images(5, YR.MINI_SIDE)
    return {"spec": spec, "sd": sd, "images": images, "ref": reference(spec, sd, images),
            "det": Y().YOLOv3.from_state_dict(sd, DEV, spec=spec, max_batch=5)}


@pytest.fixture(scope="module")
def mini_out(mini):
    rows, maps = mini["det"].forward(mini["images"].to(DEV), return_maps=True)
    torch.cuda.synchronize()
    return rows.clone(), [m.clone() for m in maps]


def test_mini_spec_has_the_shapes_the_kernels_branch_on(mini):
    table = Y().conv_table(mini["spec"])
    assert any(s[1] % 16 and i for i, s, _, _, _ in table) and sum(l["kind"] == "route" and len(l["layers"]) == 2 for l in mini["spec"]["layers"]) == 2
    assert Y().grids(mini["spec"], 64) == [2, 4, 8] and mini["spec"]["num_classes"] == 2
    assert Y().layer_shapes(mini["spec"])[-1][0] == 21


@pytest.mark.parametrize("n", [1, 3, 5])
def test_mini_against_the_reference_module(mini, n):
    rows, maps = mini["det"].forward(mini["images"][:n].to(DEV), return_maps=True)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (n, 3 * (4 + 16 + 64), 7) and [tuple(m.shape) for m in maps] == [(n, 21, g, g) for g in (2, 4, 8)]
    judge_all(rows, maps, mini["ref"], n, 2, "mini")


def test_full_yolov3_at_96_against_the_reference_module():
    spec = Y().yolov3_spec()
    sd = YR.draw_state_dict(spec)
    images = YR.draw_images(2, 96)
    ref = reference(spec, sd, images)
    det = Y().YOLOv3.from_state_dict(sd, DEV, max_batch=2)
    rows, maps = det.forward(images.to(DEV), return_maps=True)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (2, 3 * (9 + 36 + 144), 85) and [tuple(m.shape) for m in maps] == [(2, 255, g, g) for g in (3, 6, 12)]
    judge_all(rows, maps, ref, 2, 80, "yolov3@96")


def test_batch_and_chunk_invariance_to_the_bit(mini, mini_out):
    rows5, maps5 = mini_out
    x = mini["images"].to(DEV)
    det2 = Y().YOLOv3.from_state_dict(mini["sd"], DEV, spec=mini["spec"], max_batch=2)       # chunks of 2, 2, 1
    rows2, maps2 = det2.forward(x, return_maps=True)
    assert torch.equal(bits(rows2), bits(rows5)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(maps2, maps5))
    for i in (0, 4):
        r1, m1 = mini["det"].forward(x[i:i + 1], return_maps=True)
        assert torch.equal(bits(r1), bits(rows5[i:i + 1])) and all(torch.equal(bits(a), bits(b[i:i + 1])) for a, b in zip(m1, maps5))


def test_repeated_calls_and_input_forms_are_bit_equal(mini, mini_out):
    rows5, _ = mini_out
    x = mini["images"]
    assert torch.equal(bits(mini["det"](x.to(DEV))), bits(rows5))                             # again
    assert torch.equal(bits(mini["det"](x)), bits(rows5))                                      # a host tensor
    wide = torch.zeros(5, 3, 64, 80, device=DEV)
    wide[..., 7:71] = x.to(DEV)
    assert torch.equal(bits(mini["det"](wide[..., 7:71])), bits(rows5))                        # rows with a pitch
    nhwc = x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous() and torch.equal(bits(mini["det"](nhwc)), bits(rows5))      # channels last
    rows0, maps0 = mini["det"].forward(torch.zeros(0, 3, 64, 64), return_maps=True)
    assert tuple(rows0.shape) == (0, 252, 7) and [tuple(m.shape) for m in maps0] == [(0, 21, g, g) for g in (2, 4, 8)]


def test_a_nan_image_is_named_and_a_bad_side_refused(mini):
    x = mini["images"].clone()
    x[3, 1, 20, 30] = float("nan")
    from pmce_amd import _lib
    with pytest.raises(_lib.PmceError, match="image 3 has non-finite"):
        mini["det"](x)
    with pytest.raises(ValueError, match="multiple of 32"):
        mini["det"](torch.zeros(1, 3, 100, 100))
    assert tuple(mini["det"](torch.rand(1, 3, 96, 96)).shape) == (1, 3 * (9 + 36 + 144), 7)    # another side on the same handle


def test_darknet_file_gives_the_bits_of_the_state_dict(mini, mini_out, tmp_path):
    path = str(tmp_path / "mini.weights")
    YR.write_darknet(path, mini["sd"], mini["spec"])
    det = Y().YOLOv3.from_darknet_weights(path, DEV, spec=mini["spec"], max_batch=5)
    assert torch.equal(bits(det(mini["images"])), bits(mini_out[0]))
    det = Y().YOLOv3.from_checkpoint(path, DEV, spec=mini["spec"], max_batch=3)
    assert torch.equal(bits(det(mini["images"])), bits(mini_out[0]))


def test_letterbox_then_forward_is_the_two_by_hand(mini):
    frames = np.random.default_rng(5).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    index = np.asarray([1, 0, 1])
    images, (pad_x, pad_y, ratio) = Y().letterbox(frames, index, size=64)
    assert (pad_x, pad_y, ratio) == (0, 8, 53 / 64)
    by_hand = torch.stack([YR.letterbox_torch(frames[i], 64) for i in index])
    assert torch.equal(images.cpu(), by_hand)
    assert torch.equal(bits(mini["det"](images)), bits(mini["det"](by_hand)))
    rows = mini["det"](images)
    assert torch.equal(bits(rows[0]), bits(rows[2])) and not torch.equal(rows[0], rows[1])
