"""GPU tests of the detector's operators (csrc/conv.hip's activation / pitch entry, csrc/yolo.hip) through pmce_amd/yolo.py.

Float cases follow the project's rule: max |device - ref64| <= 4 x dev32, dev32 = max |ref32 - ref64| of torch's own CPU run on the same
tensors (asserted > 0 and printed; run with -s).  Bit cases compare the new entry with the old one, a batch with its single images, the
pitched with the contiguous reading.  The upsample and the letterbox are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_ref as YR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0
SENTINEL = -7.25


def Y():
    from pmce_amd import yolo
    return yolo


def EX():
    from pmce_amd import extractor
    return extractor


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    return t.contiguous().view(torch.int32)


def judge(got, ref32, ref64, what):
    dev32 = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    print(f"{what}: {err / dev32 if dev32 else float('inf'):.2f} x dev32 ({dev32:.2e})")
    assert dev32 > 0
    assert err <= FACTOR * dev32


def sliced(t_nhwc, pitch, offset, fill=SENTINEL):
    """A device NHWC tensor stored as channels offset .. offset + C of a buffer of `pitch` channels -> (buffer, view)."""
    n, h, w, c = t_nhwc.shape
    buf = torch.full((n, h, w, pitch), fill, device=DEV, dtype=torch.float32)
    view = buf[..., offset:offset + c]
    view.copy_(t_nhwc)
    return buf, view


# name: (n, Cin, H, W, Cout, k, stride, act, residual (None / "before" / "after"), in pitch, out pitch, residual pitch)
CONV_CASES = {
    "m4_cout21_leaky": (1, 16, 2, 2, 21, 1, 1, "leaky", None, None, None, None),
    "m507_cout255_linear": (3, 32, 13, 13, 255, 1, 1, "none", None, None, None, None),
    "cin3_generic_leaky": (2, 3, 9, 9, 8, 3, 1, "leaky", None, None, None, None),
    "cin24_pitched_res_after": (2, 24, 7, 7, 12, 1, 1, "leaky", "after", 40, 36, 20),
    "s2_odd_side_res_before": (2, 16, 7, 7, 32, 3, 2, "leaky", "before", None, None, None),
    "res_after_dense": (2, 32, 6, 6, 64, 3, 1, "leaky", "after", None, None, None),
    "res_after_out_pitch": (2, 32, 6, 6, 64, 3, 1, "leaky", "after", None, 96, 96),
}


def ref_conv(x, w, b, res, stride, pad, act, order):
    v = F.conv2d(x, w, b, stride=stride, padding=pad)
    if res is not None and order == "before":
        v = v + res
    if act == "leaky":
        v = F.leaky_relu(v, 0.1)
    elif act == "relu":
        v = F.relu(v)
    if res is not None and order == "after":
        v = v + res
    return v


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_entry_against_fp64(case):
    n, cin, h, w_, cout, k, stride, act, order, ldx, ldo, ldr = CONV_CASES[case]
    seed = sum(map(ord, case))
    pad = (k - 1) // 2
    x, w, b = rnd((n, cin, h, w_), seed), rnd((cout, cin, k, k), seed + 1, (cin * k * k) ** -0.5), rnd((cout,), seed + 2, 0.5)
    oh = (h + 2 * pad - k) // stride + 1
    res = rnd((n, cout, oh, oh), seed + 3) if order else None
    ref64 = ref_conv(x.double(), w.double(), b.double(), None if res is None else res.double(), stride, pad, act, order)
    ref32 = ref_conv(x, w, b, res, stride, pad, act, order)
    planes, ws = EX().pack_conv(w.to(DEV))
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    if ldx:
        _, xd = sliced(xd, ldx, 8)
    rd = None
    if res is not None:
        rd = res.permute(0, 2, 3, 1).contiguous().to(DEV)
        if ldr:
            _, rd = sliced(rd, ldr, 4)
    out_buf = out = None
    if ldo:
        out_buf = torch.full((n, oh, oh, ldo), SENTINEL, device=DEV)
        out = out_buf[..., 16:16 + cout]
    got = Y().conv2d_act(xd, planes, ws, tuple(w.shape), b.to(DEV), rd, stride=stride, pad=pad, act=act, residual_after_act=order == "after",
                         out=out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, oh, oh, cout)
    judge(got.cpu().permute(0, 3, 1, 2), ref32, ref64, case)
    if ldo:                                      # the neighbouring slices of the wider buffer are untouched
        rest = torch.cat([out_buf[..., :16], out_buf[..., 16 + cout:]], -1)
        assert bool((rest == SENTINEL).all())


def test_conv_entry_with_relu_is_the_old_entry_to_the_bit():
    n, cin, side, cout = 2, 32, 9, 96
    x, w, b, res = rnd((n, side, side, cin), 1).to(DEV), rnd((cout, cin, 3, 3), 2, 0.1), rnd((cout,), 3).to(DEV), rnd((n, side, side, cout), 4).to(DEV)
    planes, ws = EX().pack_conv(w.to(DEV))
    for r in (None, res):
        for relu in (True, False):
            old = EX().conv2d(x, "nhwc", planes, ws, tuple(w.shape), b, r, stride=1, pad=1, relu=relu)
            new = Y().conv2d_act(x, planes, ws, tuple(w.shape), b, r, stride=1, pad=1, act="relu" if relu else "none", residual_after_act=False)
            torch.cuda.synchronize()
            assert torch.equal(bits(old), bits(new))
    after = Y().conv2d_act(x, planes, ws, tuple(w.shape), b, res, stride=1, pad=1, act="relu", residual_after_act=True)
    assert not torch.equal(after, old)           # the order of residual and activation is a real choice


def test_conv_entry_is_batch_invariant_to_the_bit():
    n, cin, side, cout = 5, 24, 7, 36           # 5 x 49 rows: images share and straddle the 128-row tiles; the generic gather
    x, w, b = rnd((n, side, side, cin), 5).to(DEV), rnd((cout, cin, 3, 3), 6, 0.1), rnd((cout,), 7).to(DEV)
    planes, ws = EX().pack_conv(w.to(DEV))
    _, res = sliced(rnd((n, side, side, cout), 8).to(DEV), 48, 4)
    out = torch.full((n, side, side, 64), SENTINEL, device=DEV)[..., 8:8 + cout]
    Y().conv2d_act(x, planes, ws, tuple(w.shape), b, res, stride=1, pad=1, act="leaky", residual_after_act=True, out=out)
    for i in range(n):
        one = Y().conv2d_act(x[i:i + 1], planes, ws, tuple(w.shape), b, res[i:i + 1], stride=1, pad=1, act="leaky", residual_after_act=True)
        assert torch.equal(bits(one), bits(out[i:i + 1])), i


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (13, 13)])
@pytest.mark.parametrize("c", [4, 128])
def test_upsample_into_a_slice(h, w, c):
    x = rnd((2, c, h, w), h * w + c)
    want = F.interpolate(x, scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    buf = torch.full((2, 2 * h, 2 * w, c + 12), SENTINEL, device=DEV)
    out = buf[..., 8:8 + c]
    Y().upsample2x(x.permute(0, 2, 3, 1).contiguous().to(DEV), out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert bool((buf[..., :8] == SENTINEL).all()) and bool((buf[..., 8 + c:] == SENTINEL).all())
    dense = Y().upsample2x(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    assert torch.equal(dense.cpu(), want)


DECODE_CASES = [(2, (2, 4, 8), 64), (80, (3, 6, 12), 96), (2, (3, 6, 12), 96), (80, (2, 4, 8), 64)]
SCALE_ANCHORS = [[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]]   # stride 32, 16, 8


@pytest.mark.parametrize("nc,gs,S", DECODE_CASES)
def test_decode_exact_cases(nc, gs, S):
    """All-zero logits: x = (gx + 0.5) stride, y alike, w, h = the anchor, conf = cls = 0.5, to the bit; the row order is scale, anchor,
    gy, gx.  Then one logit set per map tells the channel order."""
    n, E = 2, 5 + nc
    maps = [torch.zeros(n, g, g, 3 * E, device=DEV) for g in gs]
    rows = Y().decode(maps, SCALE_ANCHORS, nc, S).cpu()
    assert tuple(rows.shape) == (n, 3 * sum(g * g for g in gs), E)
    want = []
    for g, anc in zip(gs, SCALE_ANCHORS):
        stride = S / g
        for a in range(3):
            for gy in range(g):
                for gx in range(g):
                    want.append([(gx + 0.5) * stride, (gy + 0.5) * stride, anc[a][0], anc[a][1]] + [0.5] * (1 + nc))
    want = torch.tensor(want, dtype=torch.float32)
    assert torch.equal(bits(rows[0]), bits(want)) and torch.equal(bits(rows[1]), bits(want))
    # image 1, map 1, anchor 2, cell (gy 1, gx 0): a large class logit on the last class and a conf logit of -40
    g = gs[1]
    maps[1][1, 1, 0, 2 * E + 4] = -40.0
    maps[1][1, 1, 0, 2 * E + E - 1] = 40.0
    rows2 = Y().decode(maps, SCALE_ANCHORS, nc, S).cpu()
    r = 3 * gs[0] ** 2 + 2 * g * g + 1 * g + 0
    changed = (bits(rows2) != bits(rows)).nonzero().tolist()
    assert changed == [[1, r, 4], [1, r, E - 1]]
    assert float(rows2[1, r, E - 1]) == 1.0 and 0.0 < float(rows2[1, r, 4]) < 1e-17


@pytest.mark.parametrize("nc,gs,S", DECODE_CASES)
def test_decode_drawn_logits(nc, gs, S):
    n, E = 3, 5 + nc
    maps = [rnd((n, 3 * E, g, g), 100 * nc + g, 1.5) for g in gs]              # NCHW, as the reference module holds them
    ref32 = torch.cat([YR.decode_scale(m, a, nc, S) for m, a in zip(maps, SCALE_ANCHORS)], 1)
    ref64 = torch.cat([YR.decode_scale(m.double(), a, nc, S) for m, a in zip(maps, SCALE_ANCHORS)], 1)
    dense = [m.permute(0, 2, 3, 1).contiguous().to(DEV) for m in maps]
    got = Y().decode(dense, SCALE_ANCHORS, nc, S)
    pitched = [sliced(m, 3 * E + 9, 0)[1] for m in dense]
    got_p = Y().decode(pitched, SCALE_ANCHORS, nc, S)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(got_p))
    got = got.cpu()
    for name, sl in (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf_cls", slice(4, E))):
        judge(got[..., sl], ref32[..., sl], ref64[..., sl], f"nc={nc} g={gs} {name}")


LETTERBOX_CASES = [(1080, 1920, 416), (37, 53, 64), (48, 48, 32), (53, 38, 64)]


@pytest.mark.parametrize("H,W,S", LETTERBOX_CASES)
@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_letterbox_is_byte_exact(H, W, S, order):
    frames = np.random.default_rng(H * W + S).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    index = np.asarray([2, 0, 2, 1, 1], np.int64)
    pad_value = 0.5 if order == "bgr" else 0.0
    want = torch.stack([YR.letterbox_torch(frames[i], S, pad_value, swap_rb=order == "bgr") for i in index])
    dev_frames = torch.from_numpy(frames).to(DEV)
    for fi in (index, torch.from_numpy(index).to(DEV)):                        # a host table (validated) and a device table (trusted)
        got, (pad_x, pad_y, ratio) = Y().letterbox(dev_frames, fi, size=S, pad_value=pad_value, channel_order=order)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3, S, S)
        assert torch.equal((got.cpu() * 255).round().to(torch.uint8), (want * 255).round().to(torch.uint8))
        assert torch.equal(got.cpu(), want)
    d = abs(H - W)
    assert (pad_x, pad_y, ratio) == ((d // 2, 0, H / S) if H > W else (0, d // 2, W / S))
    empty, _ = Y().letterbox(dev_frames, np.zeros(0, np.int64), size=S)
    assert tuple(empty.shape) == (0, 3, S, S)
    with pytest.raises(ValueError, match="there are 3 frames"):
        Y().letterbox(dev_frames, np.asarray([3]), size=S)
