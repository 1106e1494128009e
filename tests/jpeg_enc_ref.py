"""A numpy restatement of the baseline JPEG writer (pmce_amd/jpeg.py ``encode``, csrc/jpeg_encode.hip), written from ITU-T T.81 and
from the integer rules of libjpeg's default compressor (jccolor's fixed-point conversion, jcsample's h2v1 / h2v2 box filter with its
alternating bias, jccoefct's dummy blocks, jfdctint "islow", the quantiser's rounding division, jchuff with Annex K's tables) - not
from the device code.  Pure Python loops over blocks: for the tests' small images only.

    coef = coefficients(rgb, quality, subsampling)        # int16 [blocks, 64], zigzag order, blocks in scan (MCU) order, dummies included
    scan = entropy_code(coef, geometry, restart_interval) # the scan's bytes: stuffed, padded, RSTn markers inside, no EOI
    data = encode(rgb, quality=95, subsampling="4:2:0", restart_interval=0)        # the whole file

The header is the product's own host function (``jpeg.encode_header``); tests/test_jpeg_enc_host.py pins it to Pillow's bytes.
"""
import numpy as np

from jpeg_ref import K_AC_CHROMA, K_AC_LUMA, K_CHROMA_Q, K_DC_CHROMA, K_DC_LUMA, K_LUMA_Q, ZIGZAG, _codes
from pmce_amd.jpeg import encode_header

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
MAX_BLOCK_BYTES = 208              # a block's code before stuffing: 20 bits of DC, 63 x 26 bits of AC


def quant_table(base, quality):
    """jpeg_set_quality(quality, force_baseline) on one of Annex K's tables (natural order)."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, dtype=np.int64) * s + 50) // 100, 1, 255)


def geometry(width, height, subsampling):
    h, v = SAMPLING[subsampling]
    g = dict(width=width, height=height, h=h, v=v, mcus_x=-(-width // (8 * h)), mcus_y=-(-height // (8 * v)), blocks_per_mcu=h * v + 2)
    g["luma_blocks"] = (-(-width // 8), -(-height // 8))                 # width_in_blocks, height_in_blocks of the luma component
    g["n_blocks"] = g["mcus_x"] * g["mcus_y"] * g["blocks_per_mcu"]
    return g


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    for p in (y, cb, cr):
        assert p.min() >= 0 and p.max() <= 255
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def component_planes(rgb, g):
    """The three planes as the DCT reads them: luma padded to its real blocks; chroma padded on the INPUT side to the right
    (width_in_blocks * 8 * h samples) and at the bottom only to a multiple of v, downsampled, then the last downsampled row repeated."""
    H, W = rgb.shape[:2]
    h, v = g["h"], g["v"]
    y, cb, cr = ycc(rgb)
    wb, hb = g["luma_blocks"]
    planes = [_pad(y, hb * 8, wb * 8)]
    cwb, chb = g["mcus_x"], g["mcus_y"]                      # ceil(ceil(W / h) / 8) = ceil(W / 8h)
    for c in (cb, cr):
        c = _pad(c, -(-H // v) * v, cwb * 8 * h)
        if (h, v) == (2, 2):
            bias = 1 + (np.arange(cwb * 8) & 1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        elif (h, v) == (2, 1):
            bias = np.arange(cwb * 8) & 1
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        planes.append(_pad(c, chb * 8, cwb * 8))
    return planes


F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's butterfly on the last axis of d [..., 8]; ``first``: the row pass (scaled up by 2^2), else the column pass."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F["f0_541"]
    out[2] = _descale(z1 + t13 * F["f0_765"], n)
    out[6] = _descale(z1 - t12 * F["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1_175"]
    t4, t5, t6, t7 = t4 * F["f0_298"], t5 * F["f2_053"], t6 * F["f3_072"], t7 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    for o in out:                                           # 32-bit integers suffice for 8-bit samples; the row pass fits int16
        assert np.abs(o).max() < (1 << 15 if first else 1 << 31)
    for k in (2, 6, 7, 5, 3, 1):                            # (the products before the descale, bounded through their result)
        assert np.abs(out[k]).max() < (1 << (31 - n))
    return np.stack(out, -1)


def quantise(c, table):
    """c: coefficients scaled by 8, natural order [..., 64]; table [64] -> sign(c) * ((|c| + (qv >> 1)) / qv), qv = 8 * table."""
    qv = 8 * np.asarray(table, dtype=np.int64)
    q = (np.abs(c) + (qv >> 1)) // qv
    return np.where(c < 0, -q, q)


def plane_blocks(plane, table):
    """int plane [8 by, 8 bx] -> quantised int64 [by, bx, 64] in zigzag order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128
    rows = _fdct_1d(blocks, True)
    cols = _fdct_1d(rows.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    return quantise(cols.reshape(by, bx, 64), table)[..., ZIGZAG]


def coefficients(rgb, quality=95, subsampling="4:2:0"):
    """uint8 [H, W, 3] (R, G, B) -> (int16 [blocks, 64] zigzag order, scan order, geometry).  A dummy block (beyond the luma
    component's real blocks) has zero AC and the DC of the block before it in the MCU; a whole dummy row that of the last block
    before the row (jccoefct.c)."""
    rgb = np.asarray(rgb)
    g = geometry(rgb.shape[1], rgb.shape[0], subsampling)
    tables = [quant_table(K_LUMA_Q, quality), quant_table(K_CHROMA_Q, quality)]
    planes = component_planes(rgb, g)
    comp = [plane_blocks(planes[0], tables[0]), plane_blocks(planes[1], tables[1]), plane_blocks(planes[2], tables[1])]
    h, v, wb, hb = g["h"], g["v"], *g["luma_blocks"]
    out = np.zeros((g["n_blocks"], 64), dtype=np.int64)
    b = 0
    for my in range(g["mcus_y"]):
        for mx in range(g["mcus_x"]):
            first = b
            for by in range(v):
                row_first = b
                for bx in range(h):
                    y, x = my * v + by, mx * h + bx
                    if y < hb and x < wb:
                        out[b] = comp[0][y, x]
                    elif y < hb:
                        out[b, 0] = out[b - 1, 0]
                    else:
                        out[b, 0] = out[row_first - 1, 0]
                    b += 1
                assert row_first >= first
            out[b], out[b + 1] = comp[1][my, mx], comp[2][my, mx]
            b += 2
    assert np.abs(out[:, 0]).max() <= 2047 and np.abs(out[:, 1:]).max() <= 1023
    return out.astype(np.int16), g


class Bits:
    def __init__(self, stuff=True):
        self.out, self.acc, self.n, self.stuff, self.bits = bytearray(), 0, 0, stuff, 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length
        self.bits += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF and self.stuff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


DC_CODES = [_codes(*K_DC_LUMA), _codes(*K_DC_CHROMA)]
AC_CODES = [_codes(*K_AC_LUMA), _codes(*K_AC_CHROMA)]


def _value(w, v):
    s = abs(v).bit_length()
    if s:
        w.put(v if v > 0 else v + (1 << s) - 1, s)


def code_block(w, zz, pred, t):
    """One block (zigzag order) into the writer; t: 0 luma, 1 chroma tables.  -> the block's DC."""
    diff = int(zz[0]) - pred
    code, length = DC_CODES[t][abs(diff).bit_length()]
    w.put(code, length)
    _value(w, diff)
    run = 0
    for k in range(1, 64):
        val = int(zz[k])
        if val == 0:
            run += 1
            continue
        while run > 15:
            w.put(*AC_CODES[t][0xF0])
            run -= 16
        w.put(*AC_CODES[t][(run << 4) | abs(val).bit_length()])
        _value(w, val)
        run = 0
    if run:
        w.put(*AC_CODES[t][0x00])
    return int(zz[0])


def entropy_code(coef, luma_blocks_per_mcu, restart_interval=0):
    """coef int [blocks, 64] (zigzag, scan order; an MCU is ``luma_blocks_per_mcu`` luma blocks, Cb, Cr) -> the scan's bytes."""
    bpm = luma_blocks_per_mcu + 2
    assert len(coef) % bpm == 0
    w = Bits()
    pred = [0, 0, 0]
    for mcu in range(len(coef) // bpm):
        if restart_interval and mcu and mcu % restart_interval == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + ((mcu // restart_interval - 1) & 7)])
            pred = [0, 0, 0]
        for k in range(bpm):
            c = 0 if k < luma_blocks_per_mcu else k - luma_blocks_per_mcu + 1
            pred[c] = code_block(w, coef[mcu * bpm + k], pred[c], min(c, 1))
    w.flush()
    return bytes(w.out)


def unstuffed(coef, luma_blocks_per_mcu):
    """One interval, before stuffing -> (bytes, the bit offset at which each block begins, with the total at the end)."""
    bpm = luma_blocks_per_mcu + 2
    w = Bits(stuff=False)
    pred, starts = [0, 0, 0], []
    for b in range(len(coef)):
        k = b % bpm
        c = 0 if k < luma_blocks_per_mcu else k - luma_blocks_per_mcu + 1
        starts.append(w.bits)
        pred[c] = code_block(w, coef[b], pred[c], min(c, 1))
    starts.append(w.bits)
    w.flush()
    return bytes(w.out), starts


def crafted_coefficients():
    """Valid coefficients (zigzag order, MCUs of one luma block, Cb, Cr) at the coder's edges -> int16 [27, 64]: DC differences of
    +-2047, AC of +-1023, runs of 15, 16, 32 and 48 zeros, coefficient 63 non-zero, all-zero blocks, and blocks of nothing but 1023 -
    26 bits each that begin with 0xFF, so that 0xFF bytes fall at every place in a word and across the borders of blocks and pieces."""
    c = np.zeros((27, 64), dtype=np.int16)
    c[0, 0], c[3, 0], c[6, 0], c[9, 0] = 1023, -1024, 1023, 0             # luma: +1023, -2047, +2047, -1023
    c[1, 0], c[4, 0], c[7, 0] = -1024, 1023, -1024                          # Cb: -1024, +2047, -2047
    c[0, 1], c[0, 2], c[0, 63] = 1023, -1023, 1                             # no EOB
    c[1, 16] = -1                                                           # a run of 15
    c[2, 17] = 5                                                            # of 16: one ZRL
    c[3, 33], c[3, 50] = -300, 2                                            # of 32: two ZRL, then of 16
    c[4, 49], c[4, 63] = 1023, -1023                                        # of 48: three ZRL; the last coefficient
    c[5, 1:] = -1                                                           # (block 8 stays all zero, as do 10 and 11)
    c[6, 1:] = 1023
    c[7, 1:] = 1023
    c[12:24, 1:] = 1023
    c[12:24, 0] = np.array([1023, 1023, -1024] * 4)
    c[24, 63] = -1023                                                       # a run of 62: three ZRL and run 14
    c[25, 5], c[26, 62] = 1, 1
    return c


def encode(rgb, quality=95, subsampling="4:2:0", restart_interval=0) -> bytes:
    rgb = np.asarray(rgb)
    coef, g = coefficients(rgb, quality, subsampling)
    return (encode_header(g["width"], g["height"], quality, subsampling, restart_interval)
            + entropy_code(coef, g["h"] * g["v"], restart_interval) + b"\xff\xd9")
