"""A numpy restatement of the baseline JPEG reader (pmce_amd/jpeg.py, csrc/jpeg.hip), written from ITU-T T.81 and from the integer
rules that libjpeg's default decoder follows (jidctint "islow", the "fancy" chroma upsampling of jdsample, the fixed-point colour
conversion of jdcolor) - not from the device code.  Pure Python loops over bits: for the tests' small files only.

    info, coef, status = entropy_decode(data)        # coefficients int16 [blocks, 64], natural order, blocks in scan (MCU) order
    rgb, status = decode(data)                       # uint8 [H, W, 3] (a grey file: its plane in all three channels)
    data = encode(rgb_or_grey, quality=75, subsampling="420" | "444" | "grey", restart_interval=0)

The encoder (float DCT, Annex K's tables) exists to synthesise files where no JPEG library is installed, and for cases a library
does not make; its files need match nothing but ``decode`` of them.

An Exif orientation tag is not read: ``cv2.imread`` would rotate such a file, this reader (like the device's) does not.
"""
import numpy as np

STATUS_TRUNCATED, STATUS_CORRUPT = 1, 2

# ZIGZAG[k]: the natural (row-major) index of the k-th coefficient in zigzag order (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])

# T.81 Annex K: the example quantisation tables (natural order) and the typical Huffman tables (counts per length 1..16, values)
K_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                     87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                     101, 72, 92, 95, 98, 112, 100, 103, 99])
K_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                       99, 99, 99, 99] + [99] * 32)
K_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
K_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
K_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
             [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
              240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
              213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
              249, 250])
K_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
               [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
                240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
                69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
                120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
                165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
                210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247,
                248, 249, 250])


# ---------------------------------------------------------------------------------------------------------------------------------
# markers
# ---------------------------------------------------------------------------------------------------------------------------------
def read_markers(data: bytes) -> dict:
    """Walk the segments up to SOS.  -> dict(width, height, comps=[(id, h, v, tq)], scan=[(component index, td, ta)], quant={id:
    int[64] natural order}, huff={(class, id): (counts, values)}, restart_interval, scan_begin)."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    out = dict(quant={}, huff={}, restart_interval=0)
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected"
        while data[i + 1] == 0xFF:
            i += 1
        m = data[i + 1]
        L = (data[i + 2] << 8) | data[i + 3]
        body = data[i + 4:i + 2 + L]
        if m == 0xDB:
            p = 0
            while p < len(body):
                assert body[p] >> 4 == 0, "16-bit quantisation table"
                q = np.zeros(64, dtype=np.int64)
                q[ZIGZAG] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8)
                out["quant"][body[p] & 15] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                counts = list(body[p + 1:p + 17])
                n = sum(counts)
                out["huff"][(body[p] >> 4, body[p] & 15)] = (counts, list(body[p + 17:p + 17 + n]))
                p += 17 + n
        elif m in (0xC0, 0xC1):
            assert body[0] == 8
            out["height"], out["width"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]
        elif m == 0xDD:
            out["restart_interval"] = (body[0] << 8) | body[1]
        elif m == 0xDA:
            ids = [c[0] for c in out["comps"]]
            out["scan"] = [(ids.index(body[1 + 2 * c]), body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            out["scan_begin"] = i + 2 + L
            return out
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError(f"SOF{m - 0xC0} is not baseline")
        i += 2 + L


# ---------------------------------------------------------------------------------------------------------------------------------
# entropy decoding (T.81 Annex F.2.2)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Huff:
    """HUFFSIZE / HUFFCODE (T.81 Annex C) as a dictionary (length, code) -> value."""

    def __init__(self, counts, values):
        self.codes = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                self.codes[(length, code)] = values[k]
                code += 1
                k += 1
            code <<= 1


class _Bits:
    """The bits of one entropy-coded segment [begin, end): a stuffed 00 after FF is dropped; beyond the end come zero bits."""

    def __init__(self, data, begin, end):
        self.data, self.pos, self.end = data, begin, end
        self.cur, self.left, self.status = 0, 0, 0

    def bit(self):
        if self.left == 0:
            if self.pos >= self.end:
                self.status |= STATUS_TRUNCATED
                self.cur = 0
            else:
                self.cur = self.data[self.pos]
                self.pos += 1
                if self.cur == 0xFF:
                    if self.pos >= self.end:
                        self.status |= STATUS_TRUNCATED
                        self.cur = 0
                    elif self.data[self.pos] == 0:
                        self.pos += 1
                    else:
                        self.status |= STATUS_CORRUPT       # a marker inside the segment
                        self.cur, self.pos = 0, self.end
            self.left = 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table.codes:
                return table.codes[(length, code)]
        self.status |= STATUS_CORRUPT
        return None


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def scan_segments(data, info):
    """[(begin, end, first MCU, MCU count)] of the scan: one per restart interval; the scan ends at the first marker that is no RSTn."""
    n_mcu = info["mcus_x"] * info["mcus_y"]
    ri = info["restart_interval"] or n_mcu
    segs, begin, i, mcu = [], info["scan_begin"], info["scan_begin"], 0
    while True:
        if i + 1 >= len(data):
            segs.append((begin, len(data), mcu, min(ri, n_mcu - mcu)))
            break
        if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF):
            segs.append((begin, i, mcu, min(ri, n_mcu - mcu)))
            if not 0xD0 <= data[i + 1] <= 0xD7:
                break
            mcu += ri
            begin = i = i + 2
            continue
        i += 1
    return segs


def geometry(m):
    """Sampling and MCU grid from the markers' dictionary (added to it)."""
    comps = m["comps"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        hmax = vmax = 1           # a single-component scan is not interleaved: its MCU is one block whatever the factors say
        m["comps"] = comps = [(comps[0][0], 1, 1, comps[0][3])]
    m.update(hmax=hmax, vmax=vmax, mcus_x=-(-m["width"] // (8 * hmax)), mcus_y=-(-m["height"] // (8 * vmax)))
    return m


def entropy_decode(data: bytes):
    """-> (info, coefficients int16 [blocks, 64] in natural order - blocks in the order of the scan: MCU by MCU, inside an MCU per
    component v rows of h blocks - and the OR of the status bits)."""
    m = geometry(read_markers(data))
    per_mcu = sum(m["comps"][ci][1] * m["comps"][ci][2] for ci, _, _ in m["scan"])
    coef = np.zeros((m["mcus_x"] * m["mcus_y"] * per_mcu, 64), dtype=np.int16)
    tables = {k: _Huff(*v) for k, v in m["huff"].items()}
    status = 0
    for begin, end, mcu0, count in scan_segments(data, m):
        bits = _Bits(data, begin, end)
        pred = [0] * len(m["comps"])
        ok = True
        for mcu in range(mcu0, mcu0 + count):
            b = mcu * per_mcu
            for ci, td, ta in m["scan"]:
                for _ in range(m["comps"][ci][1] * m["comps"][ci][2]):
                    ok = _block(bits, tables[(0, td)], tables[(1, ta)], pred, ci, coef[b])
                    b += 1
                    if not ok:
                        break
                if not ok:
                    break
            if not ok or bits.status:
                break
        status |= bits.status
    m["blocks_per_mcu"] = per_mcu
    return m, coef, status


def _block(bits, dc, ac, pred, ci, out):
    s = bits.symbol(dc)
    if s is None or s > 15:
        bits.status |= STATUS_CORRUPT
        return False
    pred[ci] += _extend(bits.receive(s), s)
    out[0] = pred[ci]
    k = 1
    while k < 64:
        rs = bits.symbol(ac)
        if rs is None:
            return False
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        if k > 63:
            bits.status |= STATUS_CORRUPT
            return False
        out[ZIGZAG[k]] = _extend(bits.receive(s), s)
        k += 1
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# dequantisation + inverse DCT: libjpeg's jidctint ("islow"), CONST_BITS = 13, PASS1_BITS = 2
# ---------------------------------------------------------------------------------------------------------------------------------
def _fix(x):
    return int(round(x * 8192))


F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = (_fix(v) for v in (0.298631336, 0.390180644, 0.541196100, 0.765366865,
                                                                           0.899976223, 1.175875602))
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = (_fix(v) for v in (1.501321110, 1.847759065, 1.961570560, 2.053119869,
                                                                           2.562915447, 3.072711026))


def _idct_1d(x, shift):
    """x int64 [..., 8] along the last axis -> the eight outputs, descaled by ``shift`` with rounding."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 - z3 * F_1_847
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, quant):
    """coef int [n, 64] natural order, quant int [64] natural order -> uint8 [n, 8, 8]."""
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(-1, 8, 8)
    ws = _idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)        # pass 1: down the columns
    px = _idct_1d(ws, 18)                                             # pass 2: along the rows
    return np.clip(px + 128, 0, 255).astype(np.uint8)


def planes_from_coefficients(m, coef):
    """One uint8 plane per component, at the component's own resolution, padded to whole blocks."""
    per_mcu = m["blocks_per_mcu"]
    planes, first = [], 0
    for ci, _, _ in m["scan"]:
        _, h, v, tq = m["comps"][ci]
        plane = np.zeros((m["mcus_y"] * v * 8, m["mcus_x"] * h * 8), dtype=np.uint8)
        idx = (np.arange(m["mcus_x"] * m["mcus_y"])[:, None] * per_mcu + first + np.arange(h * v)[None]).reshape(-1)
        px = idct_blocks(coef[idx], m["quant"][tq]).reshape(m["mcus_y"], m["mcus_x"], v, h, 8, 8)
        plane[:] = px.transpose(0, 2, 4, 1, 3, 5).reshape(plane.shape)
        planes.append(plane)
        first += h * v
    return planes


# ---------------------------------------------------------------------------------------------------------------------------------
# chroma upsampling (jdsample's "fancy" forms) and colour conversion (jdcolor)
# ---------------------------------------------------------------------------------------------------------------------------------
def _h2_row(s, first_bias, second_bias, shift, edge_scale):
    """One row of column values s [cw] -> [2 cw]: 3/4 of the nearer value plus 1/4 of the further one; the two end samples see only
    their own column."""
    cw = len(s)
    out = np.empty(2 * cw, dtype=np.int64)
    prev, nxt = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    out[0::2] = (3 * s + prev + first_bias) >> shift
    out[1::2] = (3 * s + nxt + second_bias) >> shift
    out[0] = (edge_scale * s[0] + first_bias) >> shift
    out[-1] = (edge_scale * s[-1] + second_bias) >> shift
    return out


def upsample(plane, W, H, h, v):
    """A chroma plane (padded) of an image W x H whose luma is sampled h x v -> int64 [H, W].  Only the real extent ceil(W / h) x
    ceil(H / v) is read.  Planes of two columns or fewer are replicated, as jdsample does for them."""
    cw, ch = -(-W // h), -(-H // v)
    c = plane[:ch, :cw].astype(np.int64)
    if h == 1 and v == 1:
        return c[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(c, v, axis=0), h, axis=1)[:H, :W]
    out = np.empty((ch * v, 2 * cw), dtype=np.int64)
    for y in range(ch * v):
        if v == 1:
            row = c[y]
            out[y, 0::2] = (3 * row + np.concatenate([row[:1], row[:-1]]) + 1) >> 2
            out[y, 1::2] = (3 * row + np.concatenate([row[1:], row[-1:]]) + 2) >> 2
            out[y, 0], out[y, -1] = row[0], row[-1]
        else:
            cy = y >> 1
            far = min(max(cy + (1 if y & 1 else -1), 0), ch - 1)
            out[y] = _h2_row(3 * c[cy] + c[far], 8, 7, 4, 4)
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes):
    """-> (uint8 [H, W, 3] in R, G, B order, status)."""
    m, coef, status = entropy_decode(data)
    planes = planes_from_coefficients(m, coef)
    W, H = m["width"], m["height"]
    if len(planes) == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2), status
    h, v = m["hmax"], m["vmax"]
    return ycc_to_rgb(planes[0][:H, :W], upsample(planes[1], W, H, h, v), upsample(planes[2], W, H, h, v)), status


# ---------------------------------------------------------------------------------------------------------------------------------
# a small baseline encoder
# ---------------------------------------------------------------------------------------------------------------------------------
def _scaled_quant(base, quality):
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def _dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None]
    c = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    c[0] /= np.sqrt(2.0)
    return c


def _quantised_blocks(plane, quant):
    """plane float [8 by, 8 bx] -> int [by, bx, 64] in zigzag order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128.0
    C = _dct_matrix()
    freq = np.einsum("ui,abij,vj->abuv", C, blocks, C).reshape(by, bx, 64)
    return np.clip(np.rint(freq / quant), -1023, 1023).astype(np.int64)[..., ZIGZAG]      # the ten bits Annex K's AC tables code


def _pad_edge(plane, height, width):
    return np.pad(plane, ((0, height - plane.shape[0]), (0, width - plane.shape[1])), mode="edge")


def _codes(counts, values):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def encode(image, quality=75, subsampling="420", restart_interval=0) -> bytes:
    """uint8 [H, W, 3] (R, G, B) or [H, W] -> a baseline JFIF file.  ``subsampling``: "420", "444", or "grey" (implied by a 2-D image).
    Chroma is subsampled by the mean of 2 x 2; ``restart_interval`` is in MCUs (0: no DRI, no markers)."""
    image = np.asarray(image)
    if image.ndim == 2:
        subsampling = "grey"
    H, W = image.shape[:2]
    if subsampling == "grey":
        planes = [(image if image.ndim == 2 else image[..., 0]).astype(np.float64)]
        h = v = 1
    else:
        r, g, b = (image[..., i].astype(np.float64) for i in range(3))
        planes = [0.299 * r + 0.587 * g + 0.114 * b, -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128.0,
                  0.5 * r - 0.418687589 * g - 0.081312411 * b + 128.0]
        h = v = 2 if subsampling == "420" else 1
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    quants = [_scaled_quant(K_LUMA_Q, quality), _scaled_quant(K_CHROMA_Q, quality)]
    blocks = []
    for i, p in enumerate(planes):
        if i and h == 2:
            p = _pad_edge(p, 2 * -(-H // 2), 2 * -(-W // 2))
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0
        hc, vc = (h, v) if i == 0 else (1, 1)
        p = _pad_edge(p, my * vc * 8, mx * hc * 8)
        blocks.append(_quantised_blocks(np.clip(np.rint(p), 0, 255), quants[min(i, 1)]))
    dc = [_codes(*K_DC_LUMA), _codes(*K_DC_CHROMA)]
    ac = [_codes(*K_AC_LUMA), _codes(*K_AC_CHROMA)]

    out = bytearray(b"\xff\xd8")
    out += _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(min(len(planes), 2)):
        out += _segment(0xDB, bytes([t]) + bytes(int(x) for x in quants[t][ZIGZAG]))
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(planes)])
    for i in range(len(planes)):
        sof += bytes([i + 1, ((h << 4) | v) if i == 0 else 0x11, min(i, 1)])
    out += _segment(0xC0, sof)
    for t, (cls, tab) in enumerate(((0, K_DC_LUMA), (1, K_AC_LUMA), (0, K_DC_CHROMA), (1, K_AC_CHROMA))[:2 * min(len(planes), 2)]):
        out += _segment(0xC4, bytes([(cls << 4) | (t >> 1)]) + bytes(tab[0]) + bytes(tab[1]))
    if restart_interval:
        out += _segment(0xDD, int(restart_interval).to_bytes(2, "big"))
    sos = bytes([len(planes)])
    for i in range(len(planes)):
        sos += bytes([i + 1, (min(i, 1) << 4) | min(i, 1)])
    out += _segment(0xDA, sos + b"\x00\x3f\x00")

    w = _Writer()
    pred = [0] * len(planes)
    n_rst = 0
    for mcu in range(mx * my):
        if restart_interval and mcu and mcu % restart_interval == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (n_rst & 7)])
            n_rst += 1
            pred = [0] * len(planes)
        my_, mx_ = divmod(mcu, mx)
        for i in range(len(planes)):
            hc, vc = (h, v) if i == 0 else (1, 1)
            for by in range(vc):
                for bx in range(hc):
                    zz = blocks[i][my_ * vc + by, mx_ * hc + bx]
                    t = min(i, 1)
                    diff = int(zz[0]) - pred[i]
                    pred[i] = int(zz[0])
                    s = abs(diff).bit_length()
                    w.put(*dc[t][s])
                    if s:
                        w.put(diff if diff > 0 else diff + (1 << s) - 1, s)
                    run = 0
                    nz = np.nonzero(zz[1:])[0] + 1
                    last = 0
                    for k in nz:
                        run = int(k) - last - 1
                        while run > 15:
                            w.put(*ac[t][0xF0])
                            run -= 16
                        val = int(zz[k])
                        s = abs(val).bit_length()
                        w.put(*ac[t][(run << 4) | s])
                        w.put(val if val > 0 else val + (1 << s) - 1, s)
                        last = int(k)
                    if last != 63:
                        w.put(*ac[t][0x00])
    w.flush()
    return bytes(out) + bytes(w.out) + b"\xff\xd9"
