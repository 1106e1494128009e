"""The demo's frames from JPEG files, decoded on the GPU (csrc/jpeg.hip): what the reference does with ``cv2.imread`` four or more
times per frame (lib/utils/demo_utils.py:101-121 has ffmpeg write ``%06d.jpg``; main/run_demo.py:264-286, 392-395 and
lib/utils/_dataset_demo.py:60 read the files back), once, for a whole folder, into the uint8 [F, H, W, 3] tensor the demo's stages take.

    header = jpeg.parse(data, "000001.jpg")                     # host only: markers, tables, the scan's segments; refuses with ValueError
    frames, status = jpeg.decode([data0, data1, ...], device)   # uint8 [F, H, W, 3] in B, G, R (cv2's order), int32 [F]; no wait for the device
    frames, status = jpeg.decode(files, device, channel_order="rgb", chunk=32, out=preallocated)

Served: baseline Huffman JPEG (SOF0, and SOF1 with 8-bit samples), grey or YCbCr with luma sampling 1x1, 2x1 or 2x2 (4:4:4, 4:2:2,
4:2:0) in one interleaved scan, 8-bit quantisation tables, up to four DC and four AC Huffman tables, restart intervals.  The pixels
are those of libjpeg's default decoder, to the bit: "islow" inverse DCT, "fancy" chroma upsampling, jdcolor's
fixed-point conversion.  Refused, with a ValueError that names the file and the reason: progressive, lossless and arithmetic-coded
files, 12-bit samples, four components, 16-bit quantisation tables, an Adobe marker whose transform is not 1 on a three-component
file, any other sampling, more than one scan, DNL, a missing table, a width or height of 0 or above 16384, data that ends before SOS.

An Exif orientation tag is NOT read: ``cv2.imread`` would rotate such a file, this reader does not.  (ffmpeg's frames carry none.)

``status[f]`` is an OR of STATUS_TRUNCATED (the scan ended before its last MCU; zero bits are supplied beyond the end) and
STATUS_CORRUPT (a code of no table, a run past coefficient 63, a marker inside a restart interval); ``decode`` does not read it.
There is no fallback: without the library's kernels a call raises.

The way back (csrc/jpeg_encode.hip), what the reference does with ``cv2.imwrite`` twice per frame (main/run_demo.py:424-426):

    data, offsets, status = jpeg.encode(frames)                 # uint8 [F, H, W, 3] on the device -> baseline JFIF files on the device
    blobs = jpeg.files(data, offsets, status)                   # list[bytes]: the one host read
    header = jpeg.encode_header(width, height, quality, subsampling, restart_interval)      # host only

YCbCr 4:4:4, 4:2:2 or 4:2:0, quality 1..100, Annex K's Huffman tables, restart intervals; the files are those of libjpeg's default
compressor at the same settings, byte for byte.  Grey files, optimised or progressive tables and Exif are not written.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass, field

import numpy as np

from . import _lib

MAX_DIM = 16384
IMG_WORDS, SEG_WORDS, HUFF_WORDS = 24, 5, 546          # csrc/jpeg_entropy.hpp, include/pmce_hip.h
HUFF_MAXCODE, HUFF_VALOFF, HUFF_VALUES, HUFF_LOOK = 0, 17, 34, 290
STATUS_TRUNCATED, STATUS_CORRUPT, STATUS_RECORD = 1, 2, 4
CHANNEL_ORDERS = ("bgr", "rgb")
ENTROPY_MODES = ("auto", "serial", "parallel")
PARALLEL_RUN = 256                     # subsequences per workgroup of the parallel entropy stage (csrc/jpeg_parallel.hpp, RUN)
PARALLEL_STAGES = ("sync", "join", "join", "place", "write", "dc")       # its launches, as ``timings`` names them ("entropy_" in front)
MIN_SUBSEQUENCE, MAX_SUBSEQUENCE = 4, 1 << 16
DEFAULT_SUBSEQUENCE = 128              # bytes per lane of the parallel entropy stage: the fastest of the sweep in profiles/jpeg_bench.json
AUTO_THRESHOLD = 4096                  # "auto": a round whose longest segment has at least this many bytes takes the parallel stage
DUMP_MAGIC = b"PMCEJPG1"

_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC8: "a reserved frame type (JPG)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding, progressive (SOF10)", 0xCB: "arithmetic coding, lossless (SOF11)",
              0xCC: "arithmetic coding (DAC)", 0xCD: "arithmetic coding, differential (SOF13)",
              0xCE: "arithmetic coding, differential progressive (SOF14)", 0xCF: "arithmetic coding, differential lossless (SOF15)"}


@dataclass
class Header:
    """What ``parse`` found.  ``quant[c]``: uint16 [64] in zigzag order as stored; ``dc[c]`` / ``ac[c]``: (counts of the lengths 1..16,
    values) of component c's Huffman tables; ``segments``: int64 [n, 4] = (first byte, end byte, first MCU, MCU count), bytes counted
    from the start of the file, one row per restart interval (one row without DRI)."""
    name: str
    data: bytes
    width: int
    height: int
    ncomp: int
    h: int
    v: int
    mcus_x: int
    mcus_y: int
    restart_interval: int
    blocks_per_mcu: int
    scan_begin: int
    scan_end: int
    quant: list = field(default_factory=list)
    dc: list = field(default_factory=list)
    ac: list = field(default_factory=list)
    segments: np.ndarray = None

    @property
    def n_blocks(self) -> int:
        return self.mcus_x * self.mcus_y * self.blocks_per_mcu

    @property
    def plane_bytes(self) -> int:
        luma = (self.mcus_x * self.h * 8) * (self.mcus_y * self.v * 8)
        return luma + (2 * (self.mcus_x * 8) * (self.mcus_y * 8) if self.ncomp == 3 else 0)


def _refuse(name, why):
    raise ValueError(f"{name or '<bytes>'}: {why}")


def huffman_record(counts, values, name="") -> np.ndarray:
    """One table as the device reads it: int32 [546] = maxcode[17] | valoff[17] | values[256] | lookahead[256] (include/pmce_hip.h)."""
    rec = np.zeros(HUFF_WORDS, dtype=np.int32)
    rec[HUFF_MAXCODE:HUFF_MAXCODE + 17] = -1
    if sum(counts) > 256 or sum(counts) != len(values):
        _refuse(name, f"a Huffman table with {sum(counts)} codes and {len(values)} values")
    rec[HUFF_VALUES:HUFF_VALUES + len(values)] = np.frombuffer(bytes(values), dtype=np.uint8)
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            if code + n > (1 << length):
                _refuse(name, f"a Huffman table with more codes of {length} bits than there are")
            rec[HUFF_VALOFF + length] = k - code
            rec[HUFF_MAXCODE + length] = code + n - 1
            if length <= 8:
                for j in range(n):
                    lo = (code + j) << (8 - length)
                    rec[HUFF_LOOK + lo:HUFF_LOOK + lo + (1 << (8 - length))] = (length << 8) | values[k + j]
            code += n
            k += n
        code <<= 1
    return rec


def _scan_segments(data: bytes, scan_begin: int, n_mcu: int, restart_interval: int):
    """The scan's extent and its restart intervals, by one vectorised pass over the scan's bytes: every FF that is followed by neither 00
    (a stuffed byte) nor FF (a fill byte) begins a marker; RSTn markers split the scan, the first other marker ends it.  A scan with
    fewer intervals than its DRI promises (a file cut short) gets empty segments for the missing ones: the device reports them as
    truncated.  -> (segments int64 [n, 4], scan_end, the position of the marker that ended the scan or -1)."""
    a = np.frombuffer(data, dtype=np.uint8)[scan_begin:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, dtype=np.int64)
    nxt = a[ff + 1]
    marks = ff[(nxt != 0x00) & (nxt != 0xFF)]
    is_rst = (a[marks + 1] & 0xF8) == 0xD0
    other = np.flatnonzero(~is_rst)
    n_rst = int(other[0]) if len(other) else len(marks)
    end_marker = int(marks[n_rst]) if len(other) else -1
    scan_end = end_marker if end_marker >= 0 else len(a)
    expected = -(-n_mcu // restart_interval) if restart_interval else 1
    rst = marks[:min(n_rst, expected - 1)] if restart_interval else marks[:0]
    begins = np.concatenate([[0], rst + 2]).astype(np.int64)
    ends = np.concatenate([rst, [marks[0] if (not restart_interval and len(marks)) else scan_end]]).astype(np.int64)
    while len(a):                                 # fill bytes in front of a marker are not data (a data FF is followed by 00)
        fill = (ends > begins) & (a[np.maximum(ends - 1, 0)] == 0xFF)
        if not fill.any():
            break
        ends[fill] -= 1
    seg = np.zeros((expected, 4), dtype=np.int64)
    seg[:, 0] = seg[:, 1] = scan_end
    seg[:len(begins), 0], seg[:len(begins), 1] = begins, ends
    seg[:, :2] += scan_begin
    ri = restart_interval or n_mcu
    seg[:, 2] = np.arange(expected) * ri
    seg[:, 3] = np.minimum(ri, n_mcu - seg[:, 2])
    return seg, scan_begin + scan_end, (scan_begin + end_marker if end_marker >= 0 else -1)


def parse(data: bytes, name: str = "") -> Header:
    """Walk the markers of one file up to SOS and find the scan's extent -> ``Header``; ValueError (naming ``name`` and the reason) for
    anything this reader does not serve.  Host only.  An Exif orientation tag is not read (``cv2.imread`` would rotate such a file)."""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        _refuse(name, "not a JPEG file (no SOI marker)")
    quant, huff = {}, {}
    frame = scan = adobe = None
    restart = 0
    i = 2
    while scan is None:
        if i + 2 > n:
            _refuse(name, "the data ends before SOS")
        if data[i] != 0xFF:
            _refuse(name, f"a marker was expected at byte {i}")
        while i + 1 < n and data[i + 1] == 0xFF:      # fill bytes
            i += 1
        if i + 2 > n:
            _refuse(name, "the data ends before SOS")
        m = data[i + 1]
        if m == 0x01 or m == 0xD8 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m == 0xD9:
            _refuse(name, "the data ends before SOS (EOI)")
        if i + 4 > n:
            _refuse(name, "the data ends before SOS")
        L = (data[i + 2] << 8) | data[i + 3]
        if L < 2 or i + 2 + L > n:
            _refuse(name, "the data ends before SOS")
        body = data[i + 4:i + 2 + L]
        if m in _SOF_NAMES:
            _refuse(name, f"{_SOF_NAMES[m]} is not served, only baseline Huffman files")
        if m in (0xC0, 0xC1):
            if frame is not None:
                _refuse(name, "more than one frame header")
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                _refuse(name, "a frame header that is too short")
            if body[0] != 8:
                _refuse(name, f"{body[0]}-bit samples are not served, only 8-bit")
            height, width, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if nc == 4:
                _refuse(name, "4 components (CMYK / YCCK) are not served")
            if nc not in (1, 3):
                _refuse(name, f"{nc} components are not served, only 1 (grey) or 3 (YCbCr)")
            if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
                _refuse(name, f"a width or height of 0 or above {MAX_DIM} (got {width} x {height})")
            frame = dict(width=width, height=height, comps=[(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c])
                                                            for c in range(nc)])
        elif m == 0xDB:
            p = 0
            while p < len(body):
                if body[p] >> 4:
                    _refuse(name, "16-bit quantisation tables are not served")
                if (body[p] & 15) > 3 or p + 65 > len(body):
                    _refuse(name, "a malformed quantisation table")
                quant[body[p] & 15] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8).astype(np.uint16)
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body) or (body[p] >> 4) > 1 or (body[p] & 15) > 3:
                    _refuse(name, "a malformed Huffman table")
                counts = tuple(body[p + 1:p + 17])
                if p + 17 + sum(counts) > len(body):
                    _refuse(name, "a malformed Huffman table")
                huff[(body[p] >> 4, body[p] & 15)] = (counts, bytes(body[p + 17:p + 17 + sum(counts)]))
                p += 17 + sum(counts)
        elif m == 0xDD:
            if len(body) < 2:
                _refuse(name, "a malformed DRI segment")
            restart = (body[0] << 8) | body[1]
        elif m == 0xDC:
            _refuse(name, "DNL is not served")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if frame is None:
                _refuse(name, "SOS before the frame header")
            scan = body
            scan_begin = i + 2 + L
        i += 2 + L

    comps = frame["comps"]
    nc = len(comps)
    if nc == 3 and adobe is not None and adobe != 1:
        _refuse(name, f"an Adobe marker with transform {adobe} (not YCbCr) is not served")
    if len(scan) < 1 or scan[0] != nc or len(scan) < 1 + 2 * nc + 3:
        _refuse(name, f"a scan of {scan[0] if len(scan) else 0} of the {nc} components: more than one SOS is not served")
    if [scan[1 + 2 * c] for c in range(nc)] != [c[0] for c in comps]:
        _refuse(name, "the scan's components are not the frame's, in the frame's order")
    if (scan[1 + 2 * nc], scan[2 + 2 * nc], scan[3 + 2 * nc]) != (0, 63, 0):
        _refuse(name, "a scan that is not the whole spectrum at full precision (progressive parameters)")
    if nc == 1:
        h = v = 1                  # one component is never interleaved: its MCU is one block whatever the factors say
    else:
        h, v = comps[0][1], comps[0][2]
        if (h, v) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            _refuse(name, "sampling " + ", ".join(f"{c[1]}x{c[2]}" for c in comps) + " is not served, only 4:4:4, 4:2:2 and 4:2:0")
    hdr = Header(name=name, data=data, width=frame["width"], height=frame["height"], ncomp=nc, h=h, v=v,
                 mcus_x=-(-frame["width"] // (8 * h)), mcus_y=-(-frame["height"] // (8 * v)), restart_interval=restart,
                 blocks_per_mcu=1 if nc == 1 else h * v + 2, scan_begin=scan_begin, scan_end=scan_begin)
    for c in range(nc):
        td, ta = scan[2 + 2 * c] >> 4, scan[2 + 2 * c] & 15
        if comps[c][3] not in quant:
            _refuse(name, f"quantisation table {comps[c][3]} is referenced but not defined")
        if (0, td) not in huff or (1, ta) not in huff:
            _refuse(name, f"Huffman table {'DC ' + str(td) if (0, td) not in huff else 'AC ' + str(ta)} is referenced but not defined")
        hdr.quant.append(quant[comps[c][3]])
        hdr.dc.append(huff[(0, td)])
        hdr.ac.append(huff[(1, ta)])
        huffman_record(*hdr.dc[-1], name=name), huffman_record(*hdr.ac[-1], name=name)      # their checks
    hdr.segments, hdr.scan_end, at = _scan_segments(data, scan_begin, hdr.mcus_x * hdr.mcus_y, restart)
    # what follows the scan: nothing this reader would have to decode
    while at >= 0 and at + 2 <= n:
        m = data[at + 1]
        if m == 0xD9:
            break
        if m == 0xDA:
            _refuse(name, "more than one SOS is not served")
        if m == 0xDC:
            _refuse(name, "DNL is not served")
        if m in (0xC0, 0xC1) or m in _SOF_NAMES:
            _refuse(name, "more than one frame is not served")
        if at + 4 > n:
            break
        at += 2 + ((data[at + 2] << 8) | data[at + 3])
        while at + 1 < n and data[at] == 0xFF and data[at + 1] == 0xFF:
            at += 1
        if at + 1 < n and data[at] != 0xFF:
            break
    return hdr


def build_records(headers, chunk: int) -> dict:
    """The flat arrays of a batch (include/pmce_hip.h): ``data`` uint8, ``images`` int32 [F, 24], ``quant`` uint16 [nq, 64],
    ``huffman`` int32 [nh, 546], ``segments`` int32 [S, 5]; equal tables are stored once.  ``rounds``: per round of ``chunk`` images
    (first image, image count, first segment, segment count, coefficient blocks, plane bytes, the largest image's blocks)."""
    F = len(headers)
    images = np.zeros((F, IMG_WORDS), dtype=np.int32)
    quant, huffman, qi, hi = [], [], {}, {}
    segs, rounds, datas = [], [], []
    base = seg0 = 0
    for f, hd in enumerate(headers):
        if f % chunk == 0:
            rounds.append([f, 0, seg0, 0, 0, 0, 0])
        rd = rounds[-1]
        im = images[f]
        im[:8] = (hd.width, hd.height, hd.ncomp, hd.h, hd.v, hd.mcus_x, hd.mcus_y, hd.restart_interval)
        for c in range(hd.ncomp):
            key = hd.quant[c].tobytes()
            if key not in qi:
                qi[key] = len(quant)
                quant.append(hd.quant[c])
            im[8 + c] = qi[key]
            for word, tab in ((11, hd.dc[c]), (14, hd.ac[c])):
                if tab not in hi:
                    hi[tab] = len(huffman)
                    huffman.append(huffman_record(*tab, name=hd.name))
                im[word + c] = hi[tab]
        if rd[4] + hd.n_blocks >= 2 ** 31 or rd[5] + hd.plane_bytes >= 2 ** 31:
            raise ValueError(f"{hd.name}: {chunk} images of {hd.width} x {hd.height} per round need a workspace past 2^31: use a smaller chunk")
        im[17], im[18], im[19], im[20], im[21] = rd[4], rd[5], seg0, len(hd.segments), hd.blocks_per_mcu
        s = np.empty((len(hd.segments), SEG_WORDS), dtype=np.int64)
        s[:, 0] = f
        s[:, 1:3] = hd.segments[:, :2] + base
        s[:, 3:5] = hd.segments[:, 2:4]
        segs.append(s)
        rd[1] += 1
        rd[3] += len(hd.segments)
        rd[4] += hd.n_blocks
        rd[5] += hd.plane_bytes
        rd[6] = max(rd[6], hd.n_blocks)
        seg0 += len(hd.segments)
        base += len(hd.data)
        datas.append(np.frombuffer(hd.data, dtype=np.uint8))
        if base > 2 ** 31 - 129:
            raise ValueError(f"{hd.name}: the files of one call must stay below 2^31 - 128 bytes together: decode them in parts")
    return dict(data=np.concatenate(datas), images=images, quant=np.stack(quant), huffman=np.stack(huffman),
                segments=np.concatenate(segs).astype(np.int32), rounds=rounds)


def subsequence_records(rec: dict, subsequence: int) -> dict:
    """What the parallel entropy stage needs beside ``build_records``' arrays (include/pmce_hip.h): ``offsets`` int32 [S, 2], per
    segment its first subsequence and its first run (``PARALLEL_RUN`` subsequences), both counted from the first segment of the
    segment's round; ``totals``: per round (subsequences, runs, the longest segment's bytes).  A segment of n bytes has
    max(1, ceil(n / subsequence)) subsequences."""
    seg = rec["segments"].astype(np.int64)
    length = seg[:, 2] - seg[:, 1]
    n_sub = np.maximum(1, -(-length // subsequence))
    n_run = -(-n_sub // PARALLEL_RUN)
    offsets = np.zeros((len(seg), 2), dtype=np.int64)
    totals = []
    for _, _, s0, ns, *_ in rec["rounds"]:
        offsets[s0:s0 + ns, 0] = np.cumsum(n_sub[s0:s0 + ns]) - n_sub[s0:s0 + ns]
        offsets[s0:s0 + ns, 1] = np.cumsum(n_run[s0:s0 + ns]) - n_run[s0:s0 + ns]
        totals.append((int(n_sub[s0:s0 + ns].sum()), int(n_run[s0:s0 + ns].sum()), int(length[s0:s0 + ns].max())))
    return dict(offsets=offsets.astype(np.int32), totals=totals)


def parallel_workspace_bytes(n_sub: int, n_runs: int, n_seg: int) -> int:
    """The parallel entropy stage's workspace for one round (include/pmce_hip.h)."""
    return 32 * n_sub + 28 * n_runs + 8 * n_seg


def parallel_diagnostics(diagnostics) -> dict:
    """What ``decode(..., diagnostics=[])`` collected, read back (a host wait): over all rounds that took the parallel stage, the
    largest number of rounds in which a lane of a run decoded again, per synchronising launch (sync, join, join), the runs in which the
    last join still changed a lane, and the segments handed to the serial body."""
    most, late, serial, runs, segments = [0, 0, 0], 0, 0, 0, 0
    for ws, n_sub, n_runs, n_seg in diagnostics:
        words = ws.cpu().numpy().view(np.int32)
        at = (16 * n_sub + 16 * n_runs) // 4
        rounds = words[at:at + 3 * n_runs].reshape(3, n_runs)
        most = [max(m, int(r.max())) for m, r in zip(most, rounds)]
        late += int((rounds[2] > 0).sum())
        at += 3 * n_runs + 4 * n_sub
        serial += int(words[at:at + n_seg].sum())
        runs += n_runs
        segments += n_seg
    return dict(rounds_max_sync=most[0], rounds_max_join_1=most[1], rounds_max_join_2=most[2], runs=runs, runs_changed_by_the_last_join=late,
                segments=segments, segments_handed_to_the_serial_body=serial)


def parse_all(files, names=None, same_size: bool = True):
    """``parse`` of every file of one batch; with ``same_size`` all must have one size, else ValueError names the first file that differs."""
    if len(files) == 0:
        raise ValueError("decode: no files")
    names = list(names) if names is not None else [f"file {i}" for i in range(len(files))]
    if len(names) != len(files):
        raise ValueError(f"decode: {len(files)} files but {len(names)} names")
    headers = [parse(d, nm) for d, nm in zip(files, names)]
    w, h = headers[0].width, headers[0].height
    for hd in headers:
        if same_size and (hd.width, hd.height) != (w, h):
            raise ValueError(f"{hd.name}: {hd.width} x {hd.height}, but {headers[0].name} is {w} x {h}: all files of one call must have one size")
    return headers


def decode(files, device=None, channel_order: str = "bgr", chunk: int = 32, out=None, names=None, return_coefficients: bool = False,
           timings=None, lds_tables: bool = True, lanes: int = 0, entropy: str = "auto", subsequence: int = 0,
           diagnostics=None):
    """files: a list of ``bytes``, one JPEG file each, all of one size -> (frames uint8 [F, H, W, 3] on ``device``, status int32 [F] on
    the device), by pmce_jpeg_entropy / _idct / _colour on the current stream, ``chunk`` images per round through one workspace
    (2 bytes of coefficients and 1 of planes per padded sample: 9.4 MB per 1080p 4:2:0 image), after ONE upload of the files' bytes and their records.
    Channels are B, G, R as ``cv2.imread`` returns them, or R, G, B with ``channel_order="rgb"``.  ``out``: a contiguous uint8
    [F, H, W, 3] device tensor to fill.  Sampling, tables and restart interval may differ from file to file.  ``status`` is not
    read here (no wait for the device: the upload leaves page-locked memory asynchronously, no kernel and no result is waited for): 0 is a clean decode, see STATUS_*.  ``names`` label the files in errors.  ``return_coefficients``
    (one round only: F <= chunk) adds the entropy stage's int16 [blocks, 64] as a third result.  ``timings``: a list that receives
    (stage, start event, end event) per launch, for scripts/bench_jpeg.py.  ``lds_tables=False``: the entropy stage reads the Huffman
    tables from global memory even where they would fit into LDS (at most 16 distinct tables in the batch) - the same bits, slower;
    the form a batch with more tables takes anyway.  ``lanes``: segments per wavefront of the entropy stage, 1..64, or 0 for the
    library's choice (one until a round has more than 4096 segments) - the same bits whatever it is.  ``entropy``: "serial" is
    pmce_jpeg_entropy, one lane per restart interval; "parallel" is pmce_jpeg_entropy_parallel (csrc/jpeg_parallel.hip), many lanes per
    interval that start from guessed states and synchronise - the same coefficients and status words for every file, damaged ones
    included; "auto" takes the parallel stage for every round whose longest segment has at least ``AUTO_THRESHOLD`` bytes (what ffmpeg
    and ``cv2.imwrite`` write: no restart markers).  ``subsequence``: bytes per lane of the parallel stage, a multiple of 4 in
    4 .. 65536, or 0 for ``DEFAULT_SUBSEQUENCE`` - the same bits whatever it is.  ``timings`` names the parallel stage's launches
    "entropy_sync", "entropy_join" (twice), "entropy_place", "entropy_write" and "entropy_dc".  ``diagnostics``: a list that receives a
    copy of the parallel stage's workspace per round (made on the device, not waited for), for ``parallel_diagnostics``."""
    import torch
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be one of {CHANNEL_ORDERS} (got {channel_order!r})")
    if int(lanes) != lanes or not 0 <= int(lanes) <= 64:
        raise ValueError(f"lanes must be 0 or a whole number in 1..64 (got {lanes!r})")
    if int(chunk) != chunk or int(chunk) < 1 or int(chunk) > 65535:
        raise ValueError(f"chunk must be a whole number in 1..65535 (got {chunk!r})")
    if entropy not in ENTROPY_MODES:
        raise ValueError(f"entropy must be one of {ENTROPY_MODES} (got {entropy!r})")
    if isinstance(subsequence, bool) or int(subsequence) != subsequence or not (
            int(subsequence) == 0 or (MIN_SUBSEQUENCE <= int(subsequence) <= MAX_SUBSEQUENCE and int(subsequence) % 4 == 0)):
        raise ValueError(f"subsequence must be 0 or a multiple of 4 in {MIN_SUBSEQUENCE}..{MAX_SUBSEQUENCE} (got {subsequence!r})")
    subsequence = int(subsequence) or DEFAULT_SUBSEQUENCE
    headers = parse_all(files, names)
    F, H, W = len(headers), headers[0].height, headers[0].width
    if return_coefficients and F > chunk:
        raise ValueError(f"return_coefficients needs one round: {F} files, chunk {chunk}")
    rec = build_records(headers, int(chunk))
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (F, H, W, 3)
                and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 device tensor [{F}, {H}, {W}, 3]")
        dev = out.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    sub = subsequence_records(rec, subsequence)
    parallel = [entropy == "parallel" or (entropy == "auto" and longest >= AUTO_THRESHOLD) for _, _, longest in sub["totals"]]
    # one buffer, one upload: images | huffman | segments | quant | data | offsets, each part 16-byte aligned
    parts = [rec["images"], rec["huffman"], rec["segments"], rec["quant"], rec["data"], sub["offsets"]]
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += -(-p.nbytes // 16) * 16
    pinned = torch.zeros(total, dtype=torch.uint8, pin_memory=True)          # staged in page-locked memory: the upload is asynchronous
    host = pinned.numpy()
    for p, o in zip(parts, offs):
        host[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
    n_seg = len(rec["segments"])
    with torch.cuda.device(dev):
        buf = pinned.to(dev, non_blocking=True)
        frames = out if out is not None else torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
        status = torch.empty(F, device=dev, dtype=torch.int32)
        seg_status = torch.empty(n_seg, device=dev, dtype=torch.int32)
        n_blocks = max(r[4] for r in rec["rounds"])
        plane_bytes = max(r[5] for r in rec["rounds"])
        coef = torch.empty(n_blocks, 64, device=dev, dtype=torch.int16)
        planes = torch.empty(max(plane_bytes, 64), device=dev, dtype=torch.uint8)
        p_img, p_huf, p_seg, p_q, p_data, p_off = (C.c_void_p(buf.data_ptr() + o) for o in offs)
        lib, stream = _lib.load(), _lib.current_stream()
        ws_bytes = max([parallel_workspace_bytes(t[0], t[1], r[3]) for t, r, par in zip(sub["totals"], rec["rounds"], parallel) if par],
                       default=0)
        workspace = torch.empty(ws_bytes, device=dev, dtype=torch.uint8) if ws_bytes else None

        def timed(stage, fn):
            if timings is None:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            timings.append((stage, e0, e1))

        def entropy_parallel(s0, ns, nb, n_sub, n_runs, stage):
            _lib.check(lib.pmce_jpeg_entropy_parallel(
                p_data, len(rec["data"]), p_seg, s0, ns, p_img, F, p_huf, len(rec["huffman"]), _lib.ptr(coef), nb, _lib.ptr(seg_status),
                1 if lds_tables else 0, subsequence, p_off, n_sub, n_runs, _lib.ptr(workspace), ws_bytes, stage, stream),
                "jpeg_entropy_parallel")

        for (i0, ni, s0, ns, nb, pb, mb), (n_sub, n_runs, _), par in zip(rec["rounds"], sub["totals"], parallel):
            if not par:
                timed("entropy", lambda: _lib.check(lib.pmce_jpeg_entropy(
                    p_data, len(rec["data"]), p_seg, s0, ns, p_img, F, p_huf, len(rec["huffman"]), _lib.ptr(coef), nb, _lib.ptr(seg_status),
                    1 if lds_tables else 0, int(lanes), stream), "jpeg_entropy"))
            elif timings is None:
                entropy_parallel(s0, ns, nb, n_sub, n_runs, -1)
            else:                                  # launch by launch, so that each has its events
                for stage, name in enumerate(PARALLEL_STAGES):
                    timed("entropy_" + name, lambda: entropy_parallel(s0, ns, nb, n_sub, n_runs, stage))
            if par and diagnostics is not None:
                diagnostics.append((workspace[:parallel_workspace_bytes(n_sub, n_runs, ns)].clone(), n_sub, n_runs, ns))
            timed("idct", lambda: _lib.check(lib.pmce_jpeg_idct(
                _lib.ptr(coef), p_img, i0, ni, mb, p_q, len(rec["quant"]), nb, _lib.ptr(planes), max(pb, 64), stream), "jpeg_idct"))
            timed("colour", lambda: _lib.check(lib.pmce_jpeg_colour(
                _lib.ptr(planes), max(pb, 64), p_img, i0, ni, _lib.ptr(seg_status), n_seg, W, H, 1 if channel_order == "rgb" else 0,
                _lib.ptr(frames), _lib.ptr(status), stream), "jpeg_colour"))
    if return_coefficients:
        return frames, status, coef[:rec["rounds"][0][4]]
    return frames, status


def dump_records(files, path, coefficients=None, names=None):
    """Write the records of ``files`` (one round: every image in one coefficient buffer) as the binary file scripts/jpeg_entropy_host.cpp
    reads: the magic "PMCEJPG1"; int64 x 7 = (bytes, images, quantisation tables, Huffman tables, segments, blocks, 1 if coefficients
    follow); then images int32, huffman int32, segments int32, quant uint16, data uint8 and, if given, ``coefficients`` int16
    [blocks, 64] (the expected output of the entropy stage, in its layout) - little-endian, no padding.  The files need not be of one
    size: only the entropy stage reads these records."""
    headers = parse_all(files, names, same_size=False)
    rec = build_records(headers, len(headers))
    n_blocks = rec["rounds"][0][4]
    if coefficients is not None:
        coefficients = np.ascontiguousarray(coefficients, dtype=np.int16)
        if coefficients.shape != (n_blocks, 64):
            raise ValueError(f"coefficients must be [{n_blocks}, 64] (got {coefficients.shape})")
    with open(path, "wb") as fh:
        fh.write(DUMP_MAGIC)
        fh.write(struct.pack("<7q", len(rec["data"]), len(headers), len(rec["quant"]), len(rec["huffman"]), len(rec["segments"]), n_blocks,
                             0 if coefficients is None else 1))
        for key in ("images", "huffman", "segments", "quant", "data"):
            fh.write(np.ascontiguousarray(rec[key]).astype(rec[key].dtype.newbyteorder("<"), copy=False).tobytes())
        if coefficients is not None:
            fh.write(coefficients.astype("<i2", copy=False).tobytes())
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------------
# the writer (csrc/jpeg_encode.hip): frames on the device -> baseline JFIF files on the device, byte for byte libjpeg's default compressor
# ---------------------------------------------------------------------------------------------------------------------------------------
SUBSAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
STATUS_CAPACITY = 1                    # encode: the frame's file is longer than ``capacity``; it is served with length 0
MAX_BLOCK_BYTES = 208                  # a block's code before stuffing: 20 bits of DC and 63 x 26 bits of AC (csrc/jpeg_encode.hpp)
ENCODE_PIECE = 256                     # bytes of the unstuffed stream per lane group of the stuffing stage (csrc/jpeg_encode.hpp, PIECE)
ENCODE_STAGES = ("lengths", "offsets", "bits", "count", "place", "frames", "write")        # the entropy entry's launches, as ``timings`` names them
# T.81 Annex K.1 (natural order) and K.3 (counts of the lengths 1..16, values)
K_LUMA_QUANT = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
                62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
                112, 100, 103, 99)
K_CHROMA_QUANT = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                  99, 99) + (99,) * 32
K_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
            56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
K_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
K_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
K_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
             (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
              0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
              0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
              0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
              0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
              0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
              0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
              0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA))
K_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
               (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
                0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
                0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
                0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
                0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
                0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
                0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
                0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
                0xF9, 0xFA))


def quant_tables(quality: int):
    """``jpeg_set_quality(quality, force_baseline)`` on Annex K.1's tables -> (luma, chroma), int64 [64] each, natural order."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be a whole number in 1..100 (got {quality!r})")
    quality = int(quality)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(base, dtype=np.int64) * scale + 50) // 100, 1, 255) for base in (K_LUMA_QUANT, K_CHROMA_QUANT))


def _encode_geometry(width, height, subsampling, restart_interval):
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {tuple(SUBSAMPLINGS)} (got {subsampling!r})")
    for what, x in (("width", width), ("height", height)):
        if isinstance(x, bool) or int(x) != x or not 1 <= int(x) <= MAX_DIM:
            raise ValueError(f"{what} must be a whole number in 1..{MAX_DIM} (got {x!r})")
    if isinstance(restart_interval, bool) or int(restart_interval) != restart_interval or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be a whole number of MCUs in 0..65535 (got {restart_interval!r})")
    h, v = SUBSAMPLINGS[subsampling]
    mcus = -(-int(width) // (8 * h)) * -(-int(height) // (8 * v))
    return h, v, mcus


def encode_header(width: int, height: int, quality: int = 95, subsampling: str = "4:2:0", restart_interval: int = 0) -> bytes:
    """The file up to its scan, as libjpeg writes it: SOI, APP0 (JFIF 1.01, density 1 x 1, no unit), DQT 0 and 1, SOF0, the four DHT of
    Annex K.3 (DC 0, AC 0, DC 1, AC 1), DRI if ``restart_interval`` (MCUs) is not 0, SOS.  Host only."""
    h, v, _ = _encode_geometry(width, height, subsampling, restart_interval)
    luma, chroma = quant_tables(quality)

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, table in enumerate((luma, chroma)):
        out += seg(0xDB, bytes([t]) + bytes(int(table[n]) for n in K_ZIGZAG))
    out += seg(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big")
               + bytes([3, 1, (h << 4) | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (counts, values) in ((0x00, K_DC_LUMA), (0x10, K_AC_LUMA), (0x01, K_DC_CHROMA), (0x11, K_AC_CHROMA)):
        out += seg(0xC4, bytes([ident]) + bytes(counts) + bytes(values))
    if restart_interval:
        out += seg(0xDD, int(restart_interval).to_bytes(2, "big"))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode_capacity(width: int, height: int, subsampling: str = "4:2:0", restart_interval: int = 0, worst_case: bool = False) -> int:
    """Bytes per frame of ``encode``'s ``data``.  The default: the header and 1.5 bytes per padded luma sample (far above what quality 95
    gives a photograph).  ``worst_case``: what no frame can exceed - every block ``MAX_BLOCK_BYTES`` long and every byte stuffed, a
    padding byte and a marker per restart interval, EOI."""
    h, v, mcus = _encode_geometry(width, height, subsampling, restart_interval)
    header = len(encode_header(width, height, 95, subsampling, restart_interval))
    if not worst_case:
        return header + 3 * (mcus * h * v * 64) // 2 + 2
    intervals = -(-mcus // int(restart_interval)) if restart_interval else 1
    return header + 2 * mcus * (h * v + 2) * MAX_BLOCK_BYTES + 3 * intervals


def encode(frames, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "bgr", restart_interval: int = 0, chunk: int = 32,
           capacity=None, timings=None, return_coefficients: bool = False, guard: int = 0):
    """frames: a contiguous uint8 [F, H, W, 3] device tensor (B, G, R as the demo's stages hold them, or R, G, B with
    ``channel_order="rgb"``) -> (data uint8: the JPEG files back to back, offsets int64 [F + 1], status int32 [F]), all on the device:
    frame f's file is ``data[offsets[f]:offsets[f + 1]]``.  By pmce_jpeg_encode_coefficients / _entropy on the current stream, ``chunk``
    frames at a time through one workspace (2 bytes of coefficients per padded sample and ``MAX_BLOCK_BYTES`` per block of unstuffed
    stream: 16.5 MB per 1080p 4:2:0 frame); no wait for the device, nothing is read back.  The files are those of libjpeg's default
    compressor at the same settings, byte for byte - ``cv2.imwrite``'s are quality 95, 4:2:0, no restart markers,
    the defaults here.  ``restart_interval`` is in MCUs (0: no DRI, no markers).  ``capacity``: bytes per frame of ``data`` (default
    ``encode_capacity``; ``encode_capacity(..., worst_case=True)`` bounds every frame); a frame whose file is longer gets length 0 and
    ``STATUS_CAPACITY`` in ``status`` - never a partial file - and nothing is written beyond ``offsets[F]``.  ``timings``: a list that
    receives (stage, start event, end event) per launch, for scripts/bench_jpeg_encode.py.  ``return_coefficients`` (one round only:
    F <= chunk) adds the coefficient stage's int16 [F, blocks, 64] (zigzag order) as a fourth result.  ``guard``: for the tests - ``data`` is
    filled with 0xA5 first and has that many bytes more than F x capacity.  ``files`` reads the result back."""
    import torch
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be one of {CHANNEL_ORDERS} (got {channel_order!r})")
    if isinstance(chunk, bool) or int(chunk) != chunk or not 1 <= int(chunk) <= 65535:
        raise ValueError(f"chunk must be a whole number in 1..65535 (got {chunk!r})")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError("frames must be a uint8 tensor [F, H, W, 3] with F >= 1")
    F, H, W = (int(x) for x in frames.shape[:3])
    h, v, mcus = _encode_geometry(W, H, subsampling, restart_interval)
    header = encode_header(W, H, quality, subsampling, restart_interval)
    if capacity is None:
        capacity = encode_capacity(W, H, subsampling, restart_interval)
    if isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < 1:
        raise ValueError(f"capacity must be a whole number of bytes >= 1 (got {capacity!r})")
    chunk, capacity, restart_interval = min(int(chunk), F), int(capacity), int(restart_interval)
    if return_coefficients and F > chunk:
        raise ValueError(f"return_coefficients needs one round: {F} frames, chunk {chunk}")
    if not frames.is_cuda or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous device tensor")
    n_blocks = mcus * (h * v + 2)
    lib = _lib.load()
    ws_bytes = lib.pmce_jpeg_encode_workspace_bytes(chunk, mcus, h * v, restart_interval)
    if ws_bytes == 0 or chunk * n_blocks >= 2 ** 31:
        raise ValueError(f"{chunk} frames of {W} x {H} per round need a workspace past its limits: use a smaller chunk or a restart interval")
    tables = np.concatenate(quant_tables(quality)).astype(np.uint16)
    host = np.concatenate([tables.view(np.uint8), np.frombuffer(header, dtype=np.uint8)])
    pinned = torch.zeros(len(host), dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = host
    dev = frames.device
    with torch.cuda.device(dev):
        stream = _lib.current_stream()
        consts = pinned.to(dev, non_blocking=True)
        p_quant, p_header = C.c_void_p(consts.data_ptr()), C.c_void_p(consts.data_ptr() + 256)
        data = (torch.full((F * capacity + int(guard),), 0xA5, device=dev, dtype=torch.uint8) if guard
                else torch.empty(F * capacity, device=dev, dtype=torch.uint8))
        offsets = torch.empty(F + 1, device=dev, dtype=torch.int64)
        status = torch.empty(F, device=dev, dtype=torch.int32)
        coef = torch.empty(chunk, n_blocks, 64, device=dev, dtype=torch.int16)
        workspace = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)

        def timed(stage, fn):
            if timings is None:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            timings.append((stage, e0, e1))

        def entropy(f0, n, stage):
            _lib.check(lib.pmce_jpeg_encode_entropy(
                _lib.ptr(coef), n, mcus, h * v, restart_interval, p_header, len(header), capacity, _lib.ptr(workspace), ws_bytes,
                _lib.ptr(data), F * capacity, _lib.ptr(offsets), _lib.ptr(status), f0, stage, stream), "jpeg_encode_entropy")

        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            timed("coefficients", lambda: _lib.check(lib.pmce_jpeg_encode_coefficients(
                _lib.ptr(frames), f0, n, W, H, h, v, 1 if channel_order == "rgb" else 0, p_quant, _lib.ptr(coef), chunk * n_blocks, stream),
                "jpeg_encode_coefficients"))
            if timings is None:
                entropy(f0, n, -1)
            else:                                  # launch by launch, so that each has its events
                for stage, name in enumerate(ENCODE_STAGES):
                    timed(name, lambda: entropy(f0, n, stage))
    if return_coefficients:
        return data, offsets, status, coef[:F]
    return data, offsets, status


def encode_entropy(coefficients, luma_blocks: int, header: bytes, restart_interval: int = 0, capacity=None, guard: int = 0):
    """The entropy stages alone (pmce_jpeg_encode_entropy): coefficients int16 [F, blocks, 64] on the device, zigzag order, blocks in scan
    order with ``luma_blocks`` (1, 2 or 4) luma blocks, Cb and Cr per MCU -> (data, offsets, status) as ``encode`` gives them, the files
    beginning with ``header``.  ``guard``: that many bytes of 0xA5 are allocated behind ``data`` (the returned tensor includes them)."""
    import torch
    c = coefficients
    if not isinstance(c, torch.Tensor) or c.dtype != torch.int16 or c.ndim != 3 or c.shape[2] != 64 or c.shape[0] < 1:
        raise ValueError("coefficients must be an int16 tensor [F, blocks, 64]")
    if luma_blocks not in (1, 2, 4) or c.shape[1] < 1 or c.shape[1] % (luma_blocks + 2):
        raise ValueError(f"{c.shape[1]} blocks per frame are no whole number of MCUs of {luma_blocks} + 2 blocks")
    if isinstance(restart_interval, bool) or int(restart_interval) != restart_interval or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"restart_interval must be a whole number of MCUs in 0..65535 (got {restart_interval!r})")
    if not c.is_cuda or not c.is_contiguous():
        raise ValueError("coefficients must be a contiguous device tensor")
    F, mcus = int(c.shape[0]), int(c.shape[1]) // (luma_blocks + 2)
    header = bytes(header)
    intervals = -(-mcus // int(restart_interval)) if restart_interval else 1
    if capacity is None:
        capacity = len(header) + 2 * int(c.shape[1]) * MAX_BLOCK_BYTES + 3 * intervals
    lib = _lib.load()
    ws_bytes = lib.pmce_jpeg_encode_workspace_bytes(F, mcus, luma_blocks, int(restart_interval))
    if ws_bytes == 0:
        raise ValueError(f"{F} frames of {mcus} MCUs need a workspace past its limits")
    with torch.cuda.device(c.device):
        hdr = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(c.device)
        data = torch.full((F * int(capacity) + int(guard),), 0xA5, device=c.device, dtype=torch.uint8)
        offsets = torch.empty(F + 1, device=c.device, dtype=torch.int64)
        status = torch.empty(F, device=c.device, dtype=torch.int32)
        workspace = torch.empty(ws_bytes, device=c.device, dtype=torch.uint8)
        _lib.check(lib.pmce_jpeg_encode_entropy(_lib.ptr(c), F, mcus, luma_blocks, int(restart_interval), _lib.ptr(hdr), len(header),
                                                int(capacity), _lib.ptr(workspace), ws_bytes, _lib.ptr(data), F * int(capacity),
                                                _lib.ptr(offsets), _lib.ptr(status), 0, -1, _lib.current_stream()), "jpeg_encode_entropy")
    return data, offsets, status


def files(data, offsets, status) -> list:
    """What ``encode`` returned, as a list of ``bytes``, one file per frame.  The one host read: the offsets and the status words, then
    only the bytes in use.  A frame with a status bit raises ValueError, naming the frame."""
    off = offsets.cpu().numpy()
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if len(bad):
        raise ValueError(f"frame {int(bad[0])}: its file is longer than the capacity per frame (status {int(st[bad[0]])}): "
                         "encode with a larger capacity (encode_capacity(..., worst_case=True) holds every frame)")
    raw = data[:int(off[-1])].cpu().numpy().tobytes()
    return [raw[int(off[f]):int(off[f + 1])] for f in range(len(st))]
