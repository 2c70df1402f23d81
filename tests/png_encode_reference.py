"""Host restatement of the PNG subset that hip.png_encode_batch writes (include/oess.h), in NumPy / Python: the
expected file bytes and the form of every segment.  Checksums come from zlib, the length codes from RFC 1951's table, the runs
from a sequential walk: nothing here shares a formula with the kernel."""
import struct
import zlib

import numpy as np

SEGMENT = 16384
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def bound(H, W, channels):
    S = H * (1 + W * channels)
    return 75 + S + 17 * ((S + SEGMENT - 1) // SEGMENT)


def _predictor(x, ch):
    """Paeth predictor of every byte of x [H, W * ch] (int32) from its left, upper and upper-left neighbours, 0 outside"""
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, ch:] = x[:, :-ch]
    b[1:] = x[:-1]
    c[1:, ch:] = x[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_stream(img):
    """uint8 [H, W] or [H, W, 3] -> the filtered scanlines, filter type 4 on every row, as one uint8 vector"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    H, ch = img.shape[0], 1 if img.ndim == 2 else 3
    x = img.reshape(H, -1).astype(np.int32)
    out = np.empty((H, 1 + x.shape[1]), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((x - _predictor(x, ch)) & 255).astype(np.uint8)
    return out.reshape(-1)


def unfilter_stream(stream, H, W, channels):
    """The image whose filtered stream is `stream` (every row's first byte must be 4): PNG's Paeth reconstruction, row by row"""
    rows = np.asarray(stream, np.uint8).reshape(H, 1 + W * channels)
    assert (rows[:, 0] == 4).all()
    out = np.zeros((H, W * channels), np.int32)
    for y in range(H):
        up = out[y - 1] if y else np.zeros(W * channels, np.int32)
        for x in range(W * channels):
            a = int(out[y, x - channels]) if x >= channels else 0
            b = int(up[x])
            c = int(up[x - channels]) if x >= channels else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out[y, x] = (int(rows[y, 1 + x]) + pred) & 255
    out = out.astype(np.uint8)
    return out.reshape(H, W) if channels == 1 else out.reshape(H, W, 3)


def _rev(code, n):
    return int(format(code, "0{}b".format(n))[::-1], 2)


def _literal(v):
    return (_rev(0x30 + v, 8), 8) if v < 144 else (_rev(0x190 + v - 144, 9), 9)


def _match(m):
    """a match of m bytes at distance 1: length code, extra bits, the 5-bit distance code 0"""
    idx = max(i for i in range(29) if LEN_BASE[i] <= m)
    sym = 257 + idx
    code, n = (sym - 256, 7) if sym <= 279 else (0xC0 + sym - 280, 8)
    return _rev(code, n) | ((m - LEN_BASE[idx]) << n), n + LEN_EXTRA[idx] + 5


def segment_tokens(seg):
    """(value, bit count) of every token of one segment, LSB first"""
    seg = np.asarray(seg, np.uint8)
    cuts = np.concatenate(([0], np.flatnonzero(seg[1:] != seg[:-1]) + 1, [len(seg)]))
    out = []
    for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        lit = _literal(int(seg[s]))
        out.append(lit)
        rest = e - s - 1
        while rest >= 3:
            m = min(rest, 258)
            out.append(_match(m))
            rest -= m
        out += [lit] * rest
    return out


def _pack(tokens):
    """bytes of (value, bit count) pairs packed LSB first, zero bits to the byte"""
    vals = np.array([t[0] for t in tokens], np.int64)
    ns = np.array([t[1] for t in tokens], np.int64)
    ends = np.cumsum(ns)
    tok = np.repeat(np.arange(len(ns)), ns)
    k = np.arange(int(ends[-1])) - np.repeat(ends - ns, ns)
    bits = ((vals[tok] >> k) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes()


def coded_segment(seg, last):
    head = [((1 if last else 0) | 2, 3)]
    tail = [(0, 7)] + ([] if last else [(0, 3)])
    body = _pack(head + segment_tokens(seg) + tail)
    return body if last else body + b"\x00\x00\xff\xff"


def stored_segment(seg, last):
    n = len(seg)
    return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(seg)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(img, segment=SEGMENT):
    """(file bytes, ['coded' | 'stored' per segment], [coded length per segment]) of one image"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    stream = filtered_stream(img)
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if img.ndim == 2 else 2, 0, 0, 0)),
           _chunk(b"IDAT", b"\x78\x01")]
    forms, lengths = [], []
    nseg = (len(stream) + segment - 1) // segment
    for k in range(nseg):
        seg = stream[k * segment:(k + 1) * segment]
        last = k == nseg - 1
        coded = coded_segment(seg, last)
        lengths.append(len(coded))
        stored = len(coded) >= 5 + len(seg)
        forms.append("stored" if stored else "coded")
        out.append(_chunk(b"IDAT", stored_segment(seg, last) if stored else coded))
    out.append(_chunk(b"IDAT", struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out), forms, lengths


def idat_payload(data):
    """the concatenated IDAT payloads of a PNG file (no checks beyond the chunk walk)"""
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    assert pos == len(data)
    return b"".join(out)
