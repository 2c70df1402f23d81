"""Shapes and seeded inputs of the PNG encoder's tests, shared by the host test of the restatement and the GPU
test of the kernels.  Where a case needs a particular FILTERED stream (a run of a given length, a given mix of literals), the
stream is written down and the image is its Paeth reconstruction (png_encode_reference.unfilter_stream).  Every restated stream
stays below 100 KB."""
import functools

import numpy as np

from tests import png_encode_reference as ref

SEG = ref.SEGMENT


def _filler(n, first=1):
    """n bytes 1, 2, 1, 2 ...: no two neighbours equal, none equal to a row's filter byte 4 or to a run value used below"""
    return [(first + i) % 2 + 1 for i in range(n)]


def _image_of_rows(rows):
    """grey image whose filtered rows (without the filter byte) are `rows`"""
    W = len(rows[0])
    stream = np.array([[4] + list(r) for r in rows], np.uint8)
    return ref.unfilter_stream(stream.reshape(-1), len(rows), W, 1)


def _run_rows(lo, hi):
    """one row per run length lo ... hi: filler, one run of that length (value 100 or 200 by turns, so that the literals left
    behind a match come from the 8-bit and the 9-bit code), filler"""
    W = hi + 4
    rows = []
    for L in range(lo, hi + 1):
        post = W - 2 - L
        rows.append(_filler(2) + [100 if L % 2 else 200] * L + _filler(post))
    return _image_of_rows(rows)


def label_like(rng, H, W, classes=11, block=20):
    m = rng.integers(0, classes, ((H + block - 1) // block, (W + block - 1) // block)).astype(np.uint8)
    return np.ascontiguousarray(m.repeat(block, 0).repeat(block, 1)[:H, :W])


def colours_of(labels, rng):
    palette = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    return np.ascontiguousarray(palette[labels])


def _literal_mix(n8, n9):
    """H = 1 grey image whose stream is the filter byte, then n8 - 1 literals of the 8-bit code and n9 of the 9-bit code, no runs"""
    body = []
    for i in range(n8 - 1 + n9):
        body.append(150 + i % 2 if i < n9 else 10 + i % 2)
    return _image_of_rows([body])


@functools.lru_cache(maxsize=None)
def cases():
    """{name: uint8 image [H, W] or [H, W, 3]}"""
    rng = np.random.default_rng(37)
    c = {}
    c["one_grey"] = np.array([[7]], np.uint8)
    c["one_rgb"] = np.array([[[200, 3, 144]]], np.uint8)
    c["h1_grey"] = label_like(rng, 1, 37, block=5)
    c["h1_rgb"] = colours_of(label_like(rng, 1, 23, block=4), rng)
    c["w1_h300"] = rng.integers(0, 3, (300, 1)).astype(np.uint8) * 90
    for lo in range(1, 300, 50):                       # every run length 1 ... 300, each image one segment: no run is cut
        c[f"runs_{lo}_{lo + 49}"] = _run_rows(lo, lo + 49)
    c["all_residuals"] = _image_of_rows([list(rng.permutation(256)), list(rng.permutation(256))])
    c["zeros"] = np.zeros((20, 30), np.uint8)
    c["all255"] = np.full((20, 30), 255, np.uint8)
    c["zeros_rgb"] = np.zeros((9, 14, 3), np.uint8)
    for W in (SEG - 2, SEG - 1, SEG):                  # streams of SEG - 1, SEG and SEG + 1 bytes
        c[f"stream_{1 + W}"] = label_like(rng, 1, W, block=37)
    c["stream_3seg"] = label_like(rng, 3, SEG - 1, block=41)
    # a run of 800 equal filtered bytes across the first segment boundary (stream bytes SEG - 400 ... SEG + 400), filler around it
    W, pre = 10000, SEG - 400 - (10000 + 2)
    c["straddle"] = _image_of_rows([_filler(W), _filler(pre) + [77] * 800 + _filler(W - pre - 800)])
    c["noise"] = rng.integers(0, 256, (100, 200)).astype(np.uint8)
    c["noise_rgb"] = rng.integers(0, 256, (60, 90, 3)).astype(np.uint8)
    half = rng.integers(0, 256, (200, 200)).astype(np.uint8)
    half[100:] = 9
    c["noise_then_flat"] = half
    # 100 stream bytes whose coded form takes 3 + 8 * 75 + 9 * 25 + 7 = 835 bits = 105 bytes = 5 + 100: as long as stored
    c["coded_len_eq_stored"] = _literal_mix(75, 25)
    c["coded_one_shorter"] = _literal_mix(78, 22)      # 832 bits = 104 bytes: coded
    c["labels"] = label_like(rng, 64, 96, block=8)
    c["colours"] = colours_of(c["labels"], rng)
    c["smooth_rgb"] = np.ascontiguousarray(np.clip(np.add.outer(np.arange(50) * 3, np.arange(70) * 2)[..., None] + rng.normal(0, 2, (50, 70, 3)), 0, 255).astype(np.uint8))
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """(file bytes, forms, coded lengths) of a case, restated once"""
    return ref.encode(cases()[name])


def batch3():
    """three maps of one shape with different contents (so different file sizes)"""
    rng = np.random.default_rng(3)
    return np.stack([np.zeros((40, 50), np.uint8), label_like(rng, 40, 50, block=6), rng.integers(0, 256, (40, 50)).astype(np.uint8)])


def large_rgb():
    """2 x 440 x 640 x 3, label-like colours: checked by round trip only"""
    rng = np.random.default_rng(440)
    return np.stack([colours_of(label_like(rng, 440, 640), rng) for _ in range(2)])
