"""The host restatement of the PNG encoder's format (tests/png_encode_reference.py) writes files that Pillow and zlib accept and
that decode to the input, on every case the GPU test compares the kernels against; the library's host-only bound agrees with the
formula.  No GPU."""
import io
import zlib

import numpy as np
import pytest

from tests import png_encode_cases as pc
from tests import png_encode_reference as ref

NAMES = sorted(pc.cases())


def check_file(data, img):
    """what every file of the encoder must satisfy, whoever wrote it"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.mode == ("L" if img.ndim == 2 else "RGB")
        assert np.array_equal(np.asarray(im), img)
    with Image.open(io.BytesIO(data)) as im:
        im.verify()                                            # chunk CRCs
    raw = zlib.decompress(ref.idat_payload(data))              # Adler-32
    ch = 1 if img.ndim == 2 else 3
    assert len(raw) == img.shape[0] * (1 + img.shape[1] * ch) and raw == ref.filtered_stream(img).tobytes()
    assert len(data) <= ref.bound(img.shape[0], img.shape[1], ch)


@pytest.mark.parametrize("name", NAMES)
def test_restated_files_decode_to_the_input(name):
    img = pc.cases()[name]
    data, forms, lengths = pc.expected(name)
    check_file(data, img)
    S = ref.filtered_stream(img).size
    assert len(forms) == len(lengths) == (S + ref.SEGMENT - 1) // ref.SEGMENT


def test_cases_reach_what_they_are_there_for():
    c = pc.cases()
    # every run length 1 ... 300 stands whole in one segment
    seen = set()
    for lo in range(1, 300, 50):
        img = c[f"runs_{lo}_{lo + 49}"]
        s = ref.filtered_stream(img)
        assert s.size <= ref.SEGMENT
        for row in s.reshape(img.shape[0], -1):
            seen.add(int(np.count_nonzero((row == 100) | (row == 200))))
            assert int(np.count_nonzero(np.diff(np.flatnonzero((row == 100) | (row == 200))) != 1)) == 0
    assert seen == set(range(1, 301))
    assert set(ref.filtered_stream(c["all_residuals"]).tolist()) == set(range(256))
    for W in (ref.SEGMENT - 2, ref.SEGMENT - 1, ref.SEGMENT):
        assert ref.filtered_stream(c[f"stream_{1 + W}"]).size == 1 + W
    assert ref.filtered_stream(c["stream_3seg"]).size == 3 * ref.SEGMENT
    s = ref.filtered_stream(c["straddle"])
    assert (s[ref.SEGMENT - 400:ref.SEGMENT + 400] == 77).all() and s[ref.SEGMENT - 401] != 77 and s[ref.SEGMENT + 400] != 77
    # the run is cut at the boundary: both segments are coded and the second starts with a literal 77 again
    assert pc.expected("straddle")[1] == ["coded", "coded"]
    assert ref.segment_tokens(s[ref.SEGMENT:])[0] == ref._literal(77)
    assert set(pc.expected("noise")[1]) == {"stored"} and set(pc.expected("noise_rgb")[1]) == {"stored"}
    assert set(pc.expected("noise_then_flat")[1]) == {"stored", "coded"}
    data, forms, lengths = pc.expected("coded_len_eq_stored")
    assert lengths == [5 + 100] and forms == ["stored"]
    data, forms, lengths = pc.expected("coded_one_shorter")
    assert lengths == [4 + 100] and forms == ["coded"]
    assert len({len(ref.encode(m)[0]) for m in pc.batch3()}) == 3


def test_match_lengths_use_all_29_codes():
    codes = {max(i for i in range(29) if ref.LEN_BASE[i] <= m) for m in range(3, 259)}
    assert codes == set(range(29))
    # 258 is its own code without extra bits, not 227 + 31
    assert ref._match(258) == (ref._rev(0xC0 + 5, 8), 8 + 0 + 5) and ref._match(257)[1] == 8 + 5 + 5


def test_bound_is_the_librarys():
    from openess_amd import _lib
    lib = _lib.load()
    for H, W, ch in ((1, 1, 1), (1, 1, 3), (440, 640, 1), (440, 640, 3), (1, 16383, 1), (3, 16383, 1), (16384, 16384, 3), (300, 1, 1)):
        assert lib.oess_png_encode_bound(H, W, ch) == ref.bound(H, W, ch)
    assert lib.oess_png_encode_bound(440, 640, 3) == 75 + 440 * 1921 + 17 * 52
    for H, W, ch in ((0, 5, 1), (5, 0, 1), (16385, 5, 1), (5, 16385, 3), (5, 5, 2), (5, 5, 4), (5, 5, 0), (-1, 5, 1)):
        assert lib.oess_png_encode_bound(H, W, ch) == 0
