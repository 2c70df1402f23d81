"""hip.png_encode_batch / png_encode_files against the host restatement of the format (tests/png_encode_reference.py): the file
bytes are equal, Pillow and zlib decode them to the input, and two calls agree.  Exact everywhere: no tolerance."""

import numpy as np
import pytest
import torch

from tests import png_encode_cases as pc
from tests import png_encode_reference as ref
from tests.test_png_encode_reference import check_file

pytestmark = pytest.mark.gpu

NAMES = sorted(pc.cases())


def _encode(img):
    from openess_amd import hip
    return hip.png_encode_files(torch.from_numpy(np.ascontiguousarray(img[None])).cuda())[0]


@pytest.mark.parametrize("name", NAMES)
def test_files_equal_the_restatement(name):
    img = pc.cases()[name]
    want, forms, _ = pc.expected(name)
    got = _encode(img)
    print(f"[png_encode] {name}: {img.shape} -> {len(got)} bytes, segments {forms.count('coded')} coded / {forms.count('stored')} stored", flush=True)
    assert len(got) == len(want)
    assert got == want
    check_file(got, img)
    assert _encode(img) == got                              # bit-repeatable


def test_noise_stays_within_the_bound_and_mixed_forms_share_a_file():
    from openess_amd import hip
    for name in ("noise", "noise_rgb", "noise_then_flat"):
        img = pc.cases()[name]
        ch = 1 if img.ndim == 2 else 3
        files, sizes = hip.png_encode_batch(torch.from_numpy(img[None]).cuda())
        assert files.shape == (1, hip.png_encode_bound(img.shape[0], img.shape[1], ch)) and files.dtype == torch.uint8
        assert sizes.dtype == torch.int32 and 0 < int(sizes[0]) <= files.shape[1]
        assert bytes(files[0, :int(sizes[0])].cpu().numpy()) == pc.expected(name)[0]


def test_batch_slots_are_independent_and_out_is_reused():
    from openess_amd import hip
    maps = pc.batch3()
    want = [ref.encode(m)[0] for m in maps]
    dev = torch.from_numpy(maps).cuda()
    assert hip.png_encode_files(dev) == want
    files, sizes = hip.png_encode_batch(dev)
    assert sizes.tolist() == [len(w) for w in want] and len(set(sizes.tolist())) == 3
    # each image alone gives the same file as inside the batch
    for i in range(3):
        assert hip.png_encode_files(dev[i:i + 1].contiguous()) == [want[i]]
    # out=: the same buffers, other contents
    files.fill_(0xEE)
    sizes.fill_(-1)
    f2, s2 = hip.png_encode_batch(dev.flip(0).contiguous(), out=(files, sizes))
    assert f2 is files and s2 is sizes
    assert [bytes(files[i, :int(sizes[i])].cpu().numpy()) for i in range(3)] == want[::-1]
    # a wider slot than the bound is taken as it is
    wide = torch.empty((3, files.shape[1] + 13), dtype=torch.uint8, device='cuda')
    f3, s3 = hip.png_encode_batch(dev, out=(wide, sizes))
    assert [bytes(wide[i, :int(s3[i])].cpu().numpy()) for i in range(3)] == want


def test_nothing_outside_the_slots_and_sizes_is_written():
    from openess_amd import _lib, hip
    lib = _lib.load()
    maps = pc.batch3()
    n, H, W = maps.shape
    slot = hip.png_encode_bound(H, W, 1) + 3                 # an odd slot: the slots start on every byte alignment
    pad = 64
    dev = torch.from_numpy(maps).cuda()
    buf = torch.full((pad + n * slot + pad,), 0xA5, dtype=torch.uint8, device='cuda')
    sz = torch.full((16 + n + 16,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device='cuda')
    need = lib.oess_png_encode_scratch_bytes(n, H, W, 1)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    rc = lib.oess_png_encode_batch(dev.data_ptr(), n, H, W, 1, buf.data_ptr() + pad, slot, sz.data_ptr() + 16 * 4, ws.data_ptr(), need,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n * slot:] == 0xA5).all())
    assert bool((sz[:16] == sz[0]).all()) and bool((sz[16 + n:] == sz[0]).all()) and int(sz[0]) == 0xA5A5A5A5 - (1 << 32)
    sizes = sz[16:16 + n].tolist()
    for i in range(n):
        got = bytes(buf[pad + i * slot:pad + i * slot + sizes[i]].cpu().numpy())
        assert got == ref.encode(maps[i])[0]
        assert bool((buf[pad + i * slot + hip.png_encode_bound(H, W, 1):pad + (i + 1) * slot] == 0xA5).all())   # beyond the bound: untouched


def test_grey_files_go_back_through_the_gpu_decoder():
    from openess_amd import hip
    for maps in (pc.batch3(), np.stack([pc.cases()["labels"], pc.cases()["labels"][::-1].copy()]), pc.cases()["noise_then_flat"][None],
                 pc.cases()["stream_3seg"][None]):
        dev = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
        files = hip.png_encode_files(dev)
        blob = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).cuda()
        back, status = hip.png_decode_gray8_batch(blob, [len(f) for f in files], maps.shape[1], maps.shape[2])
        assert status.tolist() == [0] * len(files)
        assert torch.equal(back, dev.long())


def test_large_rgb_round_trip():
    from openess_amd import hip
    maps = pc.large_rgb()
    dev = torch.from_numpy(maps).cuda()
    files = hip.png_encode_files(dev)
    assert files == hip.png_encode_files(dev)
    for f, m in zip(files, maps):
        check_file(f, m)
    print(f"[png_encode] 2 x 440 x 640 x 3 label-like colours: {[len(f) for f in files]} bytes", flush=True)


def test_entry_refuses_bad_arguments_and_touches_nothing():
    from openess_amd import _lib, hip
    lib = _lib.load()
    H, W = 12, 20
    img = torch.zeros((2, H, W, 3), dtype=torch.uint8, device='cuda')
    slot = hip.png_encode_bound(H, W, 3)
    files = torch.full((2, slot), 0xA5, dtype=torch.uint8, device='cuda')
    sizes = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    need = lib.oess_png_encode_scratch_bytes(2, H, W, 3)
    ws = torch.empty(need + 16, dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    good = dict(images=img.data_ptr(), n=2, H=H, W=W, ch=3, files=files.data_ptr(), slot=slot, sizes=sizes.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.oess_png_encode_batch(a['images'], a['n'], a['H'], a['W'], a['ch'], a['files'], a['slot'], a['sizes'], a['ws'],
                                         a['ws_bytes'], st)
    bad = [dict(images=None), dict(files=None), dict(sizes=None), dict(ws=None), dict(n=0), dict(n=-1), dict(ch=2), dict(ch=4), dict(ch=0),
           dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(slot=slot - 1), dict(slot=0), dict(ws_bytes=need - 1), dict(ws_bytes=0),
           dict(ws=ws.data_ptr() + 4),
           # 49153 segments per 16384 x 16384 x 3 image: 43690 of them pass 2^31 - 1 segments, 43689 do not
           dict(n=43690, H=16384, W=16384, slot=hip.png_encode_bound(16384, 16384, 3), ws_bytes=1 << 62)]
    for kw in bad:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((files == 0xA5).all()) and sizes.tolist() == [-7, -7]
    assert lib.oess_png_encode_scratch_bytes(43690, 16384, 16384, 3) == 0 and lib.oess_png_encode_scratch_bytes(43689, 16384, 16384, 3) > 0
    assert lib.oess_png_encode_scratch_bytes(0, H, W, 3) == 0 and lib.oess_png_encode_scratch_bytes(1, H, W, 2) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert sizes.tolist() == [len(ref.encode(np.zeros((H, W, 3), np.uint8))[0])] * 2


def test_wrapper_refuses_what_it_cannot_encode():
    from openess_amd import hip
    ok = torch.zeros((2, 8, 9), dtype=torch.uint8, device='cuda')
    bad = [ok.cpu(), ok.float(), ok.to(torch.int8), ok[:, :, ::2], ok[0], ok[None, None], torch.zeros((2, 8, 9, 4), dtype=torch.uint8, device='cuda'),
           torch.zeros((2, 8, 9, 1), dtype=torch.uint8, device='cuda'), torch.zeros((0, 8, 9), dtype=torch.uint8, device='cuda'),
           torch.zeros((1, 0, 9), dtype=torch.uint8, device='cuda'), torch.zeros((1, 2, 16385), dtype=torch.uint8, device='cuda'),
           ok.cpu().numpy(), None]
    for t in bad:
        with pytest.raises(ValueError):
            hip.png_encode_batch(t)
        with pytest.raises(ValueError):
            hip.png_encode_files(t)
    bound = hip.png_encode_bound(8, 9, 1)
    files = torch.empty((2, bound), dtype=torch.uint8, device='cuda')
    sizes = torch.empty(2, dtype=torch.int32, device='cuda')
    for out in ((files[:, :-1].contiguous(), sizes), (files[:1], sizes), (files.cpu(), sizes), (files.to(torch.int8), sizes),
                (files, sizes.long()), (files, sizes[:1]), (files, sizes.cpu()), (torch.empty((2, 2 * bound), dtype=torch.uint8, device='cuda')[:, ::2], sizes)):
        with pytest.raises(ValueError):
            hip.png_encode_batch(ok, out=out)
    with pytest.raises(ValueError):
        hip.png_encode_bound(8, 9, 2)
    hip.png_encode_batch(ok, out=(files, sizes))
