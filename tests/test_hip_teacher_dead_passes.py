"""The frozen teacher without its redundant BatchNorm passes (EXPERIMENTS.md R6-13), every comparison to the bit:
  A  oess_norm_apply2_nhwc_bf16 (both branches of a downsample bottleneck normalised in one pass) against the two
     oess_norm_apply_nhwc_bf16 passes it replaces;
  B  oess_maxpool3x3s2_affine_relu_fwd_nhwc_bf16 (BatchNorm + ReLU applied per tap) against apply -> max_pool_3x3s2;
  C  oess_conv2d_stats_only_bf16 (conv1x1_w128_kernel<false>) against the storing kernel's tile statistics, nothing else written;
  the dilated ResNet-50 teacher with the three switches on and off, on a map large enough for the separate-apply route
  (2 x 3 x 576 x 576: M = 41 472 = 324 tiles) and on one that stays on the one-launch small-map kernel (2 x 3 x 64 x 96).
The reference forward of each model size is computed once per module and shared."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIE = 2.0 ** -8         # half a bf16 ulp in [1, 2): 1 + k / 128 + TIE is an exact tie in fp32


@pytest.fixture(scope="module")
def lib():
    from openess_amd import _lib
    return _lib.load()


def _check(code, what):
    from openess_amd import _lib
    _lib.check(code, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sliced(pixels, C, extra, gen, lo=-2.0, hi=2.0):
    """[pixels, C] bf16 view with pixel stride C + extra inside a wider buffer (extra = 0: dense)"""
    buf = (torch.rand(pixels, C + extra, device=DEV, generator=gen) * (hi - lo) + lo).bfloat16()
    off = (extra // 2) // 8 * 8
    return buf, buf[:, off:off + C]


# ------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("pixels", [1, 7, 4099])          # 4099: several workgroups, no multiple of 256 / 32 / 1 x 4 rows per block
@pytest.mark.parametrize("C", [8, 64, 2048])              # 2048: one thread per 16-byte chunk, one pixel row per block
def test_apply2_equals_the_two_apply_passes(lib, C, pixels, relu):
    gen = torch.Generator(device=DEV).manual_seed(1000 * C + 10 * pixels + relu)
    xb, x = _sliced(pixels, C, 16, gen)                   # three tensors, three different pixel strides, all larger than C
    x2b, x2 = _sliced(pixels, C, 24, gen)
    ob = torch.full((pixels, C + 8), 3.0, dtype=torch.bfloat16, device=DEV)
    scale, shift, scale2, shift2 = (torch.randn(C, device=DEV, generator=gen) for _ in range(4))
    scale[1], scale2[2], scale2[3] = -1.5, -0.75, 0.0     # negative and zero scales on either branch
    # channels 4 .. 7: x2 * 1 + 2^-8 with x2 = 1 + k / 128 is an exact bf16 tie (rounds to even: up for odd k, down for even);
    # channels 6, 7: so is the main branch's own sum, x * 1 + 0 + id + ... left to the random data of x
    x2[:, 4:8] = (1.0 + torch.randint(0, 128, (pixels, 4), device=DEV, generator=gen).float() / 128.0).bfloat16()
    scale2[4:8], shift2[4:8] = 1.0, TIE
    x[:, 6:8] = (1.0 + torch.randint(0, 64, (pixels, 2), device=DEV, generator=gen).float() / 64.0).bfloat16()
    scale[6:8], shift[6:8] = 1.0, 2.0 * TIE               # 1 + k/64 + 2^-7 + id (in [1, 2]) = a tie of the [2, 4) binade
    out = ob[:, 8:]
    _check(lib.oess_norm_apply2_nhwc_bf16(x.data_ptr(), x.stride(0), scale.data_ptr(), shift.data_ptr(), x2.data_ptr(), x2.stride(0),
                                          scale2.data_ptr(), shift2.data_ptr(), relu, pixels, C, out.data_ptr(), out.stride(0), _st()),
           "oess_norm_apply2_nhwc_bf16")
    ident = torch.full((pixels, C + 32), 5.0, dtype=torch.bfloat16, device=DEV)[:, 16:16 + C]
    ref = torch.full((pixels, C), 7.0, dtype=torch.bfloat16, device=DEV)
    _check(lib.oess_norm_apply_nhwc_bf16(x2.data_ptr(), x2.stride(0), scale2.data_ptr(), shift2.data_ptr(), None, 0, 0, 1, pixels, C,
                                         ident.data_ptr(), ident.stride(0), _st()), "oess_norm_apply_nhwc_bf16")
    _check(lib.oess_norm_apply_nhwc_bf16(x.data_ptr(), x.stride(0), scale.data_ptr(), shift.data_ptr(), ident.data_ptr(), ident.stride(0),
                                         relu, 1, pixels, C, ref.data_ptr(), C, _st()), "oess_norm_apply_nhwc_bf16")
    assert torch.equal(_bits(out), _bits(ref))
    assert torch.equal(ob[:, :8], torch.full_like(ob[:, :8], 3.0))           # the slice's neighbours untouched
    # the ties are ties: the identity of channels 4 .. 7 is 1 + (k + (k odd)) / 128 exactly
    k = ((x2[:, 4:8].float() - 1.0) * 128.0).round()
    assert torch.equal(ident[:, 4:8].float(), 1.0 + (k + k % 2) / 128.0)
    # in place, as the model calls it (out = x)
    _check(lib.oess_norm_apply2_nhwc_bf16(x.data_ptr(), x.stride(0), scale.data_ptr(), shift.data_ptr(), x2.data_ptr(), x2.stride(0),
                                          scale2.data_ptr(), shift2.data_ptr(), relu, pixels, C, x.data_ptr(), x.stride(0), _st()),
           "oess_norm_apply2_nhwc_bf16")
    assert torch.equal(_bits(x), _bits(ref))


# ------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 8)])
def test_affine_relu_pool_equals_apply_then_pool(lib, H, W, C):
    from openess_amd import hip
    gen = torch.Generator(device=DEV).manual_seed(100 * H + 10 * W + C)
    B = 2
    xb = (torch.randn(B, H, W, C + 16, device=DEV, generator=gen) * 2.0).bfloat16()
    x = xb[..., 8:8 + C]                                   # pixel stride C + 16
    scale = torch.rand(C, device=DEV, generator=gen) + 0.5
    shift = torch.randn(C, device=DEV, generator=gen)
    scale[1] = -1.25                                      # the maximum of the normalised taps is the MINIMUM of the raw ones
    scale[2] = 0.0
    shift[3] = -100.0                                     # every tap negative before the ReLU: 0 everywhere, borders included
    shift[4] = 100.0                                      # none clipped
    norm = torch.empty(B, H, W, C, dtype=torch.bfloat16, device=DEV)
    _check(lib.oess_norm_apply_nhwc_bf16(x.data_ptr(), x.stride(2), scale.data_ptr(), shift.data_ptr(), None, 0, 1, 1, B * H * W, C,
                                         norm.data_ptr(), C, _st()), "oess_norm_apply_nhwc_bf16")
    ref = hip.max_pool_3x3s2(norm.permute(0, 3, 1, 2))
    got = hip.max_pool_3x3s2_affine_relu(x.permute(0, 3, 1, 2), scale, shift)
    assert got.shape == ref.shape == (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert torch.equal(_bits(got.permute(0, 2, 3, 1)), _bits(ref.permute(0, 2, 3, 1)))
    assert float(got[:, 3].float().abs().max()) == 0.0
    # and against the definition (border windows: 1 x 1 is all border, 5 x 7 has odd edges on both axes)
    want = torch.nn.functional.max_pool2d(norm.permute(0, 3, 1, 2).float(), 3, 2, 1)
    assert torch.equal(got.float(), want)


# ------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("H", [256, 257])                 # 512 tiles of 256 x 256: the smallest M rule (3a) takes; a ragged last tile
def test_stats_only_conv_equals_the_storing_kernel(lib, H):
    """Cin 256 -> Cout 256 on 512 tiles: the smallest layer dispatch rule (3a) takes (it asks for K >= 256: a Cin of 64 stays on
    the short-K ring kernel and is refused here, checked at the end).  The entry takes no output pointer at all, so `nothing
    stored` is checked on what it does get: the statistics rows sit inside a poisoned buffer whose guard rows must survive, the
    input and the weights must be unchanged, and a poisoned tensor as large as the result, allocated beside the launch's
    operands, must keep its poison."""
    from openess_amd import hip
    B, W, Cin, Cout = 1, 512, 256, 256
    M = B * H * W
    tiles = (M + 127) // 128
    gen = torch.Generator(device=DEV).manual_seed(H)
    x = (torch.randn(B, H, W, Cin, device=DEV, generator=gen) * 0.5).bfloat16()
    w = torch.randn(Cout, Cin, 1, 1, device=DEV, generator=gen) * (1.0 / Cin ** 0.5)
    packed = hip.pack_conv_weight(w)
    assert hip.conv2d_route((B, H, W, Cin), None, False, Cout, 1, 1, tile_stats=True) == hip.ROUTE_CONV1X1_W128
    part_ref = torch.full((tiles, 2, Cout), 7.0, device=DEV)
    y = hip.conv2d_nhwc(x, packed, None, Cout, 1, 1, 1, 0, 1, tile_stats=part_ref)
    x0, p0 = x.clone(), packed.clone()
    guard = torch.full((tiles + 16, 2, Cout), 9.0, device=DEV)
    poison = torch.full((M, Cout), 3.0, dtype=torch.bfloat16, device=DEV)     # where a result would be as large as this
    part = guard[8:8 + tiles]
    _check(lib.oess_conv2d_stats_only_bf16(x.data_ptr(), Cin, B, H, W, Cin, packed.data_ptr(), Cout, part.data_ptr(), _st()),
           "oess_conv2d_stats_only_bf16")
    assert torch.equal(part, part_ref)
    assert torch.equal(guard[:8], torch.full_like(guard[:8], 9.0)) and torch.equal(guard[8 + tiles:], torch.full_like(guard[:8], 9.0))
    assert torch.equal(poison, torch.full_like(poison, 3.0))
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(packed.view(torch.uint8), p0.view(torch.uint8))
    # the statistics are those of the bf16-rounded results
    s1 = torch.cat([y.reshape(M, Cout).float(), torch.zeros(tiles * 128 - M, Cout, device=DEV)]).reshape(tiles, 128, Cout).double().sum(1)
    assert torch.allclose(part[:, 0].double(), s1, rtol=1e-4, atol=1e-2)
    # one tile too few: not the w128 GEMM's layer -> refused, nothing launched
    assert lib.oess_conv2d_stats_only_bf16(x.data_ptr(), Cin, B, 255, W, Cin, packed.data_ptr(), Cout, part.data_ptr(), _st()) == -22
    # K = 64: below the rule's K >= 256 (x read as a 64-channel slice of itself)
    assert lib.oess_conv2d_stats_only_bf16(x.data_ptr(), Cin, B, H, W, 64, packed.data_ptr(), Cout, part.data_ptr(), _st()) == -22


# ------------------------------------------------------------------------------------------------------------ model
SWITCHES = (("Bottleneck", "fuse_downsample_bn"), ("Bottleneck", "skip_dead_output"), ("ResNet", "fuse_stem_pool"))


def _teacher(seed=11):
    from openess_amd.models.image_model import DilationFeatureExtractor
    torch.manual_seed(seed)
    m = DilationFeatureExtractor().to(DEV)
    m.train()
    g = torch.Generator().manual_seed(seed)
    for mod in m.encoder.modules():                       # affine maps of either sign, and running statistics off their defaults
        if isinstance(mod, torch.nn.BatchNorm2d):
            with torch.no_grad():
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.5 + 0.25)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g))
    return m


def _buffers(m):
    return {k: v.clone() for k, v in m.encoder.state_dict().items() if "running_" in k or "num_batches" in k}


def _spy(monkeypatch):
    """counts the forms of hip.conv_bn_train_nhwc the model asks for"""
    from openess_amd import hip
    real, seen = hip.conv_bn_train_nhwc, {"defer": 0, "residual_affine": 0, "dead": 0, "plain": 0}

    def wrapped(*a, defer=False, residual_affine=None, want_output=True, **k):
        key = "defer" if defer else "residual_affine" if residual_affine is not None else "dead" if not want_output else "plain"
        seen[key] += 1
        return real(*a, defer=defer, residual_affine=residual_affine, want_output=want_output, **k)
    monkeypatch.setattr(hip, "conv_bn_train_nhwc", wrapped)
    return seen


def _reference(shape):
    """two forwards with every switch off: outputs and the buffers they leave"""
    from openess_amd.models import _resnet
    saved = [(getattr(_resnet, c), a, getattr(getattr(_resnet, c), a)) for c, a in SWITCHES]
    try:
        for cls, a, _ in saved:
            setattr(cls, a, False)
        m = _teacher()
        gen = torch.Generator().manual_seed(5)
        xs = [torch.rand(shape, generator=gen).to(DEV) for _ in range(2)]
        outs = [m.encode(x).clone() for x in xs]
        return xs, outs, _buffers(m)
    finally:
        for cls, a, v in saved:
            setattr(cls, a, v)


@pytest.fixture(scope="module")
def ref_large():
    return _reference((2, 3, 576, 576))


@pytest.fixture(scope="module")
def ref_small():
    return _reference((2, 3, 64, 96))


def _assert_same_buffers(got, want):
    assert got.keys() == want.keys() and len(want) == 3 * 53
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert all(int(v) == 2 for k, v in got.items() if "num_batches" in k)


def test_teacher_large_map_switches_on_equal_off(ref_large, monkeypatch):
    xs, outs, bufs = ref_large
    seen = _spy(monkeypatch)
    m = _teacher()
    for x, want in zip(xs, outs):
        got = m.encode(x)
        assert bool(torch.isfinite(got.float()).all())
        assert torch.equal(_bits(got.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1)))
    _assert_same_buffers(_buffers(m), bufs)
    # per forward: the stem and the four downsample convs deferred, the four block ends on the two-branch pass
    assert seen == {"defer": 10, "residual_affine": 8, "dead": 0, "plain": 2 * (53 - 9)}


def test_teacher_large_map_without_output_leaves_the_same_buffers(ref_large, monkeypatch):
    xs, _, bufs = ref_large
    seen = _spy(monkeypatch)
    m = _teacher()
    for x in xs:
        assert m.encode(x, want_output=False) is None
    _assert_same_buffers(_buffers(m), bufs)
    assert seen["dead"] == 2 and seen["defer"] == 10 and seen["residual_affine"] == 8
    # the switch off: the whole block runs, its result is dropped
    from openess_amd.models._resnet import Bottleneck
    monkeypatch.setattr(Bottleneck, "skip_dead_output", False)
    m2 = _teacher()
    for x in xs:
        assert m2.encode(x, want_output=False) is None
    _assert_same_buffers(_buffers(m2), bufs)
    assert seen["dead"] == 2


def test_teacher_small_map_stays_on_the_one_launch_route(ref_small, monkeypatch):
    xs, outs, bufs = ref_small
    seen = _spy(monkeypatch)
    m = _teacher()
    for x, want in zip(xs, outs):
        assert torch.equal(_bits(m.encode(x).permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1)))
    _assert_same_buffers(_buffers(m), bufs)
    m2 = _teacher()
    for x in xs:
        assert m2.encode(x, want_output=False) is None
    _assert_same_buffers(_buffers(m2), bufs)
    assert seen == {"defer": 0, "residual_affine": 0, "dead": 0, "plain": 4 * 53}
