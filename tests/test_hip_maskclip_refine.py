"""GPU tests of MaskCLIP's refinement (hip.maskclip_refine, openess_amd/csrc/maskclip_refine.hip) and of its way
through the tower (last-layer keys, MaskClipHead.refine_output, maskClipFeatureExtractor.forward / forward_fp32 with refine=True,
the online teacher of PretrainStep).

Kernel accuracy: on every case of tests/golden/maskclip_refine.npz -- operands and float64 / float32 outputs of the reference's
own refine_output -- max|out - ref64| / max|ref64| must stay within four times the same measure of the reference's float32 output,
computed from the file at run time (2.0e-7 .. 4.3e-7, bounds 8e-7 .. 1.7e-6; where the reference's float32 is exact, so must the
kernel be).  The fixture's margins (tests/test_maskclip_refine_cases.py) keep every threshold decision the same in both
precisions: no pixel and no class is left out.  Three larger cases that would not fit the fixture are drawn by the same rules and
held the same way to the float64 restatement the fixture pins.  Exact cases, the strided layouts and the composition are
torch.equal."""
import functools
import math

import pytest
import torch

from tests import maskclip_refine_cases as rc
from tests import maskclip_refine_reference as rr
from tests import vit_f32_cases as fc

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _run(c, **kw):
    from openess_amd import hip
    k = c["k"].cuda()
    if c["k_bf16"]:
        k = k.bfloat16()                                     # the stored values are bf16 values: nothing is rounded here
    return hip.maskclip_refine(c["output"].cuda(), k, c["pd"], c["ks"], **kw)


def _held(name, c):
    out = _run(c)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(c["ref64"].shape)
    err, fig = rc.rel_max(out, c["ref64"]), rc.rel_max(c["ref32"], c["ref64"])
    print(f"maskclip_refine {name}: {err:.3e} (reference fp32 {fig:.3e}, bound {rc.BOUND_FACTOR * fig:.3e})")
    assert bool(torch.isfinite(out).all())
    assert err <= rc.BOUND_FACTOR * fig
    assert torch.equal(_run(c), out), "two calls differ"


@pytest.mark.parametrize("name", list(rc.CASES))
def test_refine_matches_the_reference_float64(name):
    _held(name, rc.case(name))


@pytest.mark.parametrize("name", list(rc.EXTRA_CASES))
def test_refine_at_the_widest_shapes(name):
    _held(name, rc.extra_case(name))


# --------------------------------------------------------------------------------------------- exact cases
def test_identity_keys_return_p():
    from openess_amd import hip
    out, k = rc.identity_case()
    smoothed = hip.maskclip_refine(out.cuda(), k.cuda(), 0.5, 1.0)
    plain = hip.maskclip_refine(out.cuda(), k.cuda(), 0.5, 1e-30)
    p64 = rr.refine(out, k, 0.5, 1e-30)
    assert bool((plain.cpu().double().max(dim=1).values < 1.0).any())           # pixels were smoothed under ks_thresh = 1
    assert rc.rel_max(plain, p64) < 1e-6 and torch.equal(smoothed, plain)


def test_grouped_keys_give_dyadic_group_means():
    from openess_amd import hip
    out, k, expect = rc.grouped_case()
    assert bool((k.abs().sum(dim=1) == 0).any())                                # zero channels: the 1e-12 clamp is taken
    for kk in (k.cuda(), k.cuda().bfloat16()):
        got = hip.maskclip_refine(out.cuda(), kk, 0.5, 2.0)
        assert not bool(torch.isnan(got).any()) and torch.equal(got.cpu(), expect)


def test_smoothing_off_masks_with_minus_100_and_copies_the_rest():
    from openess_amd import hip
    c = rc.case("k11_5x7_c64_ks0")
    x = c["output"].cuda()
    saved = x.clone()
    conf = torch.softmax(100 * c["output"].double(), dim=1).flatten(2).max(dim=2).values
    masked = (conf < c["pd"])[:, :, None, None].expand_as(c["output"])
    expect = torch.where(masked, torch.full_like(c["output"], -100.0), c["output"])
    assert bool(masked.any()) and not bool(masked.all())
    for got in (hip.maskclip_refine(x, c["k"].cuda(), c["pd"], 0.0), hip.maskclip_refine(x, None, c["pd"], 1.0)):
        assert torch.equal(got.cpu(), expect)
    assert torch.equal(hip.maskclip_refine(x, None, 0.0, 1.0), x) and torch.equal(x, saved)      # nothing to do: a copy; input untouched


def test_one_class_is_exactly_one():
    c = rc.case("k1_2x3_c64")
    assert torch.equal(_run(c).cpu(), torch.ones(rc.N, 1, 2, 3))


# --------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("name,k_dtype", [("k11_3x43_c192", torch.float32), ("k11_5x7_c64_kbf16", torch.bfloat16)])
def test_strided_operands_and_sentinels(name, k_dtype):
    """k read in place from a [B (L + 1), C + 8] token matrix whose class-token rows and pad columns hold NaN; logits in the
    tower's NHWC memory; out a slice of a sentinel-filled buffer"""
    from openess_amd import hip
    c = rc.case(name)
    n, K, H, W = c["output"].shape
    L, C = H * W, c["k"].shape[2]
    dense = _run(c)
    tok = torch.full((n * (L + 1), C + 8), math.nan, dtype=k_dtype, device="cuda")
    kview = tok.view(n, L + 1, C + 8)[:, 1:, :C]
    kview.copy_(c["k"].cuda())
    assert kview.stride() == ((L + 1) * (C + 8), C + 8, 1) and bool(torch.isnan(tok).any())
    x = c["output"].cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    buf = torch.full((n, K + 1, H + 2, W + 3), SENTINEL, device="cuda")
    out = buf[:, :K, 1:H + 1, 2:W + 2]
    got = hip.maskclip_refine(x, kview, c["pd"], c["ks"], out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, dense)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[:, :K, 1:H + 1, 2:W + 2] = True
    assert bool((buf[~inside] == SENTINEL).all())
    default = hip.maskclip_refine(x, kview, c["pd"], c["ks"])
    assert default.stride() == x.stride() and torch.equal(default, dense)                       # the logits' layout


# --------------------------------------------------------------------------------------------- key path
def _mirror_layer():
    from openess_amd.models.maskclip_model import TransformerEncoderLayer
    g = rc.golden()
    C = rc.LAYER["C"]
    layer = TransformerEncoderLayer(embed_dims=C, num_heads=1, feedforward_channels=C)
    ops = {k: torch.from_numpy(g["layer/" + k]) for k in ("x", "ln1_w", "ln1_b", "in_w", "in_b", "out_w", "out_b")}
    with torch.no_grad():
        layer.ln1.weight.copy_(ops["ln1_w"]), layer.ln1.bias.copy_(ops["ln1_b"])
        a = layer.attn.attn
        a.in_proj_weight.copy_(ops["in_w"]), a.in_proj_bias.copy_(ops["in_b"])
        a.out_proj.weight.copy_(ops["out_w"]), a.out_proj.bias.copy_(ops["out_b"])
    return layer.cuda().eval(), ops, torch.from_numpy(g["layer/k64"])


def test_last_layer_keys_match_the_reference_float64():
    """the mirror's key path on the fixture's layer against the k the reference's layer returned in float64"""
    layer, ops, k64 = _mirror_layer()
    B, T, C = ops["x"].shape
    x = ops["x"].reshape(B * T, C).cuda()
    fig = rc.rel_max(rr.last_layer_k(**ops, dtype=torch.float32), k64)            # torch fp32 of the same composition, CPU
    with torch.no_grad():
        k32 = layer.forward_key_path_fp32(x)
        kbf = layer.forward_key_path(x.bfloat16())
    err = rc.rel_max(k32.view(B, T, C), k64)
    print(f"last-layer k fp32: {err:.3e} (torch fp32 {fig:.3e}, bound {rc.BOUND_FACTOR * fig:.3e})")
    assert k32.dtype == torch.float32 and err <= rc.BOUND_FACTOR * fig
    assert kbf.dtype == torch.bfloat16
    assert float((kbf.float().cpu().view(B, T, C).double() - k64).abs().max()) < 4e-2 * float(k64.abs().max())     # the bf16 v_map's tolerance


# --------------------------------------------------------------------------------------------- composition
@pytest.fixture(scope="module")
def mirrors():
    cache = {}

    def get(img_size):
        if img_size not in cache:
            cache[img_size] = fc.tower_pair(img_size)[1]
        return cache[img_size]
    return get


@pytest.mark.parametrize("case", list(range(len(fc.TOWER_CASES))))
def test_refined_forward_is_the_composition_of_its_public_pieces(case, mirrors):
    from openess_amd import hip
    img_size, hw, B = fc.TOWER_CASES[case]
    m = mirrors(img_size)
    img = fc.tower_image(case).cuda()
    hp, wp = (hw[0] + 15) // 16, (hw[1] + 15) // 16
    plain32, plain16 = m.forward_fp32(img), m(img)
    # fp32
    v_map, k = m.encoder.forward_fp32(img, return_k=True)
    _, logits = m.decoder.forward_fp32(v_map)
    assert k.dtype == torch.float32 and tuple(k.shape) == (B, hp * wp, 768) and k.stride() == ((hp * wp + 1) * 768, 768, 1)
    want = hip.bilinear_resize(hip.maskclip_refine(logits, k, 0.5, 1.0), size=hw, align_corners=False)
    got = m.forward_fp32(img, refine=True)
    assert tuple(got.shape) == (B, 11, *hw) and torch.equal(got, want) and not torch.equal(got, plain32)
    assert torch.equal(m.decoder.refine_output(logits, k), hip.maskclip_refine(logits, k, 0.5, 1.0))
    # bf16
    v_map, k = m.encoder(img, return_k=True)
    _, logits = m.decoder(v_map)
    assert k.dtype == torch.bfloat16 and tuple(k.shape) == (B, hp * wp, 768) and logits.dtype == torch.float32
    want = hip.bilinear_resize(hip.maskclip_refine(logits, k, 0.5, 1.0), size=hw, align_corners=False)
    got = m(img, refine=True)
    assert torch.equal(got, want) and not torch.equal(got, plain16)
    # the unrefined forwards are what they were, before and after a refined call
    assert torch.equal(m.forward_fp32(img), plain32) and torch.equal(m.forward_fp32(img, refine=False), plain32)
    assert torch.equal(m(img), plain16) and torch.equal(m(img, refine=False), plain16)
    assert torch.equal(m.encoder.forward_fp32(img), m.encoder.forward_fp32(img, return_k=True)[0])


# --------------------------------------------------------------------------------------------- step
def test_refined_online_teacher_labels_in_the_step():
    """tests/test_hip_maskclip_fp32.py's online-teacher check with the refined bf16 forward: the step with the refined online
    teacher equals the step fed forward(frame, refine=True).argmax(1) as offline labels (same kernels on the same labels; the
    arrival order of the step's fp32 atomics differs from run to run, hence that test's rel 2e-5)."""
    from openess_amd.training.pretrain_step import PretrainStep
    from tests.synth import damp_residual, fill_by_name
    _, m = fc.tower_pair((32, 48))
    torch.manual_seed(2)
    B, H, W, nwin = 2, 64, 96, 2
    ev = (torch.randn(B, nwin * 5, H, W) * (torch.rand(B, nwin * 5, H, W) > 0.7)).contiguous().cuda()
    frame = torch.rand(B, 3, H, W)
    with torch.no_grad():
        labels = m(frame.cuda(), refine=True).argmax(1)
    losses = []
    for teacher, pl in ((functools.partial(m, refine=True), torch.zeros_like(labels)), (None, labels)):
        st = PretrainStep(config_option="frame2voxel", img_size=(H, W), nr_events_data=nwin, if_spatial_contrastive=False, lr=1e-4,
                          online_teacher=teacher)
        for name, mod in st.models_dict.items():
            fill_by_name(mod, 100 + len(name))
            damp_residual(mod)
        ls, _, _ = st.train_step((ev, None, frame.cuda(), pl, None, None))
        losses.append(float(ls['dense_clip_loss']))
    assert losses[0] == pytest.approx(losses[1], rel=2e-5)
