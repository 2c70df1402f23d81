"""GPU tests of the fp32 MaskCLIP ViT-B/16 tower (maskClipFeatureExtractor.forward_fp32) against the float64 copy
of the CPU restatement in oracle/maskclip.py, on the oracle - mirror pair of tests/test_hip_maskclip.py::_pair:

  case 1  img_size (32, 32), image 48 x 80,   B = 2: 16 tokens, the baseline
  case 2  img_size (32, 48), image 40 x 70,   B = 2: corner padding, position-embedding resize
  case 3  img_size (32, 48), image 100 x 150, B = 1: 71 tokens, a second key tile and the padding

Logits and v_map are held to max|d| / max|ref64| within four times what torch fp32 of the same restatement shows on the CPU
(tests/vit_f32_cases.py TOWER_*_FIGURES, re-measured by tests/test_vit_f32_cases.py; 6.5e-7 .. 8.5e-7 for the logits, a bound near
3.4e-6).  The argmax, the one thing the pipeline consumes, must equal float64's on every pixel whose top-two margin is >= 1e-4
of the largest |logit|; at most 1 % of the pixels may be left out (0 %, 0.11 %, 0.07 % are)."""
import pytest
import torch

from tests import vit_f32_cases as fc

pytestmark = pytest.mark.gpu
CASES = list(range(len(fc.TOWER_CASES)))


@pytest.fixture(scope="module")
def mirrors():
    """one mirror per img_size, shared by the tests of this module and left as found"""
    cache = {}

    def get(img_size):
        if img_size not in cache:
            cache[img_size] = fc.tower_pair(img_size)[1]
        return cache[img_size]
    return get


@pytest.mark.parametrize("case", CASES)
def test_tower_fp32_matches_float64(case, mirrors):
    img_size, hw, B = fc.TOWER_CASES[case]
    _, img, ref, v64 = fc.tower_reference(case)
    m = mirrors(img_size)
    out = m.forward_fp32(img.cuda())
    v = m.encoder.forward_fp32(img.cuda())
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape) == (B, 11, hw[0], hw[1])
    assert v.dtype == torch.float32 and tuple(v.shape) == tuple(v64.shape)
    e_log, e_v = fc.rel_max(out, ref), fc.rel_max(v, v64)
    bad, left = fc.argmax_check(out, ref)
    print(f"tower fp32 case {case + 1}: logits {e_log:.3e} (figure {fc.TOWER_LOGIT_FIGURES[case]:.3e}, bound "
          f"{fc.TOWER_LOGIT_BOUNDS[case]:.3e}); v_map {e_v:.3e} (figure {fc.TOWER_VMAP_FIGURES[case]:.3e}, bound "
          f"{fc.TOWER_VMAP_BOUNDS[case]:.3e}); argmax disagreements at the margin {bad}, left out {100 * left:.2f} %")
    assert e_log <= fc.TOWER_LOGIT_BOUNDS[case]
    assert e_v <= fc.TOWER_VMAP_BOUNDS[case]
    assert left <= fc.TOWER_LEFT_OUT_CAP
    assert bad == 0
    assert torch.equal(m.forward_fp32(img.cuda()), out), "two calls differ"


def test_bf16_forward_and_state_dict_are_untouched_by_forward_fp32(mirrors):
    img_size, _, _ = fc.TOWER_CASES[1]
    o, img, _, _ = fc.tower_reference(1)
    m = mirrors(img_size)
    keys = list(m.state_dict().keys())
    assert keys == list(o.state_dict().keys())
    before = m(img.cuda())
    m.forward_fp32(img.cuda())
    assert torch.equal(m(img.cuda()), before)
    assert list(m.state_dict().keys()) == keys


def test_fp32_operands_follow_the_parameter_version(mirrors):
    """the fp32 caches are keyed by parameter version: an in-place change of a weight is seen by the next call, and undone by
    restoring it"""
    img_size, _, _ = fc.TOWER_CASES[0]
    _, img, _, _ = fc.tower_reference(0)
    m = mirrors(img_size)
    out = m.forward_fp32(img.cuda())
    w = m.encoder.layers[0].ffn.layers[1].weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(0.5)
    assert not torch.equal(m.forward_fp32(img.cuda()), out)
    with torch.no_grad():
        w.copy_(saved)
    assert torch.equal(m.forward_fp32(img.cuda()), out)


def test_fp32_online_teacher_labels_in_the_step():
    """The existing online-teacher test at 64 x 96, B = 2 with the fp32 tower: the bf16 step with online_teacher=m.forward_fp32 equals
    the step fed m.forward_fp32(frame).argmax(1) as offline labels (the two steps run the same kernels on the same labels; the
    arrival order of the fp32 atomics in the normalisation statistics and the loss reduction differs from run to run, hence rel
    2e-5), and those labels equal the float64 oracle's at the margin."""
    import copy
    from openess_amd.training.pretrain_step import PretrainStep
    from tests.synth import damp_residual, fill_by_name
    o, m = fc.tower_pair((32, 48))
    torch.manual_seed(2)
    B, H, W, nwin = 2, 64, 96, 2
    ev = (torch.randn(B, nwin * 5, H, W) * (torch.rand(B, nwin * 5, H, W) > 0.7)).contiguous().cuda()
    frame = torch.rand(B, 3, H, W)
    with torch.no_grad():
        logits = m.forward_fp32(frame.cuda())
        ref = copy.deepcopy(o).double()(frame.double())
    labels = logits.argmax(1)
    bad, left = fc.argmax_check(logits, ref)
    assert bad == 0 and left <= fc.TOWER_LEFT_OUT_CAP, (bad, left)
    losses = []
    for teacher, pl in ((m.forward_fp32, torch.zeros_like(labels)), (None, labels)):
        st = PretrainStep(config_option="frame2voxel", img_size=(H, W), nr_events_data=nwin, if_spatial_contrastive=False, lr=1e-4,
                          online_teacher=teacher)
        for name, mod in st.models_dict.items():
            fill_by_name(mod, 100 + len(name))
            damp_residual(mod)
        ls, _, _ = st.train_step((ev, None, frame.cuda(), pl, None, None))
        losses.append(float(ls['dense_clip_loss']))
    assert losses[0] == pytest.approx(losses[1], rel=2e-5)
