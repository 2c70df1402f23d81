"""maskClipFeatureExtractor.labels: the pseudo-labels from the stride-level logits on hip.argmax_labels are the
integers of forward(...).argmax(1) / forward_fp32(...).argmax(1), plain and refined, on a seeded tower at 2 x 3 x 32 x 48, K = 5."""
import pytest
import torch

from tests import vit_f32_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tower():
    m = fc.tower_pair((32, 48), K=5)[1]
    torch.manual_seed(7)
    return m, torch.rand(2, 3, 32, 48).cuda()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("refine", [False, True])
def test_labels_equal_the_argmax_of_the_forward(tower, refine, precision):
    m, img = tower
    full = (m.forward_fp32 if precision == 'fp32' else m)(img, refine=refine)
    assert tuple(full.shape) == (2, 5, 32, 48)
    got = m.labels(img, refine=refine, precision=precision)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 32, 48) and got.is_contiguous()
    assert torch.equal(got, full.argmax(1))
    if not refine:
        assert len(got.unique()) > 1                                      # not a constant map (the refined one is, on this 2 x 3 grid)
        if precision == 'bf16':
            assert torch.equal(m.labels(img), got)                        # the defaults


def test_labels_refuses_another_precision(tower):
    m, img = tower
    with pytest.raises(ValueError, match="precision"):
        m.labels(img, precision='fp16')
