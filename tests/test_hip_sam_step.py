"""if_sam_distillation in the frame2recon pre-training step (training/pretrain_trainer.py:481-482, :519-529): with
the option off the step is the step built without the keyword, bit for bit; with it on the loss dictionary carries
'sam_distillation_loss', the total is the sum of the parts, and the entry is the float64 restatement
(tests/sam_distill_reference.py) on the step's own feature and the batch's SAM features; the composed route
(pooled_student_features = False) computes the same loss; and OpenESSPretrainModel trains on the YAML key.
Geometry: the 2 x 64 x 96 batch of tests/pretrain_fp32_cases.py; DeepLabv3 leaves a 4 x 6 bf16 map of 256 channels.
Bound on the entry: the kernel bound of tests/test_hip_sam_distill.py for a bf16 map (four times torch's fp32-against-float64
figure, tools/exp_sam_distill_bounds.py)."""
import os

import pytest
import torch

from tests import pretrain_fp32_cases as pc
from tests import sam_distill_reference as sr

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
LOSS_BOUND = 4 * 1.365e-07                  # FIG[True][0] of tests/test_hip_sam_distill.py


def _step(cls=None, contrastive=True, **kw):
    from openess_amd.training.pretrain_step import PretrainStep
    st = (cls or PretrainStep)(config_option="frame2recon", img_size=(pc.H, pc.W), nr_events_data=pc.NWIN, if_spatial_contrastive=contrastive,
                               superpixel_size=pc.SPS, lr=pc.LR, **kw)
    pc.fill_models(st.models_dict)
    st.model_recon.classifier.ASPP.project[3].p = 0.0                     # no dropout: two forwards from one seed are comparable
    return st


def _batch():
    _, frame, labels, sp, S = pc.make_batch()
    return (frame.cuda(), None, frame.cuda(), labels.cuda(), sp.cuda(), S)


def _sam():
    return (1 + 0.5 * torch.randn(pc.B, 256, 64, 64, generator=torch.Generator().manual_seed(34))).cuda()


def _loss_and_grads(st, batch, **kw):
    for opt in st.optimizers_dict.values():
        opt.zero_grad()
    total, losses, _ = st.task_train_step(batch, **kw)
    total.backward()
    grads = {f"{k}.{n}": p.grad.detach().clone() for k, m in st.models_dict.items() for n, p in m.named_parameters() if p.grad is not None}
    assert grads
    return total.detach().clone(), {k: v.clone() for k, v in losses.items()}, grads


def test_option_off_is_the_step_without_the_keyword():
    (ta, la, ga), (tb, lb, gb) = _loss_and_grads(_step(sam_distillation=False), _batch(), sam_feat=_sam()), _loss_and_grads(_step(), _batch())
    assert torch.equal(ta, tb) and sorted(la) == sorted(lb) and sorted(ga) == sorted(gb) and 'sam_distillation_loss' not in la
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


@pytest.mark.parametrize("contrastive", [False, True])
def test_option_on_adds_the_reference_loss(contrastive, monkeypatch):
    from openess_amd import hip
    st = _step(contrastive=contrastive, sam_distillation=True)
    assert st.sam_distillation and st.model_recon.lazy_feats
    batch, sam = _batch(), _sam()
    with pytest.raises(ValueError, match="sam_feat"):
        st.task_train_step(batch)
    seen = []
    real_loss, real_pool = hip.sam_distill_loss, st._pool
    monkeypatch.setattr(hip, 'sam_distill_loss', lambda s, f, *a: (seen.append(('sam', f)), real_loss(s, f, *a))[1])
    monkeypatch.setattr(st, '_pool', lambda f, *a: (seen.append(('pool', f)), real_pool(f, *a))[1])
    total, losses, grads = _loss_and_grads(st, batch, sam_feat=sam)
    parts = ['sam_distillation_loss', 'dense_clip_loss'] + (['contrastive_nce_loss'] if contrastive else [])
    assert sorted(losses) == sorted(parts)
    want = 0.
    for k in (['contrastive_nce_loss'] if contrastive else []) + ['dense_clip_loss', 'sam_distillation_loss']:     # the step's order
        want = want + losses[k]
    assert torch.equal(total, want)
    assert all(bool(torch.isfinite(g.float()).all()) for g in grads.values())
    # the consumers of the student's feature read ONE stride-level map
    feats = [f for _, f in seen if isinstance(f, hip.UpsampledFeature)]
    assert [k for k, _ in seen].count('sam') == 1 and len(feats) == (2 if contrastive else 1) and all(f is feats[0] for f in feats)
    fmap = feats[0].x.detach()
    assert fmap.dtype == torch.bfloat16 and tuple(fmap.shape[:2]) == (pc.B, 256) and feats[0].size == (pc.H, pc.W)
    assert fmap.shape[2] < pc.H and fmap.shape[3] < pc.W and hip.sam_distill_supported(256, fmap.shape[2:], feats[0].size)
    loss64, _, min_norm = sr.from_map(sam, fmap.float(), (pc.H, pc.W))
    assert min_norm > sr.MIN_NORM
    err = abs(float(losses['sam_distillation_loss']) - float(loss64))
    print(f"sam step contrastive={contrastive}: sam_distillation_loss {float(losses['sam_distillation_loss']):.6f}, float64 {float(loss64):.6f}, "
          f"err {err:.3e} (bound {LOSS_BOUND:.3e})")
    assert err <= LOSS_BOUND


def test_composed_route_gives_the_same_loss():
    """pooled_student_features = False: DeepLabv3 hands over the materialised bf16 tensor and the loss takes the composed route.
    Against float64 on that tensor's own values: the kernel bound.  Against the fused step: the materialised tensor stores every
    interpolated value in bf16, |du| <= 2^-8 |u| per pixel, which moves a cosine by at most 2^-8 (|d cos| <= |du| / |u|)."""
    from openess_amd.training.pretrain_step import PretrainStep

    class Composed(PretrainStep):
        pooled_student_features = False
    batch, sam = _batch(), _sam()
    st = _step(Composed, sam_distillation=True)
    assert not st.model_recon.lazy_feats
    _, losses, _ = _loss_and_grads(st, batch, sam_feat=sam)
    st._set_modes()
    full = st.model_recon(batch[2])[1].detach()                           # train-mode BatchNorm, no dropout: the step's own feature
    assert torch.is_tensor(full) and tuple(full.shape) == (pc.B, 256, pc.H, pc.W)
    loss64, _ = sr.distill(sam.double().cpu(), full.double().cpu())
    err = abs(float(losses['sam_distillation_loss']) - float(loss64))
    _, fused, _ = _loss_and_grads(_step(sam_distillation=True), batch, sam_feat=sam)
    diff = abs(float(losses['sam_distillation_loss']) - float(fused['sam_distillation_loss']))
    print(f"sam step composed: err vs float64 {err:.3e} (bound {LOSS_BOUND:.3e}), vs the fused step {diff:.3e} (bound {2.0 ** -8:.3e})")
    assert err <= LOSS_BOUND
    assert diff <= 2.0 ** -8
    for k in ('dense_clip_loss', 'contrastive_nce_loss'):
        assert bool(torch.isfinite(losses[k])) and bool(torch.isfinite(fused[k]))


def test_trainer_trains_on_the_yaml_key(tmp_path):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, "pretrain_dsec_synthetic_frame2recon_sam.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and trainer.step.sam_distillation is True and trainer.step.config_option == 'frame2recon'
    n = 0
    for batch in trainer.device_batches(trainer.train_loader_sensor_b):
        assert tuple(batch[5].shape) == (s.batch_size_b, 256, 64, 64) and batch[5].is_cuda
        losses, _, total = trainer.train_step(batch)
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(losses['sam_distillation_loss']))
        n += 1
    assert n == 2
