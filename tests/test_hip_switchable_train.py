"""if_switchable_train on the GPU (training/pretrain_trainer.py:512-517, :550-562): before the switch epoch a
step built with the flag is the step built without it, bit for bit; from the switch epoch on the dense-CLIP pseudo-labels are the
argmax of the student's own logits (hip.argmax_labels), the batch's labels are ignored and the online teacher -- either form --
is not called; and the trainer wires the YAML key, the epoch counter and the tower's label form into the step.
Geometry: the 2 x 64 x 96, 3-window batch of tests/pretrain_fp32_cases.py (test_pretrain_step_matches_oracle's)."""
import os

import pytest
import torch
import yaml

from tests import pretrain_fp32_cases as pc

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
# (config_option, precision): both options in bf16, frame2voxel in fp32 as well (frame2recon has no fp32 pre-training)
FORMS = [("frame2voxel", "bf16"), ("frame2recon", "bf16"), ("frame2voxel", "fp32")]
IDS = ["-".join(f) for f in FORMS]


def _step(option, precision, **kw):
    from openess_amd.training.pretrain_step import PretrainStep
    st = PretrainStep(config_option=option, img_size=(pc.H, pc.W), nr_events_data=pc.NWIN, if_spatial_contrastive=True,
                      superpixel_size=pc.SPS, lr=pc.LR, precision=precision, **kw)
    pc.fill_models(st.models_dict)
    if option == "frame2recon":
        st.model_recon.classifier.ASPP.project[3].p = 0.0                 # no dropout: two steps from one seed are comparable
    return st


def _batch(option, pl=None):
    ev, frame, labels, sp, S = pc.make_batch()
    first = ev if option == "frame2voxel" else frame
    pl = labels if pl is None else pl
    return (first.cuda(), None, frame.cuda(), pl.cuda(), sp.cuda(), S)


def _loss_and_grads(st, batch):
    for opt in st.optimizers_dict.values():
        opt.zero_grad()
    total, losses, _ = st.task_train_step(batch)
    total.backward()
    grads = {f"{k}.{n}": p.grad.detach().clone() for k, m in st.models_dict.items() for n, p in m.named_parameters() if p.grad is not None}
    assert grads
    return total.detach().clone(), {k: v.clone() for k, v in losses.items()}, grads


def _assert_same(a, b):
    (ta, la, ga), (tb, lb, gb) = a, b
    assert torch.equal(ta, tb) and sorted(la) == sorted(lb) and sorted(ga) == sorted(gb)
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def _student_logits(st, batch):
    """one extra forward of the student at the step's weights, through the calls of task_train_step (autograd on, as there): the
    logits the dense loss reads"""
    st._set_modes()
    if st.config_option == "frame2voxel":
        h = st.front(batch)
        st._join_front(h)
        pred, _ = st.task_backend.forward_fp32_train(h.content) if st.precision == 'fp32' else st.task_backend(h.content)
        return pred[1].detach()
    return st.model_recon(batch[2])[0].detach()


@pytest.mark.parametrize("option,precision", FORMS, ids=IDS)
def test_before_the_switch_epoch_the_flag_changes_nothing(option, precision):
    flagged = _step(option, precision, switchable_train=True)
    flagged.epoch_count = 4
    plain = _step(option, precision)
    assert flagged.switchable_train and not flagged.switched and flagged.switch_epoch == 5
    assert not plain.switchable_train and plain.epoch_count == 0 and plain.online_labels is None
    _assert_same(_loss_and_grads(flagged, _batch(option)), _loss_and_grads(plain, _batch(option)))


@pytest.mark.parametrize("option,precision", FORMS, ids=IDS)
def test_after_the_switch_the_labels_are_the_students_own(option, precision):
    from openess_amd import hip
    plain = _step(option, precision)
    # (train-mode BatchNorm: the extra forward moves the running statistics, which no train-mode forward reads)
    logits = _student_logits(plain, _batch(option))
    own = hip.argmax_labels(logits)
    assert own.dtype == torch.int64 and tuple(own.shape) == (pc.B, pc.H, pc.W) and torch.equal(own, logits.argmax(dim=1))
    want = _loss_and_grads(plain, _batch(option, pl=own.cpu()))
    switched = _step(option, precision, switchable_train=True)
    switched.epoch_count = 5
    assert switched.switched
    got = _loss_and_grads(switched, _batch(option, pl=torch.full((pc.B, pc.H, pc.W), 255)))      # all ignored, if they were read
    _assert_same(got, want)
    assert float(got[1]['dense_clip_loss']) > 0
    # where the all-ignored labels are read they give no positive dense loss (the mean over no pixel: NaN, as F.cross_entropy's)
    unread = _step(option, precision)
    _, losses, _ = unread.task_train_step(_batch(option, pl=torch.full((pc.B, pc.H, pc.W), 255)))
    assert not float(losses['dense_clip_loss']) > 0


class _Counting:
    def __init__(self, result):
        self.calls, self.result = 0, result

    def __call__(self, frame):
        self.calls += 1
        return self.result


@pytest.mark.parametrize("option", ["frame2voxel", "frame2recon"])
def test_the_teacher_is_not_called_after_the_switch(option):
    labels = torch.randint(0, pc.K, (pc.B, pc.H, pc.W), generator=torch.Generator().manual_seed(4)).cuda()
    logits = torch.randn(pc.B, pc.K, pc.H, pc.W, generator=torch.Generator().manual_seed(5)).cuda()
    batch = _batch(option)
    # the logits form alone: once per front before the switch, as without the flag
    teacher = _Counting(logits)
    st = _step(option, "bf16", online_teacher=teacher, switchable_train=True)
    st.epoch_count = 4
    h = st.front(batch)
    st._join_front(h)
    assert teacher.calls == 1 and torch.equal(h.online_pl, logits.argmax(dim=1))
    st.epoch_count = 5
    h = st.front(batch)
    st._join_front(h)
    assert teacher.calls == 1 and h.online_pl is None
    # both forms: the label form is the one that is called
    teacher, labeller = _Counting(logits), _Counting(labels)
    st = _step(option, "bf16", online_teacher=teacher, online_labels=labeller, switchable_train=True)
    st.epoch_count = 4
    h = st.front(batch)
    st._join_front(h)
    assert (teacher.calls, labeller.calls) == (0, 1) and h.online_pl is labels
    st.epoch_count = 5
    h = st.front(batch)
    total, losses, _ = st.task_train_step(batch, front=h)
    assert (teacher.calls, labeller.calls) == (0, 1) and h.online_pl is None
    assert bool(torch.isfinite(total)) and float(losses['dense_clip_loss']) > 0
    # without the flag the label form keeps being called, whatever the epoch
    labeller = _Counting(labels)
    st = _step(option, "bf16", online_labels=labeller)
    st.epoch_count = 7
    h = st.front(batch)
    st._join_front(h)
    assert labeller.calls == 1 and h.online_pl is labels and not st.switched


def _trainer(tmp_path, path):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(path, generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and type(trainer).__name__ == 'OpenESSPretrainModel'
    pc.fill_models(trainer.models_dict)
    return trainer, s


def test_trainer_wires_the_key_and_the_epoch_counter(tmp_path):
    trainer, s = _trainer(tmp_path, os.path.join(CFG, "pretrain_dsec_synthetic_switchable.yaml"))
    assert s.if_switchable_train is True and trainer.step.switchable_train is True and trainer.step.switch_epoch == 5
    assert trainer.step.online_labels is None and trainer.step.online_teacher is None
    batch = _batch("frame2voxel", pl=torch.full((pc.B, pc.H, pc.W), 255))
    trainer.epoch_count = 4
    _, losses, _ = trainer.task_train_step(batch, front=trainer.front_step(batch))
    assert trainer.step.epoch_count == 4 and not trainer.step.switched and not float(losses['dense_clip_loss']) > 0   # labels read
    trainer.epoch_count = 5
    losses, _, total = trainer.train_step(batch)
    assert trainer.step.epoch_count == 5 and trainer.step.switched
    assert bool(torch.isfinite(total)) and float(losses['dense_clip_loss']) > 0
    trainer.epoch_count = 6
    trainer.front_step(batch)
    assert trainer.step.epoch_count == 6
    # the same YAML with the key off, and without the if_finetuning block that carries it: the flag is off
    cfg = yaml.load(open(os.path.join(CFG, "pretrain_dsec_synthetic_switchable.yaml")), yaml.Loader)
    cfg['clip']['if_switchable_train'] = False
    (tmp_path / "off.yaml").write_text(yaml.dump(cfg))
    assert _trainer(tmp_path, str(tmp_path / "off.yaml"))[0].step.switchable_train is False
    for key in ('if_finetuning', 'if_switchable_train'):
        del cfg['clip'][key]
    (tmp_path / "absent.yaml").write_text(yaml.dump(cfg))
    trainer, s = _trainer(tmp_path, str(tmp_path / "absent.yaml"))
    assert not hasattr(s, 'if_switchable_train') and trainer.step.switchable_train is False


def test_trainer_hands_the_step_the_towers_label_form(tmp_path):
    """pl_sources: online_maskclip builds online_labels from maskClipFeatureExtractor.labels with the trainer's precision / refine
    choices, next to the logits form of the same tower"""
    import functools
    from openess_amd.models.maskclip_model import maskClipFeatureExtractor
    from openess_amd.training.base_trainer_ov import online_maskclip_refine
    for name, precision, refine in (("pretrain_dsec_synthetic_online_maskclip_fp32.yaml", 'fp32', False),
                                    ("pretrain_dsec_synthetic_online_maskclip_refine.yaml", 'bf16', True)):
        trainer, s = _trainer(tmp_path, os.path.join(CFG, name))
        assert getattr(s, 'online_teacher_precision', 'bf16') == precision and (online_maskclip_refine(s) is not None) == refine
        lab = trainer.step.online_labels
        assert isinstance(lab, functools.partial) and lab.keywords == {'refine': refine, 'precision': precision}
        assert isinstance(lab.func.__self__, maskClipFeatureExtractor) and lab.func.__func__ is maskClipFeatureExtractor.labels
        assert trainer.step.online_teacher is not None and trainer.step.switchable_train is False
