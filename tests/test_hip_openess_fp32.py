"""K23: the joint OpenESS stage (OpenESSModel, train.py's default branch) in fp32, built from tests/configs/
openess_dsec_synthetic_fp32.yaml at 64 x 96, B = 2, with the weights and batch of tests/openess_fp32_cases.py (those of
test_openess_model_step_matches_oracle: fill_by_name, damp_residual, dropout p = 0).

Loss bounds (relative, step 0 against a float64 copy of OracleOpenESSStep): four times what tools/exp_openess_fp32_bounds.py
prints for torch's own fp32 CPU run of the same step against float64, with a floor of 1e-5.  Measured on the CPU:
    semseg_frame_loss 1.415e-07, semseg_recon_loss 1.897e-07, cons_feat_loss 1.577e-07, cons_pred_loss 4.319e-07,
    contrastive_nce_loss 3.776e-06        -> bounds 1e-5, 1e-5, 1e-5, 1e-5, 1.511e-5
Measured on the MI355X (lazy_features True / False):
    semseg_frame_loss 7.25e-08 / 7.25e-08, semseg_recon_loss 1.90e-07 / 1.90e-07, cons_feat_loss 9.62e-08 / 9.62e-08,
    cons_pred_loss 3.86e-07 / 3.86e-07, contrastive_nce_loss 1.79e-06 / 1.86e-06

Gradients against float64 are not repeated at this level (K22 holds every node but the new one, and that one has
tests/test_hip_upsampled_l1_f32.py).  Instead the two fp32 routes (lazy_features True: fused node and pooling matrix; False:
materialised features) share a bit-identical network forward, hence identical ReLU masks, and each is held to K22's `model`
bound of 1.85e-4 against float64: their head gradients must agree within twice that, 3.7e-4 (measured on the MI355X: 4.2e-6 at
worst, model_recon classifier.ASPP.project.0.weight)."""
import os

import pytest
import torch

from tests import openess_fp32_cases as oc
from tests import upsampled_l1_cases as uc

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
LOSS_CPU_FP32 = {'semseg_frame_loss': 1.415e-07, 'semseg_recon_loss': 1.897e-07, 'cons_feat_loss': 1.577e-07,
                 'cons_pred_loss': 4.319e-07, 'contrastive_nce_loss': 3.776e-06}
LOSS_BOUND = {k: max(4.0 * v, 1e-5) for k, v in LOSS_CPU_FP32.items()}
ROUTE_GRAD_BOUND = 2 * 1.85e-4


def _build(yaml_name, ckpt_dir):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, yaml_name), generate_log=False)
    s.ckpt_dir = str(ckpt_dir)
    s.lr_recon = s.lr_frame = 1e-4
    trainer, loop = train.build_trainer(s)
    assert type(trainer).__name__ == 'OpenESSModel' and loop == 'training'
    assert (s.semseg_num_classes, tuple(s.img_size_b), s.output_stride) == (oc.K, oc.HW, oc.OUTPUT_STRIDE)
    for name in oc.MODELS:
        oc.prepare(trainer.models_dict[name], name)
    trainer.initial = {name: {k: v.clone() for k, v in trainer.models_dict[name].state_dict().items()} for name in oc.MODELS}
    return trainer


def _reset(trainer):
    """the shared weights again (train_step moves them), default switches"""
    for name in oc.MODELS:
        trainer.models_dict[name].load_state_dict(trainer.initial[name])
    trainer.lazy_features, trainer.two_streams = True, False
    return trainer


@pytest.fixture(scope="module")
def fp32_trainer(tmp_path_factory):
    trainer = _build("openess_dsec_synthetic_fp32.yaml", tmp_path_factory.mktemp("fp32"))
    assert trainer.train_precision == 'fp32' and trainer.eval_precision == 'fp32'
    return trainer


@pytest.fixture(scope="module")
def bf16_trainer(tmp_path_factory):
    trainer = _build("openess_dsec_synthetic.yaml", tmp_path_factory.mktemp("bf16"))
    assert trainer.train_precision == 'bf16' and trainer.eval_precision == 'bf16'
    return trainer


@pytest.fixture(scope="module")
def batch():
    frame, _, recon, pl, sp = oc.batch()
    return frame.cuda(), None, recon.cuda(), pl.cuda(), sp.cuda(), None


def _params(trainer):
    return [(name, pn, p) for name in oc.MODELS for pn, p in trainer.models_dict[name].named_parameters()]


def _zero(trainer):
    for opt in trainer.optimizers_dict.values():
        opt.zero_grad()


def _grads(trainer):
    return {(name, pn): p.grad.detach().clone() for name, pn, p in _params(trainer) if p.grad is not None}


def _backward_of_step(trainer, batch, precision=None):
    """(losses, gradients) of task_train_step + backward: the step without its optimiser update"""
    _zero(trainer)
    total, losses, _ = trainer.task_train_step(batch, precision=precision)
    total.backward()
    return losses, _grads(trainer)


@pytest.mark.parametrize("lazy", [True, False])
def test_step0_losses_match_float64(fp32_trainer, batch, lazy):
    trainer = _reset(fp32_trainer)
    trainer.lazy_features = lazy
    keys = {name: list(trainer.models_dict[name].state_dict().keys()) for name in oc.MODELS}
    want = oc.oracle_losses(keys, torch.float64)
    _, losses, _ = trainer.task_train_step(batch)
    assert set(losses) == set(oc.LOSS_KEYS) == set(want)
    errs = {k: abs(float(losses[k]) - want[k]) / abs(want[k]) for k in oc.LOSS_KEYS}
    print(f"openess fp32 step 0, lazy_features={lazy}: " + " ".join(f"{k} {errs[k]:.3e}" for k in oc.LOSS_KEYS))
    for k in oc.LOSS_KEYS:
        assert errs[k] <= LOSS_BOUND[k], (lazy, k, float(losses[k]), want[k], errs[k], LOSS_BOUND[k])


def test_two_fp32_routes_agree_on_the_head_gradients(fp32_trainer, batch):
    trainer = _reset(fp32_trainer)
    out = {}
    for lazy in (True, False):
        trainer.lazy_features = lazy
        out[lazy] = _backward_of_step(trainer, batch)
    trainer.lazy_features = True
    for k in ('semseg_frame_loss', 'semseg_recon_loss', 'cons_pred_loss'):      # the network forward is the same, bit for bit
        assert torch.equal(out[True][0][k], out[False][0][k]), k
    worst = 0.0
    for name in oc.MODELS:
        for pn in oc.HEAD_PARAMS:
            e = uc.relerr(out[True][1][(name, pn)].cpu().numpy(), out[False][1][(name, pn)].cpu().numpy())
            print(f"openess fp32 routes, {name} {pn}: relerr {e:.3e}")
            worst = max(worst, e)
            assert e <= ROUTE_GRAD_BOUND, (name, pn, e)
    print(f"openess fp32 routes: worst head-gradient relerr {worst:.3e}")


def test_train_step_is_the_node_calls_made_by_hand(fp32_trainer, batch):
    from openess_amd import hip
    trainer = _reset(fp32_trainer)
    s, (frame, _, recon, pl, sp, _) = trainer.settings, batch
    _zero(trainer)
    for m in trainer.models_dict.values():
        m.train()
    logits_frame, feat_frame = trainer.model_frame.forward_fp32_train(frame, want_feats='lazy')
    assert isinstance(feat_frame, hip.UpsampledFeature) and feat_frame.x.dtype == torch.float32
    assert feat_frame.size == oc.HW and tuple(feat_frame.x.shape) == (oc.B, 256, oc.HW[0] // 16, oc.HW[1] // 16)     # case 7 of the node
    total = trainer.task_loss(logits_frame, pl) * s.weight_task_loss
    logits_recon, feat_recon = trainer.model_recon.forward_fp32_train(recon, want_feats='lazy')
    total = total + trainer.task_loss(logits_recon, pl) * s.weight_task_loss
    total = total + hip.upsampled_l1_mean(feat_frame, feat_recon)
    total = total + hip.cosine_mean_loss(logits_frame, logits_recon)
    sps = trainer.pool_superpixel_size
    S = int((sp + torch.arange(0, oc.B * sps, sps, device=sp.device)[:, None, None]).max().item()) + 1
    m = hip.pool_matrix(sp, feat_recon.x.shape[2:], sps, S, False)
    total = total + trainer.nce_loss(feat_recon.pool(sp, sps, S, matrix=m), feat_frame.pool(sp, sps, S, matrix=m))
    total.backward()
    by_hand = _grads(trainer)
    losses, _, t_loss = trainer.train_step(batch)                        # precision None: the YAML's fp32
    assert set(losses) == set(oc.LOSS_KEYS) and torch.equal(t_loss, total.detach())
    got = _grads(trainer)
    assert set(got) == set(by_hand) and len(got) > 100
    for k in by_hand:
        assert torch.equal(got[k], by_hand[k]), k


def test_precision_argument_on_a_bf16_built_trainer(fp32_trainer, bf16_trainer, batch):
    a, b = _reset(fp32_trainer), _reset(bf16_trainer)
    la, _, ta = a.train_step(batch)
    lb, _, tb = b.train_step(batch, precision='fp32')
    assert torch.equal(ta, tb) and all(torch.equal(la[k], lb[k]) for k in oc.LOSS_KEYS)
    ga, gb = _grads(a), _grads(b)
    assert set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # the default of the bf16-built trainer is still the bf16 step: another arithmetic, other bits
    lb16, _, _ = _reset(b).train_step(batch)
    assert not torch.equal(lb16['cons_feat_loss'], la['cons_feat_loss'])


def test_bad_precision_leaves_the_gradients_alone(fp32_trainer, batch):
    trainer = _reset(fp32_trainer)
    _, before = _backward_of_step(trainer, batch)
    held = {(name, pn): p.grad for name, pn, p in _params(trainer)}
    with pytest.raises(ValueError, match="precision"):
        trainer.train_step(batch, precision='fp16')
    with pytest.raises(ValueError, match="precision"):
        trainer.task_train_step(batch, precision='fp16')
    for name, pn, p in _params(trainer):
        assert p.grad is held[(name, pn)] and (p.grad is None or torch.equal(p.grad, before[(name, pn)])), (name, pn)


def test_two_streams_with_fp32_is_refused(fp32_trainer, bf16_trainer, batch):
    for trainer, precision in ((_reset(fp32_trainer), None), (_reset(bf16_trainer), 'fp32')):
        trainer.two_streams = True
        try:
            with pytest.raises(NotImplementedError, match="two_streams"):
                trainer.train_step(batch, precision=precision)
        finally:
            trainer.two_streams = False


def test_val_logits_fp32(fp32_trainer, bf16_trainer, batch):
    for trainer, precision in ((_reset(fp32_trainer), None), (_reset(bf16_trainer), 'fp32')):
        model = trainer.models_dict['model_recon']
        model.train()
        model.backbone.eval()                                             # a mixed state: every flag must come back as it was
        modes = [m.training for m in model.modules()]
        with torch.no_grad():
            got = trainer.val_logits(batch, precision=precision)
        assert [m.training for m in model.modules()] == modes
        with torch.no_grad():
            want = model.eval().forward_fp32(batch[2])[0]
        model.train()
        assert got.dtype == torch.float32 and tuple(got.shape) == (oc.B, oc.K) + oc.HW and torch.equal(got, want)
    with pytest.raises(ValueError, match="precision"):
        fp32_trainer.val_logits(batch, precision='fp16')
    with torch.no_grad():                                                 # the bf16-built trainer's default stays the bf16 forward
        bf16_trainer.models_dict['model_recon'].eval()
        assert not torch.equal(bf16_trainer.val_logits(batch).float(), want)
    bf16_trainer.models_dict['model_recon'].train()


def test_fused_node_allocates_nothing_of_the_full_resolution():
    """forward + backward of the node at case 6's geometry: the peak stays under ONE full-resolution tensor (l1_mean on the same
    operands holds the upsampled difference and its gradient).  A condition on the design, not a speed claim."""
    from openess_amd import hip
    c = uc.case(6)
    B, C, _, _, Ho, Wo, align = uc.CASES[6]
    full = B * C * Ho * Wo * 4
    a, b = c['a'].cuda().requires_grad_(True), c['b'].cuda().requires_grad_(True)

    def peak(fn):
        a.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(hip.UpsampledFeature(a, (Ho, Wo), align), hip.UpsampledFeature(b, (Ho, Wo), align)).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    fused, chain = peak(hip.upsampled_l1_mean), peak(hip.l1_mean)
    print(f"peak bytes over the operands, case 6: fused {fused}, l1_mean chain {chain}, one full-resolution tensor {full}")
    assert fused < full <= chain
