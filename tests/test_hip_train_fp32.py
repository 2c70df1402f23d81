"""GPU tests of the stage-2/3 trainers' fp32 training step (K19, `train_precision: fp32`): the wiring bit for bit against the same
calls made by hand, the step against the float64 oracle (oracle.step.OracleSupervisedStep with its modules in float64), a
free-running trajectory, the pipelined front step, repeatability, checkpoint interchange with the bf16 mode, and the encoder-only
fp32 E2VID step.  Geometry of tests/test_hip_trainers.py: finetune_dsec_synthetic.yaml, B = 2, its seeded events and ground truth
with one ignored band, weights by fill_by_name + damp_residual on both sides (tests/train_fp32_cases.py).

Bounds (the rule of K16 - K18): four times the largest error torch's OWN fp32 CPU autograd of the same oracle reaches against
float64 on the same cases, floor 1e-5; measured by tools/exp_train_fp32_bounds.py (CPU_FP32 below).  Gradients are compared per
tensor by |g - g64|_2 / |g64|_2: the event input cannot be conditioned as K18 conditions its latents, and one ReLU input that
rounds to the other side of zero moves single elements by a whole dY term (torch's fp32 CPU step 0 of the fine-tune case: 4.1e-3
on the tensors below such a flip, 2.4e-6 on the two later steps).  A bias in front of an InstanceNorm (analytically zero gradient)
is held to max|db - db64| <= bound * max|dW64| of its conv.  No other element is left out.

    figure                                torch fp32 CPU     bound      MI355X
    (b) loss, relative                    7.9e-08            1e-5       unmeasured
    (b) gradient, L2 ratio per tensor     4.13e-03           1.65e-2    unmeasured
    (b) norm bias / max|dW64|             5.9e-06            2.35e-5    unmeasured
    (c) loss along 5 free steps, 3 seeds  3.21e-03           1.28e-2    unmeasured
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import train_fp32_cases as tc
from tests.synth import fill_by_name

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")

CPU_FP32 = {'loss': 7.92e-8, 'grad_l2': 4.13e-3, 'norm_bias': 5.88e-6, 'trajectory': 3.21e-3}
BOUND = {k: max(4.0 * v, 1e-5) for k, v in CPU_FP32.items()}
KINDS = ('finetune', 'linear_probe', 'sup_only')


def _report(name, value, bound=None):
    print(f"[train_fp32] {name}: {value:.3e}" + (f" (bound {bound:.2e})" if bound is not None else ""), flush=True)
    return value


def _trainer(kind, tmp_path, train_precision='fp32', yaml_name="finetune_dsec_synthetic.yaml", fill=True):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, yaml_name), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.config_option = 'frame2voxel'
    s.if_finetuning, s.if_linear_probing, s.if_supervised_only = kind == 'finetune', kind == 'linear_probe', kind == 'sup_only'
    if train_precision is not None:
        s.train_precision = train_precision
    trainer, loop = train.build_trainer(s)
    assert loop == 'training' and type(trainer).__name__ == {'finetune': 'OpenESSFineTuneModel', 'linear_probe': 'OpenESSLinearProbeModel',
                                                             'sup_only': 'SupOnlyModel'}[kind]
    assert trainer.scaler is None
    keys = tc.fill_models(trainer.models_dict) if fill else None
    return trainer, s, keys


def _device_batch(seed=4):
    ev, gt = tc.make_batch(seed)
    return (ev.cuda(), gt.cuda(), None, None, None, None)


def _params(trainer):
    return {f"{k}.{n}": p for k, m in trainer.models_dict.items() for n, p in m.named_parameters()}


def _state(trainer):
    return {f"{k}.{n}": v.detach().clone() for k, m in trainer.models_dict.items() for n, v in m.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------- (a) wiring
@pytest.mark.parametrize("kind", KINDS)
def test_train_step_equals_the_same_calls_by_hand(kind, tmp_path):
    from openess_amd import hip
    trainer, s, _ = _trainer(kind, tmp_path)
    assert trainer.train_precision == 'fp32' and trainer.reconstructor_fp32.precision == 'fp32'
    batch = _device_batch()
    before = _state(trainer)
    losses, _, total = trainer.train_step(batch)
    assert set(losses) == {'semseg_sensor_b_loss'} and torch.equal(losses['semseg_sensor_b_loss'], total)

    other, s2, _ = _trainer(kind, tmp_path)                       # a second, identically filled model: the step by hand
    other._set_modes()
    rec = other.reconstructor_fp32
    rec.last_states_for_each_channel = {'grayscale': None}
    for i in range(s2.nr_events_data_b):                          # the full fp32 step (image included): same latents
        img, _, latent = rec.update_reconstruction(batch[0], channel_slice=(i * s2.input_channels_b, s2.input_channels_b))
        assert img is not None
    pred, _ = other.task_backend.forward_fp32_train({k: v.detach() for k, v in latent.items()})
    assert pred[1].dtype == torch.float32
    labels = F.interpolate(batch[1].float().unsqueeze(1), size=(other.input_height, other.input_width), mode='nearest').squeeze(1).long()
    loss, _ = hip.task_loss(pred[1], labels, s2.semseg_num_classes, 255, tuple(s2.task_loss))
    (loss * s2.weight_task_loss).backward()
    assert torch.equal(loss.detach() * s2.weight_task_loss, total)

    mine, theirs = _params(trainer), _params(other)
    n_trainable = 0
    for n, p in mine.items():
        if n.startswith('back_end.decoder_scale_5.'):
            assert p.requires_grad and p.grad is None and theirs[n].grad is None, n      # in the optimiser, never in the graph
            assert torch.equal(p.detach(), before[n]), n
        elif p.requires_grad:
            assert p.grad is not None and p.grad.dtype == torch.float32, n
            assert torch.equal(p.grad, theirs[n].grad), n
            assert not torch.equal(p.detach(), before[n]), n                               # the optimiser moved it
            n_trainable += p.numel()
        else:
            assert p.grad is None and torch.equal(p.detach(), before[n]), n
    K = s.semseg_num_classes
    in_optimiser = sum(p.numel() for g in trainer.optimizers_dict.values() for grp in g.param_groups for p in grp['params'])
    if kind == 'linear_probe':                                     # exactly the set tests/test_hip_trainers.py counts
        assert in_optimiser == K * K + K + (32 * K + K) and n_trainable == K * K + K
    else:
        assert n_trainable == in_optimiser - (32 * K + K)
        assert all(p.requires_grad for n, p in mine.items() if n.startswith('back_end.'))
    assert all(not p.requires_grad for n, p in mine.items() if n.startswith('front_sensor_b.'))


# ---------------------------------------------------------------------------------------------------- (b) against float64
@pytest.mark.parametrize("kind", ['finetune', 'linear_probe'])
def test_three_steps_match_the_float64_oracle(kind, tmp_path):
    trainer, s, keys = _trainer(kind, tmp_path)
    ref = tc.make_oracle(kind == 'linear_probe', s.lr_voxel, keys)
    ev, gt = tc.make_batch()
    batch = _device_batch()
    worst = {'loss': 0.0, 'grad_l2': 0.0, 'norm_bias': 0.0}
    for it in range(3):
        tc.copy_weights(ref, {n: m.state_dict() for n, m in trainer.models_dict.items()})
        l64, g64 = tc.oracle_loss_and_grads(ref, ev, gt, s.weight_task_loss)
        losses, _, total = trainer.train_step(batch)
        got = {n: p.grad for n, p in trainer.task_backend.named_parameters() if p.grad is not None}
        assert set(got) == set(g64), sorted(set(got) ^ set(g64))
        worst['loss'] = max(worst['loss'], tc.relerr(total, l64))
        for n, e in tc.grad_errors(got, g64).items():
            k = 'norm_bias' if tc.is_norm_bias(n) else 'grad_l2'
            if e > BOUND[k]:
                print(f"[train_fp32] {kind} step {it} {n}: {e:.3e} > {BOUND[k]:.2e}", flush=True)
            worst[k] = max(worst[k], e)
    for k, v in worst.items():
        _report(f"(b) {kind} {k}", v, BOUND[k])
    for k, v in worst.items():
        assert v <= BOUND[k], (kind, k, v, BOUND[k])


# ------------------------------------------------------------------------------------------------- (c) free-running trajectory
def test_five_free_steps_follow_the_float64_oracle(tmp_path):
    trainer, s, keys = _trainer('finetune', tmp_path)
    ref = tc.make_oracle(False, s.lr_voxel, keys)
    ev, gt = tc.make_batch()
    batch = _device_batch()
    dev = []
    for it in range(5):
        total = float(trainer.train_step(batch)[2])
        l64 = float(ref.train_step((ev.double(), gt))[1])
        dev.append(tc.relerr(total, l64))
        _report(f"(c) step {it} loss {total:.6f} float64 {l64:.6f} relerr", dev[-1], BOUND['trajectory'])
    bf16, _, _ = _trainer('finetune', tmp_path, train_precision='bf16')
    ref0 = tc.make_oracle(False, s.lr_voxel, keys)
    l0 = float(ref0.train_step((ev.double(), gt))[1])
    _report("(c) bf16 trainer, step-0 loss relerr against float64 (no assertion)", tc.relerr(bf16.train_step(batch)[2], l0))
    assert max(dev) <= BOUND['trajectory'], dev


# ---------------------------------------------------------------------------------------------------------- (d) pipelining
def _three_steps(trainer, pipelined):
    batches = [_device_batch(seed) for seed in (4, 5, 6)]
    losses = []
    front = trainer.front_step(batches[0]) if pipelined else None
    for i, batch in enumerate(batches):
        nxt = trainer.front_step(batches[i + 1]) if (pipelined and i + 1 < len(batches)) else None      # enqueued BEFORE step i
        if pipelined:
            assert front is not None
        losses.append(trainer.train_step(batch, front=front)[2])
        front = nxt
    torch.cuda.synchronize()
    return torch.stack(losses), _state(trainer)


@pytest.mark.parametrize("kind", ['finetune', 'linear_probe'])
def test_pipelined_front_step_changes_no_bit(kind, tmp_path):
    la, wa = _three_steps(_trainer(kind, tmp_path)[0], True)
    lb, wb = _three_steps(_trainer(kind, tmp_path)[0], False)
    assert torch.equal(la, lb), (la, lb)
    assert bool(torch.isfinite(la).all()) and len(set(la.tolist())) == 3
    for n in wa:
        assert torch.equal(wa[n], wb[n]), n


# -------------------------------------------------------------------------------------------------------- (e) repeatability
def test_two_trainers_from_one_seed_end_in_the_same_bits(tmp_path):
    runs = []
    for _ in range(2):
        trainer, _, _ = _trainer('finetune', tmp_path)
        batch = _device_batch()
        for _ in range(3):
            trainer.train_step(batch)
        opt = trainer.optimizers_dict['optimizer_voxel']
        moments = [(opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for grp in opt.param_groups for p in grp['params']
                   if p in opt.state]
        runs.append((_state(trainer), moments))
        torch.randn(1 << 20, device="cuda").sum()
    assert len(runs[0][1]) == len(runs[1][1]) > 0
    for n in runs[0][0]:
        assert torch.equal(runs[0][0][n], runs[1][0][n]), n
    for (m0, v0), (m1, v1) in zip(runs[0][1], runs[1][1]):
        assert torch.equal(m0, m1) and torch.equal(v0, v1)


# ---------------------------------------------------------------------------------------------------------- (f) interchange
def test_fp32_checkpoint_loads_into_a_bf16_trainer(tmp_path):
    fp32, s, _ = _trainer('finetune', tmp_path)
    batch = _device_batch()
    fp32.train_step(batch)
    bf16, _, _ = _trainer('finetune', tmp_path, train_precision='bf16', fill=False)
    assert bf16.train_precision == 'bf16' and getattr(bf16, 'reconstructor_fp32', None) is None
    assert sorted(fp32.models_dict) == sorted(bf16.models_dict) and sorted(fp32.optimizers_dict) == sorted(bf16.optimizers_dict)
    for name, m in fp32.models_dict.items():
        sd = m.state_dict()
        assert list(sd) == list(bf16.models_dict[name].state_dict())
        bf16.models_dict[name].load_state_dict(sd, strict=True)
    for name, opt in fp32.optimizers_dict.items():
        sd = opt.state_dict()
        own = bf16.optimizers_dict[name].state_dict()
        assert [g['params'] for g in sd['param_groups']] == [g['params'] for g in own['param_groups']]
        bf16.optimizers_dict[name].load_state_dict(sd)
        assert sorted(bf16.optimizers_dict[name].state_dict()['state']) == sorted(sd['state'])
    for n, p in _params(fp32).items():
        assert torch.equal(p.detach(), _params(bf16)[n].detach()), n
    logits = bf16.val_logits(batch)
    assert logits.shape == (tc.B, tc.K, tc.H, tc.W) and bool(torch.isfinite(logits.float()).all())
    total = bf16.train_step(batch)[2]
    assert bool(torch.isfinite(total))


# --------------------------------------------------------------------------------------------------------- (g) encoder-only
def test_encoder_only_fp32_e2vid_returns_the_same_bits():
    from types import SimpleNamespace
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    model = fill_by_name(E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG), 7).cuda().eval()
    g = torch.Generator().manual_seed(11)
    H, W = 32, 48
    windows = [(torch.randn(1, 5, H, W, generator=g) * (torch.rand(1, 5, H, W, generator=g) > 0.7)).cuda() for _ in range(2)]

    def run(step):
        states, seen = None, []
        for x in windows:
            img, states, latent = step(x, states)
            seen.append((img, {k: v.clone() for k, v in latent.items()},
                         [(st['xh'].clone(), st['cell'].clone(), st['fresh']) for st in states]))
        return seen

    unet = model.unetrecurrent
    full = run(lambda x, st: unet.forward_fp32(x, st))
    enc = run(lambda x, st: unet.forward_fp32(x, st, reconstruct=False))
    for (img_f, lat_f, st_f), (img_e, lat_e, st_e) in zip(full, enc):
        assert img_f is not None and img_f.shape == (1, 1, H, W) and img_e is None
        assert sorted(lat_f) == sorted(lat_e) == [1, 2, 4, 8]
        for k in lat_f:
            assert lat_e[k].dtype == torch.float32 and torch.equal(lat_f[k], lat_e[k]), k
        assert len(st_f) == len(st_e) == unet.num_encoders
        for (xh_f, c_f, fresh_f), (xh_e, c_e, fresh_e) in zip(st_f, st_e):
            assert torch.equal(xh_f, xh_e) and torch.equal(c_f, c_e) and fresh_f == fresh_e
    assert not torch.equal(full[0][1][8], full[1][1][8])                       # the two windows differ: the state carried over

    def reconstructor_run(**kw):
        rec = ImageReconstructor(model, H, W, 5, torch.device('cuda'), SimpleNamespace(precision='fp32'))
        out = []
        for x in windows:
            img, _, latent = rec.update_reconstruction(x, **kw)
            out.append((img, {k: v.clone() for k, v in latent.items()}))
        return out
    for (img_f, lat_f), (img_e, lat_e) in zip(reconstructor_run(), reconstructor_run(latents_only=True)):
        assert img_f is not None and img_e is None
        for k in lat_f:
            assert torch.equal(lat_f[k], lat_e[k]), k


# ---------------------------------------------------------------------------------------------------------- (h) default mode
def test_unchanged_yaml_trains_in_bf16_without_an_fp32_reconstructor(tmp_path):
    trainer, s, _ = _trainer('finetune', tmp_path, train_precision=None, fill=False)
    assert s.train_precision == 'bf16' and trainer.train_precision == 'bf16'
    assert getattr(trainer, 'reconstructor_fp32', None) is None
    assert trainer.reconstructor.precision == 'bf16'


def test_shipped_fp32_yaml_builds_the_fp32_trainer(tmp_path):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, "finetune_dsec_synthetic_fp32.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert type(trainer).__name__ == 'OpenESSFineTuneModel' and trainer.train_precision == 'fp32' and trainer.eval_precision == 'bf16'
    tc.fill_models(trainer.models_dict)
    assert bool(torch.isfinite(trainer.train_step(_device_batch())[2]))
