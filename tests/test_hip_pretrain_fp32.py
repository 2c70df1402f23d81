"""GPU tests of fp32 pre-training of frame2voxel (K20): PretrainStep(precision='fp32'), the trainer's `train_precision: fp32` and the
two tools.  Geometry of tests/test_hip_nets.py::test_pretrain_step_matches_oracle: B = 2, 64 x 96, three sub-windows,
superpixel_size 25, lr 1e-4, weights by fill_by_name + damp_residual on both sides, one ignored label band
(tests/pretrain_fp32_cases.py).  The reference is oracle.step.OracleStep with its modules in float64.

Bounds (the rule of K16 - K19): four times the largest error torch's OWN fp32 CPU autograd of the same oracle reaches against float64
on the same cases, floor 1e-5; measured by tools/exp_pretrain_fp32_bounds.py (CPU_FP32 below).  Gradients are compared per tensor by
|g - g64|_2 / |g64|_2 over every trainable tensor of the student and of the teacher's head; a conv bias in front of an InstanceNorm
(analytically zero gradient) is held to max|db - db64| <= bound * max|dW64| of its conv.  No tensor or element is left out.  The CPU
gradient figure is that of the decoder_scale_1 conv weights (9.5e-3 without the contrastive loss, 3.9e-3 with it; every tensor of
the teacher's head and of the student's head stays below 1e-5): the layers under the most ReLUs, where K19 found single elements
moved by a whole dY term when a ReLU input rounds to the other side of zero.  That cause was not traced again here.

    figure                                     torch fp32 CPU     bound      MI355X
    (b) each loss, relative                    2.4e-07            1e-5       1.5e-07
    (b) gradient, L2 ratio per tensor          9.49e-03           3.80e-2    6.09e-03
    (b) norm bias / max|dW64|                  4.8e-06            1.92e-5    6.6e-06
    (c) every loss along 3 free steps          7.62e-04           3.05e-3    2.51e-03
    (f) pooled against materialised, loss      (bound of b)       1e-5       0
    (f) pooled against materialised, gradient  (bound of b)       3.80e-2    2.0e-06 (norm bias 2.4e-06)
"""
import json
import os

import pytest
import torch

from tests import pretrain_fp32_cases as pc

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")

CPU_FP32 = {'loss': 2.43e-7, 'grad_l2': 9.49e-3, 'norm_bias': 4.82e-6, 'trajectory': 7.63e-4}
BOUND = {k: max(4.0 * v, 1e-5) for k, v in CPU_FP32.items()}


def _report(name, value, bound=None):
    print(f"[pretrain_fp32] {name}: {value:.3e}" + (f" (bound {bound:.2e})" if bound is not None else ""), flush=True)
    return value


def _step(contr=True, cls_attrs=None, **kw):
    from openess_amd.training.pretrain_step import PretrainStep
    cls = type('Step', (PretrainStep,), dict(cls_attrs)) if cls_attrs else PretrainStep
    st = cls(config_option='frame2voxel', img_size=(pc.H, pc.W), nr_events_data=pc.NWIN, if_spatial_contrastive=contr,
             superpixel_size=pc.SPS, lr=pc.LR, precision='fp32', **kw)
    keys = pc.fill_models(st.models_dict)
    return st, keys


def _device_batch(seed=3):
    ev, frame, pl, sp, S = pc.make_batch(seed)
    return (ev.cuda(), None, frame.cuda(), pl.cuda(), sp.cuda(), S)


def _params(models):
    return {f"{k}.{n}": p for k, m in models.items() for n, p in m.named_parameters()}


def _state(models):
    return {f"{k}.{n}": v.detach().clone() for k, m in models.items() for n, v in m.state_dict().items()}


def _grads(models):
    return {n: p.grad.detach().clone() for n, p in _params(models).items() if p.grad is not None}


def _by_hand(st, batch):
    """the calls of PretrainStep.front + task_train_step in fp32, one by one, on the caller's stream; returns the total loss"""
    from openess_amd import hip
    ev, _, frame, pl, sp, S = batch
    st._set_modes()
    enc = st.model_frame.encode_fp32(frame)
    rec = st.reconstructor_fp32
    assert rec.precision == 'fp32'
    rec.last_states_for_each_channel = {'grayscale': None}
    for i in range(st.nr_events_data):
        img, _, latent = rec.update_reconstruction(ev, channel_slice=(i * st.bins, st.bins), latents_only=True)
        assert img is None
    rec.last_states_for_each_channel = {'grayscale': None}
    pred, feat_voxel = st.task_backend.forward_fp32_train({k: v.detach() for k, v in latent.items()})
    assert pred[1].dtype == torch.float32
    feat_frame = st.model_frame.head_fp32_train(enc)
    dense = st.task_loss(pred[1], pl) * st.weight_task_loss
    k = hip.superpixel_pool(feat_voxel, sp, st.superpixel_size, S=S)
    q = hip.superpixel_pool(feat_frame, sp, st.superpixel_size, S=S)
    assert k.dtype == q.dtype == torch.float32 and k.shape == q.shape == (S, 256)
    total = 0. + st.nce_loss(k, q)
    return total + dense


def _check_against_by_hand(models, optimizers, before, total, other_models, other_total):
    assert torch.equal(total, other_total.detach())
    mine, theirs = _params(models), _params(other_models)
    moved = 0
    for n, p in mine.items():
        if n.startswith('back_end.decoder_scale_5.'):
            assert p.requires_grad and p.grad is None and theirs[n].grad is None, n        # in the optimiser, never in the graph
            assert torch.equal(p.detach(), before[n]), n
        elif p.requires_grad:
            assert n.startswith(('back_end.', 'model_frame.decoder.')), n
            assert p.grad is not None and p.grad.dtype == torch.float32, n
            assert torch.equal(p.grad, theirs[n].grad), n
            assert not torch.equal(p.detach(), before[n]), n                                 # the optimiser moved it
            moved += 1
        else:
            assert p.grad is None and torch.equal(p.detach(), before[n]), n
    assert moved == sum(1 for n, p in mine.items() if p.requires_grad and not n.startswith('back_end.decoder_scale_5.')) > 30
    assert all(p.requires_grad for n, p in mine.items() if n.startswith(('back_end.', 'model_frame.decoder.')))
    assert all(not p.requires_grad for n, p in mine.items() if n.startswith(('front_sensor_b.', 'model_frame.encoder.')))


# ---------------------------------------------------------------------------------------------------------------- (a) wiring
def test_train_step_equals_the_same_calls_by_hand():
    from openess_amd import hip
    st, _ = _step()
    assert st.precision == 'fp32' and st.model_frame.lazy_features and st.task_backend.materialize_ch256 == 'pooled'
    batch = _device_batch()
    before = _state(st.models_dict)
    losses, _, total = st.train_step(batch)
    assert set(losses) == {'dense_clip_loss', 'contrastive_nce_loss'}
    other, _ = _step()
    feat = other.model_frame.head_fp32_train(torch.zeros(1, 2048, 4, 4, device="cuda"))
    assert isinstance(feat, hip.UpsampledNormalizedFeature) and feat.x.dtype == torch.float32
    other_total = _by_hand(other, batch)
    other_total.backward()
    _check_against_by_hand(st.models_dict, st.optimizers_dict, before, total, other.models_dict, other_total)


# ---------------------------------------------------------------------------------------------------- (b) against float64
@pytest.mark.parametrize("contr", [False, True])
def test_one_step_matches_the_float64_oracle(contr):
    st, keys = _step(contr)
    ref = pc.make_oracle(contr, keys)
    cpu_batch = pc.make_batch()
    l64, t64, g64 = pc.oracle_loss_and_grads(ref, cpu_batch)
    losses, _, total = st.train_step(_device_batch())
    got = {n: g for n, g in _grads(st.models_dict).items()}
    assert set(got) == set(g64), sorted(set(got) ^ set(g64))
    assert set(losses) == set(l64)
    worst = {'loss': max(pc.relerr(losses[k], l64[k]) for k in l64), 'grad_l2': 0.0, 'norm_bias': 0.0}
    for n, e in pc.grad_errors(got, g64).items():
        k = 'norm_bias' if pc.is_student_norm_bias(n) else 'grad_l2'
        if e > BOUND[k]:
            print(f"[pretrain_fp32] contrastive={contr} {n}: {e:.3e} > {BOUND[k]:.2e}", flush=True)
        worst[k] = max(worst[k], e)
    head = max([e for n, e in pc.grad_errors(got, g64).items() if n.startswith('model_frame.')] or [0.0])
    _report(f"(b) contrastive={contr} teacher head gradient (no assertion of its own)", head)
    for k, v in worst.items():
        _report(f"(b) contrastive={contr} {k}", v, BOUND[k])
    for k, v in worst.items():
        assert v <= BOUND[k], (contr, k, v, BOUND[k])


# ------------------------------------------------------------------------------------------------- (c) free-running trajectory
def test_three_free_steps_follow_the_float64_oracle():
    st, keys = _step()
    ref = pc.make_oracle(True, keys)
    cpu_batch, batch = pc.make_batch(), _device_batch()
    dev = []
    for it in range(3):
        losses, _, total = st.train_step(batch)
        l64, t64 = pc.oracle_step(ref, cpu_batch)
        dev.append(max([pc.relerr(losses[k], l64[k]) for k in l64] + [pc.relerr(total, t64)]))
        _report(f"(c) step {it} total {float(total):.6f} float64 {t64:.6f} worst relerr", dev[-1], BOUND['trajectory'])
    assert max(dev) <= BOUND['trajectory'], dev


# ------------------------------------------------------------------------------------------------------------ (d) schedules
def _two_batches(mode):
    st, _ = _step(cls_attrs={'overlap_teacher': mode != 'one_stream'})
    batches = [_device_batch(seed) for seed in (3, 4)]
    out = []

    def back(batch, front):
        for opt in st.optimizers_dict.values():
            opt.zero_grad()
        total, losses, _ = st.task_train_step(batch, front=front)
        total.backward()
        grads = _grads(st.models_dict)
        for opt in st.optimizers_dict.values():
            opt.step()
        return total.detach(), grads
    if mode == 'pipeline':
        out = list(st.pipeline_steps(batches, back))
    else:
        for b in batches:
            losses, _, total = st.train_step(b)
            out.append((total, _grads(st.models_dict)))
    torch.cuda.synchronize()
    return out, _state(st.models_dict)


def test_schedules_change_no_bit():
    runs = {m: _two_batches(m) for m in ('overlap', 'one_stream', 'pipeline')}
    runs['repeat'] = _two_batches('overlap')
    (out0, state0) = runs['overlap']
    assert bool(torch.isfinite(torch.stack([t for t, _ in out0])).all()) and not torch.equal(out0[0][0], out0[1][0])
    stats = [n for n in state0 if n.startswith('model_frame.encoder.') and n.endswith(('running_mean', 'running_var'))]
    assert len(stats) > 50
    for m in ('one_stream', 'pipeline', 'repeat'):
        out, state = runs[m]
        for (t0, g0), (t1, g1) in zip(out0, out):
            assert torch.equal(t0, t1), m
            assert set(g0) == set(g1)
            for n in g0:
                assert torch.equal(g0[n], g1[n]), (m, n)
        for n in state0:
            assert torch.equal(state0[n], state[n]), (m, n)


# ---------------------------------------------------------------------------------------------------- (e) running statistics
def test_one_step_moves_the_teachers_statistics_as_one_encode_fp32_call():
    st, _ = _step()
    other, _ = _step()
    batch = _device_batch()
    before = _state({'model_frame': st.model_frame})
    st.train_step(batch)
    other._set_modes()
    other.model_frame.encode_fp32(batch[2])
    a, b = _state({'model_frame': st.model_frame}), _state({'model_frame': other.model_frame})
    n_stats = 0
    for n in a:
        if n.startswith('model_frame.encoder.'):
            assert torch.equal(a[n], b[n]), n
            if n.endswith('num_batches_tracked'):
                assert int(a[n]) == int(before[n]) + 1, n
            if n.endswith(('running_mean', 'running_var')):
                assert not torch.equal(a[n], before[n]), n
                n_stats += 1
    assert n_stats > 50


# --------------------------------------------------------------------------------------------- (f) pooled against materialised
def test_pooled_features_agree_with_the_materialised_chains():
    batch = _device_batch()
    res = {}
    for pooled in (True, False):
        st, _ = _step(cls_attrs={'pooled_teacher_features': pooled, 'pooled_student_features': pooled})
        assert st.model_frame.lazy_features == pooled and st.task_backend.materialize_ch256 == ('pooled' if pooled else True)
        for opt in st.optimizers_dict.values():
            opt.zero_grad()
        total, losses, _ = st.task_train_step(batch)
        total.backward()
        res[pooled] = (losses, _grads(st.models_dict))
    (lp, gp), (lm, gm) = res[True], res[False]
    assert set(gp) == set(gm)
    e_loss = _report("(f) loss, pooled~materialised", max(pc.relerr(lp[k], lm[k]) for k in lm), BOUND['loss'])
    errs = pc.grad_errors(gp, {n: g.cpu() for n, g in gm.items()})
    e_bias = _report("(f) norm bias", max(e for n, e in errs.items() if pc.is_student_norm_bias(n)), BOUND['norm_bias'])
    e_grad = _report("(f) gradient L2 ratio", max(e for n, e in errs.items() if not pc.is_student_norm_bias(n)), BOUND['grad_l2'])
    assert e_loss <= BOUND['loss'] and e_grad <= BOUND['grad_l2'] and e_bias <= BOUND['norm_bias']


# ------------------------------------------------------------------------------------------------------------- (g) trainer
def _trainer(tmp_path, yaml_name, fill=True):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, yaml_name), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and type(trainer).__name__ == 'OpenESSPretrainModel'
    if fill:
        pc.fill_models(trainer.models_dict)
    return trainer, s


def _trainer_batch():
    ev, _, frame, pl, sp, S = _device_batch()
    return (ev, None, frame, pl, sp, S)


def test_trainer_on_the_fp32_yaml_equals_the_step_by_hand(tmp_path):
    trainer, s = _trainer(tmp_path, "pretrain_dsec_synthetic_fp32.yaml")
    assert s.train_precision == 'fp32' and trainer.train_precision == 'fp32' and trainer.step.precision == 'fp32'
    assert trainer.reconstructor.precision == 'bf16' and trainer.step.reconstructor_fp32.precision == 'fp32'
    batch = _trainer_batch()
    before = _state(trainer.models_dict)
    losses, _, total = trainer.train_step(batch)
    other, _ = _trainer(tmp_path, "pretrain_dsec_synthetic_fp32.yaml")
    other_total = _by_hand(other.step, batch)
    other_total.backward()
    _check_against_by_hand(trainer.models_dict, trainer.optimizers_dict, before, total, other.models_dict, other_total)


def _load_into(src, dst):
    assert sorted(src.models_dict) == sorted(dst.models_dict) and sorted(src.optimizers_dict) == sorted(dst.optimizers_dict)
    for name, m in src.models_dict.items():
        sd = m.state_dict()
        assert list(sd) == list(dst.models_dict[name].state_dict())
        dst.models_dict[name].load_state_dict(sd, strict=True)
    for name, opt in src.optimizers_dict.items():
        sd = opt.state_dict()
        own = dst.optimizers_dict[name].state_dict()
        assert [g['params'] for g in sd['param_groups']] == [g['params'] for g in own['param_groups']]
        dst.optimizers_dict[name].load_state_dict(sd)
    for n, p in _params(src.models_dict).items():
        assert torch.equal(p.detach(), _params(dst.models_dict)[n].detach()), n


def test_checkpoints_load_across_the_two_precisions(tmp_path):
    batch = _trainer_batch()
    fp32, _ = _trainer(tmp_path, "pretrain_dsec_synthetic_fp32.yaml")
    bf16, _ = _trainer(tmp_path, "pretrain_dsec_synthetic.yaml", fill=False)
    assert bf16.train_precision == 'bf16' and getattr(bf16.step, 'reconstructor_fp32', None) is None
    fp32.train_step(batch)
    _load_into(fp32, bf16)
    assert bool(torch.isfinite(bf16.train_step(batch)[2]))
    _load_into(bf16, fp32)                                         # and back: the bf16 trainer's weights and moments
    assert bool(torch.isfinite(fp32.train_step(batch)[2]))


# --------------------------------------------------------------------------------------------------------------- (h) tools
def _run_tool(name, argv, capsys):
    import importlib.util
    path = os.path.join(os.path.dirname(CFG), os.pardir, "tools", name)
    spec = importlib.util.spec_from_file_location(name[:-3], os.path.abspath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bounds_tool_runs_end_to_end(capsys):
    out = _run_tool("exp_pretrain_fp32_bounds.py", ["--steps", "1", "--height", "32", "--width", "48"], capsys)
    assert set(out) == {'largest', 'bound'} and set(out['bound']) >= {'k', 'gx', 'head_conv', 'loss', 'grad_l2', 'norm_bias', 'trajectory'}
    assert all(v >= 1e-5 for v in out['bound'].values())


def test_bench_tool_runs_end_to_end(capsys):
    out = _run_tool("bench_pretrain_fp32.py", ["--steps", "1", "--warmup", "0", "--batch", "1", "--height", "32", "--width", "48", "--nwin", "2"],
                    capsys)
    assert out['size'] == [1, 32, 48] and out['node']['fused_ms'] > 0 and out['node']['materialised_ms'] > 0
    assert out['step']['bf16_ms'] > 0 and out['step']['fp32_ms'] > 0
    assert all(abs(v) < 1e3 for v in out['step']['last_loss'].values())
