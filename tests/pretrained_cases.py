"""Synthetic pretrained-weight files in the reference's layouts (K33), shared by tests/test_pretrained_host.py and
tests/test_hip_pretrained.py.  No real weight ships with either repository: every file here is written from a seed into the
test's tmp_path."""
import os
from collections import OrderedDict

import torch
import yaml

from tests.synth import damp_residual, fill_by_name

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
LIGHT = {'num_bins': 5, 'skip_type': 'sum', 'recurrent_block_type': 'convlstm', 'num_encoders': 3, 'base_num_channels': 32,
         'num_residual_blocks': 2, 'use_upsample_conv': False, 'norm': 'BN'}
GRU = dict(LIGHT, recurrent_block_type='convgru')

# image_weights name -> (key inside the file | None, prefix the encoder's keys carry there, keys the rule must drop)
TEACHER_LAYOUTS = {
    'imagenet': (None, '', ()),
    'dino': (None, '', ()),
    'moco_v1': ('state_dict', 'module.encoder_q.', ('module.encoder_q.fc.weight', 'module.encoder_q.fc.bias', 'module.encoder_k.conv1.weight')),
    'moco_v2': ('state_dict', 'module.encoder_q.', ('module.encoder_q.fc.weight', 'module.encoder_q.fc.bias', 'module.queue')),
    'moco_coco': ('state_dict', 'module.encoder_q.', ('module.encoder_q.fc.0.weight', 'module.encoder_k.conv1.weight')),
    'swav': (None, 'module.', ('module.projection_head.0.weight', 'module.prototypes.weight')),
    'deepcluster_v2': (None, 'module.', ('module.projection_head.0.weight', 'module.prototypes.prototypes0.weight')),
    'obow': ('network', '', ()),
    'pixpro': ('model', 'module.encoder.', ('module.projector.linear1.weight', 'module.encoder_k.conv1.weight')),
}


def e2vid_state(config=LIGHT, seed=41):
    """Seeded state dict of an E2VIDRecurrent of `config`, filled by parameter name (BatchNorm statistics included)."""
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    return OrderedDict((k, v.clone()) for k, v in fill_by_name(E2VIDRecurrent(config), seed).state_dict().items())


def write_e2vid(path, config=LIGHT, seed=41, spelling='model', module_prefix=False, arch='E2VIDRecurrent', state=None):
    """A reference-format checkpoint at `path`; returns the state dict (without any prefix) it holds."""
    state = e2vid_state(config, seed) if state is None else state
    saved = OrderedDict(('module.' + k, v) for k, v in state.items()) if module_prefix else state
    raw = {'arch': arch, 'state_dict': saved}
    if spelling == 'model':
        raw['model'] = dict(config)
    else:
        raw['config'] = {'model': dict(config), 'trainer': {'epochs': 1}}
    torch.save(raw, str(path))
    return state


def resnet50_keys():
    """The plain ResNet-50 key set the teacher's encoder loads (no fc.*), from a module built on the meta device."""
    from openess_amd.models._resnet import Bottleneck
    from openess_amd.models.image_model import ResNetEncoder
    with torch.device('meta'):
        enc = ResNetEncoder(block=Bottleneck, layers=[3, 4, 6, 3], replace_stride_with_dilation=[True, True, True])
    return list(enc.state_dict().keys())


def teacher_state(seed=43):
    """Seeded, well-conditioned (tests/synth.py:damp_residual) state dict of the teacher's ResNet-50 encoder."""
    from openess_amd.models._resnet import Bottleneck
    from openess_amd.models.image_model import ResNetEncoder
    enc = ResNetEncoder(block=Bottleneck, layers=[3, 4, 6, 3], replace_stride_with_dilation=[True, True, True])
    damp_residual(fill_by_name(enc, seed))
    return OrderedDict((k, v.clone()) for k, v in enc.state_dict().items())


def wrap_teacher(name, state, extra_fc=True):
    """`state` (plain encoder keys) as the object a `name` checkpoint file holds, with the keys the rule must drop added."""
    inner, prefix, drop = TEACHER_LAYOUTS[name]
    one = torch.zeros(1)
    d = OrderedDict((prefix + k, v) for k, v in state.items())
    for k in drop:
        d[k] = one
    if extra_fc and not prefix:
        d['fc.weight'], d['fc.bias'] = one, one          # a plain torchvision file: dropped by ResNetEncoder.load_state_dict
    return d if inner is None else {inner: d, 'epoch': 800}


def write_teacher(path, name, state):
    torch.save(wrap_teacher(name, state), str(path))
    return str(path)


def write_backbone(path, seed=47, num_classes=11, output_stride=32):
    """A `pre_trained_backbone` file, {'model_recon': state_dict} of a seeded well-conditioned DeepLabv3-R50; returns the dict."""
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    net = deeplabv3_resnet50(num_classes=num_classes, text_embeddings_path='', output_stride=output_stride, pretrained_backbone='')
    damp_residual(fill_by_name(net, seed))
    state = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    torch.save({'model_recon': state}, str(path))
    return state


# the synthetic configs' size (tests/configs/*_dsec_synthetic.yaml): 64 x 96, batch 2, three sub-windows of five bins, 11 classes
B, H, W, NWIN, BINS, K, SPS = 2, 64, 96, 3, 5, 11, 25


def make_batch(seed=3):
    """(events, frame, labels with one ignored band, superpixels, S) on the CPU, from a generator of their own."""
    g = torch.Generator().manual_seed(seed)
    ev = (torch.randn(B, NWIN * BINS, H, W, generator=g) * (torch.rand(B, NWIN * BINS, H, W, generator=g) > 0.7)).contiguous()
    frame = torch.rand(B, 3, H, W, generator=g)
    labels = torch.randint(0, K, (B, H // 4, W // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    labels[0, :5] = 255
    sp = torch.randint(0, SPS, (B, H // 8, W // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    S = int((sp + torch.arange(B)[:, None, None] * SPS).max()) + 1
    return ev, frame, labels, sp, S


def settings(tmp_path, base="pretrain_dsec_synthetic.yaml", model=None, dataset=None, **clip):
    """Settings of a copy of tests/configs/<base> with the clip (model, dataset) keys replaced."""
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(CFG_DIR, base)), yaml.Loader)
    cfg['clip'].update(clip)
    cfg['model'].update(model or {})
    cfg['dataset']['DSEC_events'].update(dataset or {})
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    s = Settings(str(path), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    return s
