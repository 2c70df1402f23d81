"""Mirror of e2vid/utils/loading_utils.py:load_model (:5-33): the one place an E2VID checkpoint is read.  Every consumer -- the
offline reconstruction, the online reconstruction source and the trainers' frozen front end -- goes through read_checkpoint.

Checkpoint format: the reference's, `{'arch': 'E2VIDRecurrent', 'model' | 'config': {'model': ...}, 'state_dict': ...}`.  A state
dict saved from a DataParallel wrapper (every key starts with `module.`) is accepted with the prefix stripped, as the
reference's copyStateDict does.  `arch: 'E2VID'` (the non-recurrent network) is refused by name: the reference's own
ImageReconstructor unpacks three values from a model that returns two, so no caller of it could ever run one."""
from collections import OrderedDict

import torch

from ..model.model import E2VIDRecurrent


class UnsupportedArch(NotImplementedError, AssertionError):
    """A checkpoint of another `arch`.  Also an AssertionError, which is what run_reconstruction.load_model raised for it before
    this module existed and what its callers may catch."""


def read_checkpoint(path_to_model):
    """(model config dict, state dict with CPU tensors) of the checkpoint file; raises for what is no E2VIDRecurrent checkpoint."""
    raw = torch.load(path_to_model, map_location='cpu')
    if not isinstance(raw, dict) or 'arch' not in raw or 'state_dict' not in raw:
        raise ValueError(f"{path_to_model!r} is no E2VID checkpoint: expected a dict with 'arch', 'model' (or 'config': "
                         "{'model': ...}) and 'state_dict'")
    arch = raw['arch']
    if arch != 'E2VIDRecurrent':
        raise UnsupportedArch(f"{path_to_model!r}: arch {arch!r} is not served, only 'E2VIDRecurrent' (the recurrent network "
                              "every trainer and the reconstruction read three values from)")
    if 'model' in raw:
        config = raw['model']
    elif isinstance(raw.get('config'), dict) and 'model' in raw['config']:
        config = raw['config']['model']
    else:
        raise ValueError(f"{path_to_model!r} has no model config: neither 'model' nor 'config': {{'model': ...}}")
    state_dict = raw['state_dict']
    if len(state_dict) > 0 and all(k.startswith('module.') for k in state_dict):
        state_dict = OrderedDict((k[len('module.'):], v) for k, v in state_dict.items())
    return dict(config), state_dict


def load_model(path_to_model):
    """(model, None): the E2VIDRecurrent of the checkpoint's own config with its state dict loaded (strict), on the CPU.  The
    second slot is the reference's E2VIDDecoder, which no trainer reads."""
    print('Loading model {}...'.format(path_to_model))
    config, state_dict = read_checkpoint(path_to_model)
    model = E2VIDRecurrent(config)
    model.load_state_dict(state_dict)
    return model, None
