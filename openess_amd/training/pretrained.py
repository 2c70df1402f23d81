"""Where the frozen networks' pretrained weights come from: the E2VID front end, the image teacher and the
DeepLabv3 student's backbone file, each named by the YAML.  Host code only: a load is `load_state_dict` on the module the
trainers build anyway, and the kernels' operand caches follow the parameters' version counters (engine.param_versions).

The rule for a file that is looked for and does not exist: the network keeps its seeded weights, bit for bit, and one WARNING
names the key and the path -- no repository ships the weights, and every test and the benchmark run without them.
`require_pretrained: True` (clip block) turns that into a FileNotFoundError before any model is built; it is what a real run
sets.  A file that exists and does not fit (arch, config, keys, shapes) always raises.

Each function takes `logger=None` for the quiet form the trainers' constructors call before anything is built (refusals
only); the call that builds the network passes the logger and so warns or reports once."""
import logging
import os

from ..e2vid.model.submodules import check_runs

NO_WEIGHTS = (None, '', 'none', 'random')       # image_weights values that load nothing
_DEFAULT_LOGGER = logging.getLogger("openess_amd.pretrained")


def _not_found(key, path, network, require, logger):
    if require:
        raise FileNotFoundError(f"require_pretrained: True, but {key}: {path!r} does not exist (the {network}'s pretrained weights)")
    if logger is not None:
        logger.warning("%s: %r not found: the %s keeps its seeded random weights (require_pretrained: True makes this an error)",
                       key, path, network)


def report_loaded(logger, network, path, state_dict):
    """The one line a successful load logs: file, number of tensors, parameter count."""
    (logger or _DEFAULT_LOGGER).info("loaded %s from %s: %d tensors, %d parameters", network, path, len(state_dict),
                                     sum(int(v.numel()) for v in state_dict.values()))


def e2vid_path(settings):
    """(key, path) of the front end's checkpoint: the optional `e2vid_checkpoint` of the clip block, else settings.path_to_model
    (hard-coded as in the reference's settings)."""
    path = getattr(settings, 'e2vid_checkpoint', None)
    return ('e2vid_checkpoint', path) if path else ('path_to_model', settings.path_to_model)


def check_e2vid_config(config, path, num_bins, fp32=False):
    """Refuses, by name, a checkpoint config the trainers cannot put in front of SemSegE2VID(input_c=256): another number of
    temporal bins than the dataset's, other latents than the decoder reads (three encoders from 32 channels: 256 at 1/8), and
    -- when an fp32 key is set -- what the fp32 E2VID step does not run (submodules.check_runs, UNetRecurrent.check_fp32)."""
    bins = int(config['num_bins'])
    if bins != int(num_bins):
        raise ValueError(f"{path!r}: num_bins = {bins}, the dataset's nr_temporal_bins is {num_bins}")
    enc, base = int(config.get('num_encoders', 4)), int(config.get('base_num_channels', 32))
    if enc != 3 or base != 32:
        raise ValueError(f"{path!r}: num_encoders = {enc}, base_num_channels = {base}: SemSegE2VID(input_c=256) reads the latents "
                         "of num_encoders = 3, base_num_channels = 32 (256 channels at 1/8)")
    if fp32:
        check_runs(str(config['norm']) if 'norm' in config else None, None)
        if str(config.get('skip_type', 'sum')) != 'sum':
            raise NotImplementedError("E2VID checkpoints use skip_type 'sum'")


def e2vid_source(path, key, num_bins, fp32=False, require=False, logger=None):
    """(config, state_dict) of the front end's checkpoint, checked against what the trainers can run; None when `path` is None
    (nothing asked for) or the file does not exist (see the module docstring)."""
    if not path:
        return None
    if not os.path.isfile(path):
        _not_found(key, path, 'E2VID front end', require, logger)
        return None
    from ..e2vid.utils.loading_utils import read_checkpoint
    config, state_dict = read_checkpoint(path)
    check_e2vid_config(config, path, num_bins, fp32)
    return config, state_dict


def teacher_path(image_weights, image_weights_path=None, require=False, logger=None):
    """The file the image teacher loads `image_weights` from: `image_weights_path`, else weights/<image_weights>.pt under the
    working directory (where the reference caches its download; nothing is fetched here).  None for a name that loads nothing
    or a file that does not exist."""
    if image_weights in NO_WEIGHTS:
        return None
    from ..models.image_model import IMAGE_WEIGHTS
    if image_weights not in IMAGE_WEIGHTS:
        raise ValueError(f"image_weights: {image_weights!r} is none of {sorted(IMAGE_WEIGHTS)}")
    key, path = ('image_weights_path', image_weights_path) if image_weights_path else \
        ('image_weights', os.path.join('weights', f'{image_weights}.pt'))
    if not os.path.isfile(path):
        _not_found(key, path, 'image teacher', require, logger)
        return None
    return path


def backbone_path(pretrained_backbone, require=False, logger=None):
    """The `pre_trained_backbone` file of the stage-1 DeepLabv3 student ({'model_recon': state_dict}), '' when none is named or
    the file does not exist."""
    if not pretrained_backbone:
        return ''
    if not os.path.isfile(pretrained_backbone):
        _not_found('pre_trained_backbone', pretrained_backbone, 'DeepLabv3 student', require, logger)
        return ''
    return pretrained_backbone


def load_e2vid(model, source, path, logger=None):
    """`source` = e2vid_source(...)'s (config, state_dict) into the freshly constructed front end (strict), before .to(device)."""
    model.load_state_dict(source[1])
    report_loaded(logger, 'the E2VID front end', path, source[1])
    return model
