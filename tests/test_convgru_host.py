"""K28 on the host (no GPU): the ConvGRU E2VID model constructs with the reference's state_dict keys, reference-format checkpoints
load, states of the other block type are refused, ConvLSTM models are unchanged, the C ABI grew by additions only, and the exact
cases of the GPU tests are exact on the CPU too."""
import os
import re

import numpy as np
import pytest
import torch

from tests import convgru_cases as cases
from tests import convgru_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG = {'num_bins': 5, 'skip_type': 'sum', 'recurrent_block_type': 'convgru', 'num_encoders': 3,
       'base_num_channels': 32, 'num_residual_blocks': 2, 'use_upsample_conv': False, 'norm': 'BN'}
NEW_SYMBOLS = ("oess_convgru_gates_bf16", "oess_convgru_out_bf16", "oess_convgru_gates_f32", "oess_convgru_blend_f32",
               "oess_convgru_f32_workspace_bytes")


@pytest.fixture(scope="module")
def golden_keys():
    return list(np.load(os.path.join(GOLDEN, "e2vid_convgru.npz"))["keys"])


def test_convgru_model_constructs_with_reference_keys(golden_keys):
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    from openess_amd.e2vid.model.submodules import ConvGRU
    m = E2VIDRecurrent(CFG)
    assert sorted(m.state_dict().keys()) == golden_keys
    blocks = [e.recurrent_block for e in m.unetrecurrent.encoders]
    assert all(isinstance(b, ConvGRU) for b in blocks)
    b = blocks[0]
    assert tuple(b.update_gate.weight.shape) == (64, 128, 3, 3) and float(b.reset_gate.bias.detach().abs().max()) == 0.0
    w = b.out_gate.weight.detach().flatten(1)
    assert torch.allclose(w @ w.t(), torch.eye(64), atol=1e-4)              # init.orthogonal_, as the reference


def test_reference_format_checkpoint_round_trips(tmp_path, golden_keys):
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    from openess_amd.e2vid.run_reconstruction import load_model
    torch.manual_seed(3)
    src = E2VIDRecurrent(CFG)
    path = str(tmp_path / "convgru.pth.tar")
    torch.save({'arch': 'E2VIDRecurrent', 'model': dict(CFG), 'state_dict': src.state_dict()}, path)
    m = load_model(path)
    assert m.recurrent_block_type == 'convgru' and sorted(m.state_dict().keys()) == golden_keys
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    torch.save({'arch': 'E2VID', 'model': dict(CFG), 'state_dict': src.state_dict()}, path)
    with pytest.raises(AssertionError):
        load_model(path)


def test_states_of_the_other_block_type_are_refused():
    from openess_amd.e2vid.model.unet import check_states
    gru_bf16 = {'block': 'convgru', 'hxr': None, 'h32': None, 'u': None, 'fresh': True}
    gru_fp32 = {'block': 'convgru', 'precision': 'fp32', 'hxr': None, 'fresh': True}
    lstm_bf16 = {'xh': [None, None], 'cur': 0, 'cell': None, 'fresh': True}
    lstm_fp32 = {'precision': 'fp32', 'xh': None, 'cell': None, 'fresh': True}
    check_states([None, gru_bf16], 'bf16', 'convgru')
    check_states([lstm_fp32, None], 'fp32', 'convlstm')
    check_states([lstm_bf16], 'bf16')                                        # no block type asked: the precision check alone
    with pytest.raises(ValueError, match="convlstm state"):
        check_states([None, lstm_bf16], 'bf16', 'convgru')
    with pytest.raises(ValueError, match="convgru state"):
        check_states([gru_fp32], 'fp32', 'convlstm')
    with pytest.raises(ValueError, match="is fp32"):
        check_states([gru_fp32], 'bf16', 'convgru')
    with pytest.raises(ValueError, match="is bf16"):
        check_states([gru_bf16], 'fp32', 'convgru')


def test_convlstm_model_and_default_config_unchanged():
    import json
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from openess_amd.e2vid.model.submodules import ConvLSTM
    assert E2VID_LIGHTWEIGHT_CONFIG == {'num_bins': 5, 'skip_type': 'sum', 'recurrent_block_type': 'convlstm', 'num_encoders': 3,
                                        'base_num_channels': 32, 'num_residual_blocks': 2, 'use_upsample_conv': False, 'norm': 'BN'}
    m = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG)
    keys = json.load(open(os.path.join(GOLDEN, "nets_keys.json")))["e2vid"]
    assert sorted(m.state_dict().keys()) == keys
    assert all(isinstance(e.recurrent_block, ConvLSTM) for e in m.unetrecurrent.encoders)
    with pytest.raises(AssertionError):
        E2VIDRecurrent(dict(E2VID_LIGHTWEIGHT_CONFIG, recurrent_block_type='convrnn'))


def test_abi_grew_by_additions_only():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    assert int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+OESS_ROUTE_COUNT\s+(\d+)", header).group(1)) == 24
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 and lib.oess_conv2d_route_count() == 24
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.oess_convgru_f32_workspace_bytes(100, 32) == 100 * 4 * 32 * 4 and lib.oess_convgru_f32_workspace_bytes(0, 32) == 0
    # the fp32 pointwise kernels run one thread per element on a one-dimensional grid: more elements than it addresses are refused
    import ctypes
    top = (2 ** 31 - 1) * 256
    assert lib.oess_convgru_f32_workspace_bytes(top // 512, 512) == (top // 512) * 4 * 512 * 4
    assert lib.oess_convgru_f32_workspace_bytes(top // 512 + 1, 512) == 0
    host = (ctypes.c_float * 4)()
    ptr = ctypes.addressof(host)
    view = _lib.F32View(ptr, 0, 0, 0, 1)
    big = (1024, 1024, 1024, 512)                                            # 2^39 elements > (2^31 - 1) * 256
    assert lib.oess_convgru_gates_f32(ptr, None, *big, ptr, ctypes.byref(view), None) == -22
    assert lib.oess_convgru_blend_f32(ptr, ptr, None, *big, ctypes.byref(view), None) == -22
    # the geometry rules answer on the host, before any launch
    assert lib.oess_convgru_gates_bf16(None, 64, 1, 4, 4, 64, None, None, 32, 3, 3, 1, None, None, None, 64, None, None) == -22
    assert lib.oess_convgru_out_bf16(None, 64, 1, 4, 4, 64, None, None, 32, 3, 3, 1, None, None, None, None, 64, None) == -22


@pytest.mark.parametrize("geom", cases.EXACT_GEOMS)
def test_exact_cases_are_exact_on_the_cpu(geom):
    """Torch fp32 gives exactly the host integers on the exact cases, gate by gate, and so does the float64 restatement for h'.
    Its gates are exact once rounded to fp32, the precision every kernel output has: exp(-128) = 2.6e-56 underflows in fp32 but
    not in float64, so a closed gate is 2.6e-56 there; 1 - 2.6e-56 and +-1 + 2.6e-56 are 1 and +-1 in float64, which is why h'
    is exact all the same."""
    import torch.nn.functional as F
    c = cases.exact_case(*geom)
    pre_u, pre_r, u, rh, pre_o, hn = cases.exact_expected(c)
    u64, rh64 = ref.gates(c['x'], c['h'], c['h'], c['wu'], c['bu'], c['wr'], c['br'])
    assert torch.equal(u64.float(), u.float()) and torch.equal(rh64.float(), rh.float())
    assert float((u64 - u).abs().max()) < 1e-50 and float((rh64 - rh).abs().max()) < 1e-50
    assert torch.equal(ref.blend(c['x'], rh64, c['h'], u64, c['wo'], c['bo']), hn.double())
    s = torch.cat([c['x'], c['h']], 1)
    assert torch.equal(F.conv2d(s, c['wu'], c['bu'], padding=1), pre_u.float())
    assert torch.equal(F.conv2d(s, c['wr'], c['br'], padding=1), pre_r.float())
    u32 = torch.sigmoid(pre_u.float())
    rh32 = torch.sigmoid(pre_r.float()) * c['h']
    o32 = torch.tanh(F.conv2d(torch.cat([c['x'], rh32], 1), c['wo'], c['bo'], padding=1))
    assert torch.equal(u32, u.float()) and torch.equal(rh32, rh.float())
    assert torch.equal(c['h'] * (1 - u32) + o32 * u32, hn.float())
    # every tap, both halves of the input channels and both values of each gate occur
    for n in ('u', 'r', 'o'):
        taps = c['taps'][n]
        assert {(dy, dx) for _, dy, dx, _ in taps} == {(a, b) for a in range(3) for b in range(3)}
        assert min(ci for ci, *_ in taps) < geom[3] <= max(ci for ci, *_ in taps)
    assert 0 < int(u.sum()) < u.numel() and set(rh.unique().tolist()) == {-1, 0, 1} and set(hn.unique().tolist()) == {-1, 1}
