"""Host-side checks of the fp32 image-teacher path (K17): the two new C entries in the header and the binding, what the
train-mode BatchNorm entry refuses before any launch, the wrapper's refusals, and that DeepLabv3's fp32 path still refuses train
mode.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -22, -12
NEW = ("oess_batch_norm_train_f32_workspace_bytes", "oess_batch_norm_train_fwd_f32")


def _prototype(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oess.h")).read(), flags=re.S)
    m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/oess.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def _ctype_of(arg):
    if "oess_f32_view_t" in arg:
        return "view"
    if "*" in arg or "oess_stream_t" in arg:
        return "ptr"
    return arg.split()[0] if not arg.startswith("long long") else "ll"


def test_header_and_binding_agree_on_the_new_entries():
    from openess_amd import _lib
    names = {"view": _lib.c_view, "ptr": _lib.c_vp, "int": _lib.c_int, "float": _lib.c_f, "size_t": _lib.c_sz, "ll": _lib.c_ll}
    lib = _lib.load()
    for name in NEW:
        res, args = _prototype(name)
        want_res, want_args = _lib.SIGNATURES[name]
        assert want_res is (_lib.c_sz if res == "size_t" else _lib.c_int), name
        assert [names[_ctype_of(a)] for a in args] == want_args, name
        assert hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    assert int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == _lib.ABI_VERSION     # additions only


def _views():
    from openess_amd import _lib
    buf = (ctypes.c_float * 8192)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    return buf, addr, _lib.F32View(addr, 1024, 128, 16, 1), _lib.F32View(None, 1024, 128, 16, 1)


def test_workspace_query_answers_zero_for_an_impossible_geometry():
    from openess_amd import _lib
    need = _lib.load().oess_batch_norm_train_f32_workspace_bytes
    assert need(8, 110, 160, 2048) >= 3 * 2048 * 4 and need(2, 7, 9, 6) > 0
    assert need(2, 7, 9, 0) == 0 and need(2, 7, 9, -4) == 0              # C < 1
    assert need(65536, 1, 1, 4) == 0 and need(65535, 1, 1, 4) > 0         # B > 65535
    assert need(0, 4, 4, 4) == 0 and need(1, 0, 4, 4) == 0 and need(1, 4, 0, 4) == 0


def test_batch_norm_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    lib = _lib.load()
    buf, addr, ok, null = _views()
    r = ctypes.byref
    bn = lib.oess_batch_norm_train_fwd_f32
    big = 1 << 26                                        # a claimed size: nothing is launched, so nothing is written

    def call(vin=r(ok), vout=r(ok), B=1, H=4, W=4, C=4, eps=1e-5, mom=0.1, rm=addr, rv=addr, relu=0, res=None, ws=addr, n=big):
        return bn(vin, B, H, W, C, addr, addr, eps, mom, rm, rv, addr, addr, relu, res, vout, ws, n, None)

    assert call(vin=None) == EINVAL and call(vin=r(null)) == EINVAL       # null views
    assert call(vout=None) == EINVAL and call(vout=r(null)) == EINVAL
    assert call(res=r(null)) == EINVAL
    assert call(ws=None) == EINVAL and call(ws=addr + 4) == EINVAL        # no workspace / not 16-byte aligned
    assert call(B=1, H=1, W=1) == EINVAL                                  # P = 1: torch raises there
    for B, H, W, C in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (65536, 4, 4, 4)):
        assert call(B=B, H=H, W=W, C=C) == EINVAL
    assert call(eps=-1.0) == EINVAL and call(mom=-0.5) == EINVAL and call(mom=float("nan")) == EINVAL and call(relu=2) == EINVAL
    assert call(rm=None) == EINVAL and call(rv=None) == EINVAL            # the running statistics come together
    need = lib.oess_batch_norm_train_f32_workspace_bytes(1, 4, 4, 4)
    assert call(n=need - 1) == ENOMEM and call(n=16) == ENOMEM and call(n=0) == ENOMEM
    assert call(B=1, H=1, W=2, n=16) == ENOMEM                            # P = 2 is a geometry: only the workspace is short


def test_wrapper_refuses_cumulative_momentum_and_cpu_tensors():
    from openess_amd import hip
    x = torch.zeros(2, 8, 3, 3)
    with pytest.raises(NotImplementedError, match="momentum=None"):
        hip.batch_norm_train_f32(x, torch.nn.BatchNorm2d(8, momentum=None))
    with pytest.raises(NotImplementedError, match="momentum=None"):
        hip.batch_norm_train_f32(x, dict(weight=None, bias=None, running_mean=None, running_var=None, momentum=None, eps=1e-5))
    bn = torch.nn.BatchNorm2d(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.batch_norm_train_f32(x, bn)
    assert int(bn.num_batches_tracked) == 0 and bool((bn.running_mean == 0).all())


def test_teacher_has_the_fp32_entry_points_and_refuses_what_it_does_not_run():
    from openess_amd.models import _resnet
    from openess_amd.models.image_model import DilationFeatureExtractor
    t = DilationFeatureExtractor(None)
    for name in ("forward_fp32", "encode_fp32", "head_fp32"):
        assert callable(getattr(t, name))
    assert callable(t.encoder.features_fp32) and callable(t.encoder.layer1[0].forward_train_fp32)
    with pytest.raises(ValueError, match="float32"):
        t.forward_fp32(torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16))
    for mode in (t.train(), t.eval()):                                    # both BatchNorm forms end at the kernels' refusal
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mode.forward_fp32(torch.zeros(1, 3, 32, 32))
    t.eval()
    with pytest.raises(ValueError, match="eval-mode"):
        _resnet.conv_bn_train_f32(t.encoder.conv1, t.encoder.bn1, torch.zeros(1, 3, 32, 32))


def test_deeplab_fp32_still_refuses_train_mode():
    from openess_amd.models._resnet import conv_bn_f32
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    net = deeplabv3_resnet50(num_classes=11, text_embeddings_path=None, output_stride=16, pretrained_backbone='').train()
    with pytest.raises(NotImplementedError, match="train mode"):
        net.check_fp32()
    with pytest.raises(NotImplementedError, match="train mode"):
        net.forward_fp32(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm is not built"):
        conv_bn_f32(net.backbone.conv1, net.backbone.bn1, torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm is not built"):
        net.backbone.layer1[0].forward_fp32(torch.zeros(1, 64, 8, 8))
