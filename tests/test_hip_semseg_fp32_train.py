"""GPU tests of the fp32 backward of the SemSegE2VID decoder's layers (K18: conv_wgrad_f32.hip, semseg_bwd_f32.hip and the fp32
autograd functions of openess_amd.hip), every gradient against float64 torch autograd on the CPU.

Error measure: relerr = max|got - want| / max|want|.  The bound of a group is four times the largest relerr torch's OWN fp32 CPU
autograd reaches against float64 on that group's cases, with a floor of 1e-5 (the rule of K16 / K17).  Measured on the CPU
(CPU_FP32_RELERR below; every group stays under the floor, so every bound is the floor):

    group      torch fp32 CPU vs float64    bound
    wgrad      1.04e-06 (dW), 1.00e-06 (db) 1e-5
    dgrad      4.1e-07                      1e-5
    norm       9.1e-07                      1e-5
    upsample   0 (a four-term sum)          1e-5
    blocks     6.7e-07                      1e-5
    decoder    2.2e-06                      1e-5

ReLU masks: a pre-activation near zero can take another sign in fp32 than in float64, which moves the gradient by a whole dY
term; no tolerance covers that.  Every case with a ReLU therefore conditions its seeded input (condition_relu_margin: a few
least-norm steps in float64 that push the few near-zero pre-activations out of the band, rounded to fp32 after every step) and
the test asserts, on the float64 reference, that no ReLU input lies below 1e-4 of its layer's largest magnitude before it
compares.  No element is left out of any comparison.

A conv bias in front of an InstanceNorm has an analytically zero gradient (float64: about 1e-17); relerr against that is
meaningless, so those are held to max|db - db64| <= bound * max|dW64| of the same conv.

forward_fp32_train composes the head in fp32 under autograd, forward_fp32 in float64 rounded once: their logits agree within the
decoder bound, not bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nets as on
from tests.synth import fill_by_name

pytestmark = pytest.mark.gpu

CPU_FP32_RELERR = {'wgrad': 1.04e-6, 'dgrad': 4.1e-7, 'norm': 9.1e-7, 'upsample': 0.0, 'blocks': 6.7e-7, 'decoder': 2.2e-6}
BOUND = {k: max(4.0 * v, 1e-5) for k, v in CPU_FP32_RELERR.items()}
RELU_MARGIN = 1e-4


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _report(name, value, bound):
    print(f"[semseg_fp32_train] {name}: {value:.3e} (bound {bound:.0e})", flush=True)
    return value


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ ReLU margins
def relu_margin(pre):
    """smallest |v| / max|v| over the ReLU inputs `pre` (a list of float64 tensors), the worst layer"""
    return min(float(v.detach().abs().min() / v.detach().abs().max()) for v in pre)


def condition_relu_margin(run, free, target=3.0 * RELU_MARGIN, accept=2.0 * RELU_MARGIN, iters=60):
    """`free`: float64 leaf tensors (fp32-representable); run(free) -> the float64 ReLU inputs that depend on them.  Moves `free`
    by least-norm steps (Polyak's step on the hinge sum of (target * max|v| - |v|)+), rounding to fp32 after every step, until
    no ReLU input lies below accept * max|v| of its layer.  Deterministic; returns the conditioned tensors."""
    free = [t.detach().float().double().requires_grad_(True) for t in free]
    for _ in range(iters):
        pre = run(free)
        if relu_margin(pre) >= accept:
            break
        loss = sum(torch.relu(target * float(v.detach().abs().max()) - v.abs()).sum() for v in pre)
        grads = torch.autograd.grad(loss, free, allow_unused=True)
        gg = sum(float((g * g).sum()) for g in grads if g is not None)
        step = float(loss.detach()) / max(gg, 1e-300)
        free = [(t.detach() if g is None else t.detach() - step * g).float().double().requires_grad_(True)
                for t, g in zip(free, grads)]
    return [t.detach() for t in free]


class _ReluInputs:
    """collects the inputs of every nn.ReLU of a module during a forward"""

    def __init__(self, module):
        self.pre = []
        self.handles = [m.register_forward_hook(lambda m, i, o: self.pre.append(i[0])) for m in module.modules()
                        if isinstance(m, nn.ReLU)]

    def close(self):
        for h in self.handles:
            h.remove()


# ------------------------------------------------------------------------------------------------------------ convolution
# (B, Cin, Cout, H, W, R)
CONV_CASES = [(2, 32, 16, 5, 7, 3), (1, 16, 33, 3, 5, 3), (2, 256, 128, 4, 6, 3), (1, 6, 11, 9, 13, 1), (2, 64, 32, 33, 47, 3)]
X_SLICE_CASE, DY_NCHW_CASE, SPLIT_CASE = 0, 2, 4


@functools.lru_cache(maxsize=None)
def conv_case(i):
    """fp32 inputs and the float64 gradients of y = conv(x, w) + b with cotangent dy"""
    B, Cin, Cout, H, W, R = CONV_CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, R, R, generator=g) / (Cin * R * R) ** 0.5
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    return (x, w, b, dy), conv_grads(x, w, b, dy, torch.float64)


def conv_grads(x, w, b, dy, dtype):
    x, w, b = (t.to(dtype).requires_grad_(True) for t in (x, w, b))
    return torch.autograd.grad(F.conv2d(x, w, b, padding=(w.shape[2] - 1) // 2), [x, w, b], dy.to(dtype))


def _conv_operands(i):
    """device x and dy of case i: x of X_SLICE_CASE is a channel slice of a wider channels_last buffer, dy of DY_NCHW_CASE NCHW"""
    (x, w, b, dy), _ = conv_case(i)
    B, Cin, Cout, H, W, R = CONV_CASES[i]
    if i == X_SLICE_CASE:
        wide = torch.full((B, H, W, Cin + 12), 3.0, device="cuda")
        wide[..., 8:8 + Cin] = x.permute(0, 2, 3, 1).cuda()
        xd = wide[..., 8:8 + Cin].permute(0, 3, 1, 2)
    else:
        xd = _cl(x)
    gd = dy.cuda().contiguous() if i == DY_NCHW_CASE else _cl(dy)
    return xd, gd


@pytest.mark.parametrize("i", range(len(CONV_CASES)))
def test_conv_wgrad_f32_matches_float64(i):
    from openess_amd import hip
    B, Cin, Cout, H, W, R = CONV_CASES[i]
    _, (_, dw64, db64) = conv_case(i)
    xd, gd = _conv_operands(i)
    nsplit = hip.conv2d_wgrad_f32_splits(B, H, W, Cin, Cout, R)
    if i == SPLIT_CASE:
        assert nsplit > 1 and (B * H * W) % 16 != 0              # several ranges, and a last K step with masked pixels
    dw, db = hip.conv2d_wgrad_f32(xd, gd, R)
    assert dw.shape == dw64.shape and db.shape == db64.shape and dw.dtype == db.dtype == torch.float32
    e_w, e_b = relerr(_np(dw), dw64.numpy()), relerr(_np(db), db64.numpy())
    _report(f"wgrad {CONV_CASES[i]} splits {nsplit} dW", e_w, BOUND['wgrad'])
    _report(f"wgrad {CONV_CASES[i]} db", e_b, BOUND['wgrad'])
    assert e_w <= BOUND['wgrad'] and e_b <= BOUND['wgrad']
    dw2, none = hip.conv2d_wgrad_f32(xd, gd, R, want_db=False)
    assert none is None and torch.equal(dw2, dw)
    dw3, db3 = hip.conv2d_wgrad_f32(xd, gd, R)
    assert torch.equal(dw3, dw) and torch.equal(db3, db)


@pytest.mark.parametrize("i", range(len(CONV_CASES)))
def test_conv2d_f32_train_gradients_match_float64(i):
    from openess_amd import hip
    (x, w, b, dy), (dx64, dw64, db64) = conv_case(i)
    xd, gd = _conv_operands(i)
    xd = xd.detach().requires_grad_(True)
    wp, bp = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = hip.conv2d_f32_train(xd, wp, bp)
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=(w.shape[2] - 1) // 2)
    assert relerr(_np(y), y64.numpy()) <= BOUND['dgrad']
    dx, dw, db = torch.autograd.grad(y, [xd, wp, bp], gd)
    assert dx.shape == dx64.shape and dx.dtype == torch.float32
    assert _report(f"dgrad {CONV_CASES[i]}", relerr(_np(dx), dx64.numpy()), BOUND['dgrad']) <= BOUND['dgrad']
    assert relerr(_np(dw), dw64.numpy()) <= BOUND['wgrad'] and relerr(_np(db), db64.numpy()) <= BOUND['wgrad']
    # a gradient nobody asks for is not computed: the latents of the frozen encoder
    y2 = hip.conv2d_f32_train(xd.detach(), wp, None)
    dw2, = torch.autograd.grad(y2, [wp], gd)
    assert torch.equal(dw2, dw)


# ------------------------------------------------------------------------------------------------------------ InstanceNorm
# (B, C, H, W, layout)
NORM_SHAPES = [(2, 16, 5, 7, 'cl'), (1, 6, 3, 5, 'nchw'), (2, 256, 4, 6, 'cl'), (1, 32, 33, 47, 'cl')]


def norm64(x, relu, res):
    y = F.instance_norm(x, eps=1e-5)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


@functools.lru_cache(maxsize=None)
def norm_case(i, variant):
    """unit spread on a per-channel offset of +-50 (K17's stability case); fp32 inputs, the float64 gradients and the ReLU margin"""
    B, C, H, W, _ = NORM_SHAPES[i]
    g = torch.Generator().manual_seed(200 + 10 * i + len(variant))
    x = torch.randn(B, C, H, W, generator=g) + 50.0 * torch.where(torch.rand(1, C, 1, 1, generator=g) > 0.5, 1.0, -1.0)
    res = torch.randn(B, C, H, W, generator=g) if variant == 'residual' else None
    dy = torch.randn(B, C, H, W, generator=g)
    relu = variant == 'relu'
    margin = None
    if relu:
        x, = condition_relu_margin(lambda f: [F.instance_norm(f[0], eps=1e-5)], [x.double()])
        margin = relu_margin([F.instance_norm(x, eps=1e-5)])
        x = x.float()
    return (x, res, dy, relu), norm_grads(x, res, dy, relu, torch.float64), margin


def norm_grads(x, res, dy, relu, dtype):
    x = x.to(dtype).requires_grad_(True)
    res = None if res is None else res.to(dtype).requires_grad_(True)
    y = norm64(x, relu, res)
    return torch.autograd.grad(y, [x] if res is None else [x, res], dy.to(dtype))


@pytest.mark.parametrize("variant", ['plain', 'relu', 'residual'])
@pytest.mark.parametrize("i", range(len(NORM_SHAPES)))
def test_instance_norm_f32_backward_matches_float64(i, variant):
    from openess_amd import hip
    (x, res, dy, relu), want, margin = norm_case(i, variant)
    if relu:
        assert margin >= RELU_MARGIN, margin
    dev = (lambda t: t.cuda().contiguous()) if NORM_SHAPES[i][4] == 'nchw' else _cl
    xd, gd = dev(x).requires_grad_(True), dev(dy)
    rd = None if res is None else dev(res).requires_grad_(True)
    y = hip.instance_norm_f32_train(xd, relu=relu, residual=rd)
    assert torch.equal(y, hip.instance_norm_f32(xd.detach(), relu=relu, residual=None if rd is None else rd.detach()))
    got = torch.autograd.grad(y, [xd] if rd is None else [xd, rd], gd)
    assert got[0].shape == x.shape and got[0].dtype == torch.float32
    e = relerr(_np(got[0]), want[0].numpy())
    assert _report(f"norm bwd {NORM_SHAPES[i]} {variant}", e, BOUND['norm']) <= BOUND['norm']
    if rd is not None:
        assert torch.equal(got[1], gd)                       # the residual sees dY itself
    got2 = torch.autograd.grad(hip.instance_norm_f32_train(xd, relu=relu, residual=rd), [xd], gd)
    assert torch.equal(got2[0], got[0])


# ------------------------------------------------------------------------------------------------------ upsample + concat
@pytest.mark.parametrize("B,C,H,W,Cs,layout", [(2, 16, 5, 7, 8, 'cl'), (1, 16, 4, 6, 0, 'cl'), (2, 6, 3, 5, 5, 'nchw'), (1, 8, 1, 1, 4, 'cl'),
                                               (1, 128, 30, 40, 128, 'cl')])
def test_upsample_concat_f32_backward(B, C, H, W, Cs, layout):
    from openess_amd import hip
    gen = torch.Generator().manual_seed(B * 31 + C + Cs)
    x = torch.randn(B, C, H, W, generator=gen)
    skip = torch.randn(B, Cs, 2 * H, 2 * W, generator=gen) if Cs else None
    g = torch.randn(B, C + Cs, 2 * H, 2 * W, generator=gen)
    dev = (lambda t: t.cuda().contiguous()) if layout == 'nchw' else _cl
    xd = dev(x).requires_grad_(True)
    sd = None if skip is None else dev(skip).requires_grad_(True)
    gd = dev(g)
    y = hip.upsample2x_concat_f32_train(xd, sd)
    assert torch.equal(y, hip.upsample2x_concat_f32(xd.detach(), None if sd is None else sd.detach()))
    got = torch.autograd.grad(y, [xd] if sd is None else [xd, sd], gd)
    g64 = g.double()[:, :C]
    want = g64[:, :, 0::2, 0::2] + g64[:, :, 0::2, 1::2] + g64[:, :, 1::2, 0::2] + g64[:, :, 1::2, 1::2]
    assert got[0].shape == x.shape
    assert _report(f"upsample bwd {(B, C, H, W, Cs)}", relerr(_np(got[0]), want.numpy()), BOUND['upsample']) <= BOUND['upsample']
    if sd is not None:
        # the skip's gradient is the channel slice of the incoming gradient where it lies: same storage, offset and strides
        assert got[1].data_ptr() == gd[:, C:].data_ptr() == gd.data_ptr() + 4 * C * gd.stride(1)
        assert got[1].stride() == gd.stride() and got[1].shape == skip.shape
        assert torch.equal(got[1].cpu(), g[:, C:])


# ------------------------------------------------------------------------------------------------------------ the blocks
BLOCK_SHAPES = [(2, 32, 6, 10), (1, 256, 4, 6)]


@functools.lru_cache(maxsize=None)
def block_case(kind, i):
    """float64 oracle block, conditioned fp32 input, cotangent, the float64 gradients (input, then parameters by name)"""
    B, C, H, W = BLOCK_SHAPES[i]
    torch.manual_seed(300 + 10 * i + len(kind))
    ref = (on.INSResBlock(C, C) if kind == 'res' else on.ReLUINSConv2d(C, C // 2, 3, 1, 1)).double()
    for p in ref.parameters():                 # fp32-representable parameters, shared with the product
        p.data = p.data.float().double()
    x = torch.randn(B, C, H, W)
    hooks = _ReluInputs(ref)

    def run(free):
        hooks.pre.clear()
        ref(free[0])
        return list(hooks.pre)
    x, = condition_relu_margin(run, [x.double()])
    x.requires_grad_(True)
    hooks.pre.clear()
    y = ref(x)
    margin = relu_margin(hooks.pre)
    hooks.close()
    dy = torch.randn(y.shape)
    names = [n for n, _ in ref.named_parameters()]
    grads = torch.autograd.grad(y, [x] + [p for _, p in ref.named_parameters()], dy.double())
    return ref, x.detach().float(), dy, names, grads, margin


def check_param_grads(tag, names, got, want, bound, norm_biases):
    """relerr per parameter; a bias in front of an InstanceNorm against bound * max|dW64| of its conv"""
    worst = 0.0
    w64 = dict(zip(names, want))
    for n, a, b in zip(names, got, want):
        assert a is not None, n
        if n in norm_biases:
            scale = float(w64[n[:-len('bias')] + 'weight'].abs().max())
            e = float((a.detach().cpu().double() - b).abs().max()) / scale
        else:
            e = relerr(_np(a), b.numpy())
        worst = max(worst, e)
        assert e <= bound, (tag, n, e)
    return worst


@pytest.mark.parametrize("i", range(len(BLOCK_SHAPES)))
@pytest.mark.parametrize("kind", ['res', 'conv'])
def test_block_forward_f32_train_gradients_match_float64(kind, i):
    from openess_amd.models.style_networks import INSResBlock, ReLUINSConv2d
    B, C, H, W = BLOCK_SHAPES[i]
    ref, x, dy, names, want, margin = block_case(kind, i)
    assert margin >= RELU_MARGIN, margin
    net = INSResBlock(C, C) if kind == 'res' else ReLUINSConv2d(C, C // 2, 3, 1, 1)
    net.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    net = net.cuda()
    xd = _cl(x).requires_grad_(True)
    y = net.forward_f32_train(xd)
    with torch.no_grad():
        assert relerr(_np(y), ref(x.double()).numpy()) <= BOUND['blocks']
    params = dict(net.named_parameters())
    got = torch.autograd.grad(y, [xd] + [params[n] for n in names], _cl(dy))
    e_x = relerr(_np(got[0]), want[0].numpy())
    _report(f"block {kind} {BLOCK_SHAPES[i]} dX", e_x, BOUND['blocks'])
    assert e_x <= BOUND['blocks']
    worst = check_param_grads(f"block {kind}", names, got[1:], want[1:], BOUND['blocks'], {n for n in names if n.endswith('bias')})
    _report(f"block {kind} {BLOCK_SHAPES[i]} parameters", worst, BOUND['blocks'])


# ------------------------------------------------------------------------------------------------------------ the decoder
DECODER_FRAMES = [(1, 32, 48), (2, 40, 56)]
DECODER_KW = dict(skip_connect=True, skip_type='concat', text_embeddings_path=None, materialize_ch256=False)


def _product_decoder(seed, linear_probing):
    from openess_amd.models.style_networks import SemSegE2VID
    net = SemSegE2VID(256, 11, if_linear_probing=linear_probing, **DECODER_KW)
    fill_by_name(net, seed)
    return net


def oracle_decoder(seed, linear_probing, keys, dtype=torch.float64):
    ref = on.SemSegE2VID(256, 11)
    if linear_probing:
        ref.linear_probe = nn.Conv2d(11, 11, 1)
    fill_by_name(ref, seed, keys)
    return ref.to(dtype)


def oracle_logits(ref, lat, linear_probing):
    lg = ref(lat)[0][1]
    return ref.linear_probe(lg) if linear_probing else lg


def decoder_grads(ref, lat, cot, linear_probing, names):
    """gradients of (logits * cot).sum() by parameter name (text_embeddings, a buffer of the oracle, included)"""
    ref.text_embeddings.requires_grad_(not linear_probing)
    named = dict(ref.named_parameters())
    named['text_embeddings'] = ref.text_embeddings
    if linear_probing:
        names = [n for n in names if n.startswith('linear_probe.')]
    loss = (oracle_logits(ref, lat, linear_probing) * cot).sum()
    return names, torch.autograd.grad(loss, [named[n] for n in names])


@functools.lru_cache(maxsize=None)
def decoder_case(f, linear_probing):
    B, H, W = DECODER_FRAMES[f]
    seed = 40 + f
    net = _product_decoder(seed, linear_probing)
    keys = sorted(net.state_dict().keys())
    ref = oracle_decoder(seed, linear_probing, keys)
    g = torch.Generator().manual_seed(400 + f)
    lat = {1: torch.randn(B, 32, H, W, generator=g), 2: torch.randn(B, 64, H // 2, W // 2, generator=g),
           4: torch.randn(B, 128, H // 4, W // 4, generator=g), 8: torch.randn(B, 256, H // 8, W // 8, generator=g)}
    cot = torch.randn(B, 11, H, W, generator=g)
    hooks = _ReluInputs(ref)

    def run(free):
        hooks.pre.clear()
        ref({1: lat[1].double(), 2: free[0], 4: free[1], 8: free[2]})
        return list(hooks.pre)
    l2, l4, l8 = condition_relu_margin(run, [lat[2].double(), lat[4].double(), lat[8].double()])
    lat = {1: lat[1], 2: l2.float(), 4: l4.float(), 8: l8.float()}
    lat64 = {k: v.double() for k, v in lat.items()}
    hooks.pre.clear()
    with torch.no_grad():
        logits64 = oracle_logits(ref, lat64, linear_probing)
    margin = relu_margin(hooks.pre)
    hooks.close()
    trainable = [n for n, p in net.named_parameters() if p.requires_grad and not n.startswith('decoder_scale_5.')]
    names, grads = decoder_grads(ref, lat64, cot.double(), linear_probing, trainable)
    return net, lat, cot, logits64, names, grads, margin


def _decoder_backward(net, lat, cot):
    for p in net.parameters():
        p.grad = None
    out, x256 = net.forward_fp32_train(lat)
    (out[1] * cot).sum().backward()
    return out


@pytest.mark.parametrize("linear_probing", [False, True])
@pytest.mark.parametrize("f", range(len(DECODER_FRAMES)))
def test_decoder_forward_fp32_train_gradients_match_float64(f, linear_probing):
    net, lat, cot, logits64, names, want, margin = decoder_case(f, linear_probing)
    assert margin >= RELU_MARGIN, margin
    net = net.cuda().train()
    latd = {k: _cl(v) for k, v in lat.items()}
    cotd = _cl(cot)
    out = _decoder_backward(net, latd, cotd)
    assert set(out) == {1, 2, 4, 8} and out[8] is latd[8] and out[1].dtype == torch.float32
    e = relerr(_np(out[1]), logits64.numpy())
    assert _report(f"decoder {DECODER_FRAMES[f]} lp={linear_probing} logits", e, BOUND['decoder']) <= BOUND['decoder']
    params = dict(net.named_parameters())
    if linear_probing:
        assert sorted(names) == ['linear_probe.bias', 'linear_probe.weight']
        for n, p in params.items():
            assert (p.grad is not None) == n.startswith('linear_probe.'), n
    else:
        # every trainable parameter the forward uses (decoder_scale_5 is in the state_dict, never in the graph)
        assert set(names) == {n for n in params if not n.startswith('decoder_scale_5.')} and 'text_embeddings' in names
    norm_biases = {n for n in names if n.startswith('decoder_scale_') and n.endswith('bias')}
    worst = check_param_grads(f"decoder {DECODER_FRAMES[f]}", names, [params[n].grad for n in names], want, BOUND['decoder'], norm_biases)
    _report(f"decoder {DECODER_FRAMES[f]} lp={linear_probing} parameter gradients", worst, BOUND['decoder'])
    # repeatability: a second backward pass gives the same bits
    first = {n: params[n].grad.clone() for n in names}
    _decoder_backward(net, latd, cotd)
    for n in names:
        assert torch.equal(params[n].grad, first[n]), n


@pytest.mark.parametrize("linear_probing", [False, True])
def test_forward_fp32_train_agrees_with_forward_fp32(linear_probing):
    """The head is composed in fp32 under autograd here and in float64 (rounded once) in forward_fp32: not bit-equal."""
    net, lat, *_ = decoder_case(0, linear_probing)
    net = net.cuda()
    latd = {k: _cl(v) for k, v in lat.items()}
    out_t, _ = net.forward_fp32_train(latd)
    net.eval()
    out_e, _ = net.forward_fp32(latd)
    assert out_t[1].requires_grad and not out_e[1].requires_grad
    e = relerr(_np(out_t[1]), _np(out_e[1]))
    assert _report(f"forward_fp32_train vs forward_fp32 lp={linear_probing}", e, BOUND['decoder']) <= BOUND['decoder']
    assert relerr(_np(out_t[2]), _np(out_e[2])) <= BOUND['decoder'] and relerr(_np(out_t[4]), _np(out_e[4])) <= BOUND['decoder']


# ------------------------------------------------------------------------------------------------------------ refusals
def test_f32_train_functions_refuse_before_any_launch(monkeypatch):
    from openess_amd import hip
    from openess_amd.models.style_networks import SemSegE2VID
    x = torch.randn(1, 8, 6, 6, device="cuda")
    w = torch.randn(8, 8, 3, 3, device="cuda", requires_grad=True)

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip._lib, "load", boom)
    with pytest.raises(ValueError, match="fp32"):
        hip.conv2d_f32_train(x.bfloat16(), w, None)
    with pytest.raises(ValueError, match="stride 2"):
        hip.conv2d_f32_train(x, w, None, stride=2)
    with pytest.raises(ValueError, match="dilation 2"):
        hip.conv2d_f32_train(x, w, None, dilation=2, pad=2)
    with pytest.raises(ValueError, match="stride 2"):
        hip.conv2d_wgrad_f32(x, x, 3, stride=2)
    with pytest.raises(ValueError, match="dilation 2"):
        hip.conv2d_wgrad_f32(x, x, 3, dilation=2, pad=2)
    with pytest.raises(ValueError, match="fp32"):
        hip.conv2d_wgrad_f32(x.bfloat16(), x, 3)
    with pytest.raises(ValueError, match="fp32"):
        hip.instance_norm_f32_train(x.bfloat16())
    with pytest.raises(ValueError, match="fp32"):
        hip.upsample2x_concat_f32_train(x.bfloat16())
    net = SemSegE2VID(256, 11, **DECODER_KW).cuda()
    lat = {1: torch.zeros(1, 32, 16, 16), 2: torch.zeros(1, 64, 8, 8), 4: torch.zeros(1, 128, 4, 4), 8: torch.zeros(1, 256, 2, 2)}
    with pytest.raises(ValueError, match="fp32 latents"):
        net.forward_fp32_train({k: v.cuda().bfloat16() for k, v in lat.items()})


def test_wgrad_f32_entry_point_refuses_geometry_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    q = lib.oess_conv2d_wgrad_f32_workspace_bytes
    assert q(2, 33, 47, 64, 32, 3, 3, 1, 1, 1) > 0 and q(1, 9, 13, 6, 11, 1, 1, 1, 0, 1) == (6 * 11 + 11) * 4
    for bad in ((2, 33, 47, 64, 32, 3, 3, 2, 1, 1), (2, 33, 47, 64, 32, 3, 3, 1, 2, 2), (2, 33, 47, 64, 32, 5, 5, 1, 2, 1),
                (2, 33, 47, 64, 32, 3, 3, 1, 0, 1), (0, 33, 47, 64, 32, 3, 3, 1, 1, 1)):
        assert q(*bad) == 0
        assert lib.oess_conv2d_wgrad_f32(None, None, *bad, None, None, None, 0, None) == -22
    assert lib.oess_instance_norm_bwd_f32(None, None, None, None, 1, 4, 4, 8, 0, None, None, 0, None) == -22
    assert lib.oess_downsample_sum2x_f32(None, 1, 4, 4, 8, None, None) == -22
    assert lib.oess_instance_norm_train_fwd_f32(None, 1, 4, 4, 8, 1e-5, 0, None, None, None, None, None, 0, None) == -22
