"""Host-side mirror of e2vid/model/submodules.py (reference lines cited per class).  Parameter names
and shapes are identical to the reference so its checkpoints load unchanged; forward passes run on the
HIP kernels (MFMA conv + fused gate kernel).  Inference only: the reference keeps E2VID frozen and runs
it under no_grad (e2vid/image_reconstructor.py:81)."""

import torch
import torch.nn as nn

from ... import engine, hip


def check_runs(norm, bn, activation=None):
    """The layer configurations the HIP paths (bf16 and fp32) run: no InstanceNorm, BatchNorm in eval mode (it is folded into
    the packed weights: the E2VID front end is frozen, pretrain_trainer.py:370-373), relu / no activation.  Raises otherwise."""
    if norm == 'IN':
        raise NotImplementedError("norm='IN' E2VID variants are not on the HIP paths")
    if bn is not None and bn.training:
        raise RuntimeError("E2VID runs in eval mode on the HIP paths (BatchNorm is folded into the packed weights)")
    if activation not in (None, 'relu'):
        raise NotImplementedError("only relu / None activations are on the HIP paths")


class _ConvNormAct(nn.Module):
    """conv -> (BN | IN) -> activation: the constructor ConvLayer, TransposedConvLayer and UpsampleConvLayer share, under the
    reference's parameter names (conv2d / transposed_conv2d, norm_layer)."""
    transposed = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation='relu', norm=None):
        super().__init__()
        bias = False if norm == 'BN' else True
        if self.transposed:
            self.transposed_conv2d = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride=2, padding=padding,
                                                        output_padding=1, bias=bias)
        else:
            self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=bias)
        self.activation_name = activation
        self.norm = norm
        if norm == 'BN':
            self.norm_layer = nn.BatchNorm2d(out_channels)
        elif norm == 'IN':
            self.norm_layer = nn.InstanceNorm2d(out_channels, track_running_stats=True)
        self._pw = engine.PackedWeight()
        self._pw32 = engine.PackedWeightF32()

    @property
    def bn(self):
        """The BatchNorm2d to fold into the packed weights, or None."""
        return self.norm_layer if self.norm == 'BN' else None


class ConvLayer(_ConvNormAct):
    """e2vid/model/submodules.py:7-31.  conv -> (BN | IN) -> activation.  BN is folded into the packed
    weights (module is in eval mode on this path); ReLU is fused in the conv epilogue."""

    def forward_f32(self, x, x2=None, act='layer', out=None):
        """fp32 inference (K14): act(conv(x [+ x2]) + bias) with eval-mode BatchNorm folded; act='layer' = this layer's own
        activation (ReLU / none), or None / 'relu' / 'sigmoid' (the prediction layer's sigmoid of unet.py:170)."""
        check_runs(self.norm, self.bn, self.activation_name if act == 'layer' else None)
        if act == 'layer':
            act = self.activation_name
        c = self.conv2d
        pw = self._pw32.get(c.weight, c.bias, self.bn)
        return hip.conv2d_f32(x, pw.packed, pw.bias, c.out_channels, c.kernel_size[0], c.kernel_size[1], c.stride[0], c.padding[0],
                              act=act, x2=x2, out=out)

    def _packed(self, cin_pad):
        """The bf16 operand (engine.PackedWeight) for an input of `cin_pad` (zero-padded) channels."""
        return self._pw.get(self.conv2d.weight, self.conv2d.bias, self.bn, cin_pad=cin_pad)

    def forward(self, x, out=None):
        check_runs(self.norm, self.bn, self.activation_name)
        c = self.conv2d
        return engine.conv2d_infer(x, self._packed(x.shape[1]), c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0], 1,
                                   relu=self.activation_name == 'relu', out=out)


class TransposedConvLayer(_ConvNormAct):
    """e2vid/model/submodules.py:34-62: ConvTranspose2d(k, stride 2, padding, output_padding 1) -> BN -> relu.  Only the offline
    reconstruction path runs it (unet.py:165-166; the training path stops at the latents).  A transposed convolution IS the
    data gradient of the strided convolution with the same weight tensor, so it runs on the same two kernels as autograd's
    dgrad: zero insertion (oess_zero_insert_nhwc_bf16) + the MFMA conv on the rotated / transposed packing
    (engine.PackedWeight, layout='transposed'); the eval-mode BatchNorm is folded into that packing and ReLU is fused in the
    epilogue."""
    transposed = True

    def forward_f32(self, x, skip=None):
        """fp32 inference (K14): relu(BN(ConvTranspose2d(x + skip))) as four phase sub-convolutions in one launch."""
        check_runs(self.norm, self.bn, self.activation_name)
        t = self.transposed_conv2d
        if t.kernel_size != (5, 5) or t.stride != (2, 2) or t.padding != (2, 2) or t.output_padding != (1, 1):
            raise NotImplementedError("the fp32 transposed convolution is the 5x5 / stride 2 / padding 2 / output_padding 1 form")
        pw = self._pw32.get(t.weight, t.bias, self.bn, transposed=True)
        return hip.conv_transpose2d_f32(x, pw.packed, pw.bias, t.out_channels, act=self.activation_name, x2=skip)

    def forward(self, x):
        check_runs(self.norm, self.bn, self.activation_name)
        t = self.transposed_conv2d
        k, pad = t.kernel_size[0], t.padding[0]
        pw = self._pw.get(t.weight, t.bias, self.bn, layout='transposed')
        B, Cin, H, W = x.shape
        Ho, Wo = (H - 1) * 2 - 2 * pad + k + 1, (W - 1) * 2 - 2 * pad + k + 1
        z = hip.zero_insert(engine.nhwc(x), 2, Ho - (k - 1) + 2 * pad, Wo - (k - 1) + 2 * pad)
        y = hip.conv2d_nhwc(z, pw.packed, pw.bias, t.out_channels, k, k, 1, (k - 1) - pad, 1, relu=self.activation_name == 'relu')
        return engine.from_nhwc(y)


class UpsampleConvLayer(_ConvNormAct):
    """e2vid/model/submodules.py:65-93: bilinear x2 (align_corners=False) -> conv -> BN -> relu.  Only the offline
    reconstruction path runs it (unet.py:165-166), in either precision.  bf16 (forward, K30): the skip sum and the interpolation
    are one streaming kernel (oess_upsample_bilinear2x_sum_nhwc_bf16: fp32 inside, one rounding to bf16), the convolution is the
    MFMA conv on the layer's regular packing with the eval-mode BatchNorm folded in and ReLU fused in the epilogue, as in
    ConvLayer.  fp32 (forward_f32, K14): one launch, the interpolation gathered inside the conv's operand load."""

    def forward(self, x, skip=None):
        """relu(BN(conv(upsample2x(x [+ skip])))) on logical-NCHW channels_last bf16 tensors (channel slices of wider buffers are
        fine); the sum is taken in fp32 inside the upsampling kernel, so the decoder input is rounded once."""
        check_runs(self.norm, self.bn, self.activation_name)
        c = self.conv2d
        up = hip.upsample2x_sum_nhwc(engine.nhwc(x), None if skip is None else engine.nhwc(skip))
        pw = self._pw.get(c.weight, c.bias, self.bn)
        y = hip.conv2d_nhwc(up, pw.packed, pw.bias, c.out_channels, c.kernel_size[0], c.kernel_size[1], c.stride[0], c.padding[0], 1,
                            relu=self.activation_name == 'relu')
        return engine.from_nhwc(y)

    def forward_f32(self, x, skip=None):
        """fp32 inference (K14): act(BN(conv(upsample2x(x + skip)))) in one launch."""
        check_runs(self.norm, self.bn, self.activation_name)
        c = self.conv2d
        pw = self._pw32.get(c.weight, c.bias, self.bn)
        return hip.conv2d_f32(x, pw.packed, pw.bias, c.out_channels, c.kernel_size[0], c.kernel_size[1], c.stride[0], c.padding[0],
                              act=self.activation_name, x2=skip, upsample2x=True)


class ResidualBlock(nn.Module):
    """e2vid/model/submodules.py:140-172.  Runs only on the offline reconstruction path (after the latents are taken)."""

    def __init__(self, in_channels, out_channels, stride=1, downsample=None, norm=None):
        super().__init__()
        bias = False if norm == 'BN' else True
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=bias)
        self.norm = norm
        if norm == 'BN':
            self.bn1 = nn.BatchNorm2d(out_channels)
            self.bn2 = nn.BatchNorm2d(out_channels)
        elif norm == 'IN':
            self.bn1 = nn.InstanceNorm2d(out_channels)
            self.bn2 = nn.InstanceNorm2d(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self.downsample = downsample
        self._pw1, self._pw2 = engine.PackedWeight(), engine.PackedWeight()
        self._pw32 = (engine.PackedWeightF32(), engine.PackedWeightF32())

    def _checked_bns(self):
        """(bn1, bn2) to fold into the two convs, or (None, None); raises for the configurations the HIP paths do not run."""
        bn1, bn2 = (self.bn1, self.bn2) if self.norm == 'BN' else (None, None)
        check_runs(self.norm, bn1)
        if self.downsample is not None:
            raise NotImplementedError("E2VID residual blocks use no downsample")
        return bn1, bn2

    def forward_f32(self, x):
        """fp32 inference (K14): relu(bn2(conv2(relu(bn1(conv1(x))))) + x), the residual add and ReLU in the second conv's epilogue."""
        bn1, bn2 = self._checked_bns()
        C = self.conv1.out_channels
        p1 = self._pw32[0].get(self.conv1.weight, self.conv1.bias, bn1)
        y = hip.conv2d_f32(x, p1.packed, p1.bias, C, 3, 3, self.conv1.stride[0], 1, act='relu')
        p2 = self._pw32[1].get(self.conv2.weight, self.conv2.bias, bn2)
        return hip.conv2d_f32(y, p2.packed, p2.bias, C, 3, 3, 1, 1, act='relu', residual=x)

    def forward(self, x):
        """conv-bn-relu-conv-bn + residual + relu (:154-172); eval-mode BatchNorm folded, residual add and ReLU in the conv epilogue."""
        bn1, bn2 = self._checked_bns()
        C = self.conv1.out_channels
        p1 = self._pw1.get(self.conv1.weight, self.conv1.bias, bn1, cin_pad=x.shape[1])
        y = engine.conv2d_infer(x, p1, C, 3, 1, 1, 1, relu=True)
        p2 = self._pw2.get(self.conv2.weight, self.conv2.bias, bn2, cin_pad=C)
        return engine.conv2d_infer(y, p2, C, 3, 1, 1, 1, relu=True, residual=x)


class ConvLSTM(nn.Module):
    """e2vid/model/submodules.py:175-214.  State = (hidden, cell).  Here the state lives in two buffers:
    `xh` = the cat(x, h) NHWC bf16 buffer read by the Gates conv (x written by the encoder conv, h by the
    fused gate kernel -> no torch.cat), and `cell` in fp32."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        pad = kernel_size // 2
        self.Gates = nn.Conv2d(input_size + hidden_size, 4 * hidden_size, kernel_size, padding=pad)
        self._pw = engine.PackedWeight()
        self._pw_gates, self._pw_gates_x = engine.PackedWeight(), engine.PackedWeight()
        self._pw32, self._pw32_x = engine.PackedWeightF32(), engine.PackedWeightF32()

    def step_f32(self, state):
        """fp32 step (K14) on a RecurrentConvLayer.new_state_f32 state whose x half was just written: gates conv + cell update;
        h goes to the h half of the same cat(x, h) buffer (the gates are complete before it is written).  A fresh state (zero h
        and c, submodules.py:190-198) convolves the x half alone.  Returns the hidden state view [B, C, H, W]."""
        g = self.Gates
        C = self.hidden_size
        xh = state['xh']
        h_view = engine.from_nhwc(xh[..., C:])
        k, pad = g.kernel_size[0], g.padding[0]
        if state['fresh']:
            pw = self._pw32_x.get(g.weight, g.bias, cin=self.input_size)
            inp = engine.from_nhwc(xh[..., :self.input_size])
        else:
            pw = self._pw32.get(g.weight, g.bias)
            inp = engine.from_nhwc(xh)
        hip.convlstm_step_f32(inp, pw.packed, pw.bias, C, k, pad, state['cell'], h_view, prev_cell_is_zero=state['fresh'])
        state['fresh'] = False
        return h_view

    def fused_args(self, state):
        """Arguments of hip.convlstm_fused (or one problem of hip.convlstm_fused_group) for this state: xh, packed gates, bias,
        cell, hidden view, k, pad, prev_cell_is_zero.  The caller flips state['cur'] / clears state['fresh'] after the launch."""
        g = self.Gates
        cur = state['cur']
        xh = state['xh'][cur]
        k, pad = g.kernel_size[0], g.padding[0]
        pw = self._pw_gates.get(g.weight, g.bias, layout='gates')
        h_view = engine.nhwc(state['xh'][1 - cur][:, self.input_size:])
        if state['fresh']:
            # first sub-window: h_prev = 0 and c_prev = 0 (submodules.py:190-198), so the h half of the Gates
            # reduction contributes nothing -> convolve the x half only (half the K loop), same cell update
            pwx = self._pw_gates_x.get(g.weight, g.bias, layout='gates', cin=self.input_size)
            return (engine.nhwc(xh[:, :self.input_size]), pwx.packed, pw.bias, state['cell'], h_view, k, pad, True)
        return (engine.nhwc(xh), pw.packed, pw.bias, state['cell'], h_view, k, pad, False)

    def w128_ok(self, B, H, W):
        """Geometry rule of oess_convlstm_w128_group_bf16 (include/oess.h): 3 x 3 / pad 1 Gates, 64-channel multiples, a 256-pixel tile
        spans no more rows than the map has, 32-bit extents."""
        g = self.Gates
        C = self.hidden_size
        return (g.kernel_size == (3, 3) and g.padding == (1, 1) and C % 64 == 0 and self.input_size % 64 == 0 and H >= 8
                and (256 + W - 2) // W + 1 <= H and B * H * W * max(2 * (self.input_size + C), 4 * C) < 2 ** 31 and B * H * W * W < 2 ** 32
                and ((B * H * W + 255) // 256) * (C // 64) <= 9000)          # per-workgroup tile lists hold 124 entries (three levels: <= 62 at this bound)

    @staticmethod
    def cell_nhwc(state):
        """The cell state in the reference's order, fp32 [B, H, W, C] (a copy when the state keeps it w128-tiled)."""
        if 'cell_tiled' not in state:
            return state['cell']
        B, H, W, C = state['cell_tiled']
        return hip.convlstm_w128_cell_relayout(state['cell'], B * H * W, C, False).reshape(B, H, W, C)

    def step(self, state):
        """state: dict(xh=[two cat(x, h) buffers, B x (Cin+Ch) x H x W cl bf16], cur=index of the buffer whose x half
        was just written and whose h half holds h_prev, cell=fp32 [B,H,W,Ch], fresh=bool).
        Fused path (hidden % 32 == 0): ONE kernel = Gates conv + cell update; the new h goes to the OTHER cat buffer
        (the conv still reads h_prev around every tile), which becomes current.  Otherwise conv + gate kernel."""
        g = self.Gates
        cur = state['cur']
        xh = state['xh'][cur]
        k, pad = g.kernel_size[0], g.padding[0]
        if 'cell_tiled' in state:
            if not hip.convlstm_w128_group([self.fused_args(state)]):
                raise RuntimeError("oess_convlstm_w128_group_bf16 refused a state that ConvLSTM.w128_ok accepted")
            h_view = state['xh'][1 - cur][:, self.input_size:]
            state['cur'] = 1 - cur
        elif self.hidden_size % 32 == 0:
            hip.convlstm_fused(*self.fused_args(state))
            h_view = state['xh'][1 - cur][:, self.input_size:]
            state['cur'] = 1 - cur
        else:
            pw = self._pw.get(g.weight, g.bias, None, cin_pad=xh.shape[1])
            gates = engine.conv2d_infer(xh, pw, g.out_channels, k, 1, pad, 1, out=state.get('gates'))
            state['gates'] = gates
            h_view = xh[:, self.input_size:]
            hip.convlstm_gates(engine.nhwc(gates), state['cell'], engine.nhwc(h_view), prev_cell_is_zero=state['fresh'])
        state['fresh'] = False
        return h_view


class ConvGRU(nn.Module):
    """e2vid/model/submodules.py:217-253.  State = the hidden state.  Here it lives in ONE NHWC bf16 buffer `hxr` = [B, H, W, 3C]
    ordered h | x | r*h (x written by the encoder conv, r*h by the gates launch, h by the output launch: no torch.cat, no copy,
    no ping-pong: no launch writes a window it convolves) plus `h32`, the fp32 master of h (the blend h (1 - u) + o u does not
    round h to bf16 once per sub-window), and `u`, the update gate between the two launches.  K28 of DESIGN.md."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        pad = kernel_size // 2
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.reset_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        self.update_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        self.out_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=pad)
        for g in (self.reset_gate, self.update_gate, self.out_gate):
            nn.init.orthogonal_(g.weight)
            nn.init.constant_(g.bias, 0.)
        # operands by (phase, fresh): the gates pair (update, reset) and the out gate, for the two-part window and for x alone
        self._pw = {(ph, fr): engine.PackedWeight() for ph in ('gates', 'out') for fr in (False, True)}
        self._pw32 = {(ph, fr): engine.PackedWeightF32() for ph in ('gates', 'out') for fr in (False, True)}

    def _weights(self, phase, fresh, dtype, interleave):
        """(weight, bias) of one launch in `dtype`.  gates: update and reset stacked (rows 2 hc + gate when `interleave`, else
        update | reset), input channels reordered from the reference's (x | h) to the state buffer's (h | x); out: the out gate in
        its own (x | r*h) order.  fresh: the x half alone (h = 0)."""
        X = self.input_size
        if phase == 'out':
            w, b = self.out_gate.weight.detach().to(dtype), self.out_gate.bias.detach().to(dtype)
            return (w[:, :X] if fresh else w), b
        ws = [g.weight.detach().to(dtype) for g in (self.update_gate, self.reset_gate)]
        ws = [w[:, :X] if fresh else torch.cat([w[:, X:], w[:, :X]], 1) for w in ws]
        w = torch.stack(ws, 1).flatten(0, 1) if interleave else torch.cat(ws, 0)
        return w, torch.cat([self.update_gate.bias.detach().to(dtype), self.reset_gate.bias.detach().to(dtype)])

    def _convs(self, phase):
        return (self.out_gate,) if phase == 'out' else (self.update_gate, self.reset_gate)

    def _packed(self, phase, fresh):
        """The bf16 operand (engine.PackedWeight) of one launch, repacked when a gate parameter's version moves."""
        pw = self._pw[(phase, fresh)]
        ver = tuple(engine.param_versions(c.weight, c.bias) for c in self._convs(phase))
        if pw.key is None or pw.key[0] != ver:
            with torch.no_grad():
                w, b = self._weights(phase, fresh, torch.float32, True)
            pw.get(w.contiguous(), b.contiguous(), ver=ver)
        return pw

    def _packed_f32(self, phase, fresh):
        params = [p for c in self._convs(phase) for p in (c.weight, c.bias)]
        return self._pw32[(phase, fresh)].get_composed(params, lambda: self._weights(phase, fresh, torch.float64, False))

    def new_state(self, B, H, W, device):
        """A fresh bf16 state: nothing is zero-filled, the first step convolves the x window alone and reads no h."""
        C = self.hidden_size
        f32 = lambda: torch.empty((B, H, W, C), dtype=torch.float32, device=device)
        return {'block': 'convgru', 'hxr': engine.empty_cl(B, 3 * C, H, W, device), 'h32': f32(), 'u': f32(), 'fresh': True}

    def new_state_f32(self, B, H, W, device):
        C = self.hidden_size
        return {'block': 'convgru', 'precision': 'fp32', 'hxr': torch.empty((B, H, W, 3 * C), dtype=torch.float32, device=device),
                'fresh': True}

    def x_window(self, state):
        """The [B, C, H, W] view the encoder conv writes (either precision)."""
        C = self.hidden_size
        return engine.from_nhwc(state['hxr'][..., C:2 * C]) if state.get('precision') == 'fp32' else state['hxr'][:, C:2 * C]

    def step(self, state, rh_f32=None):
        """One bf16 step on a new_state state whose x window was just written: two launches (hip.convgru_gates,
        hip.convgru_out).  3 x 3 gates, input_size == hidden_size, hidden_size % 32 == 0; anything else is refused by the entry
        points (there is no unfused bf16 form).  rh_f32: optional fp32 [B, H, W, C] receiving r*h before its rounding (tests).
        Returns the bf16 hidden state view [B, C, H, W]."""
        g = self.out_gate
        C, fresh = self.hidden_size, state['fresh']
        if self.input_size != C:
            raise ValueError("the bf16 ConvGRU kernels need input_size == hidden_size")
        k, pad = g.kernel_size[0], g.padding[0]
        buf = engine.nhwc(state['hxr'])
        pa, pb = self._packed('gates', fresh), self._packed('out', fresh)
        win_a = buf[..., C:2 * C] if fresh else buf[..., :2 * C]
        win_b = buf[..., C:2 * C] if fresh else buf[..., C:]
        hip.convgru_gates(win_a, pa.packed, pa.bias, state['h32'], state['u'], buf[..., 2 * C:], k, pad, h_is_zero=fresh, rh_f32=rh_f32)
        hip.convgru_out(win_b, pb.packed, pb.bias, state['u'], state['h32'], buf[..., :C], k, pad, h_is_zero=fresh)
        state['fresh'] = False
        return state['hxr'][:, :C]

    def step_f32(self, state):
        """One fp32 step (K28) on a new_state_f32 state whose x window was just written: hip.convgru_step_f32, four launches.
        Returns the hidden state view [B, C, H, W]."""
        g = self.out_gate
        fresh = state['fresh']
        pa, pb = self._packed_f32('gates', fresh), self._packed_f32('out', fresh)
        h = hip.convgru_step_f32(state['hxr'], pa.packed, pa.bias, pb.packed, pb.bias, self.hidden_size, g.kernel_size[0], g.padding[0],
                                 h_is_zero=fresh)
        state['fresh'] = False
        return h


def state_block_type(state):
    """'convgru' for a ConvGRU state (either precision), 'convlstm' for any other state, None for None."""
    if state is None:
        return None
    return 'convgru' if isinstance(state, dict) and state.get('block') == 'convgru' else 'convlstm'


class RecurrentConvLayer(nn.Module):
    """e2vid/model/submodules.py:96-115.  recurrent_block_type 'convlstm' or 'convgru'; a state belongs to one block type and one
    precision (unet.check_states)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0,
                 recurrent_block_type='convlstm', activation='relu', norm=None):
        super().__init__()
        assert recurrent_block_type in ('convlstm', 'convgru')
        self.recurrent_block_type = recurrent_block_type
        self.conv = ConvLayer(in_channels, out_channels, kernel_size, stride, padding, activation, norm)
        RecurrentBlock = ConvLSTM if recurrent_block_type == 'convlstm' else ConvGRU
        self.recurrent_block = RecurrentBlock(input_size=out_channels, hidden_size=out_channels, kernel_size=3)

    def _state_shape(self, x):
        """(B, Ho, Wo, Co) of the encoder conv's output for the input x."""
        B, _, H, W = x.shape
        c = self.conv.conv2d
        Ho = (H + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
        Wo = (W + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
        return B, Ho, Wo, c.out_channels

    def new_state(self, x):
        B, Ho, Wo, Co = self._state_shape(x)
        if self.recurrent_block_type == 'convgru':
            return self.recurrent_block.new_state(B, Ho, Wo, x.device)
        # fused ConvLSTM path: the first step convolves the x half only (zero state) and every later read of a cat(x, h) buffer
        # follows the encoder conv's write of its x half and the previous step's write of its h half -> no zero fill needed
        # (6 fills of up to 157 MB per pre-training step); the conv + gate-kernel path reads h_prev = 0 from the buffer itself
        make = engine.empty_cl if self.recurrent_block.hidden_size % 32 == 0 else engine.zeros_cl
        st = {'xh': [make(B, 2 * Co, Ho, Wo, x.device), make(B, 2 * Co, Ho, Wo, x.device)], 'cur': 0, 'fresh': True}
        if self.recurrent_block.w128_ok(B, Ho, Wo):
            # the cell state only ever feeds the next ConvLSTM step (submodules.py:205-212): it lives in the gate kernel's own
            # "w128-tiled" layout (hip.convlstm_w128_group); ConvLSTM.cell_nhwc(state) gives the reference's [B, H, W, C] order
            st['cell'] = torch.empty(hip.convlstm_w128_cell_elems(B * Ho * Wo, Co), dtype=torch.float32, device=x.device)
            st['cell_tiled'] = (B, Ho, Wo, Co)
        else:
            st['cell'] = torch.empty((B, Ho, Wo, Co), dtype=torch.float32, device=x.device)
        return st

    def conv_s2_args(self, x, state):
        """One problem of hip.conv5x5s2_group for this layer's encoder conv (x -> x half of the current cat(x, h) buffer), or None
        when the layer is not a 5x5 / stride-2 / pad-2 conv with a foldable norm and relu / no activation."""
        m, c = self.conv, self.conv.conv2d
        if not (c.kernel_size == (5, 5) and c.stride == (2, 2) and c.padding == (2, 2) and m.activation_name in (None, 'relu')
                and m.norm != 'IN' and not (m.norm == 'BN' and m.norm_layer.training) and x.shape[1] % 32 == 0
                and c.out_channels % 64 == 0 and x.dtype == torch.bfloat16 and x.stride(1) == 1):
            return None
        pw = m._packed(x.shape[1])
        out = state['xh'][state['cur']][:, :c.out_channels]
        return (engine.nhwc(x), pw.packed, pw.bias, c.out_channels, m.activation_name == 'relu', engine.nhwc(out))

    def run_conv(self, x, prev_state):
        state = prev_state if prev_state is not None else self.new_state(x)
        if self.recurrent_block_type == 'convgru':
            self.conv(x, out=self.recurrent_block.x_window(state))  # x -> the x window of the h | x | r*h buffer
            return state
        Co = self.conv.conv2d.out_channels
        self.conv(x, out=state['xh'][state['cur']][:, :Co])         # x -> first half of the current cat(x, h) buffer
        return state

    def new_state_f32(self, x):
        """State of the fp32 path: one cat(x, h) buffer fp32 [B, Ho, Wo, 2 C] (x half written by the encoder conv, h half by the
        ConvLSTM step), the cell fp32 [B, Ho, Wo, C], 'fresh' = no previous state; 'precision' tells it from a bf16 state."""
        B, Ho, Wo, Co = self._state_shape(x)
        if self.recurrent_block_type == 'convgru':
            return self.recurrent_block.new_state_f32(B, Ho, Wo, x.device)
        return {'precision': 'fp32', 'xh': torch.empty((B, Ho, Wo, 2 * Co), dtype=torch.float32, device=x.device),
                'cell': torch.empty((B, Ho, Wo, Co), dtype=torch.float32, device=x.device), 'fresh': True}

    def forward_f32(self, x, prev_state):
        """fp32 inference (K14): encoder conv into the x half of the state's cat(x, h) buffer, then the ConvLSTM step.
        Returns (h view [B, C, Ho, Wo], state)."""
        state = prev_state if prev_state is not None else self.new_state_f32(x)
        if self.recurrent_block_type == 'convgru':
            self.conv.forward_f32(x, out=self.recurrent_block.x_window(state))
            return self.recurrent_block.step_f32(state), state
        Co = self.conv.conv2d.out_channels
        self.conv.forward_f32(x, out=engine.from_nhwc(state['xh'][..., :Co]))
        return self.recurrent_block.step_f32(state), state

    def forward(self, x, prev_state):
        state = self.run_conv(x, prev_state)
        h = self.recurrent_block.step(state)
        return h, state
