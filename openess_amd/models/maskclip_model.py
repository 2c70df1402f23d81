"""Mirror of the MaskCLIP ViT-B/16 image tower of models/maskclip_model.py: same module tree and
state_dict keys as the reference (`encoder.layers.N.ln1`, `encoder.layers.N.attn.attn.in_proj_weight`,
`encoder.layers.N.ffn.layers.0.0.weight`, `encoder.ln0/ln1`, `encoder.patch_embed.projection.weight`, `decoder.proj`,
`decoder.text_embeddings`), so `load_checkpoint1`-style loading of a MaskCLIP checkpoint's `backbone.*` keys works
unchanged; the forward runs on liboess kernels:

  patch embedding 16x16/16  -> MFMA conv (oess_conv2d_fwd_bf16)            maskclip_model.py:317-446, 812-813
  LayerNorm (eps 1e-6)      -> oess_layernorm_bf16                         :486-501, 706-718
  in_proj / out_proj / FFN  -> MFMA 1x1 convs over the token axis, bias / residual / GELU fused   :496-512
  attention                 -> oess_attention_d64_bf16                     :538
  last layer                -> value path only (:518-536): v = out_proj(W_v ln1(x)) + x ; v += ffn(ln2(v)) ; the
                               attention branch of that layer is dead for MaskClipHead (feat = proj(v), :181-183)
  head                      -> proj (1x1 conv) -> oess_l2norm -> text-embedding classifier (1x1 conv, fp32 logits)
                               -> bilinear resize to the image, align_corners=False            :157-222, 903-908

Every module also has `forward_fp32` (K25): the same graph in the reference's arithmetic on the fp32 token kernels
(oess_layernorm_f32, oess_attention_d64_f32, oess_linear_tokens_f32 on the f32-input MFMA), fp32 operands in caches of their
own; the patch embedding there is a re-layout of the corner-padded image into [B hp wp, 3 * 16 * 16] rows and a token GEMM.

MaskCLIP's test-time refinement (K26; MaskClipHead.refine_output, :224-250, whose call the reference comments out at :213-214):
`forward(img, refine=True)` / `forward_fp32(img, refine=True)` run cls_seg -> refine_output -> resize, with the last layer's keys
(:519-533; forward_key_path) and prompt denoising + key smoothing on hip.maskclip_refine (oess_maskclip_refine_f32).  Off by
default: refine=False runs no key GEMM and returns what it always returned.

Frozen (the reference sets requires_grad=False on encoder and decoder, :888-891): inference only.
The reference trainers construct this model but never call it; here it is callable as an online
teacher: `maskClipFeatureExtractor(img) -> logits [B, K, H, W]`."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import engine, hip


def _linear_tokens(x2d, weight, bias, pw, act=0, residual=None, rows=None, out_f32=False):
    """y = act(x @ W^T + b [+ residual]) for a bf16 token matrix [rows, Cin] on the MFMA conv kernel (1x1 conv, NHWC
    view [1, 1, rows, Cin]).  `weight` may be a row slice of a parameter (its version is taken from the base tensor)."""
    base = weight._base if weight._base is not None else weight
    bver = None if bias is None else (bias._base if bias._base is not None else bias)._version
    pw.get(weight.detach()[:, :, None, None], None if bias is None else bias.detach(), None, cin_pad=x2d.shape[1],
           ver=(base._version, bver, weight.data_ptr()))
    x4 = x2d.view(1, 1, x2d.shape[0], x2d.shape[1])
    r4 = None if residual is None else residual.view(1, 1, residual.shape[0], residual.shape[1])
    y = hip.conv2d_nhwc(x4, pw.packed, pw.bias, weight.shape[0], 1, 1, 1, 0, 1, relu=act, residual=r4, out_f32=out_f32)
    return y.view(x2d.shape[0], weight.shape[0])


def _linear_tokens_f32(x2d, weight, bias, pw, act=None, residual=None):
    """y = act(x @ W^T + b [+ residual]) for fp32 tokens [rows, Cin] on the fp32 conv kernel.  `weight` / `bias` may be row
    slices of a parameter (a view carries its base's version counter; every cache serves one fixed slice)."""
    pw.get(weight.detach()[:, :, None, None], None if bias is None else bias.detach())
    return hip.linear_tokens_f32(x2d, pw.packed, pw.bias, weight.shape[0], act=act, residual=residual)


class _Attn(nn.Module):
    def __init__(self, dims, heads):
        super().__init__()
        self.attn = nn.MultiheadAttention(dims, heads, bias=True)        # parameter container (mmcv wrapper layout)


class _FFN(nn.Module):
    def __init__(self, dims, hidden):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(dims, hidden), nn.GELU(), nn.Dropout(0.0)),
                                    nn.Linear(hidden, dims), nn.Dropout(0.0))


class TransformerEncoderLayer(nn.Module):
    """maskclip_model.py:448-541."""

    def __init__(self, embed_dims=768, num_heads=12, feedforward_channels=3072):
        super().__init__()
        self.num_heads = num_heads
        self.ln1 = nn.LayerNorm(embed_dims, eps=1e-6)
        self.attn = _Attn(embed_dims, num_heads)
        self.ln2 = nn.LayerNorm(embed_dims, eps=1e-6)
        self.ffn = _FFN(embed_dims, feedforward_channels)
        self._pw = {k: engine.PackedWeight() for k in ('qkv', 'v', 'out', 'fc1', 'fc2', 'k', 'k_out')}
        self._pw32 = {k: engine.PackedWeightF32() for k in ('qkv', 'v', 'out', 'fc1', 'fc2', 'k', 'k_out')}

    def _ffn_fp32(self, x):
        y = hip.layer_norm_tokens_f32(x, self.ln2.weight, self.ln2.bias, self.ln2.eps)
        fc1, fc2 = self.ffn.layers[0][0], self.ffn.layers[1]
        h = _linear_tokens_f32(y, fc1.weight, fc1.bias, self._pw32['fc1'], act='gelu')
        return _linear_tokens_f32(h, fc2.weight, fc2.bias, self._pw32['fc2'], residual=x)

    def forward_fp32(self, x, B, L):
        """x: fp32 tokens [B*L, C] -> same shape (full block)."""
        a = self.attn.attn
        y = hip.layer_norm_tokens_f32(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        qkv = _linear_tokens_f32(y, a.in_proj_weight, a.in_proj_bias, self._pw32['qkv'])
        o = hip.attention_d64_f32(qkv, B, L, self.num_heads)
        x = _linear_tokens_f32(o, a.out_proj.weight, a.out_proj.bias, self._pw32['out'], residual=x)
        return self._ffn_fp32(x)

    def forward_value_path_fp32(self, x):
        """forward_value_path on fp32 tokens."""
        a = self.attn.attn
        C = x.shape[1]
        y = hip.layer_norm_tokens_f32(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        v = _linear_tokens_f32(y, a.in_proj_weight[2 * C:], a.in_proj_bias[2 * C:], self._pw32['v'])
        v = _linear_tokens_f32(v, a.out_proj.weight, a.out_proj.bias, self._pw32['out'], residual=x)
        return self._ffn_fp32(v)

    def forward_key_path_fp32(self, x):
        """forward_key_path on fp32 tokens."""
        a = self.attn.attn
        C = x.shape[1]
        y = hip.layer_norm_tokens_f32(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        k = _linear_tokens_f32(y, a.in_proj_weight[C:2 * C], a.in_proj_bias[C:2 * C], self._pw32['k'])
        return _linear_tokens_f32(k, a.out_proj.weight, a.out_proj.bias, self._pw32['k_out'])

    def _ffn(self, x):
        y = hip.layer_norm_tokens(x, self.ln2.weight, self.ln2.bias, self.ln2.eps)
        fc1, fc2 = self.ffn.layers[0][0], self.ffn.layers[1]
        h = _linear_tokens(y, fc1.weight, fc1.bias, self._pw['fc1'], act=2)                  # Linear + GELU
        return _linear_tokens(h, fc2.weight, fc2.bias, self._pw['fc2'], residual=x)          # identity + Linear

    def forward(self, x, B, L):
        """x: bf16 tokens [B*L, C] -> same shape (full block)."""
        a = self.attn.attn
        y = hip.layer_norm_tokens(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        qkv = _linear_tokens(y, a.in_proj_weight, a.in_proj_bias, self._pw['qkv'])
        o = hip.attention_d64(qkv, B, L, self.num_heads)
        x = _linear_tokens(o, a.out_proj.weight, a.out_proj.bias, self._pw['out'], residual=x)
        return self._ffn(x)

    def forward_value_path(self, x):
        """:518-536 with return_qkv: v = out_proj(in_proj_v(ln1(x))) + x ; v = v + ffn(ln2(v))."""
        a = self.attn.attn
        C = x.shape[1]
        y = hip.layer_norm_tokens(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        v = _linear_tokens(y, a.in_proj_weight[2 * C:], a.in_proj_bias[2 * C:], self._pw['v'])
        v = _linear_tokens(v, a.out_proj.weight, a.out_proj.bias, self._pw['out'], residual=x)
        return self._ffn(v)

    def forward_key_path(self, x):
        """:519-533 with return_qkv, the k of q, k, v: k = out_proj(in_proj_k(ln1(x))), rows C:2C of in_proj; no residual (only v
        gets `+= x`) and no FFN.  The keys MaskClipHead.refine_output smooths with (K26); packed operands of its own."""
        a = self.attn.attn
        C = x.shape[1]
        y = hip.layer_norm_tokens(x, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        k = _linear_tokens(y, a.in_proj_weight[C:2 * C], a.in_proj_bias[C:2 * C], self._pw['k'])
        return _linear_tokens(k, a.out_proj.weight, a.out_proj.bias, self._pw['k_out'])


class VisionTransformer(nn.Module):
    """maskclip_model.py:545-851 with its constructor defaults (ViT-B/16, pre_norm, final_norm, return_qkv on the last
    layer).  forward(img) -> v_map [B, 768, H/16, W/16] (the value-path feature MaskClipHead consumes)."""

    def __init__(self, img_size=(224, 224), patch_size=16, in_channels=3, embed_dims=768, num_layers=12, num_heads=12,
                 mlp_ratio=4):
        super().__init__()
        if num_heads * 64 != embed_dims:
            raise ValueError("the attention kernel is specialised for head dimension 64")
        self.img_size, self.patch_size, self.embed_dims = tuple(img_size), patch_size, embed_dims
        self.patch_embed = nn.Module()
        self.patch_embed.projection = nn.Conv2d(in_channels, embed_dims, patch_size, patch_size, bias=False)
        n_patches = (img_size[0] // patch_size) * (img_size[1] // patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dims))
        self.pos_embed = nn.Parameter(torch.zeros(1, n_patches + 1, embed_dims))
        self.layers = nn.ModuleList([TransformerEncoderLayer(embed_dims, num_heads, mlp_ratio * embed_dims)
                                     for _ in range(num_layers)])
        self.ln0 = nn.LayerNorm(embed_dims, eps=1e-6)
        self.ln1 = nn.LayerNorm(embed_dims, eps=1e-6)
        self._pw_patch = engine.PackedWeight()
        self._pw_patch32 = engine.PackedWeightF32()
        self._pos_cache = {}

    def _pos(self, hw):
        """:770-797 resize_pos_embed: bicubic, align_corners=False, class-token weight kept (cached per grid size)."""
        key = (hw, self.pos_embed._version)
        if key not in self._pos_cache:
            ph, pw = self.img_size[0] // self.patch_size, self.img_size[1] // self.patch_size
            pe = self.pos_embed.detach().float()
            if hw != (ph, pw):
                grid = pe[:, -ph * pw:].reshape(1, ph, pw, -1).permute(0, 3, 1, 2)
                grid = F.interpolate(grid, size=hw, mode='bicubic', align_corners=False)
                pe = torch.cat((pe[:, 0:1], grid.flatten(2).transpose(1, 2)), dim=1)
            self._pos_cache = {key: pe}
        return self._pos_cache[key]

    @torch.no_grad()
    def forward(self, img, return_k=False):
        """return_k: (v_map, k) with k the last layer's keys [B, hp wp, C] (:841-848; forward_key_path), a view of the token
        matrix past its class-token rows, not normalised by ln1 of the encoder (only v is, :846)."""
        B, Cin, H, W = img.shape
        p, C = self.patch_size, self.embed_dims
        Hp, Wp = (H + p - 1) // p * p, (W + p - 1) // p * p
        x8 = torch.zeros((B, Hp, Wp, 8), dtype=torch.bfloat16, device=img.device)      # corner padding + 3 -> 8 channels
        x8[:, :H, :W, :Cin] = img.permute(0, 2, 3, 1)
        pw = self._pw_patch.get(self.patch_embed.projection.weight, None, None, cin_pad=8)
        patches = hip.conv2d_nhwc(x8, pw.packed, None, C, p, p, p, 0, 1)                # [B, hp, wp, C]
        hp, wp = patches.shape[1], patches.shape[2]
        L = hp * wp + 1
        tok = torch.empty((B, L, C), dtype=torch.float32, device=img.device)
        tok[:, 0] = self.cls_token.detach()[0, 0]
        tok[:, 1:] = patches.view(B, hp * wp, C)
        tok += self._pos((hp, wp))
        x = hip.layer_norm_tokens(tok.to(torch.bfloat16).view(B * L, C), self.ln0.weight, self.ln0.bias, self.ln0.eps)
        for layer in self.layers[:-1]:
            x = layer(x, B, L)
        v = self.layers[-1].forward_value_path(x)
        v = hip.layer_norm_tokens(v, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        v_map = v.view(B, L, C)[:, 1:].reshape(B, hp, wp, C).permute(0, 3, 1, 2)        # logical NCHW, NHWC memory
        if return_k:
            return v_map, self.layers[-1].forward_key_path(x).view(B, L, C)[:, 1:]
        return v_map


    @torch.no_grad()
    def forward_fp32(self, img, return_k=False):
        """forward in fp32: v_map [B, 768, H/16, W/16] fp32 (return_k: and the fp32 keys, as in forward).  Stride equals kernel in the patch embedding, so it is a re-layout
        of the corner-padded image into one row per patch, (c, dy, dx) order like the flattened weight, and a token GEMM."""
        B, Cin, H, W = img.shape
        p, C = self.patch_size, self.embed_dims
        hp, wp = (H + p - 1) // p, (W + p - 1) // p
        xp = torch.zeros((B, Cin, hp * p, wp * p), dtype=torch.float32, device=img.device)
        xp[:, :, :H, :W] = img
        rows = xp.view(B, Cin, hp, p, wp, p).permute(0, 2, 4, 1, 3, 5).reshape(B * hp * wp, Cin * p * p)
        w = self.patch_embed.projection.weight
        patches = _linear_tokens_f32(rows, w.view(w.shape[0], -1), None, self._pw_patch32)
        L = hp * wp + 1
        tok = torch.empty((B, L, C), dtype=torch.float32, device=img.device)
        tok[:, 0] = self.cls_token.detach()[0, 0]
        tok[:, 1:] = patches.view(B, hp * wp, C)
        tok += self._pos((hp, wp))
        x = hip.layer_norm_tokens_f32(tok.view(B * L, C), self.ln0.weight, self.ln0.bias, self.ln0.eps)
        for layer in self.layers[:-1]:
            x = layer.forward_fp32(x, B, L)
        v = self.layers[-1].forward_value_path_fp32(x)
        v = hip.layer_norm_tokens_f32(v, self.ln1.weight, self.ln1.bias, self.ln1.eps)
        v_map = v.view(B, L, C)[:, 1:].reshape(B, hp, wp, C).permute(0, 3, 1, 2)        # logical NCHW, NHWC memory
        if return_k:
            return v_map, self.layers[-1].forward_key_path_fp32(x).view(B, L, C)[:, 1:]
        return v_map


class MaskClipHead(nn.Module):
    """maskclip_model.py:52-222 (vit=True): logits = conv2d(normalize(proj(v)), text_embeddings)."""

    def __init__(self, text_categories=16, text_channels=512, in_channels=768, ks_thresh=1, pd_thresh=0.5):
        super().__init__()
        if not 0 <= ks_thresh < float('inf') or not 0 <= pd_thresh < float('inf'):
            raise ValueError(f"ks_thresh and pd_thresh must be finite and >= 0, got {ks_thresh!r}, {pd_thresh!r}")
        self.ks_thresh, self.pd_thresh = ks_thresh, pd_thresh            # :72-73, :124-125
        self.align_corners = False
        self.num_classes = text_categories
        self.register_buffer('text_embeddings', torch.randn(text_categories, text_channels))
        self.proj = nn.Conv2d(in_channels, text_channels, 1, bias=False)
        self.image_mapping_local = nn.Conv2d(in_channels, 512, 1)           # constructed by the reference, never used (:125)
        self._pw_proj, self._pw_text = engine.PackedWeight(), engine.PackedWeight()
        self._pw_proj32, self._pw_text32 = engine.PackedWeightF32(), engine.PackedWeightF32()

    @torch.no_grad()
    def forward(self, v_map):
        B, C, hp, wp = v_map.shape
        v2 = engine.nhwc(v_map).reshape(B * hp * wp, C)
        feat = _linear_tokens(v2, self.proj.weight[:, :, 0, 0], None, self._pw_proj)
        feat = hip.l2_normalize(feat.view(B, hp, wp, -1).permute(0, 3, 1, 2), eps=1e-30)    # feat / feat.norm(dim=1) (:217)
        f2 = engine.nhwc(feat).reshape(B * hp * wp, -1)
        logits = _linear_tokens(f2, self.text_embeddings, None, self._pw_text, out_f32=True)
        return v_map, logits.view(B, hp, wp, -1).permute(0, 3, 1, 2)


    @torch.no_grad()
    def forward_fp32(self, v_map):
        """forward on an fp32 v_map: (v_map, fp32 logits [B, K, hp, wp])."""
        B, C, hp, wp = v_map.shape
        v2 = engine.nhwc(v_map).reshape(B * hp * wp, C)
        feat = _linear_tokens_f32(v2, self.proj.weight[:, :, 0, 0], None, self._pw_proj32)
        feat = hip.l2_normalize(feat.view(B, hp, wp, -1).permute(0, 3, 1, 2), eps=1e-30)
        f2 = engine.nhwc(feat).reshape(B * hp * wp, -1)
        logits = _linear_tokens_f32(f2, self.text_embeddings, None, self._pw_text32)
        return v_map, logits.view(B, hp, wp, -1).permute(0, 3, 1, 2)

    @torch.no_grad()
    def refine_output(self, output, k):
        """:224-250: prompt denoising (pd_thresh) and key smoothing (ks_thresh, k [B, hp wp, C] or None) of the fp32 logits
        [B, K, hp, wp] on hip.maskclip_refine.  Returns a new tensor (the reference writes the -100 rows into `output`):
        probabilities when smoothing runs, the denoised logits otherwise."""
        return hip.maskclip_refine(output, k, pd_thresh=self.pd_thresh, ks_thresh=self.ks_thresh)


class maskClipFeatureExtractor(nn.Module):
    """maskclip_model.py:854-915.  Checkpoint / text-embedding / projection files are optional here (the reference
    requires them): pass paths to load them with the reference's key mapping, or load a state_dict afterwards."""

    def __init__(self, text_embeddings_path=None, visual_projs_path=None, text_categories=16, maskclip_checkpoint=None,
                 preprocessing=None, test_cfg=dict(mode='whole'), img_size=(224, 224), ks_thresh=1, pd_thresh=0.5):
        super().__init__()
        self.encoder = VisionTransformer(img_size=img_size)
        self.decoder = MaskClipHead(text_categories=text_categories, ks_thresh=ks_thresh, pd_thresh=pd_thresh)
        self.align_corners = self.decoder.align_corners
        self.num_classes = self.decoder.num_classes
        self.test_cfg = test_cfg
        self.checkpoint = maskclip_checkpoint
        if text_embeddings_path:
            self.decoder.text_embeddings[:, :] = torch.load(text_embeddings_path, map_location='cpu')[:, :]
        if visual_projs_path:                                               # load_visual_projs (:132-143)
            sd = torch.load(visual_projs_path, map_location='cpu')['proj']
            self.decoder.proj.load_state_dict({k: (v[:, :, None, None] if 'weight' in k and v.ndim == 2 else v) for k, v in sd.items()})
        if maskclip_checkpoint:                                             # load_checkpoint1 (:20-50)
            pre = torch.load(maskclip_checkpoint, map_location='cpu')['state_dict']
            pre = {(k[len('backbone.'):] if k.startswith('backbone.') else k): v for k, v in pre.items()}
            mine = self.encoder.state_dict()
            mine.update({k: v for k, v in pre.items() if k in mine and mine[k].shape == v.shape})
            self.encoder.load_state_dict(mine)
        for p in self.parameters():
            p.requires_grad = False

    # (Two half batches on two HIP streams -- the tower couples no samples, and its token GEMMs leave 15-20 % of their last round of
    #  tiles empty -- were measured in round 5: 4.17 vs 4.22 ms, bit-identical; not kept.)
    @torch.no_grad()
    def forward(self, img, refine=False):
        """refine=True (K26): MaskCLIP's order cls_seg -> refine_output -> resize -> (argmax), with the decoder's thresholds; the
        result then holds resized probabilities (ks_thresh > 0) instead of logits.  refine=False runs no key GEMM."""
        if not refine:
            v_map = self.encoder(img)
            _, logits = self.decoder(v_map)
            return hip.bilinear_resize(logits.float(), size=(img.shape[2], img.shape[3]), align_corners=self.align_corners)
        v_map, k = self.encoder(img, return_k=True)
        _, logits = self.decoder(v_map)
        refined = self.decoder.refine_output(logits.float(), k)
        return hip.bilinear_resize(refined, size=(img.shape[2], img.shape[3]), align_corners=self.align_corners)

    @torch.no_grad()
    def forward_fp32(self, img, refine=False):
        """The tower in the reference's arithmetic: fp32 logits [B, K, H, W] (the online teacher of
        `online_teacher_precision: fp32`; its argmax is the dense-CLIP pseudo-label map).  refine: as in forward, on fp32 keys."""
        if not refine:
            v_map = self.encoder.forward_fp32(img.float())
            _, logits = self.decoder.forward_fp32(v_map)
            return hip.bilinear_resize(logits, size=(img.shape[2], img.shape[3]), align_corners=self.align_corners)
        v_map, k = self.encoder.forward_fp32(img.float(), return_k=True)
        _, logits = self.decoder.forward_fp32(v_map)
        refined = self.decoder.refine_output(logits, k)
        return hip.bilinear_resize(refined, size=(img.shape[2], img.shape[3]), align_corners=self.align_corners)

    @torch.no_grad()
    def labels(self, img, refine=False, precision='bf16'):
        """int64 [B, H, W] pseudo-labels: the integers of forward(img, refine).argmax(1) (precision='fp32': of forward_fp32),
        from the stride-level fp32 logits (or the refined output) on hip.argmax_labels -- the [B, K, H, W] tensor that only the
        argmax read is never written."""
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        fp32 = precision == 'fp32'
        enc = self.encoder.forward_fp32 if fp32 else self.encoder
        dec = self.decoder.forward_fp32 if fp32 else self.decoder
        x = img.float() if fp32 else img
        if not refine:
            _, low = dec(enc(x))
        else:
            v_map, k = enc(x, return_k=True)
            _, logits = dec(v_map)
            low = self.decoder.refine_output(logits.float(), k)
        return hip.argmax_labels(low.float(), size=(img.shape[2], img.shape[3]), align_corners=self.align_corners)
