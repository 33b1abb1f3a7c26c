"""Model-stage-1 / model-stage-2 module API on MI355X.

Mirrors /root/reference/src/mamba_clip/model.py's public surface:
  ClipModel (model.py:998-1112)      forward(image, text) -> {"image_features", "text_features",
                                     "logit_scale" (=exp), ["logit_bias"]}; encode_image/encode_text;
                                     get_logits; lock_text_tower; set_grad_checkpointing
  ClipClassifier (model.py:1115-1205) frozen stage-1 CLIP + MLP head; classify
  SS2D / SS_Conv_SSM / VSSLayer / VSSM (model.py:297-995): the MedMamba
                                     cross-scan vision backbone ("medmamba")
  init_model (model.py:1257-1289)    factory returning (model, preprocess_train, preprocess_val, tokenizer)

Towers the reference obtains from open_clip / HF hub (not available offline,
SURVEY.md 8c) are defined here and random-initialised:
  VisionTransformer  ViT-B/16 (timm vit_base_patch16_224 shape: 12 pre-LN
                     blocks, 768 wide, cls pooling, proj -> embed_dim)
  MambaTextEncoder   Mamba LM text tower (Mamba-130M: 24 x d_model 768,
                     d_inner 1536, d_state 16, RMSNorm, fp32 residual stream); with pad_id it
                     pools each caption's last token and computes transformers.MambaModel
  BertTextEncoder    PubMedBERT-base shape (12 x 768, ctx 256) for BiomedCLIP
  HFBertTextEncoder  the same tower computing transformers.BertModel (post-LN, token types, padding mask)
  ClipTextEncoder    the CLIP text transformer (12 x 512, 77 tokens, causal attention, end-of-text
                     pooling) computing transformers.CLIPTextModelWithProjection
Hot ops run on the HIP library: selective scan, causal conv1d, fused
add+RMSNorm / add+LayerNorm, patch im2col, short-sequence attention
(attention.hip), contrastive loss; dense projections are plain library GEMMs
(hipBLASLt through torch, launched data-parallel: see __init__.py).
"""
import math
import os
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint

from . import GEMM_GRIDS_DATA_PARALLEL
from .ops import (GradHandoff, GradSlab, _compute_dtype, add_layernorm, add_pos, add_rmsnorm, attn_supported,
                  causal_conv1d, keep_slots, l2_normalize, last_token_rmsnorm, linear_sk, mlp, neg_exp_many,
                  pack_key_mask, packed_attention, patch_im2col, patch_keep_indices, qkv_proj, split_rows,
                  split_rows_n, ss2d_conv_stack, ss2d_merge_ln_gate, ss2d_proj, ss2d_proj_ok, token_embed,
                  token_embed_gather, weight_cast_scope, wleft_mm)
from .selective_scan_interface import (SS2D_REVERSE_GROUPS, SS2D_U_GROUPS, SelectiveScanFn, fine_state_scope,
                                       grouped_scan_fn, selective_scan_fn)


# ============================================================================ Mamba text tower
def _dt_bias_init(d_inner, dt_min=0.001, dt_max=0.1, dt_init_floor=1e-4):
    """softplus^-1 of dt ~ logU[dt_min, dt_max] (model.py:459-468 semantics)."""
    dt = torch.exp(torch.rand(d_inner) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
    dt = dt.clamp(min=dt_init_floor)
    return dt + torch.log(-torch.expm1(-dt))


def mixer_scan(x, delta, A, Bm, Cm, D, z, delta_bias, dz_slab, du_handoff=None, dbc_slab=None):
    """The mixer's scan call (selective_scan_fn semantics, softplus on) with dz written into
    the in_proj gradient slab, dB / dC into the x_proj gradient slab and du handed to x_proj's
    backward (ops.GradHandoff)."""
    return SelectiveScanFn.apply(x, delta, A, Bm, Cm, D, z, delta_bias, True, False, dz_slab, du_handoff, dbc_slab)


class MambaMixer(nn.Module):
    """One Mamba mixer: in_proj -> causal conv1d+SiLU -> x_proj/dt_proj -> selective scan (z-gated) -> out_proj.

    Channel-major activations: every projection is ONE 2-D GEMM on the
    (channels, batch*seqlen) matrix, and the conv / scan see it as a
    (batch, channels, seqlen) view with strides (seqlen, batch*seqlen, 1) --
    unit stride along the sequence, no transposes or copies between the GEMMs
    (the HIP kernels take batch/channel strides and write outputs and
    gradients in the same layout).
    """

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto"):
        super().__init__()
        self.d_model, self.d_state, self.d_conv = d_model, d_state, d_conv
        self.d_inner = int(expand * d_model)
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.in_proj = nn.Linear(d_model, 2 * self.d_inner, bias=False)
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, d_conv, groups=self.d_inner, padding=d_conv - 1)
        self.x_proj = nn.Linear(self.d_inner, self.dt_rank + 2 * d_state, bias=False)
        self.dt_proj = nn.Linear(self.dt_rank, self.d_inner, bias=True)
        std = self.dt_rank ** -0.5
        nn.init.uniform_(self.dt_proj.weight, -std, std)
        with torch.no_grad():
            self.dt_proj.bias.copy_(_dt_bias_init(self.d_inner))
        A = torch.arange(1, d_state + 1, dtype=torch.float32).repeat(self.d_inner, 1)
        self.A_log = nn.Parameter(torch.log(A))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(self.d_inner))
        self.D._no_weight_decay = True
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=False)
        self.du_handoff = True   # scan du -> x_proj's dX epilogue (ops.GradHandoff)

    def forward(self, hidden, A=None):  # (B, L, d_model) contiguous; A: -exp(A_log) when the tower formed it
        Bsz, L, dm = hidden.shape
        dt_in = hidden.dtype
        di, R, N = self.d_inner, self.dt_rank, self.d_state
        H = hidden.reshape(Bsz * L, dm)
        # projections: weight-left GEMMs with split-K weight gradients (ops.wleft_mm / linear_sk)
        xz = wleft_mm(self.in_proj.weight, H.t())                             # (2*di, B*L)
        # the conv / scan backward kernels write dx / dz into one (2*di, B*L) slab: the split's
        # gradient is that slab, no concatenation (ops.GradSlab)
        slab = GradSlab(2 * di, Bsz * L, xz.dtype, xz.device) if xz.requires_grad else None
        x, z = split_rows(xz, di, slab)
        x = x.view(di, Bsz, L).transpose(0, 1)                                # (B, di, L) channel-major
        z = z.view(di, Bsz, L).transpose(0, 1)
        x = causal_conv1d(x, self.conv1d.weight, self.conv1d.bias, silu=True, dx_slab=slab)
        x_cm = x.transpose(0, 1).reshape(di, Bsz * L)                          # view
        if A is None:
            A = -torch.exp(self.A_log.float())
        dz = (slab, di) if slab is not None else None
        # x's gradient: the scan's du is handed to x_proj's backward, which adds its dX in the
        # GEMM epilogue (ops.GradHandoff) instead of autograd summing the two producers
        hand = GradHandoff() if (self.du_handoff and x.is_cuda and x.requires_grad) else None
        x_dbl = wleft_mm(self.x_proj.weight, x_cm, hand)                   # (R+2N, B*L)
        # dt_proj's backward writes d(dt_raw) and the scan's writes dB / dC straight into one
        # (R+2N, B*L) gradient slab: no transpose copies of dB / dC, no concatenation
        pslab = GradSlab(R + 2 * N, Bsz * L, x_dbl.dtype, x_dbl.device) if x_dbl.requires_grad else None
        dt_raw, Bm, Cm = split_rows_n(x_dbl, (R, N, N), pslab)
        delta = wleft_mm(self.dt_proj.weight, dt_raw, out_slab=(pslab, 0) if pslab is not None else None)
        delta = delta.view(di, Bsz, L).transpose(0, 1)
        Bm = Bm.view(N, Bsz, L).transpose(0, 1)                           # (B, N, L)
        Cm = Cm.view(N, Bsz, L).transpose(0, 1)
        y = mixer_scan(x, delta, A, Bm, Cm, self.D.float(), z, self.dt_proj.bias.float(), dz, hand,
                       (pslab, R, R + N) if pslab is not None else None)
        y2 = y.transpose(0, 1).reshape(di, Bsz * L)                            # view: y keeps x's layout
        out = linear_sk(y2.t(), self.out_proj.weight)                          # (B*L, d_model)
        return out.view(Bsz, L, dm)


class MambaLayer(nn.Module):
    """Pre-norm block: (hidden, residual) -> add+RMSNorm -> mixer (mamba_ssm Block semantics)."""

    def __init__(self, d_model, d_state=16, eps=1e-5):
        super().__init__()
        self.mixer = MambaMixer(d_model, d_state=d_state)
        self.norm_weight = nn.Parameter(torch.ones(d_model))
        self.eps = eps

    def forward(self, hidden, residual, A=None):
        normed, residual = add_rmsnorm(hidden, residual, self.norm_weight, self.eps)
        return self.mixer(normed, A), residual


class MambaTextEncoder(nn.Module):
    """Mamba LM text tower for CLIP: tokens (B, T) int64 -> (B, output_dim).

    pad_id=None (the default): pools the hidden state at the last position T - 1, where the
    synthetic tokens put end-of-text; right only for captions as long as the context.
    pad_id=<int>: pools at each caption's last token that is not pad_id, through the last-token
    add + RMSNorm kernel (ops.last_token_rmsnorm) -- transformers.MambaModel's hidden row len - 1.
    The tower is causal, so the layers need no masking: padding behind a caption never reaches its
    rows.  Right padding only (left padding would put pad tokens in front of the caption, inside
    its history); pad ids inside a caption are allowed, the search is for the LAST non-pad token; a
    row of nothing but pad pools position 0.  load_hf_mamba_state_dict fills the tower from an
    HF-named state dict; tests/golden/mamba_hf_tiny*.safetensors pin it to transformers.

    The sequence is padded to a multiple of 8 positions after the real tokens (causal: padding never
    reaches earlier positions) so every activation row is 16-B aligned.
    """

    def __init__(self, vocab_size=50280, context_length=77, d_model=768, n_layer=24, d_state=16,
                 output_dim=512, pad_id=None):
        super().__init__()
        self.vocab_size, self.context_length, self.d_model = vocab_size, context_length, d_model
        self.output_dim = output_dim
        self.pad_id = None if pad_id is None else int(pad_id)
        self.embedding = nn.Embedding(vocab_size, d_model)
        nn.init.normal_(self.embedding.weight, std=0.02)
        self.layers = nn.ModuleList([MambaLayer(d_model, d_state) for _ in range(n_layer)])
        self.norm_f = nn.Parameter(torch.ones(d_model))
        self.proj = nn.Linear(d_model, output_dim, bias=False)
        nn.init.normal_(self.proj.weight, std=d_model ** -0.5)

    def lock_units(self):
        """(embeddings, [layer, ...], final norm) as lists of (name, parameter) for lock_text_tower."""
        return ([("embedding.weight", self.embedding.weight)],
                [list(l.named_parameters(prefix=f"layers.{i}")) for i, l in enumerate(self.layers)],
                [("norm_f", self.norm_f)])

    def forward_hidden(self, tokens):
        """The pooled row after the final norm, (B, d_model): what `proj` projects."""
        Bsz, T = tokens.shape
        Lp = (T + 7) // 8 * 8
        given = tokens
        if Lp != T:
            tokens = F.pad(tokens, (0, Lp - T))
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
        hidden = self.embedding(tokens).to(dt)
        residual = None
        # every mixer's A = -exp(A_log) in one launch (ops.NegExpManyFn)
        As = (neg_exp_many([l.mixer.A_log for l in self.layers]) if hidden.is_cuda
              else [None] * len(self.layers))
        ckpt = self.grad_checkpointing and torch.is_grad_enabled()
        n = len(self.layers)

        def run(layer, hidden, residual, A):
            # each layer's scan may keep fine saved states within budget / n_layer (a static choice: the
            # same in the checkpoint recompute, which runs on the autograd thread)
            with fine_state_scope(n):
                return layer(hidden, residual, A)
        for layer, A in zip(self.layers, As):
            if ckpt:   # recompute the layer in backward instead of keeping its activations
                hidden, residual = torch.utils.checkpoint.checkpoint(run, layer, hidden, residual, A, use_reentrant=False)
            else:
                hidden, residual = run(layer, hidden, residual, A)
        if self.pad_id is not None:
            # the final norm on the pooled rows only, at each caption's last non-pad token of the T given
            return last_token_rmsnorm(given, self.pad_id, hidden, residual, self.norm_f)[0]
        normed, _ = add_rmsnorm(hidden, residual, self.norm_f)
        return normed[:, T - 1]                                     # EOT position

    def forward(self, tokens):
        return self.proj(self.forward_hidden(tokens))

    def load_hf_mamba_state_dict(self, sd):
        return load_hf_mamba_state_dict(self, sd)

    grad_checkpointing = False

    def set_grad_checkpointing(self, enable=True):
        """Activation checkpointing per Mamba layer (torch.utils.checkpoint, non-reentrant): the reference's
        ClipModel.set_grad_checkpointing (model.py:1099-1102) turns it on in open_clip's towers."""
        self.grad_checkpointing = bool(enable)


_HF_MAMBA_MIXER = ("A_log", "D", "conv1d.weight", "conv1d.bias", "in_proj.weight", "x_proj.weight", "dt_proj.weight",
                   "dt_proj.bias", "out_proj.weight")


def load_hf_mamba_state_dict(model, sd):
    """Copy a transformers MambaModel / MambaForCausalLM state dict (HF names, with or without a leading
    "backbone.") into a MambaTextEncoder: embeddings.weight -> embedding.weight, layers.i.norm.weight ->
    layers.i.norm_weight, layers.i.mixer.* under the same names, norm_f.weight -> norm_f.  Strict: a
    missing or an unexpected key raises KeyError, a shape mismatch ValueError naming the tensor; only
    lm_head.weight is ignored.  The projection after the pooled row is not part of the HF model and
    keeps its values."""
    sd = {(k[9:] if k.startswith("backbone.") else k): v for k, v in sd.items()}
    sd = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    want = {"embeddings.weight": model.embedding.weight, "norm_f.weight": model.norm_f}
    for i, layer in enumerate(model.layers):
        want[f"layers.{i}.norm.weight"] = layer.norm_weight
        for name in _HF_MAMBA_MIXER:
            want[f"layers.{i}.mixer.{name}"] = layer.mixer.get_parameter(name)
    missing, unexpected = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or unexpected:
        raise KeyError(f"load_hf_mamba_state_dict: missing {missing}, unexpected {unexpected}")
    for name, param in want.items():
        if sd[name].shape != param.shape:
            raise ValueError(f"load_hf_mamba_state_dict: {name} is {tuple(sd[name].shape)}, "
                             f"the tower has {tuple(param.shape)}")
    with torch.no_grad():
        for name, param in want.items():
            param.copy_(sd[name])
    return model


def _run_blocks(blocks, m, h, ckpt):
    for blk in blocks:
        m, h = torch.utils.checkpoint.checkpoint(blk, m, h, use_reentrant=False) if ckpt else blk(m, h)
    return m, h


# ============================================================================ ViT-B/16 visual tower
class PatchEmbed(nn.Module):
    """Conv2d(k = s = patch) as im2col (HIP) + one GEMM."""

    def __init__(self, img_size=224, patch=16, in_chans=3, dim=768, bias=True):
        super().__init__()
        self.patch, self.grid = patch, img_size // patch
        self.proj = nn.Conv2d(in_chans, dim, patch, patch, bias=bias)

    def forward(self, x, keep=None):
        """(B, C, H, W) float, or (B, H, W, C) uint8 raw images -> (B, H/P * W/P, dim); with keep
        ((B, n_keep) int32 patch indices, patch dropout) only those patches: (B, n_keep, dim)."""
        Bsz = x.shape[0]
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else (
            torch.float32 if x.dtype == torch.uint8 else x.dtype)
        # the input cast (and for raw images ToTensor + Normalize) happens inside the patch kernel
        if keep is None:
            cols = patch_im2col(x, self.patch, dt)
        elif x.is_cuda:   # the gather kernel reads the kept patches only: the GEMM below shrinks with them
            cols = patch_im2col(x, self.patch, dt, keep=keep)
        else:             # off the GPU: every patch's row, the kept ones picked with torch
            cols = patch_im2col(x, self.patch, dt)
            idx = keep.long()[:, :, None].expand(-1, -1, cols.shape[1])
            cols = cols.view(Bsz, -1, cols.shape[1]).gather(1, idx).reshape(-1, cols.shape[1])
        w = self.proj.weight.reshape(self.proj.weight.shape[0], -1)
        if cols.is_cuda:   # split-K weight gradient (ops.wgrad): 188 -> 85 us at C2
            out = linear_sk(cols, w, self.proj.bias)
        else:
            out = F.linear(cols, w.to(dt), self.proj.bias.to(dt) if self.proj.bias is not None else None)
        return out.reshape(Bsz, -1, w.shape[0])


def _gpu_sdpa_backends():
    """Backend priority for the towers' attention on MI355X: the memory-efficient
    kernel first (measured at C2, 197 tokens x 12 heads x 64: attention block
    fwd+bwd 2.36 ms vs 2.51 ms for the default choice), then flash, then math."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    order = [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION, SDPBackend.MATH]
    try:
        return sdpa_kernel(order, set_priority=True)
    except TypeError:  # older torch: no priority argument
        return sdpa_kernel(order)


class Attention(nn.Module):
    """causal=True: query i attends to the keys j <= i (the CLIP text transformer): the fused path runs
    mc_attn_causal_fwd / _bwd, the fallback SDPA with is_causal=True; not combined with a padding mask."""

    def __init__(self, dim, heads, causal=False):
        super().__init__()
        self.heads = heads
        self.causal = bool(causal)
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.fused_attention = True   # mc_attn_fwd/bwd where supported (bf16/f16, head_dim 64, N <= 256)

    last_path = None   # "fused" / "sdpa": what the latest forward ran (tests assert the kernel under test)

    def forward(self, x, key_mask=None, valid=None):
        """valid: (B, N) bool key-padding mask (HF attention_mask[:, None, None, :]), None = attend to
        every key; key_mask: its pack_key_mask words, packed once per tower forward (packed here if
        the fused path needs them and only `valid` came)."""
        Bsz, N, C = x.shape
        if valid is None and key_mask is not None:
            raise ValueError("Attention: key_mask needs the boolean `valid` it was packed from")
        if self.causal and valid is not None:
            raise ValueError("Attention: causal attention takes no key-padding mask")
        if self.fused_attention and x.is_cuda and attn_supported(N, C // self.heads, _compute_dtype(x)):
            # packed qkv projection -> fused attention kernel (ops.PackedAttentionFn: the whole
            # sequence of a head in LDS) -> output projection; o is already (B, N, C) and the
            # backward writes dq / dk / dv into the packed projection gradient
            self.last_path = "fused"
            qkv = linear_sk(x, self.qkv.weight, self.qkv.bias)
            if valid is not None and key_mask is None:
                key_mask = pack_key_mask(valid)
            if self.causal:
                return linear_sk(packed_attention(qkv, self.heads, causal=True), self.proj.weight, self.proj.bias)
            return linear_sk(packed_attention(qkv, self.heads, key_mask), self.proj.weight, self.proj.bias)
        self.last_path = "sdpa"
        # unbind (not index) the q/k/v slices: its backward stacks the three
        # gradients in one write instead of zero-filling and accumulating a
        # (3, B, H, N, D) buffer three times and copying it contiguous again
        # q, k, v: (B, H, N, D) views of the packed qkv output; the backward packs dq / dk / dv and
        # the qkv bias gradient in one pass (ops.QKVProjFn)
        q, k, v = qkv_proj(x, self.qkv.weight, self.qkv.bias, self.heads)
        am = valid[:, None, None, :] if valid is not None else None   # True = attend
        if x.is_cuda:
            with _gpu_sdpa_backends():
                o = F.scaled_dot_product_attention(q, k, v, attn_mask=am, is_causal=self.causal)
        else:
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=am, is_causal=self.causal)
        return linear_sk(o.transpose(1, 2).reshape(Bsz, N, C), self.proj.weight, self.proj.bias)


class ViTBlock(nn.Module):
    """Pre-LN transformer block (timm Block parameters: norm1, attn, norm2, fc1/fc2 MLP).

    forward(m, h) takes the previous block's branch output m and residual
    stream h (x = h + m) and returns its own (m', h'): each residual add is
    fused into the following LayerNorm (mc_add_layernorm), the way the Mamba
    blocks fuse add + RMSNorm.  Same math as x = x + attn(norm1(x));
    x = x + mlp(norm2(x)).

    causal: causal self-attention (the CLIP text transformer).  act: "gelu", the exact GELU inside the
    fused MLP (ops.mlp), or "quick_gelu", x * sigmoid(1.702 x) of the OpenAI CLIP weights, which runs
    unfused: fc1 GEMM, torch elementwise, fc2 GEMM (ops.mlp's epilogue is exact-GELU only).
    """

    def __init__(self, dim, heads, mlp_ratio=4.0, eps=1e-6, causal=False, act="gelu"):
        super().__init__()
        if act not in ("gelu", "quick_gelu"):
            raise ValueError(f"ViTBlock: act must be 'gelu' or 'quick_gelu', got {act!r}")
        self.act = act
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, heads, causal=causal)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.fc1 = nn.Linear(dim, int(dim * mlp_ratio))
        self.fc2 = nn.Linear(int(dim * mlp_ratio), dim)

    def forward(self, m, h=None):
        y, h = add_layernorm(m, h, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        a = self.attn(y)
        y, h = add_layernorm(a, h, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        if self.act == "quick_gelu":
            u = linear_sk(y, self.fc1.weight, self.fc1.bias)
            return linear_sk(u * torch.sigmoid(1.702 * u), self.fc2.weight, self.fc2.bias), h
        return mlp(y, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias), h


class VisionTransformer(nn.Module):
    """ViT-B/16 image tower: (B, 3, 224, 224) -> (B, output_dim).

    patch_dropout = p (FLIP; open_clip's PatchDropout with exclude_first_token=True, the reference's
    --force-patch-dropout): while the module is training and 0 < p < 1, every image keeps a uniformly
    random subset of n_keep = max(1, int(n * (1 - p))) of its n patches plus the class token, each kept
    patch with the position row of its original place, and the blocks run on n_keep + 1 tokens.  The
    kept patches stay in ascending patch order (memory order) where open_clip leaves them in topk
    order: behind the position add the tower is permutation-equivariant over the patch tokens and it
    pools the class row, so the features do not depend on that order.  In eval() or with p == 0 the
    forward runs the ops it runs without the option.  The indices come from torch's generator of the
    input's device (ops.patch_keep_indices: torch.manual_seed governs them, no host sync);
    `last_keep` holds those of the latest dropped forward, None after a full one.

    The defaults are the timm shape.  pre_norm=True, eps=1e-5, patch_bias=False (and act="quick_gelu"
    for the OpenAI weights) give the CLIP vision tower of transformers / open_clip: `ln_pre` normalises
    every token row right after the position add (per token, so patch dropout commutes with it);
    load_hf_clip_state_dict fills it, tests/golden/clip_hf_tiny_vision*.safetensors pin it to
    transformers.CLIPVisionModelWithProjection."""

    last_keep = None

    def __init__(self, img_size=224, patch=16, width=768, layers=12, heads=12, output_dim=512, patch_dropout=0.0,
                 pre_norm=False, eps=1e-6, patch_bias=True, act="gelu"):
        super().__init__()
        if not 0.0 <= patch_dropout < 1.0:
            raise ValueError(f"VisionTransformer: patch_dropout must be in [0, 1), got {patch_dropout}")
        self.patch_dropout = float(patch_dropout)
        self.output_dim = output_dim
        self.patch_embed = PatchEmbed(img_size, patch, 3, width, bias=patch_bias)
        n = (img_size // patch) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, width))
        self.pos_embed = nn.Parameter(torch.randn(1, n + 1, width) * 0.02)
        if pre_norm:
            self.ln_pre = nn.LayerNorm(width, eps=eps)
        self.blocks = nn.ModuleList([ViTBlock(width, heads, eps=eps, act=act) for _ in range(layers)])
        self.norm = nn.LayerNorm(width, eps=eps)
        self.head = nn.Linear(width, output_dim, bias=False)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def patch_dropout_active(self):
        return self.training and 0.0 < self.patch_dropout < 1.0

    def _blocks_out(self, x, keep=None):
        """(m, h) behind the last block: the hidden state is m + h."""
        if self.training and (keep is not None or self.patch_dropout_active()):
            # the selection sits in front of the blocks: gradient checkpointing recomputes blocks only
            n = self.pos_embed.shape[1] - 1
            if keep is None:
                keep, slot = patch_keep_indices(x.shape[0], n, max(1, int(n * (1.0 - self.patch_dropout))), x.device)
            else:
                keep = keep.to(device=x.device, dtype=torch.int32)
                slot = keep_slots(keep, n)
            self.last_keep = keep
            m, h = token_embed_gather(self.cls_token, self.patch_embed(x, keep), self.pos_embed, keep, slot), None
        else:
            self.last_keep = None
            x = self.patch_embed(x)
            # cat([cls, x]) + pos with a deterministic backward (ops.TokenEmbedFn)
            m, h = token_embed(self.cls_token, x, self.pos_embed), None
        if hasattr(self, "ln_pre"):
            m = add_layernorm(m, None, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps)[0]
        return _run_blocks(self.blocks, m, h, self.grad_checkpointing and torch.is_grad_enabled())

    def forward_hidden(self, x, keep=None):
        """The token rows behind the last block, before the final norm (B, tokens, width):
        transformers' CLIPVisionModel last_hidden_state."""
        m, h = self._blocks_out(x, keep)
        return m + h

    def forward(self, x, keep=None):
        """keep ((B, n_keep) distinct patch indices per image) replaces the random draw; it is there for
        tests and is honoured in training mode only."""
        m, h = self._blocks_out(x, keep)
        # final norm on the pooled (cls) rows only: same values as norm(x)[:, 0]
        y, _ = add_layernorm(m[:, 0], h[:, 0], self.norm.weight, self.norm.bias, self.norm.eps)
        return self.head(y)

    def lock(self, unlocked_groups=0, freeze_bn_stats=False):
        for p in self.parameters():
            p.requires_grad = False

    grad_checkpointing = False

    def set_grad_checkpointing(self, enable=True):
        """Activation checkpointing per transformer block (timm / open_clip semantics)."""
        self.grad_checkpointing = bool(enable)


# ============================================================================ BERT text tower (BiomedCLIP shape)
class BertTextEncoder(nn.Module):
    """PubMedBERT-base-shaped encoder (12 x 768, ctx 256), CLS pooling + MLP projection."""

    def __init__(self, vocab_size=30522, context_length=256, width=768, layers=12, heads=12, output_dim=512):
        super().__init__()
        self.vocab_size, self.context_length, self.output_dim = vocab_size, context_length, output_dim
        self.tok = nn.Embedding(vocab_size, width)
        self.pos = nn.Parameter(torch.randn(1, context_length, width) * 0.02)
        self.ln = nn.LayerNorm(width, eps=1e-12)
        self.blocks = nn.ModuleList([ViTBlock(width, heads) for _ in range(layers)])
        self.proj = nn.Sequential(nn.Linear(width, (width + output_dim) // 2, bias=False), nn.GELU(),
                                  nn.Linear((width + output_dim) // 2, output_dim, bias=False))

    def lock_units(self):
        """(embeddings incl. their LayerNorm, [block, ...], nothing after) for lock_text_tower."""
        return ([("tok.weight", self.tok.weight), ("pos", self.pos), ("ln.weight", self.ln.weight),
                 ("ln.bias", self.ln.bias)],
                [list(b.named_parameters(prefix=f"blocks.{i}")) for i, b in enumerate(self.blocks)], [])

    grad_checkpointing = False

    def set_grad_checkpointing(self, enable=True):
        """Activation checkpointing per encoder layer (HF gradient_checkpointing semantics)."""
        self.grad_checkpointing = bool(enable)

    def forward(self, tokens):
        m, h = self.ln(add_pos(self.tok(tokens), self.pos)), None
        m, h = _run_blocks(self.blocks, m, h, self.grad_checkpointing and torch.is_grad_enabled())
        return self.proj(m[:, 0] + h[:, 0])


# ============================================================================ HF-faithful BERT text tower
class PostLNBlock(nn.Module):
    """One transformers.BertLayer: post-LN, h1 = LN(x + attn(x, mask)); h2 = LN(h1 + fc2(gelu(fc1(h1))))
    with eps 1e-12 and the exact (erf) GELU of hidden_act="gelu".  Each residual add is the fused
    add + LayerNorm (mc_add_layernorm) whose normalised output is the next input."""

    def __init__(self, dim, heads, mlp_dim, eps=1e-12):
        super().__init__()
        self.attn = Attention(dim, heads)
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.fc1 = nn.Linear(dim, mlp_dim)
        self.fc2 = nn.Linear(mlp_dim, dim)
        self.norm2 = nn.LayerNorm(dim, eps=eps)

    def forward(self, x, key_mask=None, valid=None):
        # the hidden state comes first: add_layernorm works in its first operand's dtype, so under
        # autocast the LayerNorm outputs stay fp32 as they do in HF (the projections cast their input)
        h1 = add_layernorm(x, self.attn(x, key_mask, valid), self.norm1.weight, self.norm1.bias, self.norm1.eps)[0]
        m = mlp(h1, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        return add_layernorm(h1, m, self.norm2.weight, self.norm2.bias, self.norm2.eps)[0]


class HFBertTextEncoder(nn.Module):
    """transformers.BertModel (add_pooling_layer=False) as BiomedCLIP's text tower: word + position +
    token-type-0 embeddings -> LayerNorm (eps 1e-12) -> post-LN layers that attend only to
    tokens != pad_token_id -> the CLS row of the last hidden state -> the bias-free Linear-GELU-Linear
    projection of BertTextEncoder.  load_hf_bert_state_dict fills it from an HF-named state dict;
    tests/golden/bert_hf_tiny.safetensors pins it to transformers.  Padded query rows are computed (they
    are rows of last_hidden_state); the fused attention skips key tiles that are all padding."""

    def __init__(self, vocab_size=30522, context_length=256, max_positions=512, type_vocab_size=2, width=768,
                 layers=12, heads=12, output_dim=512, pad_token_id=0, mlp_dim=None):
        super().__init__()
        self.vocab_size, self.context_length, self.output_dim = vocab_size, context_length, output_dim
        self.pad_token_id = pad_token_id
        self.tok = nn.Embedding(vocab_size, width)
        self.pos = nn.Embedding(max_positions, width)
        self.tok_type = nn.Embedding(type_vocab_size, width)
        self.ln = nn.LayerNorm(width, eps=1e-12)
        self.blocks = nn.ModuleList([PostLNBlock(width, heads, mlp_dim or 4 * width) for _ in range(layers)])
        self.proj = nn.Sequential(nn.Linear(width, (width + output_dim) // 2, bias=False), nn.GELU(),
                                  nn.Linear((width + output_dim) // 2, output_dim, bias=False))
        for m in self.modules():   # HF BertPreTrainedModel._init_weights (initializer_range 0.02)
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=0.02)
                if getattr(m, "bias", None) is not None:
                    nn.init.zeros_(m.bias)

    def lock_units(self):
        """(embeddings incl. their LayerNorm, [layer, ...], nothing after) for lock_text_tower."""
        return ([("tok.weight", self.tok.weight), ("pos.weight", self.pos.weight), ("tok_type.weight", self.tok_type.weight),
                 ("ln.weight", self.ln.weight), ("ln.bias", self.ln.bias)],
                [list(b.named_parameters(prefix=f"blocks.{i}")) for i, b in enumerate(self.blocks)], [])

    grad_checkpointing = False

    def set_grad_checkpointing(self, enable=True):
        """Activation checkpointing per encoder layer (HF gradient_checkpointing semantics)."""
        self.grad_checkpointing = bool(enable)

    def forward_hidden(self, tokens):
        """last_hidden_state of the HF model, (B, N, width)."""
        N = tokens.shape[1]
        if N > self.pos.num_embeddings:
            raise ValueError(f"{N} tokens, the position table has {self.pos.num_embeddings}")
        valid = tokens != self.pad_token_id
        # position rows 0..N-1 plus token-type row 0, one (1, N, width) table added to every caption
        x = self.ln(add_pos(self.tok(tokens), (self.pos.weight[:N] + self.tok_type.weight[0]).unsqueeze(0)))
        # the key bits of the fused kernel, packed once for all layers (no sync); fp32 / CPU: SDPA takes `valid`
        a0 = self.blocks[0].attn
        fused = a0.fused_attention and x.is_cuda and attn_supported(N, x.shape[-1] // a0.heads, _compute_dtype(x))
        key_mask = pack_key_mask(valid) if fused else None
        ckpt = self.grad_checkpointing and torch.is_grad_enabled()
        for blk in self.blocks:
            if ckpt:
                x = torch.utils.checkpoint.checkpoint(blk, x, key_mask, valid, use_reentrant=False)
            else:
                x = blk(x, key_mask, valid)
        return x

    def forward(self, tokens):
        return self.proj(self.forward_hidden(tokens)[:, 0])

    def load_hf_bert_state_dict(self, sd):
        return load_hf_bert_state_dict(self, sd)


_HF_BERT_IGNORED = ("pooler.", "embeddings.position_ids")
_HF_BERT_LAYER = {   # HF BertLayer name -> PostLNBlock name (query / key / value go into the packed qkv)
    "attention.output.dense": "attn.proj", "attention.output.LayerNorm": "norm1",
    "intermediate.dense": "fc1", "output.dense": "fc2", "output.LayerNorm": "norm2",
}


def load_hf_bert_state_dict(model, sd):
    """Copy a transformers.BertModel state dict (HF names, with or without a leading "bert.") into an
    HFBertTextEncoder.  Strict: a missing or an unexpected key raises KeyError; only pooler.* and
    embeddings.position_ids are ignored (the tower pools the CLS row itself).  The projection after the
    CLS row is not part of BertModel and keeps its values."""
    sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in sd.items()}
    sd = {k: v for k, v in sd.items() if not k.startswith(_HF_BERT_IGNORED)}
    want = {"embeddings.word_embeddings.weight": model.tok.weight,
            "embeddings.position_embeddings.weight": model.pos.weight,
            "embeddings.token_type_embeddings.weight": model.tok_type.weight,
            "embeddings.LayerNorm.weight": model.ln.weight, "embeddings.LayerNorm.bias": model.ln.bias}
    packed = {}
    for i, blk in enumerate(model.blocks):
        pre = f"encoder.layer.{i}."
        for hf, ours in _HF_BERT_LAYER.items():
            mod = blk.get_submodule(ours)
            want[f"{pre}{hf}.weight"], want[f"{pre}{hf}.bias"] = mod.weight, mod.bias
        for wb in ("weight", "bias"):
            names = [f"{pre}attention.self.{n}.{wb}" for n in ("query", "key", "value")]
            packed[tuple(names)] = getattr(blk.attn.qkv, wb)
    expected = set(want) | {n for names in packed for n in names}
    missing, unexpected = sorted(expected - set(sd)), sorted(set(sd) - expected)
    if missing or unexpected:
        raise KeyError(f"load_hf_bert_state_dict: missing {missing}, unexpected {unexpected}")
    with torch.no_grad():
        for name, param in want.items():
            if sd[name].shape != param.shape:
                raise ValueError(f"load_hf_bert_state_dict: {name} is {tuple(sd[name].shape)}, "
                                 f"the tower has {tuple(param.shape)}")
            param.copy_(sd[name])
        for names, param in packed.items():
            cat = torch.cat([sd[n] for n in names], 0)
            if cat.shape != param.shape:
                raise ValueError(f"load_hf_bert_state_dict: {names[0]} (+ key, value) pack to {tuple(cat.shape)}, "
                                 f"the tower has {tuple(param.shape)}")
            param.copy_(cat)
    return model


# ============================================================================ CLIP text transformer
class _PoolRowsFn(torch.autograd.Function):
    """x[b, idx[b]] for x (B, N, C) and idx (B,) int64 on x's device.  Backward: zeros with row idx[b]
    of batch b set to the gradient -- one row per batch, so the write is an index_copy with distinct
    targets (deterministic; the scatter_add of gather's backward is not).  No host sync."""

    @staticmethod
    def forward(ctx, x, idx):
        Bsz, N, C = x.shape
        flat = torch.arange(Bsz, device=x.device) * N + idx
        ctx.save_for_backward(flat)
        ctx.shape = (Bsz, N, C)
        return x.reshape(Bsz * N, C).index_select(0, flat)

    @staticmethod
    def backward(ctx, g):
        (flat,) = ctx.saved_tensors
        Bsz, N, C = ctx.shape
        dx = g.new_zeros(Bsz * N, C)
        dx.index_copy_(0, flat, g.contiguous())
        return dx.view(Bsz, N, C), None


class ClipTextEncoder(nn.Module):
    """The CLIP text transformer (openai/clip-vit-base-patch16 and the open_clip ViT-B/16 checkpoints):
    tokens (B, T <= context_length) int64 -> (B, output_dim).  Token + position embeddings (no embedding
    LayerNorm) -> causal pre-LN blocks (ViTBlock(causal=True): the fused causal attention kernels under
    bf16 / f16 autocast) -> the end-of-text row -> final LayerNorm -> bias-free text_projection.  The
    final LayerNorm runs on the pooled rows only: the same values as ln_final(x)[arange, idx].

    Pooling index: eot_token_id=None -> tokens.argmax(-1) (open_clip; the OpenAI tokenizer gives
    end-of-text the largest id); an id -> the first position holding it (transformers, eos_token_id != 2).
    The tower is causal, so whatever follows the end-of-text token never reaches the pooled row: no
    padding mask.  act="quick_gelu" (the OpenAI weights; "gelu" for the LAION ones) runs the MLP
    unfused (ViTBlock).  load_hf_clip_state_dict fills the tower; tests/golden/clip_hf_tiny_text*.safetensors
    pin it to transformers.CLIPTextModelWithProjection."""

    def __init__(self, vocab_size=49408, context_length=77, width=512, layers=12, heads=8, output_dim=512,
                 eps=1e-5, act="quick_gelu", eot_token_id=None, mlp_dim=None):
        super().__init__()
        self.vocab_size, self.context_length, self.output_dim = vocab_size, context_length, output_dim
        self.eot_token_id = None if eot_token_id is None else int(eot_token_id)
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(1, context_length, width))
        self.blocks = nn.ModuleList([ViTBlock(width, heads, (mlp_dim or 4 * width) / width, eps=eps, causal=True, act=act)
                                     for _ in range(layers)])
        self.ln_final = nn.LayerNorm(width, eps=eps)
        self.text_projection = nn.Linear(width, output_dim, bias=False)
        # open_clip's CLIP text init
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std, attn_std, fc_std = (width ** -0.5) * ((2 * layers) ** -0.5), width ** -0.5, (2 * width) ** -0.5
        for blk in self.blocks:
            nn.init.normal_(blk.attn.qkv.weight, std=attn_std)
            nn.init.normal_(blk.attn.proj.weight, std=proj_std)
            nn.init.normal_(blk.fc1.weight, std=fc_std)
            nn.init.normal_(blk.fc2.weight, std=proj_std)
            for b in (blk.attn.qkv.bias, blk.attn.proj.bias, blk.fc1.bias, blk.fc2.bias):
                nn.init.zeros_(b)
        nn.init.normal_(self.text_projection.weight, std=width ** -0.5)

    def lock_units(self):
        """(embeddings, [block, ...], final norm) as lists of (name, parameter) for lock_text_tower."""
        return ([("token_embedding.weight", self.token_embedding.weight),
                 ("positional_embedding", self.positional_embedding)],
                [list(b.named_parameters(prefix=f"blocks.{i}")) for i, b in enumerate(self.blocks)],
                [("ln_final.weight", self.ln_final.weight), ("ln_final.bias", self.ln_final.bias)])

    grad_checkpointing = False

    def set_grad_checkpointing(self, enable=True):
        """Activation checkpointing per transformer block (open_clip semantics)."""
        self.grad_checkpointing = bool(enable)

    def pool_index(self, tokens):
        """(B,) int64 end-of-text positions, computed on the tokens' device (no host sync)."""
        if self.eot_token_id is None:
            return tokens.argmax(-1)
        return (tokens == self.eot_token_id).int().argmax(-1)   # the first match (0 when there is none)

    def _blocks_out(self, tokens):
        T = tokens.shape[1]
        if T > self.context_length:
            raise ValueError(f"{T} tokens, the position table has {self.context_length}")
        m, h = add_pos(self.token_embedding(tokens), self.positional_embedding), None
        return _run_blocks(self.blocks, m, h, self.grad_checkpointing and torch.is_grad_enabled())

    def forward_hidden(self, tokens):
        """transformers' last_hidden_state: every row after the final LayerNorm, (B, T, width)."""
        m, h = self._blocks_out(tokens)
        return add_layernorm(m, h, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)[0]

    def forward(self, tokens):
        m, h = self._blocks_out(tokens)
        idx = self.pool_index(tokens)
        y, _ = add_layernorm(_PoolRowsFn.apply(m, idx), _PoolRowsFn.apply(h, idx), self.ln_final.weight,
                             self.ln_final.bias, self.ln_final.eps)
        return self.text_projection(y)


_HF_CLIP_LAYER = {   # HF CLIPEncoderLayer name -> ViTBlock name (q_proj | k_proj | v_proj go into the packed qkv)
    "self_attn.out_proj": "attn.proj", "layer_norm1": "norm1", "layer_norm2": "norm2", "mlp.fc1": "fc1", "mlp.fc2": "fc2",
}


def _hf_clip_blocks(blocks, pre, want, packed):
    for i, blk in enumerate(blocks):
        p = f"{pre}encoder.layers.{i}."
        for hf, ours in _HF_CLIP_LAYER.items():
            mod = blk.get_submodule(ours)
            want[f"{p}{hf}.weight"], want[f"{p}{hf}.bias"] = (mod.weight, None), (mod.bias, None)
        for wb in ("weight", "bias"):
            packed[tuple(f"{p}self_attn.{n}.{wb}" for n in ("q_proj", "k_proj", "v_proj"))] = getattr(blk.attn.qkv, wb)


def load_hf_clip_state_dict(clip_model, sd):
    """Copy a transformers.CLIPModel state dict (text_model.*, vision_model.*, text_projection.weight,
    visual_projection.weight, logit_scale) into a ClipModel of a pre_norm VisionTransformer and a
    ClipTextEncoder.  q_proj | k_proj | v_proj pack into attn.qkv; class_embedding -> cls_token and
    position_embedding.weight -> pos_embed / positional_embedding (reshaped to our (1, n, width));
    pre_layrnorm (HF's spelling) -> ln_pre, post_layernorm -> norm, visual_projection -> head,
    final_layer_norm -> ln_final.  Strict: a missing or an unexpected key raises KeyError, a shape
    mismatch ValueError naming the tensor; only *.position_ids buffers are ignored."""
    vis, txt = clip_model.visual, clip_model.text
    if not (isinstance(vis, VisionTransformer) and hasattr(vis, "ln_pre") and isinstance(txt, ClipTextEncoder)):
        raise TypeError("load_hf_clip_state_dict: needs a pre_norm VisionTransformer and a ClipTextEncoder")
    sd = {k: v for k, v in sd.items() if not k.endswith(".position_ids")}
    # HF name -> (parameter, shape the HF tensor is viewed as, or None for its own)
    want = {"logit_scale": (clip_model.logit_scale, None),
            "text_projection.weight": (txt.text_projection.weight, None),
            "visual_projection.weight": (vis.head.weight, None),
            "text_model.embeddings.token_embedding.weight": (txt.token_embedding.weight, None),
            "text_model.embeddings.position_embedding.weight": (txt.positional_embedding, "lead1"),
            "text_model.final_layer_norm.weight": (txt.ln_final.weight, None),
            "text_model.final_layer_norm.bias": (txt.ln_final.bias, None),
            "vision_model.embeddings.class_embedding": (vis.cls_token, "lead2"),
            "vision_model.embeddings.patch_embedding.weight": (vis.patch_embed.proj.weight, None),
            "vision_model.embeddings.position_embedding.weight": (vis.pos_embed, "lead1"),
            "vision_model.pre_layrnorm.weight": (vis.ln_pre.weight, None),
            "vision_model.pre_layrnorm.bias": (vis.ln_pre.bias, None),
            "vision_model.post_layernorm.weight": (vis.norm.weight, None),
            "vision_model.post_layernorm.bias": (vis.norm.bias, None)}
    if vis.patch_embed.proj.bias is not None:
        want["vision_model.embeddings.patch_embedding.bias"] = (vis.patch_embed.proj.bias, None)
    packed = {}
    _hf_clip_blocks(txt.blocks, "text_model.", want, packed)
    _hf_clip_blocks(vis.blocks, "vision_model.", want, packed)
    expected = set(want) | {n for names in packed for n in names}
    missing, unexpected = sorted(expected - set(sd)), sorted(set(sd) - expected)
    if missing or unexpected:
        raise KeyError(f"load_hf_clip_state_dict: missing {missing}, unexpected {unexpected}")
    copies = []
    for name, (param, lead) in want.items():
        t = sd[name]
        shape = tuple(t.shape) if lead is None else (1,) * int(lead[4:]) + tuple(t.shape)
        if shape != tuple(param.shape):
            raise ValueError(f"load_hf_clip_state_dict: {name} is {tuple(t.shape)}, the model has {tuple(param.shape)}")
        copies.append((param, t.reshape(shape)))
    for names, param in packed.items():
        parts = [sd[n] for n in names]
        if any(t.shape != parts[0].shape for t in parts) or (3 * parts[0].shape[0],) + tuple(parts[0].shape[1:]) != tuple(param.shape):
            raise ValueError(f"load_hf_clip_state_dict: {names[0]} (+ k_proj, v_proj) are {[tuple(t.shape) for t in parts]}, "
                             f"the packed qkv has {tuple(param.shape)}")
        copies.append((param, torch.cat(parts, 0)))
    with torch.no_grad():
        for param, t in copies:
            param.copy_(t)
    return clip_model


# ============================================================================ CLIP wrapper (model.py:998-1112)
def _is_norm_param(name):
    """Parameters of the modules the reference's lock_text_tower keeps under `freeze_layer_norm`:
    those under a module literally named "LayerNorm" (model.py:1076, 1094-1096), i.e. HF BERT's
    embedding / attention-output / output LayerNorms = our BERT tower's ln / norm1 / norm2.  The
    Mamba LM's RMSNorms (HF names norm / norm_f) match no "LayerNorm" and are frozen with the rest."""
    return any(part in ("ln", "norm1", "norm2") for part in name.split("."))


class ClipModel(nn.Module):
    """ClipModel(model) as the reference (model.py:1001-1009): wraps a CLIP-like model and SHARES its
    visual / text towers and its logit_scale / logit_bias parameters.  ClipModel(visual, text) builds
    one from two towers with fresh logit_scale = log(1/0.07) (and optional logit_bias)."""
    output_dict = True

    def __init__(self, model, text=None, init_logit_scale=math.log(1 / 0.07), init_logit_bias=None):
        super().__init__()
        self.output_dict = True
        if text is None:                      # reference form: a model with .visual / .text / .logit_scale
            self.visual = model.visual
            self.text = model.text
            self.logit_scale = model.logit_scale
            self.logit_bias = getattr(model, "logit_bias", None)
        else:
            self.visual = model
            self.text = text
            self.logit_scale = nn.Parameter(torch.ones([]) * init_logit_scale)
            self.logit_bias = nn.Parameter(torch.ones([]) * init_logit_bias) if init_logit_bias is not None else None
        self.context_length = getattr(self.text, "context_length", None)
        self.vocab_size = getattr(self.text, "vocab_size", None)

    # image and text towers on two HIP streams (ClipModel.forward).  Under a multi-process group only
    # when train.wrap_ddp joined the streams in its comm hook (ddp_streams_joined): DDP launches a
    # gradient bucket's all-reduce behind one stream, and a bucket may hold gradients of both towers.
    concurrent_towers = os.environ.get("MAMBA_CLIP_AMD_CONCURRENT_TOWERS", "1") != "0"
    ddp_streams_joined = False
    last_main_stream = None
    _side_streams = {}

    @property
    def side_priority(self):
        """HIP priority of the text-tower stream (-1 high, 0 normal, 1 low where the device has it):
        high beside the BERT tower (C3 25.3 -> 25.0 ms per step), normal beside the Mamba tower
        (C2 69.9 -> 70.8 ms at high); profiles/r04/stream_priority/.  Beside the CLIP text transformer
        it stays at the default, normal: unmeasured."""
        return -1 if isinstance(self.text, (BertTextEncoder, HFBertTextEncoder)) else 0

    def side_tower_module(self):
        """The tower that runs on the side stream: the text tower, for every text tower (the image
        tower there measured the same on one box).  train.wrap_ddp probes for this method."""
        return self.text

    def side_stream_for(self, device):
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, int(self.side_priority))
        if key not in ClipModel._side_streams:
            ClipModel._side_streams[key] = torch.cuda.Stream(device=device, priority=key[1])
        return ClipModel._side_streams[key]

    def _side_stream(self, image, text):
        # Only when no kernel of either tower waits on another workgroup of its launch: our HIP kernels
        # never do, and the library GEMMs do not when hipBLASLt launches them data-parallel (one
        # workgroup per output tile, GEMM_GRIDS_DATA_PARALLEL).  Its default stream-K
        # grids split tiles over workgroups that wait on each other's partial sums, so two of them on
        # two streams can each hold part of the CUs and wait forever (the round-3 C3 hang); the C2
        # Mamba tower ran such split launches too (tools/sk_probe.sh).
        if not (self.concurrent_towers and GEMM_GRIDS_DATA_PARALLEL and image is not None
                and text is not None and image.is_cuda and torch.is_grad_enabled()):
            return None
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1 and not self.ddp_streams_joined:
            return None
        return self.side_stream_for(image.device)

    def _towers_two_streams(self, image, text, side, main, dt):
        """(image_features, text_features) with the text tower on `side`.  Each tower runs in its own
        weight-cast scope (a no-op outside autocast, dt None) entered on its own stream."""
        text.record_stream(side)
        with torch.cuda.stream(side), weight_cast_scope(self.text, dt):
            text_features = self.encode_text(text, normalize=True)
        with weight_cast_scope(self.visual, dt):
            image_features = self.encode_image(image, normalize=True)
        main.wait_stream(side)
        text_features.record_stream(main)
        return image_features, text_features

    def encode_image(self, image, normalize: bool = False):
        f = self.visual(image)
        return l2_normalize(f) if normalize else f

    def encode_text(self, text, normalize: bool = False):
        f = self.text(text)
        return l2_normalize(f) if normalize else f

    def forward(self, image, text, secondary_text=None):
        # under CUDA autocast: the towers' Linear weights cast to 16 bits in one launch per tower and forward
        # (ops.weight_cast_scope) instead of one cast per weight and use
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
        side = self._side_stream(image, text)
        secondary = None
        if side is None:
            with weight_cast_scope(self, dt):
                image_features = self.encode_image(image, normalize=True) if image is not None else None
                text_features = self.encode_text(text, normalize=True) if text is not None else None
                if secondary_text is not None:
                    secondary = self.encode_text(secondary_text, normalize=True)
        else:
            # the towers are independent until the loss: one of them runs on a second HIP stream (its
            # backward follows it there: autograd runs each backward op on its forward op's stream and joins
            # the streams at the end of backward).  Each tower's weight casts are made on the stream that
            # uses them, so nothing allocated on one stream is read on the other except the inputs (recorded)
            # and the side tower's features (recorded for the loss on the main stream).
            main = torch.cuda.current_stream()
            self.last_main_stream = main                 # train._join_streams_allreduce joins it
            side.wait_stream(main)                       # the inputs, the parameters the optimizer updated
            image_features, text_features = self._towers_two_streams(image, text, side, main, dt)
            if secondary_text is not None:
                with weight_cast_scope(self.text, dt):
                    secondary = self.encode_text(secondary_text, normalize=True)
        if self.output_dict:
            out = {"image_features": image_features, "text_features": text_features,
                   "logit_scale": self.logit_scale.exp()}
            if secondary is not None:
                out["secondary_text_features"] = secondary
            if self.logit_bias is not None:
                out["logit_bias"] = self.logit_bias
            return out
        out = (image_features, text_features, self.logit_scale.exp())
        if secondary is not None:
            out += (secondary,)
        if self.logit_bias is not None:
            out += (self.logit_bias,)
        return out

    def lock_image_tower(self, unlocked_groups=0, freeze_bn_stats=False):
        self.visual.lock(unlocked_groups=unlocked_groups, freeze_bn_stats=freeze_bn_stats)

    def lock_text_tower(self, unlocked_layers: int = 0, freeze_layer_norm: bool = True):
        """model.py:1072-1097: freeze the text transformer -- embeddings, every layer (and the final
        norm) -- or, with unlocked_layers = k, [embeddings, *layers][:-k]; norm parameters follow
        `not freeze_layer_norm`.  The output projection stays trainable (it is not part of the
        HF transformer the reference freezes)."""
        emb, layers, final = self.text.lock_units()
        units = [emb, *layers, final] if not unlocked_layers else [emb, *layers][:-unlocked_layers]
        for unit in units:
            for n, p in unit:
                p.requires_grad = (not freeze_layer_norm) if _is_norm_param(n) else False

    def set_grad_checkpointing(self, enable=True):
        """model.py:1099-1102: both towers recompute their blocks / layers in backward."""
        for t in (self.visual, self.text):
            if hasattr(t, "set_grad_checkpointing"):
                t.set_grad_checkpointing(enable)

    def get_logits(self, image, text, precision=None):
        """(logits_per_image, logits_per_text) = scale * I @ T.T (model.py:1104-1112).

        precision="fp8": the similarity matmul runs on the fp8 MFMA path with
        row-wise e4m3fn quantisation of the normalised features (config 5).
        """
        from .ops import gemm_nt, similarity_fp8
        i = self.encode_image(image, normalize=True)
        t = self.encode_text(text, normalize=True)
        scale = self.logit_scale.exp().float().reshape(())
        if precision == "fp8":
            image_logits = similarity_fp8(i, t, scale)
        else:
            dt = i.dtype if i.dtype == torch.bfloat16 else torch.float32
            image_logits = gemm_nt(i.to(dt), t.to(dt), alpha_dev=scale)
        if self.logit_bias is not None:
            image_logits = image_logits + self.logit_bias
        return image_logits, image_logits.T


# ============================================================================ stage-2 head (model.py:1115-1205)
def unwrap_model(m):
    return m.module if hasattr(m, "module") else m


class ClipClassifier(nn.Module):
    def __init__(self, clip_model, feature_dim=None, num_classes: int = 2, use_visual_only=False,
                 use_text_only=False, use_inner_prod=False):
        super().__init__()
        self.clip_model = unwrap_model(clip_model)
        self.num_classes = num_classes
        for p in self.clip_model.parameters():
            p.requires_grad = False
        if feature_dim is None:
            i_dim = getattr(self.clip_model.visual, "output_dim", None)
            t_dim = getattr(self.clip_model.text, "output_dim", None)
            if i_dim is None or t_dim is None:
                raise ValueError("Could not find image and text feature dimensions in the model")
            feature_dim = i_dim + t_dim
        self.use_visual_only, self.use_text_only, self.use_inner_prod = use_visual_only, use_text_only, use_inner_prod
        out_dim = feature_dim if (use_visual_only or use_text_only or use_inner_prod) else feature_dim // 2
        self.fc = nn.Sequential(nn.Linear(feature_dim, out_dim), nn.ReLU(), nn.Linear(out_dim, num_classes))

    def forward(self, image, text):
        with torch.no_grad():
            out = self.clip_model(image, text)
        i, t = out["image_features"], out["text_features"]
        if self.use_visual_only:
            return self.fc(i.float())
        if self.use_text_only:
            return self.fc(t.float())
        if self.use_inner_prod:
            return self.fc((i * t).float())
        return self.fc(torch.cat((i, t), dim=1).float())

    def get_logits(self, image_features, text_features):
        # the reference's clup_model typo (Appendix A.6) is not reproduced
        logits = image_features * text_features
        if self.clip_model.logit_bias is not None:
            logits = logits + self.clip_model.logit_bias
        return logits

    def classify(self, image, text):
        probabilities = F.softmax(self.forward(image, text), dim=1)
        return torch.argmax(probabilities, dim=1), probabilities


# ============================================================================ MedMamba / VSSM (model.py:174-995)
class PatchEmbed2D(nn.Module):
    """Conv2d k = s = patch (model.py:174-201) as im2col + GEMM, channels-last output."""

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None, **kwargs):
        super().__init__()
        self.patch = patch_size if isinstance(patch_size, int) else patch_size[0]
        self.proj = nn.Conv2d(in_chans, embed_dim, self.patch, self.patch)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):  # (B, C, H, W) float, or (B, H, W, C) uint8 raw images
        Bsz, H, W = (x.shape[0], x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[0], x.shape[2], x.shape[3])
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else (
            torch.float32 if x.dtype == torch.uint8 else x.dtype)
        cols = patch_im2col(x, self.patch, dt)
        w = self.proj.weight.reshape(self.proj.weight.shape[0], -1).to(cols.dtype)
        y = F.linear(cols, w, self.proj.bias.to(cols.dtype)).reshape(Bsz, H // self.patch, W // self.patch, -1)
        return self.norm(y) if self.norm is not None else y


class PatchMerging2D(nn.Module):
    """2x2 neighbourhood concat -> LN -> Linear(4C, 2C) (model.py:204-246)."""

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x):
        Bsz, H, W, C = x.shape
        h2, w2 = H // 2, W // 2
        parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
        x = torch.cat([p[:, :h2, :w2] for p in parts], -1)
        return self.reduction(self.norm(x))


class SS2D(nn.Module):
    """2-D selective scan over four directions (model.py:297-647), scan on the HIP kernel.

    Parameter names/shapes match the reference so its state dicts load as-is.
    """

    def __init__(self, d_model, d_state=16, d_conv=3, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1,
                 dt_init="random", dt_scale=1.0, dt_init_floor=1e-4, dropout=0.0, conv_bias=True, bias=False,
                 **kwargs):
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = int(expand * d_model)
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        K, di, R, N = 4, self.d_inner, self.dt_rank, d_state
        self.in_proj = nn.Linear(d_model, 2 * di, bias=bias)
        self.conv2d = nn.Conv2d(di, di, d_conv, groups=di, bias=conv_bias, padding=(d_conv - 1) // 2)
        self.act = nn.SiLU()
        xw = torch.empty(K, R + 2 * N, di)
        for k in range(K):
            nn.init.kaiming_uniform_(xw[k], a=math.sqrt(5))
        self.x_proj_weight = nn.Parameter(xw)
        std = R ** -0.5 * dt_scale
        dtw = torch.empty(K, di, R)
        if dt_init == "constant":
            nn.init.constant_(dtw, std)
        elif dt_init == "random":
            nn.init.uniform_(dtw, -std, std)
        else:
            raise NotImplementedError
        self.dt_projs_weight = nn.Parameter(dtw)
        self.dt_projs_bias = nn.Parameter(torch.stack([_dt_bias_init(di, dt_min, dt_max, dt_init_floor)
                                                       for _ in range(K)]))
        A = torch.arange(1, N + 1, dtype=torch.float32).repeat(K * di, 1)
        self.A_logs = nn.Parameter(torch.log(A))
        self.A_logs._no_weight_decay = True
        self.Ds = nn.Parameter(torch.ones(K * di))
        self.Ds._no_weight_decay = True
        self.out_norm = nn.LayerNorm(di)
        self.out_proj = nn.Linear(di, d_model, bias=bias)
        self.dropout = nn.Dropout(dropout) if dropout > 0.0 else None

    def _scan_u(self, u):  # u = [x, x^T] (B, 2, d, L) fp32 -> (B, 4 d, L), directions in their own frames
        """model.py:503-565 with the cross-scan inside the kernels: u holds x and x^T once (the
        reference stacks [x, x^T, flip x, flip x^T]); the per-direction projections read it in place;
        directions 2 / 3 walk u blocks 0 / 1 backwards (grouped_scan_fn), so their outputs come back
        un-flipped.  Blocks 1 / 3 stay in the transposed (W, H) frame: the merge reads them there."""
        Bsz, _, d, L = u.shape
        K = 4
        wx, wdt = self.x_proj_weight.to(u.dtype), self.dt_projs_weight.to(u.dtype)
        if ss2d_proj_ok(u, wx, wdt):
            # both projections on mc_ss2d_group_proj, no permuted operand copies (ops.SS2DProjFn)
            dts, Bs, Cs = ss2d_proj(u, wx, wdt, self.dt_rank, self.d_state)
        else:
            x_dbl = torch.einsum("bjdl,ijcd->bijcl", u, wx.view(2, 2, -1, d)).reshape(Bsz, K, -1, L)   # k = 2 i + j
            dts, Bs, Cs = torch.split(x_dbl, [self.dt_rank, self.d_state, self.d_state], dim=2)
            dts = torch.einsum("bkrl,kdr->bkdl", dts, wdt)
        return grouped_scan_fn(u.float().reshape(Bsz, 2 * d, L), dts.float().reshape(Bsz, K * d, L),
                               -torch.exp(self.A_logs.float()), Bs.float(), Cs.float(), self.Ds.float(),
                               self.dt_projs_bias.float().reshape(-1), delta_softplus=True,
                               reverse_groups=SS2D_REVERSE_GROUPS, u_groups=SS2D_U_GROUPS)

    def forward_core(self, x):  # (B, d, H, W) -> four (B, d, L) maps, fp32, reference order
        """The reference's forward_corev0 contract (model.py:503-565) on a conv output: y1 .. y4 back in
        the (H, W) frame.  Not on the forward path (forward fuses the stack and the merge)."""
        Bsz, d, H, W = x.shape
        L = H * W
        u = torch.stack([x.reshape(Bsz, d, L), x.transpose(2, 3).reshape(Bsz, d, L)], dim=1).float()
        out = self._scan_u(u).view(Bsz, 4, d, L)
        back = lambda t: t.reshape(Bsz, d, W, H).transpose(2, 3).reshape(Bsz, d, L)  # noqa: E731
        return out[:, 0], out[:, 2], back(out[:, 1]), back(out[:, 3])

    def forward(self, x, **kwargs):  # (B, H, W, C)
        # model.py:630-647.  x / z stay channels-last halves of in_proj's output (no permute copy);
        # ss2d_conv_stack writes silu(conv2d(x)) straight into the scan input u = [x, x^T] (fp32), and
        # ss2d_merge_ln_gate sums the four directions (the two column-major ones read transposed),
        # applies out_norm and the silu(z) gate, channels-last for out_proj (mc_ss2d.h)
        x, z = self.in_proj(x).chunk(2, dim=-1)
        u = ss2d_conv_stack(x, self.conv2d.weight, self.conv2d.bias)
        y = ss2d_merge_ln_gate(self._scan_u(u), z, self.out_norm.weight, self.out_norm.bias, self.out_norm.eps)
        out = self.out_proj(y)
        return self.dropout(out) if self.dropout is not None else out

def channel_shuffle(x, groups):
    Bsz, H, W, C = x.shape
    return x.view(Bsz, H, W, groups, C // groups).transpose(3, 4).reshape(Bsz, H, W, C)


class SS_Conv_SSM(nn.Module):
    """Half the channels through a conv stack, half through SS2D; shuffle; residual (model.py:666-723)."""

    def __init__(self, hidden_dim=0, drop_path=0.0, norm_layer=partial(nn.LayerNorm, eps=1e-6), attn_drop_rate=0.0,
                 d_state=16, **kwargs):
        super().__init__()
        h = hidden_dim // 2
        self.ln_1 = norm_layer(h)
        self.self_attention = SS2D(d_model=h, dropout=attn_drop_rate, d_state=d_state, **kwargs)
        self.drop_path = nn.Identity() if drop_path == 0 else _DropPath(drop_path)
        self.conv33conv33conv11 = nn.Sequential(
            nn.BatchNorm2d(h), nn.Conv2d(h, h, 3, 1, 1), nn.BatchNorm2d(h), nn.ReLU(),
            nn.Conv2d(h, h, 3, 1, 1), nn.BatchNorm2d(h), nn.ReLU(), nn.Conv2d(h, h, 1, 1), nn.ReLU())

    def forward(self, inp):
        left, right = inp.chunk(2, dim=-1)
        x = self.drop_path(self.self_attention(self.ln_1(right)))
        left = self.conv33conv33conv11(left.permute(0, 3, 1, 2).contiguous()).permute(0, 2, 3, 1).contiguous()
        return channel_shuffle(torch.cat((left, x), dim=-1), groups=2) + inp


class _DropPath(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        keep = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(1 - self.p)
        return x * keep / (1 - self.p)


class VSSLayer(nn.Module):
    def __init__(self, dim, depth, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None,
                 use_checkpoint=False, d_state=16, **kwargs):
        super().__init__()
        self.dim, self.use_checkpoint = dim, use_checkpoint
        self.blocks = nn.ModuleList([
            SS_Conv_SSM(hidden_dim=dim, drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                        norm_layer=norm_layer, attn_drop_rate=attn_drop, d_state=d_state)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x):
        for blk in self.blocks:
            x = torch.utils.checkpoint.checkpoint(blk, x, use_reentrant=False) if self.use_checkpoint else blk(x)
        return self.downsample(x) if self.downsample is not None else x


class VSSM(nn.Module):
    """MedMamba backbone + head (model.py:868-995); "medmamba" = depths [2,2,8,2], dims [64,128,256,512]."""

    def __init__(self, patch_size=4, in_chans=3, num_classes=1000, depths=(2, 2, 4, 2), dims=(96, 192, 384, 768),
                 d_state=16, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=nn.LayerNorm,
                 patch_norm=True, use_checkpoint=False, **kwargs):
        super().__init__()
        depths, dims = list(depths), list(dims)
        self.num_classes, self.num_layers = num_classes, len(depths)
        self.embed_dim, self.num_features, self.dims = dims[0], dims[-1], dims
        self.patch_embed = PatchEmbed2D(patch_size, in_chans, dims[0], norm_layer if patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([
            VSSLayer(dims[i], depths[i], d_state=math.ceil(dims[0] / 6) if d_state is None else d_state,
                     attn_drop=attn_drop_rate, drop_path=dpr[sum(depths[:i]): sum(depths[: i + 1])],
                     norm_layer=norm_layer, downsample=PatchMerging2D if i < self.num_layers - 1 else None,
                     use_checkpoint=use_checkpoint)
            for i in range(self.num_layers)])
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.output_dim = num_classes if num_classes > 0 else self.num_features
        self.apply(self._init_weights)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward_backbone(self, x):
        x = self.pos_drop(self.patch_embed(x))
        for layer in self.layers:
            x = layer(x)
        return x

    def forward(self, x):
        x = self.forward_backbone(x).permute(0, 3, 1, 2)
        return self.head(torch.flatten(self.avgpool(x), 1))


# ============================================================================ factory (model.py:1257-1289)
MODEL_CONFIGS = {
    # C1: tiny plumbing config (BASELINE configs[0]): Mamba text d_model 128, L = 256, d_state 16, 32-dim output
    "tiny-mamba-clip": dict(vision=dict(img_size=32, patch=8, width=64, layers=2, heads=4, output_dim=32),
                            text=dict(vocab_size=1000, context_length=256, d_model=128, n_layer=2, output_dim=32)),
    # C2: ViT-B/16 + Mamba-130M text (BASELINE configs[1])
    "vit_b16-mamba130m": dict(vision=dict(), text=dict(vocab_size=50280, context_length=77, d_model=768,
                                                        n_layer=24, output_dim=512)),
    # C2 with padded captions pooled at their last token (pad id 0): the tower state-spaces/mamba-130m-hf
    # loads into (load_hf_mamba_state_dict)
    "vit_b16-mamba130m-hf": dict(vision=dict(), text=dict(vocab_size=50280, context_length=77, d_model=768,
                                                           n_layer=24, output_dim=512, pad_id=0)),
    # C4 text tower (BASELINE configs[3])
    "mamba790m-text": dict(vision=dict(), text=dict(vocab_size=50280, context_length=4096, d_model=1536,
                                                     n_layer=48, output_dim=512)),
    # C3: BiomedCLIP-shaped (ViT-B/16 + PubMedBERT-256), random init (BASELINE configs[2])
    "biomedclip-vit_b16-pubmedbert256": dict(vision=dict(), bert=dict()),
    # C3 with the text tower that computes transformers.BertModel (post-LN, token types, padding mask):
    # the one BiomedCLIP's PubMedBERT weights load into (load_hf_bert_state_dict)
    "biomedclip-vit_b16-pubmedbert256-hf": dict(vision=dict(), hf_bert=dict()),
    # openai/clip-vit-base-patch16: the CLIP vision tower (pre-LN before the blocks, eps 1e-5, no patch bias,
    # quick_gelu) with the CLIP text transformer (12 x 512, 8 heads, 77 tokens, causal, end-of-text pooling):
    # the model a transformers.CLIPModel state dict loads into (load_hf_clip_state_dict)
    "clip-vit_b16-hf": dict(vision=dict(pre_norm=True, eps=1e-5, patch_bias=False, act="quick_gelu"), clip_text=dict()),
}


def build_clip(name, force_patch_dropout=None, **clip_kwargs):
    """``clip_kwargs`` (init_logit_scale, init_logit_bias) go to ClipModel: SigLIP training starts from
    log 10 and -10 (pipeline.py:213-216).  ``force_patch_dropout`` (None = 0) is the visual tower's
    patch_dropout (the reference's --force-patch-dropout, cli/main.py:355-356)."""
    cfg = MODEL_CONFIGS[name]
    visual = VisionTransformer(**cfg["vision"], patch_dropout=force_patch_dropout or 0.0)
    if "clip_text" in cfg:
        text = ClipTextEncoder(**cfg["clip_text"])
    elif "hf_bert" in cfg:
        text = HFBertTextEncoder(**cfg["hf_bert"])
    else:
        text = BertTextEncoder(**cfg["bert"]) if "bert" in cfg else MambaTextEncoder(**cfg["text"])
    return ClipModel(visual, text, **clip_kwargs)


def init_model(model, tokenizer=None, aug_cfg=None, is_clip=False, use_tokenizer=False, **model_kwargs):
    """Returns (model, preprocess_train, preprocess_val, tokenizer) like model.py:1257-1289.
    ``model_kwargs`` (init_logit_scale, init_logit_bias, force_patch_dropout) reach build_clip for a
    config name: the ClipModel's initial scale / bias and the visual tower's patch dropout.

    "medmamba" -> VSSM(depths=[2,2,8,2], dims=[64,128,256,512], num_classes=2);
    a MODEL_CONFIGS name -> a random-init ClipModel (no hub access offline);
    a callable -> model().  Preprocessing is identity on synthetic tensors.
    """
    if model == "medmamba":
        model = VSSM(depths=[2, 2, 8, 2], dims=[64, 128, 256, 512], num_classes=2)
    elif isinstance(model, str):
        if model not in MODEL_CONFIGS:
            raise ValueError(f"unknown model {model!r}: offline build knows {sorted(MODEL_CONFIGS)}")
        model = build_clip(model, **model_kwargs)
    elif callable(model):
        model = model()
    if is_clip and not isinstance(model, ClipModel):
        model = ClipModel(model)          # shares the towers AND logit_scale / logit_bias (model.py:1274-1275)
    if use_tokenizer and tokenizer is not None and callable(tokenizer):
        tokenizer = tokenizer()
    identity = (lambda x: x)
    return model, identity, identity, tokenizer
