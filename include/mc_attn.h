/*
 * mc_attn.h -- C ABI of the fused short-sequence multi-head attention (libmamba_clip_amd.so).
 *
 * The towers' self-attention (ViT-B/16 image tower: 197 tokens; BERT text tower: <= 256
 * tokens; 12 heads of 64).  The reference gets it from timm / open_clip / HF through
 * torch's scaled_dot_product_attention (model.py:1019-1064 builds
 * the towers); it replaces that call for the unmasked, dropout-free case:
 *   o = softmax(scale * q k^T) v          per (batch, head)
 * Two variants of the same kernels follow below: with a key-padding mask (mc_attn_masked_*: the
 * BERT text tower's padded captions) and with the causal mask (mc_attn_causal_*: the CLIP text
 * transformer, 77 tokens).
 * One workgroup owns one (batch, head): the whole sequence's K / V (and, backward, Q / dO)
 * sit in LDS, so the softmax is exact in one pass (no online rescaling) and dQ / dK / dV
 * need no cross-workgroup sums.
 *
 * Layout: every tensor is addressed as base + b * bs + n * ns + h * hs + d (element
 * strides, d contiguous), so q / k / v can be slices of one packed (B, N, 3, H, D)
 * projection output and o / dq / dk / dv can be written straight into the layouts the
 * next GEMM reads.  Requirements: head_dim == 64, 1 <= seqlen <= 256, dtype bf16 or f16,
 * 16-B aligned rows (pointers and the three strides multiples of 8 elements).
 * Batch and head strides are 64-bit and free (any sign, any size).  Token strides are not: the
 * kernels read K / V (every kernel) and, backward at seqlen > 224, Q / dO / O through 32-bit
 * buffer byte offsets, so q_ns (every entry point) and o_ns (the backward ones) must be
 * >= 0 with ((seqlen - 1) * ns + 64) * 2 bytes <= 2^31 -- at seqlen 256 ns <= 4210752 elements;
 * anything else returns MC_ERR_SHAPE before a launch.  (o_ns of the forward and dq_ns are only
 * written through, with 64-bit addresses: no limit.)
 * Same conventions as mc_scan.h: device pointers, asynchronous on `stream`,
 * MC_OK / MC_ERR_* return codes.
 */
#ifndef MAMBA_CLIP_AMD_MC_ATTN_H
#define MAMBA_CLIP_AMD_MC_ATTN_H

#include <stddef.h>
#include <stdint.h>

#include "mc_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MC_ATTN_HEAD_DIM 64
#define MC_ATTN_MAX_SEQ 256

typedef struct {
  int32_t batch, heads, seqlen, head_dim, dtype;
  float scale;                        /* softmax scale, 1/sqrt(head_dim) for SDPA's default */
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;           /* element strides of q, k and v (shared) */
  void* o; int64_t o_bs, o_ns, o_hs;
  float* lse;                         /* (batch, heads, seqlen) fp32: ln sum exp(scale q.k), for the backward */
} mc_attn_fwd_params;

/* o = softmax(scale q k^T) v and the row log-sum-exp. */
int mc_attn_fwd(const mc_attn_fwd_params* p, void* stream);

typedef struct {
  int32_t batch, heads, seqlen, head_dim, dtype;
  float scale;
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;           /* shared by q, k, v */
  const void* o; const void* dout;
  int64_t o_bs, o_ns, o_hs;           /* shared by o and dout */
  const float* lse;                   /* from mc_attn_fwd */
  void* dq; void* dk; void* dv;
  int64_t dq_bs, dq_ns, dq_hs;        /* shared by dq, dk, dv */
  float* dsum;                        /* (batch, 3, heads, head_dim) fp32, nullable: per-batch sums over the
                                         sequence of dq | dk | dv as stored -- summed over the batch, the bias
                                         gradient of a packed qkv projection (no second pass over dq / dk / dv) */
} mc_attn_bwd_params;

/* dq, dk, dv of the above given dout (recomputes the probabilities from q, k and lse). */
int mc_attn_bwd(const mc_attn_bwd_params* p, void* stream);

/*
 * Key-padding-masked variant (the BERT text tower: captions padded to the context length):
 *   o = softmax(scale * q k^T + (key_mask ? 0 : -inf)) v
 * key_mask is (batch, MC_ATTN_MASK_WORDS) 32-bit words, 4-B aligned: bit j of word t of batch b
 * set = key 32 t + j may be attended to (HF's attention_mask[:, None, None, :]: one mask per batch
 * row, shared by its heads and queries, holes allowed).  Bits of keys >= seqlen are ignored.
 * Every query row is computed, padded ones too (they are rows of the hidden state); lse is over
 * the valid keys; dk / dv of masked keys are stored as exact zeros.  A 32-key tile whose word is
 * zero is skipped.  A batch row with no valid key is not a supported input (o, dq, dk, dv come
 * out zero, lse 0: finite, not HF's uniform average).  Other fields, requirements and return
 * codes as the unmasked entry points; results are bitwise reproducible (no atomics), and with
 * every bit set bitwise equal to the unmasked entry points'.
 */
#define MC_ATTN_MASK_WORDS (MC_ATTN_MAX_SEQ / 32)

typedef struct {
  int32_t batch, heads, seqlen, head_dim, dtype;
  float scale;
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;
  void* o; int64_t o_bs, o_ns, o_hs;
  float* lse;
  const uint32_t* key_mask;           /* (batch, MC_ATTN_MASK_WORDS) */
} mc_attn_masked_fwd_params;

int mc_attn_masked_fwd(const mc_attn_masked_fwd_params* p, void* stream);

typedef struct {
  int32_t batch, heads, seqlen, head_dim, dtype;
  float scale;
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;
  const void* o; const void* dout;
  int64_t o_bs, o_ns, o_hs;
  const float* lse;                   /* from mc_attn_masked_fwd with the same key_mask */
  void* dq; void* dk; void* dv;
  int64_t dq_bs, dq_ns, dq_hs;
  float* dsum;
  const uint32_t* key_mask;           /* (batch, MC_ATTN_MASK_WORDS) */
} mc_attn_masked_bwd_params;

int mc_attn_masked_bwd(const mc_attn_masked_bwd_params* p, void* stream);

/*
 * Causal variant (the CLIP text transformer: 77 tokens, pooled at the end-of-text token):
 *   o = softmax(scale * q k^T + (j <= i ? 0 : -inf)) v
 * Query i attends to the keys j <= i; lse is over those keys; dq / dk / dv / dsum are the
 * gradients of that.  The parameter structs, requirements, token-stride limits and return codes
 * are those of mc_attn_fwd / mc_attn_bwd.  32-key tiles above the diagonal are never visited, tiles
 * below it run the unmasked instructions, the diagonal tile pays one select per score.  Every query
 * has itself as a key, so no row is empty; row i of o, lse and dq depends on rows <= i of the
 * inputs only, bit for bit.  Query 0 has one key: its dS is stored as the exact zero it is.
 * Bitwise reproducible (no atomics).  Not combined with the key-padding mask: with end-of-text
 * pooling the tokens after it cannot reach the pooled row.
 */
int mc_attn_causal_fwd(const mc_attn_fwd_params* p, void* stream);
int mc_attn_causal_bwd(const mc_attn_bwd_params* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MAMBA_CLIP_AMD_MC_ATTN_H */
