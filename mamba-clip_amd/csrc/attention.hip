// attention.hip -- fused multi-head self-attention for short sequences (mc_attn.h): the ViT-B/16
// image tower (197 tokens) and the BERT text tower (<= 256 tokens), 12 heads of 64, bf16 / f16.
//
// Replaces torch's scaled_dot_product_attention inside the towers' blocks (timm / open_clip / HF
// attention behind the reference's model dict, model.py:1019-1064).  At
// N = 197 the library kernels are tiled for long sequences and run at ~7 % of the MFMA rate; here
// one workgroup owns one (batch, head) and keeps the whole sequence in LDS:
//  * forward: K and V images in LDS; each wave takes 32-query blocks and computes S^T = K Q^T on
//    v_mfma_f32_32x32x16 with the KEY on the accumulator rows and the query on the lane, so the
//    softmax over keys is in-lane (plus one permlane32 swap for the other lane half) and exact
//    (the full row is in registers: no online rescale); the probabilities, converted to 16-bit,
//    are directly the B operand of O^T = V^T P^T (V^T by ds_read_b64_tr_b16 transposed reads).
//  * backward: Q, K, V, dO images in LDS plus the row constants lse and delta = rowsum(dO o O).
//    Phase 1: wave w owns key tile w and sweeps the query blocks with the key on the lane
//    (S = Q K^T, dP = dO V^T), so P and dS = P (dP - delta) are the B operands of dV^T += dO^T P
//    and dK^T += Q^T dS.  Phase 2: wave w owns query block w and sweeps the key tiles in the
//    forward orientation (S^T, dP^T) for dQ^T += K^T dS^T.  Recomputing S / dP in phase 2 costs
//    8 of the 28 MFMAs per tile pair and removes every cross-wave sum (no atomics, deterministic).
// LDS images: [rows][64 x 16-bit], 16-B chunk c of row r at slot c ^ g((r >> 1) & 7) with
// g(m) = m ^ ((m & 1) << 2): the row reads of the 32x32x16 operands (ds_read_b128, 16 rows of
// one chunk per lane group) and the transposed reads (rows r..r+3 x 4 chunks per half-wave) are
// both conflict-free (64 banks x 4 B).
//
// Key-masked variant (mc_attn_masked_fwd / _bwd, the padded captions of the BERT text tower): the
// same two kernels instantiated with kMask = true; every added instruction sits under
// `if constexpr (kMask)` and the arguments gain the mask pointer in a derived struct, so the
// unmasked instantiations compile to what they were.  The words of a batch row (ANDed with the
// keys < N) live in one VGPR, word t on lane t, and come out wave-uniform through v_readlane: a
// tile whose word is 0 is skipped by a scalar branch, a tile whose word is all ones takes the
// unmasked instructions, only a mixed tile pays the per-key selects.
//
// Causal variant (mc_attn_causal_fwd / _bwd, the CLIP text transformer: 77 tokens, pooled at the
// end-of-text token): a third instantiation, kCausal = true, every added instruction under
// `if constexpr (kCausal)`; same argument structs as the unmasked kernels.  Query i sees keys j <= i.
// The 32 x 32 tiles already fit: a tile below the diagonal (key tile < query block) takes the
// unmasked instructions, a tile above it is never visited (the sweeps end / start at the diagonal,
// wave-uniform bounds), and only the diagonal tile pays one select per score: -1e30 above the
// diagonal in both forward passes, P = dS = 0 there in the backward (selects, so an overflowed P
// cannot leave a NaN).  Keys past N lie above the diagonal of every stored query, so the ragged last
// tile needs no test of its own.  Query 0 sees key 0 alone: P = 1 and dS = 0 exactly, and the
// backward stores that zero instead of the rounding residue of dP - delta.
#include <algorithm>
#include <type_traits>

#include "mc_common.h"
#include "../../include/mc_attn.h"

namespace mc {
namespace attn {

constexpr int kD = 64;            // head dim
constexpr int kRowB = kD * 2;     // bytes per 16-bit row
constexpr int kFwdWaves = 8;   // one 32-query block per wave (N <= 256); two workgroups per CU
constexpr int kBwdWaves = 8;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

template <typename T> struct M32;
template <> struct M32<bf16_t> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mma(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct M32<f16_t> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mma(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

__device__ __forceinline__ uint32_t img_off(int r, int c) {
  const int m = (r >> 1) & 7;
  return (uint32_t)(r * kRowB + 16 * (c ^ (m ^ ((m & 1) << 2))));
}
// 16-B row chunk c of row r (A / B operand of a 32x32x16 MFMA in natural k order)
__device__ __forceinline__ uint4 row_chunk(const char* img, int r, int c) {
  return *reinterpret_cast<const uint4*>(img + img_off(r, c));
}
// Transposed operand: rows r0 + {0..3} and r0 + 8 + {0..3} of the 16 columns d0 + [0, 16) of this
// lane's group (lane 4q + p of the group addresses row q, columns 4p..4p+3; lane i receives column i).
// Elements j of the result are rows r0 + 8 (j >> 2) + (j & 3): the k order of an accumulator tile
// used as the other operand (rows 16 s + 8 (j >> 2) + 4 h + (j & 3) with r0 = 16 s + 4 h).
__device__ __forceinline__ uint4 tr_chunk(const char* img, int r0, int d0, int lane) {
  const int li = lane & 15, q = li >> 2, d = d0 + 4 * (li & 3);
  const char* pa = img + img_off(r0 + q, d >> 3) + (d & 7) * 2;
  const char* pb = img + img_off(r0 + 8 + q, d >> 3) + (d & 7) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)pa);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)pb);
  return make_uint4((uint32_t)(uint16_t)lo.x | ((uint32_t)(uint16_t)lo.y << 16),
                    (uint32_t)(uint16_t)lo.z | ((uint32_t)(uint16_t)lo.w << 16),
                    (uint32_t)(uint16_t)hi.x | ((uint32_t)(uint16_t)hi.y << 16),
                    (uint32_t)(uint16_t)hi.z | ((uint32_t)(uint16_t)hi.w << 16));
}
// registers 8 s .. 8 s + 7 of an accumulator tile as a 16-bit operand fragment (k-step s)
template <typename TI>
__device__ __forceinline__ uint4 acc_frag(const f32x16& x, int s) {
  return make_uint4(cvt_pk2<TI>(x[8 * s + 0], x[8 * s + 1]), cvt_pk2<TI>(x[8 * s + 2], x[8 * s + 3]),
                    cvt_pk2<TI>(x[8 * s + 4], x[8 * s + 5]), cvt_pk2<TI>(x[8 * s + 6], x[8 * s + 7]));
}
__device__ __forceinline__ float swap_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float swap_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int kCtrl>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_xor4(float v) {   // banks 0 / 2 take lane + 4, banks 1 / 3 lane - 4
  const int iv = __float_as_int(v);
  const int lo = __builtin_amdgcn_update_dpp(iv, iv, 0x104, 0xF, 0x5, false);
  return __int_as_float(__builtin_amdgcn_update_dpp(lo, iv, 0x114, 0xF, 0xA, false));
}
// Column sums of a stored tile pair (x0: d in [0, 32), x1: [32, 64); lane = output row, accumulator
// rows = d), rows with `valid` false excluded.  Halving butterfly over the 32 lanes of each half:
// lane bit 4 by permlane16 swaps (32 -> 16 values), bits 3, 2, 1, 0 by DPP (16 -> 1); lane l ends
// with the sum of value index l & 31 = 16 db + r, i.e. d = 32 db + (r & 3) + 8 (r >> 2) + 4 hh.
// ~96 VALU per tile instead of a 5-step all-reduce of all 32 values.
__device__ __forceinline__ float tile_colsum(const f32x16& x0, const f32x16& x1, float mul, int lane) {
  float w[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(x0[r] * mul), __float_as_uint(x1[r] * mul), false, false);
    w[r] = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  }
  const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
  float u[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) u[k] = (b3 ? w[k + 8] : w[k]) + dpp_mov<0x128>(b3 ? w[k] : w[k + 8]);   // row_ror:8
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = (b2 ? u[k + 4] : u[k]) + row_xor4(b2 ? u[k] : u[k + 4]);
  float q[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) q[k] = (b1 ? t[k + 2] : t[k]) + dpp_mov<0x4E>(b1 ? t[k] : t[k + 2]);   // lane ^ 2
  return (b0 ? q[1] : q[0]) + dpp_mov<0xB1>(b0 ? q[0] : q[1]);                                        // lane ^ 1
}

// Store a transposed accumulator pair (x0: d in [0, 32), x1: [32, 64); column = this lane's row
// `row`, accumulator rows = d) as 16-B pieces: permlane32 swaps turn each lane's 4-element groups
// into 8 consecutive d (T21).  rows >= nrows are dropped.
// csum (LDS, 64 floats, nullable): the tile's column sums (fp32, rows < nrows).
template <typename TI>
__device__ __forceinline__ void store_rows(TI* base, int64_t ns, int row, int nrows, int lane, const f32x16& x0,
                                           const f32x16& x1, float mul, float* csum = nullptr) {
  const int hh = lane >> 5;
  if (csum) {   // the tile's column sums (fp32, before the 16-bit rounding of the stores)
    const int i = lane & 31, r = i & 15;
    csum[32 * (i >> 4) + (r & 3) + 8 * (r >> 2) + 4 * hh] = tile_colsum(x0, x1, row < nrows ? mul : 0.f, lane);
  }
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const f32x16& x = db ? x1 : x0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x[8 * m + i]), __float_as_uint(x[8 * m + 4 + i]),
                                                        false, false);
        v[i] = __uint_as_float(r[0]) * mul;
        v[4 + i] = __uint_as_float(r[1]) * mul;
      }
      const int d0 = db * 32 + 16 * m + 8 * hh;
      if (row < nrows) *reinterpret_cast<uint4*>(base + (int64_t)row * ns + d0) = pack_f<TI>(v);
    }
  }
}

// One global_load_lds_dwordx4: 16 B per lane from gsrc to LDS byte address m0v + 16 * lane (m0v
// wave-uniform), asm so hipcc does not track it (the caller waits with its own vmcnt); M0 is
// compiler-reserved: saved and restored in the statement.
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t m0v) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(m0v) : "memory");
}
typedef __attribute__((address_space(3))) char lds_char;

struct FwdArgs {
  int B, H, N;
  float scale, c2;   // c2 = scale * log2(e)
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;
  void* o; int64_t o_bs, o_ns, o_hs;
  float* lse;
};
struct FwdArgsM : FwdArgs { const uint32_t* mask; };   // (B, kMaskWords) key bits, kMask kernels only
constexpr int kMaskWords = MC_ATTN_MASK_WORDS;
template <bool kMask, typename A, typename AM> struct ArgsOf { typedef A type; };
template <typename A, typename AM> struct ArgsOf<true, A, AM> { typedef AM type; };

// Mask words of batch row b: lane t < NT holds word t with the bits of keys >= N cleared, every
// other lane 0.  word_of(wv, t), t wave-uniform, is then a scalar.
template <int NT>
__device__ __forceinline__ uint32_t load_mask_words(const uint32_t* mask, int b, int N, int lane) {
  uint32_t w = 0;
  if (lane < NT) {
    const int nb = N - 32 * lane;   // >= 1: NT = ceil(N / 32)
    w = mask[(int64_t)b * kMaskWords + lane] & (nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1u);
  }
  return w;
}
__device__ __forceinline__ uint32_t word_of(uint32_t wv, int t) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wv, t);
}
// accumulator register r holds row (r & 3) + 8 (r >> 2) + 4 hh of its tile: bit of that row in wl = w >> 4 hh
__device__ __forceinline__ bool row_bit(uint32_t wl, int r) { return (wl >> ((r & 3) + 8 * (r >> 2))) & 1u; }

template <typename TI, int NT, bool kMask = false, bool kCausal = false>
__global__ __launch_bounds__(64 * kFwdWaves, 2) void attn_fwd_kernel(const typename ArgsOf<kMask, FwdArgs, FwdArgsM>::type a) {
  using M = M32<TI>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int Np = NT * 32;
  char* kimg = smem;
  char* vimg = smem + Np * kRowB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l32 = lane & 31;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int N = a.N;
  const int64_t off = (int64_t)b * a.q_bs + (int64_t)h * a.q_hs;
  const TI* qg = reinterpret_cast<const TI*>(a.q) + off;
  const TI* kg = reinterpret_cast<const TI*>(a.k) + off;
  const TI* vg = reinterpret_cast<const TI*>(a.v) + off;

  // K / V images: every piece of a thread in flight at once (buffer loads: rows past N read 0)
  constexpr int kPer = (Np * 8 + 64 * kFwdWaves - 1) / (64 * kFwdWaves);
  const uint32_t rng = (uint32_t)(((int64_t)(N - 1) * a.q_ns + kD) * (int64_t)sizeof(TI));
  const __amdgpu_buffer_rsrc_t rk = make_rsrc(kg, rng), rv = make_rsrc(vg, rng);
  uint4 kr[kPer], vr[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + 64 * kFwdWaves * j, r = i >> 3, c = i & 7;
    const uint32_t o = r < N ? (uint32_t)(r * a.q_ns + 8 * c) * (uint32_t)sizeof(TI) : 0x80000000u;
    kr[j] = buf_ld16(rk, o);
    vr[j] = buf_ld16(rv, o);
  }
  // this wave's 32-query block (B operand: lane = query, 16-B chunks 2 s + hh of its row)
  const int qt = wave;
  const int q = qt * 32 + l32;
  int tEnd = NT;   // kCausal: the key tiles up to the diagonal one (wave-uniform)
  if constexpr (kCausal) tEnd = __builtin_amdgcn_readfirstlane(qt) + 1;
  uint4 qf[4];
  {
    const TI* qrow = qg + (int64_t)min(q, N - 1) * a.q_ns;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = ld16(qrow + 16 * s + 8 * hh);
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + 64 * kFwdWaves * j, r = i >> 3, c = i & 7;
    if (i < Np * 8) {
      *reinterpret_cast<uint4*>(kimg + img_off(r, c)) = kr[j];
      *reinterpret_cast<uint4*>(vimg + img_off(r, c)) = vr[j];
    }
  }
  uint32_t wv = 0;   // kMask: this batch row's mask words (lane t = word t)
  if constexpr (kMask) wv = load_mask_words<NT>(a.mask, b, N, lane);
  __syncthreads();
  if (qt < NT) {
    // S^T tiles: rows = keys t*32 + (r & 3) + 8 (r >> 2) + 4 hh, column = this lane's query.
    // Two passes over the key tiles (the row max, then the probabilities and P V): recomputing
    // S costs 4 MFMAs per tile and keeps one tile of scores live instead of all NT (no spills).
    // kMask: w = the tile's mask word (keys >= N already cleared); masked keys score -1e30 like
    // the keys past N, so their probabilities are exactly 0.
    // kCausal: the diagonal tile t == qt scores -1e30 where key > query (that covers the keys past N
    // of every stored query); both passes go through here, so both make the comparison.
    auto s_tile = [&](int t, uint32_t w) __attribute__((always_inline)) {
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = M::mma(row_chunk(kimg, t * 32 + l32, 2 * s + hh), qf[s], acc);
      if constexpr (kMask) {
        if (w != 0xFFFFFFFFu) {   // wave-uniform
          const uint32_t wl = w >> (4 * hh);
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (!row_bit(wl, r)) acc[r] = -1e30f;
        }
      } else if constexpr (kCausal) {
        if (t == tEnd - 1) {   // wave-uniform
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((r & 3) + 8 * (r >> 2) + 4 * hh > l32) acc[r] = -1e30f;
        }
      } else if (t == NT - 1 && Np > N) {   // keys past N (last tile only)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= N) acc[r] = -1e30f;
      }
      return acc;
    };
    float m = -1e30f;
#pragma unroll 1
    for (int t = 0; t < tEnd; ++t) {
      uint32_t w = 0;
      if constexpr (kMask) {
        w = word_of(wv, t);
        if (w == 0) continue;   // no valid key in the tile
      }
      const f32x16 st = s_tile(t, w);
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, st[r]);
    }
    m = swap_max(m);
    const float mc = m * a.c2;
    // O^T = V^T P^T: two 32-row d blocks, lane = query
    float l = 0.f;
    f32x16 o0 = {}, o1 = {};
#pragma unroll 1
    for (int t = 0; t < tEnd; ++t) {
      uint32_t w = 0;
      if constexpr (kMask) {
        w = word_of(wv, t);
        if (w == 0) continue;
      }
      f32x16 st = s_tile(t, w);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fast_exp2(st[r] * a.c2 - mc);
        st[r] = p;
        l += p;
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const uint4 pf = acc_frag<TI>(st, s2);
        const int r0 = t * 32 + 16 * s2 + 4 * hh;
        o0 = M::mma(tr_chunk(vimg, r0, 16 * ((lane >> 4) & 1), lane), pf, o0);
        o1 = M::mma(tr_chunk(vimg, r0, 32 + 16 * ((lane >> 4) & 1), lane), pf, o1);
      }
    }
    l = swap_sum(l);
    if constexpr (kMask) {   // no valid key at all (unsupported input): o = 0, lse = 0, not NaN / -inf
      const bool none = l == 0.f;
      store_rows<TI>(reinterpret_cast<TI*>(a.o) + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs, a.o_ns, q, N, lane, o0, o1,
                     none ? 0.f : 1.f / l);
      if (hh == 0 && q < N) a.lse[(int64_t)bh * N + q] = none ? 0.f : m * a.scale + fast_log2(l) * kLn2;
    } else {
    store_rows<TI>(reinterpret_cast<TI*>(a.o) + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs, a.o_ns, q, N, lane, o0, o1,
                   1.f / l);
    if (hh == 0 && q < N) a.lse[(int64_t)bh * N + q] = m * a.scale + fast_log2(l) * kLn2;
    }
  }
}

struct BwdArgs {
  int B, H, N;
  float scale, c2;
  const void* q; const void* k; const void* v;
  int64_t q_bs, q_ns, q_hs;
  const void* o; const void* g;
  int64_t o_bs, o_ns, o_hs;
  const float* lse;
  void* dq; void* dk; void* dv;
  int64_t d_bs, d_ns, d_hs;
  float* dsum;   // (B, 3, H, 64) or null
};
struct BwdArgsM : BwdArgs { const uint32_t* mask; };

template <typename TI, int NT, bool kMask = false, bool kCausal = false>
__global__ __launch_bounds__(64 * kBwdWaves, 1) void attn_bwd_kernel(const typename ArgsOf<kMask, BwdArgs, BwdArgsM>::type a) {
  using M = M32<TI>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int Np = NT * 32;
  constexpr int kImg = Np * kRowB;
  // N <= 224: persistent over heads with the next head's q / dO / O streamed into LDS during phase 2
  // (the images fit 160 KB with the O staging image); N = 256: one head per workgroup
  constexpr bool kPersist = NT <= 7;
  char* qimg = smem;
  char* kimg = smem + kImg;
  char* vimg = smem + 2 * kImg;
  char* gimg = smem + 3 * kImg;
  char* oimg = smem + 4 * kImg;                                              // kPersist only
  float* lse2 = reinterpret_cast<float*>(smem + (kPersist ? 5 : 4) * kImg);   // lse * log2(e); +inf past N (P = 0)
  float* dlt = lse2 + Np;                                                     // rowsum(dO o O)
  float* csl = dlt + Np;                                                      // [dq | dk | dv][wave][64] tile column sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l32 = lane & 31, g16 = 16 * ((lane >> 4) & 1);
  const int N = a.N, total = a.B * a.H;
  constexpr int kPer = (Np * 8 + 64 * kBwdWaves - 1) / (64 * kBwdWaves);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_char*)smem);

  // q / dO / O rows of head bh -> qimg / gimg / oimg by LDS-DMA (lane-linear 1-KB pieces = 8 rows:
  // lane L takes slot L % 8 of row L / 8 and loads the chunk that belongs there, c = slot ^ g(row);
  // rows past N repeat row N - 1, harmless: their P and dS are 0, their outputs are not stored)
  float lv = 0.f;
  auto dma_qgo = [&](int bh) __attribute__((always_inline)) {
    const int b = bh / a.H, h = bh % a.H;
    const TI* qg = reinterpret_cast<const TI*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * a.q_hs;
    const TI* gg = reinterpret_cast<const TI*>(a.g) + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs;
    const TI* og = reinterpret_cast<const TI*>(a.o) + (int64_t)b * a.o_bs + (int64_t)h * a.o_hs;
#pragma unroll
    for (int k = 0; k < (Np / 8 + kBwdWaves - 1) / kBwdWaves; ++k) {
      const int j = wave + kBwdWaves * k;
      if (j < Np / 8) {
        const uint32_t blk = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(1024 * j));   // wave-uniform M0 base
        const int r = 8 * j + (lane >> 3), m = (r >> 1) & 7;
        const int c = (lane & 7) ^ (m ^ ((m & 1) << 2));
        const int64_t rr = min(r, N - 1);
        glds16(qg + rr * a.q_ns + 8 * c, blk);
        glds16(gg + rr * a.o_ns + 8 * c, blk + (uint32_t)(3 * kImg));
        glds16(og + rr * a.o_ns + 8 * c, blk + (uint32_t)(4 * kImg));
      }
    }
    if (tid < Np) lv = a.lse[(int64_t)bh * N + min(tid, N - 1)];
  };
  if constexpr (kPersist) dma_qgo(blockIdx.x);

#pragma unroll 1
  for (int bh = blockIdx.x; bh < total; bh += gridDim.x) {
  const int b = bh / a.H, h = bh % a.H;
  const int64_t off = (int64_t)b * a.q_bs + (int64_t)h * a.q_hs;
  const int64_t offo = (int64_t)b * a.o_bs + (int64_t)h * a.o_hs;
  const TI* qg = reinterpret_cast<const TI*>(a.q) + off;
  const TI* kg = reinterpret_cast<const TI*>(a.k) + off;
  const TI* vg = reinterpret_cast<const TI*>(a.v) + off;
  const TI* og = reinterpret_cast<const TI*>(a.o) + offo;
  const TI* gg = reinterpret_cast<const TI*>(a.g) + offo;
  uint32_t wv = 0;   // kMask: the mask words of this head's batch row (re-read per head: b changes)
  if constexpr (kMask) wv = load_mask_words<NT>(a.mask, b, N, lane);

  if constexpr (kPersist) {
    // ---- K / V of this head (registers -> images), delta from the streamed dO / O images, lse2
    const uint32_t rq = (uint32_t)(((int64_t)(N - 1) * a.q_ns + kD) * (int64_t)sizeof(TI));
    const __amdgpu_buffer_rsrc_t rsk = make_rsrc(kg, rq), rsv = make_rsrc(vg, rq);
    uint4 kv[kPer], vv[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + 64 * kBwdWaves * j, r = i >> 3, c = i & 7;
      const uint32_t o1 = r < N ? (uint32_t)(r * a.q_ns + 8 * c) * (uint32_t)sizeof(TI) : 0x80000000u;
      kv[j] = buf_ld16(rsk, o1);
      vv[j] = buf_ld16(rsv, o1);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's LDS-DMA pieces (and K / V) landed
    __syncthreads();                      // ... and everyone's
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + 64 * kBwdWaves * j, r = i >> 3, c = i & 7;
      float part = 0.f;
      if (i < Np * 8) {
        const uint4 gq = row_chunk(gimg, r, c), oq = row_chunk(oimg, r, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) part += elem_f<TI>(gq, e) * elem_f<TI>(oq, e);
      }
      part += __shfl_xor(part, 1);
      part += __shfl_xor(part, 2);
      part += __shfl_xor(part, 4);
      if (i < Np * 8) {
        *reinterpret_cast<uint4*>(kimg + img_off(r, c)) = kv[j];
        *reinterpret_cast<uint4*>(vimg + img_off(r, c)) = vv[j];
        if (c == 0) dlt[r] = r < N ? part : 0.f;
      }
    }
    if (tid < Np) lse2[tid] = tid < N ? lv * kLog2e : __builtin_huge_valf();
  } else {
  // ---- prologue: four images, delta and lse2.  Every piece of a thread in flight at once (buffer
  // loads: rows past N read 0); 8 consecutive threads hold one row (delta's partial dots)
  {
    const uint32_t rq = (uint32_t)(((int64_t)(N - 1) * a.q_ns + kD) * (int64_t)sizeof(TI));
    const uint32_t ro = (uint32_t)(((int64_t)(N - 1) * a.o_ns + kD) * (int64_t)sizeof(TI));
    const __amdgpu_buffer_rsrc_t rsq = make_rsrc(qg, rq), rsk = make_rsrc(kg, rq), rsv = make_rsrc(vg, rq);
    const __amdgpu_buffer_rsrc_t rso = make_rsrc(og, ro), rsg = make_rsrc(gg, ro);
    uint4 qv[kPer], kv[kPer], vv[kPer], gv[kPer], ov[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + 64 * kBwdWaves * j, r = i >> 3, c = i & 7;
      const uint32_t o1 = r < N ? (uint32_t)(r * a.q_ns + 8 * c) * (uint32_t)sizeof(TI) : 0x80000000u;
      const uint32_t o2 = r < N ? (uint32_t)(r * a.o_ns + 8 * c) * (uint32_t)sizeof(TI) : 0x80000000u;
      qv[j] = buf_ld16(rsq, o1);
      kv[j] = buf_ld16(rsk, o1);
      vv[j] = buf_ld16(rsv, o1);
      gv[j] = buf_ld16(rsg, o2);
      ov[j] = buf_ld16(rso, o2);
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid + 64 * kBwdWaves * j, r = i >> 3, c = i & 7;
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) part += elem_f<TI>(gv[j], e) * elem_f<TI>(ov[j], e);
      part += __shfl_xor(part, 1);
      part += __shfl_xor(part, 2);
      part += __shfl_xor(part, 4);
      if (i < Np * 8) {
        *reinterpret_cast<uint4*>(qimg + img_off(r, c)) = qv[j];
        *reinterpret_cast<uint4*>(kimg + img_off(r, c)) = kv[j];
        *reinterpret_cast<uint4*>(vimg + img_off(r, c)) = vv[j];
        *reinterpret_cast<uint4*>(gimg + img_off(r, c)) = gv[j];
        if (c == 0) {
          dlt[r] = part;
          lse2[r] = r < N ? a.lse[(int64_t)bh * N + r] * kLog2e : __builtin_huge_valf();
        }
      }
    }
  }
  }
  __syncthreads();

  // ---- phase 1: wave = key tile; dV^T += dO^T P, dK^T += Q^T dS over the query blocks.  (Issuing
  // the next block's S / dP MFMAs before this block's gradient MFMAs, with K / V re-read from LDS
  // to make room, measured 12 % slower: 325 vs 290 us at C2.)
  if (wave < NT) {
    const int kt = wave;
    uint4 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = row_chunk(kimg, kt * 32 + l32, 2 * s + hh);
      vf[s] = row_chunk(vimg, kt * 32 + l32, 2 * s + hh);
    }
    f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
    // kMask: the key is this lane's column of all four accumulators and of P / dS, so a masked key
    // touches nothing but its own dK / dV rows: they are cleared after the sweep (a select, so an
    // overflowed P of a masked key cannot leave a NaN), and a tile without a valid key skips the sweep.
    uint32_t kw = 0xFFFFFFFFu;
    if constexpr (kMask) kw = word_of(wv, kt);
    // kCausal: the query blocks from the diagonal one on; in the diagonal block P = dS = 0 where
    // query < key (selects: an overflowed P above the diagonal cannot leave a NaN), and dS of query 0
    // (one key: P = 1, dS = 0 exactly) is stored as that zero.
    int qt0 = 0;
    if constexpr (kCausal) qt0 = __builtin_amdgcn_readfirstlane(kt);
#pragma unroll 1
    for (int qt = qt0; qt < (kw != 0 ? NT : 0); ++qt) {
      f32x16 sa = {}, pa = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = M::mma(row_chunk(qimg, qt * 32 + l32, 2 * s + hh), kf[s], sa);
        pa = M::mma(row_chunk(gimg, qt * 32 + l32, 2 * s + hh), vf[s], pa);
      }
      // rows of this lane's accumulators: queries qt*32 + 8 j + 4 hh + i  (register 4 j + i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 L = *reinterpret_cast<const f32x4*>(lse2 + qt * 32 + 8 * j + 4 * hh);
        const f32x4 Dl = *reinterpret_cast<const f32x4*>(dlt + qt * 32 + 8 * j + 4 * hh);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = fast_exp2(sa[4 * j + i] * a.c2 - L[i]);
          sa[4 * j + i] = p;
          pa[4 * j + i] = p * (pa[4 * j + i] - Dl[i]);
        }
      }
      if constexpr (kCausal) {
        if (qt == qt0) {   // wave-uniform
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool above = 8 * (r >> 2) + 4 * hh + (r & 3) < l32;
            if (above) sa[r] = 0.f;
            if (above) pa[r] = 0.f;
          }
          if (qt0 == 0 && hh == 0) pa[0] = 0.f;   // query 0
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const uint4 pf = acc_frag<TI>(sa, s2), df = acc_frag<TI>(pa, s2);
        const int r0 = qt * 32 + 16 * s2 + 4 * hh;
        dv0 = M::mma(tr_chunk(gimg, r0, g16, lane), pf, dv0);
        dv1 = M::mma(tr_chunk(gimg, r0, 32 + g16, lane), pf, dv1);
        dk0 = M::mma(tr_chunk(qimg, r0, g16, lane), df, dk0);
        dk1 = M::mma(tr_chunk(qimg, r0, 32 + g16, lane), df, dk1);
      }
    }
    if constexpr (kMask) {
      if (kw != 0xFFFFFFFFu && !((kw >> l32) & 1u)) dk0 = dk1 = dv0 = dv1 = f32x16{};
    }
    const int64_t doff = (int64_t)b * a.d_bs + (int64_t)h * a.d_hs;
    store_rows<TI>(reinterpret_cast<TI*>(a.dk) + doff, a.d_ns, kt * 32 + l32, N, lane, dk0, dk1, a.scale,
                   a.dsum ? csl + (1 * kBwdWaves + wave) * kD : nullptr);
    store_rows<TI>(reinterpret_cast<TI*>(a.dv) + doff, a.d_ns, kt * 32 + l32, N, lane, dv0, dv1, 1.f,
                   a.dsum ? csl + (2 * kBwdWaves + wave) * kD : nullptr);
  }

  // ---- phase 2: wave = query block; dQ^T += K^T dS^T over the key tiles (forward orientation)
  const int qt = wave, q = qt * 32 + l32;
  uint4 qf[4], gf[4];
  float L = 0.f, Dl = 0.f;
  if (wave < NT) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = row_chunk(qimg, q, 2 * s + hh);
      gf[s] = row_chunk(gimg, q, 2 * s + hh);
    }
    L = lse2[q];
    Dl = dlt[q];
  }
  if constexpr (kPersist) {   // q / dO images and the row constants are free: stream the next head's
    __syncthreads();
    if (bh + (int)gridDim.x < total) dma_qgo(bh + gridDim.x);
  }
  if (wave < NT) {
    f32x16 dq0 = {}, dq1 = {};
    int ktEnd = NT;   // kCausal: the key tiles up to the diagonal one
    if constexpr (kCausal) ktEnd = __builtin_amdgcn_readfirstlane(qt) + 1;
#pragma unroll 1
    for (int kt = 0; kt < ktEnd; ++kt) {
      uint32_t w = 0;
      if constexpr (kMask) {
        w = word_of(wv, kt);
        if (w == 0) continue;   // no valid key in the tile: dS = 0
      }
      f32x16 sa = {}, pa = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = M::mma(row_chunk(kimg, kt * 32 + l32, 2 * s + hh), qf[s], sa);
        pa = M::mma(row_chunk(vimg, kt * 32 + l32, 2 * s + hh), gf[s], pa);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fast_exp2(sa[r] * a.c2 - L);
        pa[r] = p * (pa[r] - Dl);
      }
      if constexpr (kMask) {
        if (w != 0xFFFFFFFFu) {   // keys on the accumulator rows, as in the forward
          const uint32_t wl = w >> (4 * hh);
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (!row_bit(wl, r)) pa[r] = 0.f;
        }
      }
      if constexpr (kCausal) {
        if (kt == ktEnd - 1) {   // diagonal tile: keys on the accumulator rows; query 0 has dS = 0
          const bool q0 = q == 0;
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((r & 3) + 8 * (r >> 2) + 4 * hh > l32 || q0) pa[r] = 0.f;
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const uint4 df = acc_frag<TI>(pa, s2);
        const int r0 = kt * 32 + 16 * s2 + 4 * hh;
        dq0 = M::mma(tr_chunk(kimg, r0, g16, lane), df, dq0);
        dq1 = M::mma(tr_chunk(kimg, r0, 32 + g16, lane), df, dq1);
      }
    }
    const int64_t doff = (int64_t)b * a.d_bs + (int64_t)h * a.d_hs;
    store_rows<TI>(reinterpret_cast<TI*>(a.dq) + doff, a.d_ns, q, N, lane, dq0, dq1, a.scale,
                   a.dsum ? csl + wave * kD : nullptr);
  }
  if (a.dsum) {   // per-(batch, head) column sums, tiles in fixed order (deterministic)
    __syncthreads();
    if (tid < 3 * kD) {
      const int o = tid / kD, d = tid % kD;
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < NT; ++w) acc += csl[(o * kBwdWaves + w) * kD + d];
      a.dsum[(((int64_t)b * 3 + o) * a.H + h) * kD + d] = acc;
    }
  }
  __syncthreads();   // images, row constants and column sums are reused by the next head
  }
}

size_t fwd_lds(int NT) { return (size_t)2 * NT * 32 * kRowB; }
size_t bwd_lds(int NT) {
  return (size_t)(NT <= 7 ? 5 : 4) * NT * 32 * kRowB + (size_t)2 * NT * 32 * 4 + (size_t)3 * kBwdWaves * kD * 4;
}
static int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// A = FwdArgs / BwdArgs: the unmasked kernels, or with kCausal the causal ones; A = FwdArgsM /
// BwdArgsM: the kMask instantiations
template <typename TI, int NT, bool kCausal, typename A>
void launch_fwd_nt(const A& a, hipStream_t s) {
  constexpr bool kMask = std::is_same<A, FwdArgsM>::value;
  hipLaunchKernelGGL((attn_fwd_kernel<TI, NT, kMask, kCausal>), dim3(a.B * a.H), dim3(64 * kFwdWaves), fwd_lds(NT), s, a);
}
template <typename TI, int NT, bool kCausal, typename A>
void launch_bwd_nt(const A& a, hipStream_t s) {
  constexpr bool kMask = std::is_same<A, BwdArgsM>::value;
  // NT <= 7: persistent, one workgroup per CU walks the heads (the LDS of one head fills the CU)
  const int grid = NT <= 7 ? std::min(a.B * a.H, num_cus()) : a.B * a.H;
  hipLaunchKernelGGL((attn_bwd_kernel<TI, NT, kMask, kCausal>), dim3(grid), dim3(64 * kBwdWaves), bwd_lds(NT), s, a);
}
template <typename TI, bool kCausal, typename A>
void launch_fwd(const A& a, hipStream_t s) {
  switch ((a.N + 31) / 32) {
    case 1: launch_fwd_nt<TI, 1, kCausal>(a, s); break;
    case 2: launch_fwd_nt<TI, 2, kCausal>(a, s); break;
    case 3: launch_fwd_nt<TI, 3, kCausal>(a, s); break;
    case 4: launch_fwd_nt<TI, 4, kCausal>(a, s); break;
    case 5: launch_fwd_nt<TI, 5, kCausal>(a, s); break;
    case 6: launch_fwd_nt<TI, 6, kCausal>(a, s); break;
    case 7: launch_fwd_nt<TI, 7, kCausal>(a, s); break;
    default: launch_fwd_nt<TI, 8, kCausal>(a, s); break;
  }
}
template <typename TI, bool kCausal, typename A>
void launch_bwd(const A& a, hipStream_t s) {
  switch ((a.N + 31) / 32) {
    case 1: launch_bwd_nt<TI, 1, kCausal>(a, s); break;
    case 2: launch_bwd_nt<TI, 2, kCausal>(a, s); break;
    case 3: launch_bwd_nt<TI, 3, kCausal>(a, s); break;
    case 4: launch_bwd_nt<TI, 4, kCausal>(a, s); break;
    case 5: launch_bwd_nt<TI, 5, kCausal>(a, s); break;
    case 6: launch_bwd_nt<TI, 6, kCausal>(a, s); break;
    case 7: launch_bwd_nt<TI, 7, kCausal>(a, s); break;
    default: launch_bwd_nt<TI, 8, kCausal>(a, s); break;
  }
}

static bool rows_ok(const void* p, int64_t bs, int64_t ns, int64_t hs) {
  return p && aligned16(p) && bs % 8 == 0 && ns % 8 == 0 && hs % 8 == 0;
}
static int check_common(int B, int H, int N, int D, int dtype, const char* who) {
  MC_CHECK(B >= 0 && H > 0, MC_ERR_SHAPE, "%s: bad batch / heads (%d, %d)", who, B, H);
  MC_CHECK(D == MC_ATTN_HEAD_DIM, MC_ERR_SHAPE, "%s: head_dim %d (only %d is built)", who, D, MC_ATTN_HEAD_DIM);
  MC_CHECK(N >= 1 && N <= MC_ATTN_MAX_SEQ, MC_ERR_SHAPE, "%s: seqlen %d outside [1, %d]", who, N, MC_ATTN_MAX_SEQ);
  MC_CHECK(dtype == MC_DTYPE_BF16 || dtype == MC_DTYPE_F16, MC_ERR_DTYPE, "%s: dtype %d (bf16 / f16 only)", who, dtype);
  return MC_OK;
}
// The kernels address K / V (every kernel) and, in the N > 224 backward, Q / dO / O through 32-bit
// buffer byte offsets n * ns * sizeof(T) under a range of ((N - 1) * ns + 64) * sizeof(T) bytes, with
// offset 0x80000000 as the "reads zero" row past N: beyond 2^31 bytes the offsets wrap and the
// sentinel falls inside the range.  N and the dtype (16-bit) are already validated.
static int check_token_stride(int64_t ns, int N, const char* who, const char* name) {
  const int64_t es = 2;   // bf16 / f16
  MC_CHECK(ns >= 0 && ns <= INT64_MAX / (2 * MC_ATTN_MAX_SEQ) && ((int64_t)(N - 1) * ns + kD) * es <= ((int64_t)1 << 31),
           MC_ERR_SHAPE, "%s: token stride %s = %lld: negative, or ((seqlen - 1) * %s + %d) * %d bytes exceed 2^31 (32-bit buffer offsets)",
           who, name, (long long)ns, name, kD, (int)es);
  return MC_OK;
}

}  // namespace attn
}  // namespace mc

using namespace mc;

// Shared by the unmasked, the masked and the causal entry points (P: the parameter struct, A: FwdArgs[M] / BwdArgs[M])
template <bool kCausal = false, typename P, typename A>
static int run_fwd(const P* p, A& a, void* stream, const char* who) {
  MC_CHECK(p, MC_ERR_INVALID, "%s: null params", who);
  const int rc = attn::check_common(p->batch, p->heads, p->seqlen, p->head_dim, p->dtype, who);
  if (rc != MC_OK) return rc;
  MC_CHECK(attn::rows_ok(p->q, p->q_bs, p->q_ns, p->q_hs) && attn::rows_ok(p->k, p->q_bs, p->q_ns, p->q_hs) &&
               attn::rows_ok(p->v, p->q_bs, p->q_ns, p->q_hs) && attn::rows_ok(p->o, p->o_bs, p->o_ns, p->o_hs) && p->lse,
           MC_ERR_INVALID, "%s: q / k / v / o need 16-B aligned rows (strides %% 8 elements), lse non-null", who);
  if (const int rs = attn::check_token_stride(p->q_ns, p->seqlen, who, "q_ns"); rs != MC_OK) return rs;
  if constexpr (std::is_same<A, attn::FwdArgsM>::value) {
    MC_CHECK(p->key_mask && ((uintptr_t)p->key_mask & 3) == 0, MC_ERR_INVALID, "%s: key_mask null or not 4-B aligned", who);
    a.mask = p->key_mask;
  }
  if (p->batch == 0) return MC_OK;
  a.B = p->batch; a.H = p->heads; a.N = p->seqlen;
  a.scale = p->scale; a.c2 = p->scale * kLog2e;
  a.q = p->q; a.k = p->k; a.v = p->v;
  a.q_bs = p->q_bs; a.q_ns = p->q_ns; a.q_hs = p->q_hs;
  a.o = p->o; a.o_bs = p->o_bs; a.o_ns = p->o_ns; a.o_hs = p->o_hs;
  a.lse = p->lse;
  if (p->dtype == MC_DTYPE_BF16) attn::launch_fwd<bf16_t, kCausal>(a, (hipStream_t)stream);
  else attn::launch_fwd<f16_t, kCausal>(a, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  MC_CHECK(e == hipSuccess, MC_ERR_LAUNCH, "%s: launch failed: %s", who, hipGetErrorString(e));
  return MC_OK;
}

template <bool kCausal = false, typename P, typename A>
static int run_bwd(const P* p, A& a, void* stream, const char* who) {
  MC_CHECK(p, MC_ERR_INVALID, "%s: null params", who);
  const int rc = attn::check_common(p->batch, p->heads, p->seqlen, p->head_dim, p->dtype, who);
  if (rc != MC_OK) return rc;
  MC_CHECK(attn::rows_ok(p->q, p->q_bs, p->q_ns, p->q_hs) && attn::rows_ok(p->k, p->q_bs, p->q_ns, p->q_hs) &&
               attn::rows_ok(p->v, p->q_bs, p->q_ns, p->q_hs) && attn::rows_ok(p->o, p->o_bs, p->o_ns, p->o_hs) &&
               attn::rows_ok(p->dout, p->o_bs, p->o_ns, p->o_hs) && attn::rows_ok(p->dq, p->dq_bs, p->dq_ns, p->dq_hs) &&
               attn::rows_ok(p->dk, p->dq_bs, p->dq_ns, p->dq_hs) && attn::rows_ok(p->dv, p->dq_bs, p->dq_ns, p->dq_hs) &&
               p->lse,
           MC_ERR_INVALID, "%s: every tensor needs 16-B aligned rows (strides %% 8 elements), lse non-null", who);
  if (const int rs = attn::check_token_stride(p->q_ns, p->seqlen, who, "q_ns"); rs != MC_OK) return rs;
  if (const int rs = attn::check_token_stride(p->o_ns, p->seqlen, who, "o_ns"); rs != MC_OK) return rs;
  if constexpr (std::is_same<A, attn::BwdArgsM>::value) {
    MC_CHECK(p->key_mask && ((uintptr_t)p->key_mask & 3) == 0, MC_ERR_INVALID, "%s: key_mask null or not 4-B aligned", who);
    a.mask = p->key_mask;
  }
  if (p->batch == 0) return MC_OK;
  a.B = p->batch; a.H = p->heads; a.N = p->seqlen;
  a.scale = p->scale; a.c2 = p->scale * kLog2e;
  a.q = p->q; a.k = p->k; a.v = p->v;
  a.q_bs = p->q_bs; a.q_ns = p->q_ns; a.q_hs = p->q_hs;
  a.o = p->o; a.g = p->dout; a.o_bs = p->o_bs; a.o_ns = p->o_ns; a.o_hs = p->o_hs;
  a.lse = p->lse;
  a.dq = p->dq; a.dk = p->dk; a.dv = p->dv;
  a.d_bs = p->dq_bs; a.d_ns = p->dq_ns; a.d_hs = p->dq_hs;
  a.dsum = p->dsum;
  if (p->dtype == MC_DTYPE_BF16) attn::launch_bwd<bf16_t, kCausal>(a, (hipStream_t)stream);
  else attn::launch_bwd<f16_t, kCausal>(a, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  MC_CHECK(e == hipSuccess, MC_ERR_LAUNCH, "%s: launch failed: %s", who, hipGetErrorString(e));
  return MC_OK;
}

extern "C" int mc_attn_fwd(const mc_attn_fwd_params* p, void* stream) {
  attn::FwdArgs a;
  return run_fwd(p, a, stream, "mc_attn_fwd");
}
extern "C" int mc_attn_bwd(const mc_attn_bwd_params* p, void* stream) {
  attn::BwdArgs a;
  return run_bwd(p, a, stream, "mc_attn_bwd");
}
extern "C" int mc_attn_masked_fwd(const mc_attn_masked_fwd_params* p, void* stream) {
  attn::FwdArgsM a;
  return run_fwd(p, a, stream, "mc_attn_masked_fwd");
}
extern "C" int mc_attn_masked_bwd(const mc_attn_masked_bwd_params* p, void* stream) {
  attn::BwdArgsM a;
  return run_bwd(p, a, stream, "mc_attn_masked_bwd");
}
extern "C" int mc_attn_causal_fwd(const mc_attn_fwd_params* p, void* stream) {
  attn::FwdArgs a;
  return run_fwd<true>(p, a, stream, "mc_attn_causal_fwd");
}
extern "C" int mc_attn_causal_bwd(const mc_attn_bwd_params* p, void* stream) {
  attn::BwdArgs a;
  return run_bwd<true>(p, a, stream, "mc_attn_causal_bwd");
}
