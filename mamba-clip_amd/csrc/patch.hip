// patch.hip -- the image input path of the towers' patch embedding (include/mc_ops.h:
// mc_patch_embed_input), gfx950.
//
// Reference: the ISIC dataset's images go through timm / open_clip transforms (resize, crop,
// ToTensor, Normalize(mean, std): src/mamba_clip/data.py get_transform 37-108, IsicChallengeDataset
// 242-386) into a float NCHW batch, then the visual tower's patch-embed conv (k = s = P).  Here the
// last two host-side steps and the conv's input reshuffle are one device pass:
//   patches[(b * ph + i) * pw + j, (c * P + ky) * P + kx] = scale[c] * img(b, c, i*P + ky, j*P + kx) + shift[c]
// from either a float NCHW batch (scale / shift nullable: a plain im2col + cast) or the raw decoded
// uint8 NHWC images (scale = 1 / (255 std), shift = -mean / std: ToTensor + Normalize).
// One thread writes 4 consecutive patch columns (kx .. kx+3 of one (c, ky)): 4 contiguous input
// pixels, one 8-B (16-bit) / 16-B (fp32) store; consecutive threads walk the patch row in memory order.
#include "mc_common.h"
#include "../../include/mc_ops.h"

namespace mc {
namespace patch {

template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 load4<bf16_t>(const bf16_t* p) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  return f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
               __uint_as_float(w.y & 0xffff0000u)};
}
template <> __device__ __forceinline__ f32x4 load4<f16_t>(const f16_t* p) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  return f32x4{(float)__builtin_bit_cast(f16_t, (uint16_t)(w.x & 0xffffu)), (float)__builtin_bit_cast(f16_t, (uint16_t)(w.x >> 16)),
               (float)__builtin_bit_cast(f16_t, (uint16_t)(w.y & 0xffffu)), (float)__builtin_bit_cast(f16_t, (uint16_t)(w.y >> 16))};
}
template <typename T> __device__ __forceinline__ void store4(T* p, f32x4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, f32x4 v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(cvt_pk2<bf16_t>(v.x, v.y), cvt_pk2<bf16_t>(v.z, v.w));
}
template <> __device__ __forceinline__ void store4<f16_t>(f16_t* p, f32x4 v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(cvt_pk2<f16_t>(v.x, v.y), cvt_pk2<f16_t>(v.z, v.w));
}

struct Args {
  int batch, C, H, W, P, ph, pw;
  const void* img;
  const float* scale;
  const float* shift;
  void* out;
  const int32_t* keep;   // gather form: (batch, n_keep) patch indices, else null
  int n_keep;            // output rows per image (ph * pw without keep)
};

// Output row prow -> (image b, patch row i, patch column j).  The gather form reads the patch index
// from keep and clamps it into [0, ph * pw), so no index value addresses outside image b.
template <bool kGather>
__device__ __forceinline__ void patch_of_row(const Args& a, int64_t prow, int& b, int& i, int& j) {
  if constexpr (kGather) {
    b = (int)(prow / a.n_keep);
    const int idx = min(max(a.keep[prow], 0), a.ph * a.pw - 1);
    i = idx / a.pw;
    j = idx - i * a.pw;
  } else {
    j = (int)(prow % a.pw), i = (int)((prow / a.pw) % a.ph), b = (int)(prow / ((int64_t)a.pw * a.ph));
  }
}

// float NCHW input: unit = (patch row, c, ky, kx / 4)
template <typename TI, typename TO, bool kGather>
__global__ __launch_bounds__(256) void patch_nchw_kernel(const Args a) {
  const int q = a.P / 4;                        // 4-column groups per patch row
  const int per_row = a.C * a.P * q;            // units per patch row
  const int64_t total = (int64_t)a.batch * a.n_keep * per_row;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prow = u / per_row;
    const int r = (int)(u - prow * per_row);
    const int g = r % q, ky = (r / q) % a.P, c = r / (q * a.P);
    int b, i, j;
    patch_of_row<kGather>(a, prow, b, i, j);
    const TI* src = reinterpret_cast<const TI*>(a.img) + (((int64_t)b * a.C + c) * a.H + i * a.P + ky) * a.W + j * a.P + 4 * g;
    f32x4 v = load4<TI>(src);
    if (a.scale) v = v * a.scale[c] + a.shift[c];
    store4<TO>(reinterpret_cast<TO*>(a.out) + prow * (int64_t)a.C * a.P * a.P + ((int64_t)c * a.P + ky) * a.P + 4 * g, v);
  }
}

// uint8 NHWC input (decoded images): unit = (patch row, ky, kx / 4); 4 pixels x C bytes in, C stores out
template <typename TO, int C, bool kGather>
__global__ __launch_bounds__(256) void patch_nhwc_u8_kernel(const Args a) {
  const int q = a.P / 4;
  const int per_row = a.P * q;
  const int64_t total = (int64_t)a.batch * a.n_keep * per_row;
  float sc[C], sh[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    sc[c] = a.scale ? a.scale[c] : 1.f;
    sh[c] = a.scale ? a.shift[c] : 0.f;
  }
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prow = u / per_row;
    const int r = (int)(u - prow * per_row);
    const int g = r % q, ky = r / q;
    int b, i, j;
    patch_of_row<kGather>(a, prow, b, i, j);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(a.img) +
                         ((((int64_t)b * a.H + i * a.P + ky) * a.W + j * a.P + 4 * g) * C);
    uint8_t px[4 * C];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) px[k] = src[k];   // 4 * C contiguous bytes (12 for RGB)
    TO* dst = reinterpret_cast<TO*>(a.out) + prow * (int64_t)C * a.P * a.P + (int64_t)ky * a.P + 4 * g;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 v = f32x4{(float)px[c], (float)px[C + c], (float)px[2 * C + c], (float)px[3 * C + c]} * sc[c] + sh[c];
      store4<TO>(dst + (int64_t)c * a.P * a.P, v);
    }
  }
}

template <typename TI, bool kGather>
static void launch_nchw(int otype, const Args& a, dim3 grid, hipStream_t s) {
  if (otype == MC_DTYPE_F32) hipLaunchKernelGGL((patch_nchw_kernel<TI, float, kGather>), grid, dim3(256), 0, s, a);
  else if (otype == MC_DTYPE_BF16) hipLaunchKernelGGL((patch_nchw_kernel<TI, bf16_t, kGather>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((patch_nchw_kernel<TI, f16_t, kGather>), grid, dim3(256), 0, s, a);
}
template <int C, bool kGather>
static void launch_u8(int otype, const Args& a, dim3 grid, hipStream_t s) {
  if (otype == MC_DTYPE_F32) hipLaunchKernelGGL((patch_nhwc_u8_kernel<float, C, kGather>), grid, dim3(256), 0, s, a);
  else if (otype == MC_DTYPE_BF16) hipLaunchKernelGGL((patch_nhwc_u8_kernel<bf16_t, C, kGather>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((patch_nhwc_u8_kernel<f16_t, C, kGather>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------- token embedding over kept patches
// Patch dropout (open_clip PatchDropout, exclude_first_token): the tower runs on the class token and
// n_keep of the n patches per image.  One thread moves one 16-B vector of a token row.
template <typename T> __device__ __forceinline__ float rnd(float v) { return to_f(from_f<T>(v)); }

// kVec fp32 values at p (16-B aligned)
template <int N> __device__ __forceinline__ void ld_f32(const float* __restrict__ p, float (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; k += 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + k);
    v[k] = q.x, v[k + 1] = q.y, v[k + 2] = q.z, v[k + 3] = q.w;
  }
}

// out[b, 0] = rnd(rnd(cls) + rnd(pos[0]));  out[b, 1 + s] = rnd(x[b, s] + rnd(pos[1 + keep[b, s]])):
// the bits of cat([cls.to(dt), x], 1) + pos.to(dt) on the kept rows (rnd = round to T, adds in fp32)
template <typename T>
__global__ __launch_bounds__(256) void token_embed_gather_fwd_kernel(int batch, int n, int n_keep, int cols,
                                                                     const float* __restrict__ cls,
                                                                     const T* __restrict__ x, const float* __restrict__ pos,
                                                                     const int32_t* __restrict__ keep, T* __restrict__ out) {
  constexpr int V = ElemTraits<T>::kVec;
  const int cpr = cols / V;                      // vectors per row
  const int64_t total = (int64_t)batch * (n_keep + 1) * cpr;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = u / cpr;                 // b * (n_keep + 1) + s
    const int c0 = (int)(u - row * cpr) * V;
    const int64_t b = row / (n_keep + 1);
    const int s = (int)(row - b * (n_keep + 1));
    float a[V], p[V];
    if (s == 0) {
      ld_f32<V>(cls + c0, a);
      ld_f32<V>(pos + c0, p);
#pragma unroll
      for (int k = 0; k < V; ++k) a[k] = rnd<T>(a[k]);
    } else {
      const int64_t xr = b * n_keep + (s - 1);
      const int idx = min(max(keep[xr], 0), n - 1);   // clamped: no index value reads outside the table
      const uint4 q = ld16(x + xr * cols + c0);
      ld_f32<V>(pos + (int64_t)(1 + idx) * cols + c0, p);
#pragma unroll
      for (int k = 0; k < V; ++k) a[k] = elem_f<T>(q, k);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) a[k] += rnd<T>(p[k]);
    st16(out + row * cols + c0, pack_f<T>(a));
  }
}

// dpos[0] = sum_b dm[b, 0];  dpos[1 + j] = sum over the samples b that kept patch j of dm[b, 1 + slot[b, j]].
// One thread owns one 16-B column group of one table row and adds the samples in the order b = 0, 1, ...
// (fp32, no atomics); kU rows of dm are in flight per thread.  A position nobody kept gets its zeros here.
template <typename T>
__global__ __launch_bounds__(256) void token_embed_gather_bwd_kernel(int batch, int n, int n_keep, int cols,
                                                                     const T* __restrict__ dm,
                                                                     const int32_t* __restrict__ slot,
                                                                     float* __restrict__ dpos) {
  constexpr int V = ElemTraits<T>::kVec, kU = 8;
  const int cpr = cols / V;
  const int total = (n + 1) * cpr;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= total) return;
  const int r = u / cpr, c0 = (u - r * cpr) * V;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  for (int b0 = 0; b0 < batch; b0 += kU) {
    uint4 q[kU];
#pragma unroll
    for (int i = 0; i < kU; ++i) {
      const int b = b0 + i;
      q[i] = make_uint4(0u, 0u, 0u, 0u);         // + 0.0 leaves the sum as it is
      if (b < batch) {
        const int sl = r == 0 ? 0 : slot[(int64_t)b * n + (r - 1)];
        if (r == 0 || (sl >= 0 && sl < n_keep))  // anything else: sample b dropped this patch
          q[i] = ld16(dm + ((int64_t)b * (n_keep + 1) + (r == 0 ? 0 : 1 + sl)) * cols + c0);
      }
    }
#pragma unroll
    for (int i = 0; i < kU; ++i) {
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += elem_f<T>(q[i], k);
    }
  }
  float* o = dpos + (int64_t)r * cols + c0;
#pragma unroll
  for (int k = 0; k < V; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
}

}  // namespace patch
}  // namespace mc

using namespace mc;

// mc_patch_embed_input (keep == nullptr: every patch, n_keep = ph * pw) and its gather form
static int patch_input(const char* who, const mc_patch_input_params* p, bool gather, const int32_t* keep,
                       int32_t n_keep, void* stream) {
  MC_CHECK(p != nullptr, MC_ERR_INVALID, "%s: null params", who);
  MC_CHECK(p->batch >= 0 && p->channels > 0 && p->patch > 0 && p->patch % 4 == 0 && p->height % p->patch == 0 &&
               p->width % p->patch == 0,
           MC_ERR_SHAPE, "%s: patch must be a multiple of 4 dividing H and W (got P %d, %dx%d)", who, p->patch,
           p->height, p->width);
  const bool u8 = p->in_dtype == MC_DTYPE_U8;
  MC_CHECK(u8 ? p->layout == MC_LAYOUT_NHWC : p->layout == MC_LAYOUT_NCHW, MC_ERR_DTYPE,
           "%s: uint8 input is NHWC (decoded images), float input NCHW", who);
  MC_CHECK(u8 || p->in_dtype == MC_DTYPE_F32 || p->in_dtype == MC_DTYPE_BF16 || p->in_dtype == MC_DTYPE_F16,
           MC_ERR_DTYPE, "%s: bad input dtype %d", who, p->in_dtype);
  MC_CHECK(p->out_dtype == MC_DTYPE_F32 || p->out_dtype == MC_DTYPE_BF16 || p->out_dtype == MC_DTYPE_F16,
           MC_ERR_DTYPE, "%s: bad output dtype %d", who, p->out_dtype);
  MC_CHECK(!u8 || p->channels == 3 || p->channels == 1, MC_ERR_SHAPE, "%s: uint8 input has 1 or 3 channels", who);
  patch::Args a;
  a.batch = p->batch; a.C = p->channels; a.H = p->height; a.W = p->width; a.P = p->patch;
  a.ph = a.H / a.P; a.pw = a.W / a.P;
  MC_CHECK(!gather || (n_keep >= 1 && (int64_t)n_keep <= (int64_t)a.ph * a.pw), MC_ERR_SHAPE,
           "%s: n_keep %d outside [1, %lld patches]", who, n_keep, (long long)a.ph * a.pw);
  MC_CHECK((int64_t)a.ph * a.pw <= INT32_MAX, MC_ERR_SHAPE, "%s: too many patches per image", who);
  if (p->batch == 0) return MC_OK;   // empty batch: nothing to read, pointers may be null
  MC_CHECK(p->img && p->out && (!p->scale) == (!p->shift), MC_ERR_INVALID,
           "%s: img / out non-null; scale and shift both given or both null", who);
  MC_CHECK(!gather || (keep && reinterpret_cast<uintptr_t>(keep) % 4 == 0), MC_ERR_INVALID,
           "%s: keep must be a 4-B aligned (batch, n_keep) int32 table", who);
  const int ib = p->in_dtype == MC_DTYPE_F32 ? 16 : 8;
  MC_CHECK(u8 || ((reinterpret_cast<uintptr_t>(p->img) % ib) == 0), MC_ERR_INVALID, "%s: misaligned image", who);
  MC_CHECK((reinterpret_cast<uintptr_t>(p->out) % (p->out_dtype == MC_DTYPE_F32 ? 16 : 8)) == 0, MC_ERR_INVALID,
           "%s: misaligned output", who);
  a.img = p->img; a.scale = p->scale; a.shift = p->shift; a.out = p->out;
  a.keep = gather ? keep : nullptr;
  a.n_keep = gather ? n_keep : a.ph * a.pw;
  const int64_t units = (int64_t)a.batch * a.n_keep * (u8 ? 1 : a.C) * a.P * (a.P / 4);
  const dim3 grid((unsigned)std::min<int64_t>((units + 255) / 256, 65536));
  hipStream_t s = (hipStream_t)stream;
#define MC_PATCH_LAUNCH(G)                                                                       \
  do {                                                                                           \
    if (u8) {                                                                                    \
      if (a.C == 3) patch::launch_u8<3, G>(p->out_dtype, a, grid, s);                            \
      else patch::launch_u8<1, G>(p->out_dtype, a, grid, s);                                     \
    } else if (p->in_dtype == MC_DTYPE_F32) patch::launch_nchw<float, G>(p->out_dtype, a, grid, s);   \
    else if (p->in_dtype == MC_DTYPE_BF16) patch::launch_nchw<bf16_t, G>(p->out_dtype, a, grid, s);   \
    else patch::launch_nchw<f16_t, G>(p->out_dtype, a, grid, s);                                 \
  } while (0)
  if (gather) MC_PATCH_LAUNCH(true);
  else MC_PATCH_LAUNCH(false);
#undef MC_PATCH_LAUNCH
  return check_launch(who);
}

extern "C" int mc_patch_embed_input(const mc_patch_input_params* p, void* stream) {
  return patch_input("mc_patch_embed_input", p, false, nullptr, 0, stream);
}

extern "C" int mc_patch_embed_input_gather(const mc_patch_input_params* p, const int32_t* keep, int32_t n_keep,
                                           void* stream) {
  return patch_input("mc_patch_embed_input_gather", p, true, keep, n_keep, stream);
}

// the shape and dtype checks both token-embedding entry points share
static int token_embed_check(const char* who, const mc_token_embed_gather_params* p) {
  MC_CHECK(p != nullptr, MC_ERR_INVALID, "%s: null params", who);
  MC_CHECK(p->dtype == MC_DTYPE_F32 || p->dtype == MC_DTYPE_BF16 || p->dtype == MC_DTYPE_F16, MC_ERR_DTYPE,
           "%s: bad dtype %d", who, p->dtype);
  MC_CHECK(p->batch >= 0 && p->n >= 1 && p->n_keep >= 1 && p->n_keep <= p->n && p->cols >= 1, MC_ERR_SHAPE,
           "%s: bad shape (batch %d, n %d, n_keep %d, cols %d)", who, p->batch, p->n, p->n_keep, p->cols);
  const int V = p->dtype == MC_DTYPE_F32 ? 4 : 8;
  MC_CHECK(p->cols % V == 0, MC_ERR_SHAPE, "%s: cols %d is not a multiple of %d (16-B vectors)", who, p->cols, V);
  MC_CHECK((int64_t)(p->n + 1) * (p->cols / V) <= INT32_MAX, MC_ERR_SHAPE, "%s: position table too large", who);
  return MC_OK;
}

extern "C" int mc_token_embed_gather_fwd(const mc_token_embed_gather_params* p, void* stream) {
  static const char* who = "mc_token_embed_gather_fwd";
  MC_TRY(token_embed_check(who, p));
  if (p->batch == 0) return MC_OK;   // empty batch: nothing to write, pointers may be null
  MC_CHECK(p->cls && p->pos && p->x && p->keep && p->out, MC_ERR_INVALID, "%s: null cls / pos / x / keep / out", who);
  MC_CHECK(aligned16(p->cls) && aligned16(p->pos) && aligned16(p->x) && aligned16(p->out) &&
               reinterpret_cast<uintptr_t>(p->keep) % 4 == 0,
           MC_ERR_INVALID, "%s: cls / pos / x / out must be 16-B aligned, keep 4-B", who);
  const int V = p->dtype == MC_DTYPE_F32 ? 4 : 8;
  const int64_t units = (int64_t)p->batch * (p->n_keep + 1) * (p->cols / V);
  const dim3 grid((unsigned)std::min<int64_t>((units + 255) / 256, 65536));
  hipStream_t s = (hipStream_t)stream;
#define MC_TE_FWD(T)                                                                                              \
  hipLaunchKernelGGL((patch::token_embed_gather_fwd_kernel<T>), grid, dim3(256), 0, s, p->batch, p->n, p->n_keep, \
                     p->cols, p->cls, reinterpret_cast<const T*>(p->x), p->pos, p->keep, reinterpret_cast<T*>(p->out))
  if (p->dtype == MC_DTYPE_F32) MC_TE_FWD(float);
  else if (p->dtype == MC_DTYPE_BF16) MC_TE_FWD(bf16_t);
  else MC_TE_FWD(f16_t);
#undef MC_TE_FWD
  return check_launch(who);
}

extern "C" int mc_token_embed_gather_bwd(const mc_token_embed_gather_params* p, void* stream) {
  static const char* who = "mc_token_embed_gather_bwd";
  MC_TRY(token_embed_check(who, p));
  if (p->batch == 0) return MC_OK;   // empty batch: no sample to sum, pointers may be null (dpos is left alone)
  MC_CHECK(p->dm && p->slot && p->dpos, MC_ERR_INVALID, "%s: null dm / slot / dpos", who);
  MC_CHECK(aligned16(p->dm) && aligned16(p->dpos) && reinterpret_cast<uintptr_t>(p->slot) % 4 == 0, MC_ERR_INVALID,
           "%s: dm / dpos must be 16-B aligned, slot 4-B", who);
  const int V = p->dtype == MC_DTYPE_F32 ? 4 : 8;
  const dim3 grid((unsigned)(((int64_t)(p->n + 1) * (p->cols / V) + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
#define MC_TE_BWD(T)                                                                                              \
  hipLaunchKernelGGL((patch::token_embed_gather_bwd_kernel<T>), grid, dim3(256), 0, s, p->batch, p->n, p->n_keep, \
                     p->cols, reinterpret_cast<const T*>(p->dm), p->slot, p->dpos)
  if (p->dtype == MC_DTYPE_F32) MC_TE_BWD(float);
  else if (p->dtype == MC_DTYPE_BF16) MC_TE_BWD(bf16_t);
  else MC_TE_BWD(f16_t);
#undef MC_TE_BWD
  return check_launch(who);
}
