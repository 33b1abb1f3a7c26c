// scan_common.h -- pieces shared by the selective-scan forward and backward.
#pragma once

#include "mc_common.h"
#include "../../include/mc_scan.h"

namespace mc {
namespace scan {

constexpr int kT = 32;             // sequence positions per forward tile
constexpr int kS = MC_SCAN_CHUNK;  // positions per saved chunk state (32)
constexpr int kFineS = MC_SCAN_STATE_INTERVAL_FINE;   // the fine saved-state interval (8)
constexpr int kRows = 64;          // channels per workgroup: one wave

inline int padded_dstate(int dstate) { return dstate <= 8 ? 8 : (dstate <= 16 ? 16 : 32); }

// LDS hand-off between the lanes of a ONE-WAVE workgroup.  A wave's LDS
// instructions are performed in program order, so a compiler barrier is all
// the ordering a cross-lane exchange needs.  __syncthreads() would also lower
// to a vmcnt(0)/lgkmcnt(0) drain: every chunk would wait for the previous
// chunk's global stores and for prefetch loads still in flight (measured in
// the backward: ~2/3 of the wave's cycles sat in those drains).
static_assert(kRows == 64, "wave_lds_sync() is only valid for one-wave workgroups");
__device__ __forceinline__ void wave_lds_sync() { asm volatile("" ::: "memory"); }

// Workgroup barrier for LDS hand-offs only: this wave's LDS operations are
// complete, global loads / stores stay in flight (gfx950 has the back-off
// barrier, so s_barrier itself forces no vmcnt drain; __syncthreads()'s fence
// would wait for every prefetch still in flight).
__device__ __forceinline__ void lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Lane id the compiler cannot hoist or CSE (asm volatile): values derived from
// it are rebuilt where used instead of occupying VGPRs across a hot loop.
__device__ __forceinline__ int opaque_lane_id() {
  int v;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(v));
  return v;
}

// Packed (two positions) softplus and silu of the lane-pair kernels (scan_fwd_pair.hip, scan_bwd_pair.hip):
// the arithmetic around the transcendental ops runs as v_pk_* (one issue for two positions).
__device__ __forceinline__ f32x2 softplus2_log1p(f32x2 x) {
  // softplus(x) = max(x, 0) + log1p(exp(-|x|)): exp never overflows, and above 20 the log1p
  // term is below half an ulp of x, which is torch's threshold (x > 20 -> x) exactly.
  // -|arg| is a free VOP3 input modifier on v_exp_f32.
  const f32x2 arg = x * kLog2e;
  const f32x2 t = f32x2{fast_exp2(-fabsf(arg.x)), fast_exp2(-fabsf(arg.y))};
  const f32x2 tp = t + 1.f;
  const f32x2 lg = f32x2{fast_log2(tp.x), fast_log2(tp.y)};
  return lg * kLn2 + f32x2{fmaxf(x.x, 0.f), fmaxf(x.y, 0.f)};
}
__device__ __forceinline__ f32x2 silu2(f32x2 z) {
  const f32x2 arg = z * -kLog2e;
  const f32x2 ep = f32x2{fast_exp2(arg.x), fast_exp2(arg.y)} + 1.f;
  return z * f32x2{fast_rcp(ep.x), fast_rcp(ep.y)};
}

// a * {s.lo, s.lo} (kHi = 0) or a * {s.hi, s.hi} (kHi = 1).  kHi = 0 is one v_pk_mul_f32 with op_sel_hi only
// (the HIGH result reads s.lo; the compiler otherwise moves an odd-register scalar to an even register first).
// kHi = 1 is two scalar ops reading s.hi directly: the packed op_sel:[0,1] form (the LOW result reading a
// source's HIGH half), issued from inline asm, returned wrong low-half results on gfx950 for lanes 48-63 now
// and then while another kernel ran beside it (run-to-run differences of the two-stream training step,
// DESIGN 4.9), so it is not used.  Where one s.hi feeds several products, hi_to_lo() moves it to a low half
// once and the packed kHi = 0 form broadcasts it.
template <int kHi>
__device__ __forceinline__ f32x2 pk_mul_bcast(f32x2 a, f32x2 s) {
  if constexpr (kHi) {
    float x, y;
    asm("v_mul_f32 %0, %2, %4\n\tv_mul_f32 %1, %3, %4" : "=&v"(x), "=&v"(y) : "v"(a.x), "v"(a.y), "v"(s.y));
    return f32x2{x, y};
  } else {
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(s));
    return r;
  }
}
// a * s.{lo|hi} + c, in the same two forms
template <int kHi>
__device__ __forceinline__ f32x2 pk_fma_bcast(f32x2 a, f32x2 s, f32x2 c) {
  if constexpr (kHi) {
    float x, y;
    asm("v_fma_f32 %0, %2, %4, %5\n\tv_fma_f32 %1, %3, %4, %6" : "=&v"(x), "=&v"(y)
        : "v"(a.x), "v"(a.y), "v"(s.y), "v"(c.x), "v"(c.y));
    return f32x2{x, y};
  } else {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(s), "v"(c));
    return r;
  }
}
__device__ __forceinline__ f32x2 hi_to_lo(f32x2 s) {   // {s.hi, unspecified}: one v_mov, no op_sel
  f32x2 r = __builtin_nondeterministic_value(r);
  r.x = s.y;
  return r;
}

// Row staging of the pair backward (scan_bwd_pair.hip).  Per 32-position chunk a wave copies 32 rows x
// 64 B of one 16-bit array to LDS with two 64-lane LDS-DMA instructions of 16 B per lane: lane `lane`
// of instruction `i` takes row 16 i + lane / 4, 16-B piece lane % 4 (8 positions), and the hardware
// puts it at m0 + 16 lane, i.e. the block is [row][64 B].  The DMA checks no range, so a row past
// `nrows` (a wave without rows keeps its anchor row) and a piece past the sequence end are clamped to
// the last valid row / piece of the same array; what they fetch is never used.  Host-callable so that
// the offsets can be checked without a GPU.
constexpr int kStageRowBytes = kS * 2;                  // one staged row: 32 positions, 16 bit
constexpr int kStageInstrBytes = 64 * 16;               // one DMA instruction: 16 rows
constexpr int kStageArrayBytes = 32 * kStageRowBytes;   // one array of a wave
// element offset of the piece's source from the wave's first row (seqlen % 8 == 0, seqlen >= 8)
__host__ __device__ inline int64_t stage_src_elem(int lane, int i, int chunk, int nrows, int seqlen, int64_t row_stride) {
  const int last_row = nrows > 0 ? nrows - 1 : 0;
  const int row = 16 * i + (lane >> 2), pos = chunk * kS + 8 * (lane & 3);
  return (int64_t)(row < last_row ? row : last_row) * row_stride + (pos < seqlen - 8 ? pos : seqlen - 8);
}
// LDS byte of (row, chunk position) in a staged array, and where lane `lane` of instruction `i` lands
__host__ __device__ inline uint32_t stage_row_byte(int row, int pos) { return (uint32_t)(row * kStageRowBytes + pos * 2); }
__host__ __device__ inline uint32_t stage_dst_byte(int lane, int i) { return (uint32_t)(i * kStageInstrBytes + lane * 16); }

// Forward kernel arguments (scan_fwd.hip, scan_fwd_pair.hip).
struct FwdArgs {
  int batch, dim, seqlen, dstate, n_groups, n_chunks, n_states, nblk, total_blocks;
  int softplus;
  int64_t u_bs, u_ds, dt_bs, dt_ds, z_bs, z_ds, o_bs, o_ds;
  const void* u; const void* delta; const float* A; const float* bct;
  const float* D; const void* z; const float* delta_bias;
  void* out; float* chunk_states; float* last_state;
  void* out_y; int64_t y_bs, y_ds;   // nullable: pre-gate y + D u (training with z: the backward's dz input)
  int rev_groups, u_groups;          // grouped directions (0 = off; element-wise path only)
  // B / C rows as given (the pair kernel reads them directly; the others read the relaid bct)
  const void* B; const void* C;
  int64_t B_bs, B_gs, B_ns, C_bs, C_gs, C_ns;
  int state_interval;                // positions per saved state (pair kernel: 8 or 32; others 32)
};

// ---------------------------------------------------------------- host side
// Channels per workgroup and dstate of the lane-pair kernels (scan_fwd_pair.hip, scan_bwd_pair.hip): the
// plans size their 32-bit span checks, slabs and grids from these.
constexpr int kPCh = 32;          // forward: channels per (one-wave) workgroup
constexpr int kPN = 16;           // forward: dstate
constexpr int kQW = 4;            // backward: waves per workgroup
constexpr int kQCh = 32;          // backward: channels per wave
constexpr int kQN = 16;           // backward: dstate

// MC_DISPATCH_T / MC_DISPATCH_BOOL (mc_common.h) plus the scan's own axes: every launcher is one nested expression.
#define MC_DISPATCH_T16(dtype, ...)                                 \
  do {                                                              \
    if ((dtype) == MC_DTYPE_BF16) { using T = bf16_t; __VA_ARGS__; } \
    else { using T = f16_t; __VA_ARGS__; }                          \
  } while (0)

// padded dstate (8 / 16 / 32) as the compile-time constant kN
#define MC_DISPATCH_NP(np, ...)                               \
  do {                                                        \
    if ((np) == 8) { constexpr int kN = 8; __VA_ARGS__; }      \
    else if ((np) == 16) { constexpr int kN = 16; __VA_ARGS__; } \
    else { constexpr int kN = 32; __VA_ARGS__; }               \
  } while (0)

// the three row modes of scan_fwd_kernel (0 element-wise, 1 aligned, 2 aligned and whole chunks) as kAl
#define MC_DISPATCH_ALIGNED3(mode, ...)                        \
  do {                                                         \
    if ((mode) == 2) { constexpr int kAl = 2; __VA_ARGS__; }    \
    else if ((mode) == 1) { constexpr int kAl = 1; __VA_ARGS__; } \
    else { constexpr int kAl = 0; __VA_ARGS__; }                \
  } while (0)

int validate_common(int batch, int dim, int seqlen, int dstate, int n_groups, int itype, int wtype, const char* who);

inline int elem_bytes(int dtype) { return dtype == MC_DTYPE_F32 ? 4 : 2; }

// 16-B vector eligibility: pointer (null = absent, fine) aligned, strides in whole vectors
inline bool vec_ok(const void* p, int64_t s0, int64_t s1, int64_t s2, int eb) {
  const int64_t v = 16 / eb;
  return p == nullptr || (aligned16(p) && s0 % v == 0 && s1 % v == 0 && s2 % v == 0);
}

// A (batch, dim, seqlen) row tensor, seqlen stride 1; p null = absent (passes every check).
struct Rows {
  const void* p;
  int64_t bs, ds;
};
inline bool rows_vec_ok(const Rows& r, int eb) { return vec_ok(r.p, r.bs, r.ds, 0, eb); }
// a workgroup addresses its `rows` rows (plus `tail` positions past the first element of the last row)
// with 32-bit byte offsets
inline bool rows_span32(const Rows& r, int rows, int64_t tail, int eb) {
  return !r.p || ((int64_t)(rows - 1) * (r.ds < 0 ? -r.ds : r.ds) + tail) * eb < ((int64_t)1 << 31);
}
template <size_t kCount>
inline bool all_vec_ok(const Rows (&t)[kCount], int eb) {
  for (const Rows& r : t) if (!rows_vec_ok(r, eb)) return false;
  return true;
}
template <size_t kCount>
inline bool all_span32(const Rows (&t)[kCount], int rows, int64_t tail, int eb) {
  for (const Rows& r : t) if (!rows_span32(r, rows, tail, eb)) return false;
  return true;
}
// B / C as the pair kernels read them: 16-B aligned rows, strides in whole vectors, a group's dstate rows
// ascending and within 32-bit byte offsets
inline bool bc_rows_ok(const void* t, int64_t bs, int64_t gs, int64_t ns, int dstate, int seqlen, int eb) {
  return vec_ok(t, bs, gs, ns, eb) && ns >= 0 && ((int64_t)(dstate - 1) * ns + seqlen) * eb < ((int64_t)1 << 31);
}
// what both pair kernels ask of a call beyond its row tensors
template <typename Params>
inline bool pair_shape_ok(const Params* p, int dstate) {
  const int eb = elem_bytes(p->wtype);
  return elem_bytes(p->itype) == 2 && p->wtype == p->itype && p->dstate == dstate && p->seqlen % 8 == 0 &&
         p->reverse_groups == 0 && p->u_groups == 0 &&
         bc_rows_ok(p->B, p->B_batch_stride, p->B_group_stride, p->B_dstate_stride, dstate, p->seqlen, eb) &&
         bc_rows_ok(p->C, p->C_batch_stride, p->C_group_stride, p->C_dstate_stride, dstate, p->seqlen, eb);
}

inline bool has_dirs(int reverse_groups, int u_groups) { return reverse_groups != 0 || u_groups != 0; }
// grouped directions, vector modes: a mirrored 16-B block is aligned only when seqlen is whole vectors
inline bool dirs_vec_ok(bool dirs, int seqlen, int eb) { return !dirs || seqlen % (16 / eb) == 0; }

template <typename Params>
int check_dirs(const Params* p, const char* who) {
  if (!has_dirs(p->reverse_groups, p->u_groups)) return MC_OK;
  MC_CHECK(!p->z && p->u_groups >= 0 && p->u_groups <= p->n_groups && p->n_groups <= 31 &&
               (p->reverse_groups >> p->n_groups) == 0,
           MC_ERR_SHAPE, "%s: reverse_groups / u_groups need no z, 0 <= u_groups <= n_groups <= 31 and "
           "a mask within n_groups (got mask 0x%x, u_groups %d, n_groups %d)", who, p->reverse_groups, p->u_groups,
           p->n_groups);
  return MC_OK;
}

// The fields BwdArgs (scan_bwd.hip) and BwdPairArgs (scan_bwd_pair.hip) share, from validated params;
// `rows`: channels per workgroup of the kernel the args are for.
struct BwdSlabs {
  float* bc; float* a; float* d; float* bias;   // partial sums in the workspace (layouts: BwdArgs)
};
template <typename Args>
void fill_bwd_args(Args& a, const mc_scan_bwd_params* p, const BwdSlabs& w, int rows) {
  a.batch = p->batch; a.dim = p->dim; a.seqlen = p->seqlen; a.n_groups = p->n_groups;
  a.n_states = mc_scan_n_states(p->seqlen, p->state_interval);
  a.state_ratio = p->state_interval == kFineS ? kS / kFineS : 1;
  a.nblk = (p->dim / p->n_groups + rows - 1) / rows;
  a.total_blocks = p->batch * p->n_groups * a.nblk;
  a.u_bs = p->u_batch_stride; a.u_ds = p->u_dim_stride;
  a.dt_bs = p->delta_batch_stride; a.dt_ds = p->delta_dim_stride;
  a.z_bs = p->z_batch_stride; a.z_ds = p->z_dim_stride;
  a.go_bs = p->dout_batch_stride; a.go_ds = p->dout_dim_stride;
  a.du_bs = p->du_batch_stride; a.du_ds = p->du_dim_stride;
  a.ddt_bs = p->ddelta_batch_stride; a.ddt_ds = p->ddelta_dim_stride;
  a.dz_bs = p->dz_batch_stride; a.dz_ds = p->dz_dim_stride;
  a.u = p->u; a.delta = p->delta; a.z = p->z; a.dout = p->dout;
  a.A = p->A; a.D = p->D; a.delta_bias = p->delta_bias; a.chunk_states = p->chunk_states;
  a.du = p->du; a.ddelta = p->ddelta; a.dz = p->dz;
  a.slab_bc = w.bc; a.slab_a = w.a; a.slab_d = w.d; a.slab_bias = w.bias;
}

}  // namespace scan
}  // namespace mc
