// scan_bwd.hip -- selective-scan backward for MI355X (gfx950, CDNA4).
//
// Reverse-mode of the recurrence in scan_fwd.hip (reference semantics
// /root/reference/src/mamba_clip/model.py:83-169; the op behind
// selective_scan_cuda.bwd reached through mamba_ssm's SelectiveScanFn):
//   gy_t  = dout_t * silu(z_t)                  dz_t = dout_t * y_t * silu'(z_t)
//   h_t,n = C_t,n gy_t + a_{t+1,n} h_{t+1,n}     (adjoint of the state, a = exp(dt A))
//   dC_t,n = sum_d gy_t x_t,n        dB_t,n = sum_d h_t,n dt_t u_t
//   du_t  = D gy_t + sum_n h_t,n dt_t B_t,n
//   ddt_t = sum_n h_t,n (A_n a_t,n x_{t-1,n} + B_t,n u_t),  ddelta_t = ddt_t * sigmoid(delta_t + bias)
//   dA_n  = sum_{b,t} h_t,n dt_t a_t,n x_{t-1,n}    dD = sum gy u    dbias = sum ddelta
//   (y_t = sum_n C_t,n x_t,n + D u_t is recomputed here; the forward stores no pre-gate output)
//
// Design:
//  * A workgroup = TWO waves on the same 64 channels of one (batch, group).
//    The state pairs (n, n+1) are split between the waves (kN/4 pairs each),
//    so the rows and the B/C block staged in LDS serve both, and each wave's
//    per-pair state fits in registers.  2 waves/SIMD at 16-bit I/O.
//  * The sequence is walked in reverse in chunks of kTC = 32 positions -- the
//    forward's saved-state interval (MC_SCAN_CHUNK).  Each chunk's rows of
//    u / delta / z / dout are fetched with coalesced 16-B loads (whole 64-B
//    row segments per 4 lanes), prefetched into registers one chunk ahead,
//    and transposed through LDS (XOR-swizzled: conflict-free own-row reads).
//  * Inside a chunk, the states at the starts of its four 8-position
//    sub-tiles are recomputed from the saved chunk state (a forward sweep over
//    24 positions, kept in LDS), then the sub-tiles are processed in reverse:
//    per pair a forward sweep (x, a kept in VGPRs), the dC reduction, the
//    reverse adjoint sweep and the dB reduction (in-register transpose-reduce).
//  * Per-position sums over the pairs (S = sum h B, Q = sum h A a x, Y = sum C x)
//    are exchanged between the two waves through LDS; each wave finishes four
//    of the sub-tile's positions, writes du / ddelta / dz over the consumed LDS
//    rows, and the chunk's outputs leave as coalesced 16-B stores.
//  * dB / dC per sub-tile go to a per-workgroup slab (one coalesced 16-B store
//    per lane); small second kernels sum the slabs: deterministic, no atomics.
#include <cstdlib>
#include <type_traits>

#include "scan_common.h"

namespace mc {
namespace scan {

constexpr int kTC = kS;          // positions per backward chunk == saved-state interval (32)
constexpr int kTB = 8;           // positions per sub-tile (the pair loop's register tile)
constexpr int kSub = kTC / kTB;  // sub-tiles per chunk
constexpr int kWG = 2 * kRows;   // threads per workgroup: two waves
static_assert(kTC % kTB == 0, "chunk must be whole sub-tiles");

struct BwdArgs {
  int batch, dim, seqlen, dstate, n_groups, n_states, nblk, total_blocks, softplus;
  int state_ratio;    // saved states per kS-position chunk (kS / the forward's state interval)
  int64_t u_bs, u_ds, dt_bs, dt_ds, z_bs, z_ds, go_bs, go_ds;
  int64_t du_bs, du_ds, ddt_bs, ddt_ds, dz_bs, dz_ds;  // output strides (seqlen stride 1)
  const void* u; const void* delta; const void* z; const void* dout;
  const float* A; const float* bq; const float* D; const float* delta_bias;
  const float* chunk_states;
  void* du; void* ddelta; void* dz;
  float* slab_bc;                    // [b*G+g][nblk][seqlen][2][kN]  (dB partials, then dC partials)
  int64_t bc_out_s[2][3];            // dB / dC output strides: batch, group, dstate (seqlen stride 1)
  float* slab_a;                     // [b][kN][dim] (dA partials, one owner per element)
  float* slab_d;                     // [b][dim]
  float* slab_bias;                  // [b][dim]
  int rev_groups, u_groups;          // grouped directions (0 = off; element-wise path only)
};

__device__ __forceinline__ float dpp_f(float v, int ctrl_sel) {
  // ctrl_sel: 0 -> row_ror:8 (xor 8), 1 -> xor 4 (row_shl/shr:4 by bank), 2 -> quad_perm[2,3,0,1] (xor 2),
  // 3 -> quad_perm[1,0,3,2] (xor 1).  Every partner is lane ^ bit exactly: the
  // halving stages need partners that agree on the bits already reduced
  // (row_ror:4 is NOT xor 4 -- it can flip bit 3; tools/ubench/reduce_check.hip).
  const int iv = __float_as_int(v);
  int r;
  if (ctrl_sel == 0) r = __builtin_amdgcn_update_dpp(iv, iv, 0x128, 0xF, 0xF, false);
  else if (ctrl_sel == 1) {
    // xor 4 inside each 16-lane row, on the VALU (no LDS, so no lgkmcnt wait):
    // banks 0/2 (lanes 0-3, 8-11) take lane + 4 (row_shl:4), banks 1/3 take lane - 4 (row_shr:4)
    const int lo = __builtin_amdgcn_update_dpp(iv, iv, 0x104, 0xF, 0x5, false);
    r = __builtin_amdgcn_update_dpp(lo, iv, 0x114, 0xF, 0xA, false);
  }
  else if (ctrl_sel == 2) r = __builtin_amdgcn_update_dpp(iv, iv, 0x4E, 0xF, 0xF, false);
  else r = __builtin_amdgcn_update_dpp(iv, iv, 0xB1, 0xF, 0xF, false);
  return __int_as_float(r);
}

// NV per-lane values -> NV sums over the wave's 64 lanes (NV in {8, 16, 32}).
// Halving stages over lane bits 5, 4, 3, ... pair value j with j + NV/2^k;
// the remaining low lane bits are summed in full.  Afterwards lane l holds
// the sum of value index l / (64 / NV).
template <int NV>
__device__ __forceinline__ float wave_transpose_reduce(float (&v)[NV], int lane) {
  static_assert(NV == 8 || NV == 16 || NV == 32, "NV in {8, 16, 32}");
#pragma unroll
  for (int j = 0; j < NV / 2; ++j) {   // lane bit 5
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[j]), __float_as_uint(v[j + NV / 2]), false, false);
    v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int j = 0; j < NV / 4; ++j) {   // lane bit 4
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[j]), __float_as_uint(v[j + NV / 4]), false, false);
    v[j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
#pragma unroll
  for (int j = 0; j < NV / 8; ++j) {   // lane bit 3 via row_ror:8 (== xor 8 inside a row)
    const float keep = b3 ? v[j + NV / 8] : v[j], send = b3 ? v[j] : v[j + NV / 8];
    v[j] = keep + dpp_f(send, 0);
  }
  if constexpr (NV >= 16) {
#pragma unroll
    for (int j = 0; j < NV / 16; ++j) {   // lane bit 2 via xor 4
      const float keep = b2 ? v[j + NV / 16] : v[j], send = b2 ? v[j] : v[j + NV / 16];
      v[j] = keep + dpp_f(send, 1);
    }
  } else {
    v[0] += dpp_f(v[0], 1);
  }
  if constexpr (NV >= 32) {             // lane bit 1 via quad_perm [2,3,0,1]
    const float keep = b1 ? v[1] : v[0], send = b1 ? v[0] : v[1];
    v[0] = keep + dpp_f(send, 2);
  } else {
    v[0] += dpp_f(v[0], 2);
  }
  return v[0] + dpp_f(v[0], 3);         // lane bit 0 via quad_perm [1,0,3,2]
}

// LDS image of one array's chunk rows: 64 rows x RB bytes, 16-B blocks XOR-
// swizzled by row so that 64 lanes reading their own rows at one column hit
// distinct bank groups (ds_read_b128 lane groups) and the staging writes
// (8 lanes = 2 whole rows) are contiguous.
template <typename TI>
struct ChunkRows {
  static constexpr int RB = kTC * (int)sizeof(TI);   // bytes per row segment: 64 (16-bit) / 128 (fp32)
  static constexpr int VPR = RB / 16;                // 16-B vectors per row segment
  static constexpr int kShift = VPR == 4 ? 2 : 1;
  static constexpr int kBytes = kRows * RB;
  __device__ static __forceinline__ int off(int r, int c) { return r * RB + ((c ^ ((r >> kShift) & (VPR - 1))) << 4); }
};

// 2 waves per SIMD where registers and LDS allow it (16-bit rows, kN <= 16): <= 256 VGPRs,
// <= 40 KB LDS per workgroup; fp32 rows or kN = 32 run at one wave per SIMD.
// kDirs: grouped-direction addressing (reverse_groups / u_groups) compiled in; the plain
// instantiation carries none of it.
template <typename TI, int kN, bool kAligned, bool kSP, bool kDirs = false>
__global__ __launch_bounds__(kWG, (sizeof(TI) == 2 && kN <= 16) ? 2 : 1) void scan_bwd_kernel(const BwdArgs a) {
  using CR = ChunkRows<TI>;
  constexpr int VI = ElemTraits<TI>::kVec;   // elements per 16-B vector
  constexpr int VPR = CR::VPR;
  constexpr int kVT = kTB / VI;              // 16-B vectors per sub-tile row (1 for 16-bit, 2 for fp32)
  constexpr int kP = kN / 2;                 // state pairs
  constexpr int kPW = kP / 2;                // pairs per wave
  constexpr int kQC = kTC * kP;              // B/C quads per chunk
  constexpr int kQPer = (kQC + kWG - 1) / kWG;
  constexpr int kEH = kTB / 2;               // positions of a sub-tile each wave finishes
  static_assert(kPW >= 2 && kPW % 2 == 0, "kN in {8, 16, 32}");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* rows = smem;                                                   // [4][CR::kBytes]: u, delta, z, dout
  f32x2* st_all = reinterpret_cast<f32x2*>(smem + 4 * CR::kBytes);     // [wave][kSub-1][kPW][64]
  f32x4* bql = reinterpret_cast<f32x4*>(st_all + 2 * (kSub - 1) * kPW * kRows);   // [t][p]
  float* xch = reinterpret_cast<float*>(bql + kQC);                    // [wave][64][3][kEH]
  float* dbc = xch + 2 * kRows * 3 * kEH;                              // [kTB][2][kN]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  f32x2* st = st_all + wave * (kSub - 1) * kPW * kRows;
  const int lin = xcd_remap(blockIdx.x, a.total_blocks);
  const int dblk = lin % a.nblk;
  const int bg = lin / a.nblk;
  const int g = bg % a.n_groups, b = bg / a.n_groups;
  const int H = a.dim / a.n_groups;
  const int dbase = g * H + dblk * kRows;
  const int nrows = min(kRows, H - dblk * kRows);
  const int L_ = a.seqlen;
  const bool hasZ = a.z != nullptr;
  constexpr bool softplus = kSP;
  const bool my_ok = lane < nrows;
  const int my_d = dbase + lane;
  const int my_r = min(lane, nrows - 1);      // lanes past the group end mirror a valid row (never stored)
  const int my_dc = dbase + my_r;

  // ---- the arrays this wave stages: wave 0 -> u, delta; wave 1 -> z, dout
  const TI* src0 = reinterpret_cast<const TI*>(wave == 0 ? a.u : (hasZ ? a.z : a.dout));
  const TI* src1 = reinterpret_cast<const TI*>(wave == 0 ? a.delta : a.dout);
  const int64_t bs0 = wave == 0 ? a.u_bs : (hasZ ? a.z_bs : a.go_bs), ds0 = wave == 0 ? a.u_ds : (hasZ ? a.z_ds : a.go_ds);
  const int64_t bs1 = wave == 0 ? a.dt_bs : a.go_bs, ds1 = wave == 0 ? a.dt_ds : a.go_ds;
  // grouped directions: reversed groups walk mirrored positions; u_groups > 0 shares u blocks
  // (vector path: the host guarantees seqlen % VI == 0, so a mirrored 16-B block is aligned)
  const bool rev = kDirs && ((a.rev_groups >> g) & 1);
  const int row0 = (kDirs && a.u_groups && wave == 0) ? (g % a.u_groups) * H + dblk * kRows : dbase;
  const TI* rb0 = src0 + (int64_t)b * bs0 + (int64_t)row0 * ds0;
  const TI* rb1 = src1 + (int64_t)b * bs1 + (int64_t)dbase * ds1;
  const int slot0 = wave == 0 ? 0 : 2, slot1 = wave == 0 ? 1 : 3;
  const bool stage0 = wave == 0 || hasZ;     // wave 1 without z stages dout only
  auto span = [&](int64_t ds) __attribute__((always_inline)) -> uint32_t { return (uint32_t)(((int64_t)(nrows - 1) * ds + L_) * (int64_t)sizeof(TI)); };
  const __amdgpu_buffer_rsrc_t rs0 = make_rsrc(rb0, span(ds0)), rs1 = make_rsrc(rb1, span(ds1));
  const float* bqsrc = a.bq + (int64_t)bg * L_ * (4 * kP);
  const __amdgpu_buffer_rsrc_t rs_bq = make_rsrc(bqsrc, (uint32_t)L_ * kP * 16u);
  // chunk states [b][row][n_states][N]; the fine interval is position-major, [b][n_states][row][N]
  const bool pm = a.state_ratio != 1;
  const uint32_t cs_rs = pm ? (uint32_t)a.dstate : (uint32_t)(a.n_states * a.dstate);   // floats per row step
  const uint32_t cs_ks = pm ? (uint32_t)(a.dim * a.dstate) : (uint32_t)a.dstate;        // floats per state step
  const float* csb = a.chunk_states + (int64_t)b * a.dim * a.n_states * a.dstate + (int64_t)dbase * cs_rs;
  const __amdgpu_buffer_rsrc_t rs_cs =
      make_rsrc(csb, nrows > 0 ? ((uint32_t)(nrows - 1) * cs_rs + (uint32_t)(a.n_states - 1) * cs_ks + a.dstate) * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rs_slab =
      make_rsrc(a.slab_bc + ((int64_t)bg * a.nblk + dblk) * L_ * (2 * kN), (uint32_t)L_ * (2 * kN) * 4u);

  // ---- per-lane constants of this wave's pairs (global pair p = wave * kPW + pl)
  f32x2 A2[kPW], hcar[kPW], dA2[kPW];
  {
    // unconditional loads (clamped index), masked after: no load sits behind a branch
    const float* arow = a.A + (int64_t)my_dc * a.dstate;
    float av[2 * kPW];
#pragma unroll
    for (int i = 0; i < 2 * kPW; ++i) av[i] = arow[min(2 * kPW * wave + i, a.dstate - 1)];
#pragma unroll
    for (int pl = 0; pl < kPW; ++pl) {
      const int n0 = 2 * (wave * kPW + pl);
      A2[pl].x = n0 < a.dstate ? av[2 * pl] * kLog2e : 0.f;
      A2[pl].y = n0 + 1 < a.dstate ? av[2 * pl + 1] * kLog2e : 0.f;
      hcar[pl] = f32x2{0.f, 0.f};
      dA2[pl] = f32x2{0.f, 0.f};
    }
  }
  const float Dv = a.D ? a.D[my_dc] : 0.f;
  const float biasv = a.delta_bias ? a.delta_bias[my_dc] : 0.f;
  float dDacc = 0.f, dbacc = 0.f;

  // ---- prefetch registers: this wave's two row arrays of one chunk, its share
  // of the chunk's B/C quads, and the saved state at the chunk start (own pairs)
  uint4 pf0[VPR], pf1[VPR];
  f32x4 pq[kQPer];
  f32x4 px0[kPW / 2];
  auto prefetch = [&](int c) __attribute__((always_inline)) {
    const int l0 = c * kTC;
    const bool valid = c >= 0;
#pragma unroll
    for (int k = 0; k < VPR; ++k) {
      const int j = lane + k * kRows;
      const int r = min(j / VPR, nrows - 1), cc = j % VPR;
      const int col0 = l0 + cc * VI;
      if constexpr (kAligned) {
        // chunk -1: an offset past every buffer range reads 0 (no branch around the loads)
        // reversed group: ascending mirrored block (mc_common.h ld16_rev; a block past the end
        // reads an unused neighbour or wraps out of range; steps >= L are zeroed before use)
        const int cm = rev ? L_ - l0 - kTC + cc * VI : col0;
        const uint32_t o0 = valid ? (uint32_t)(r * ds0 + cm) * (uint32_t)sizeof(TI) : 0x80000000u;
        const uint32_t o1 = valid ? (uint32_t)(r * ds1 + cm) * (uint32_t)sizeof(TI) : 0x80000000u;
        pf0[k] = buf_ld16(rs0, o0);   // (reversed groups: element order flipped at staging, not here --
        pf1[k] = buf_ld16(rs1, o1);   //  touching the values would wait for the loads)
      } else {
        if (rev) {
          const int nvr = valid ? max(0, min(VI, L_ - (l0 + (VPR - 1 - cc) * VI))) : 0;
          const int cm = valid ? L_ - l0 - kTC + cc * VI : 0;
          pf0[k] = ld16_top(rb0 + (int64_t)r * ds0, cm, nvr);   // flipped at staging
          pf1[k] = ld16_top(rb1 + (int64_t)r * ds1, cm, nvr);
        } else {
          const int nv = valid ? max(0, min(VI, L_ - col0)) : 0;
          pf0[k] = ld16_masked(rb0 + (int64_t)r * ds0 + (valid ? col0 : 0), nv);
          pf1[k] = ld16_masked(rb1 + (int64_t)r * ds1 + (valid ? col0 : 0), nv);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kQPer; ++k) {
      const int q = tid + k * kWG;
      const uint32_t o = valid && q < kQC ? (uint32_t)((l0 * kP + q) * 16) : 0x80000000u;
      pq[k] = __builtin_bit_cast(f32x4, buf_ld16(rs_bq, o));
    }
    // saved state after chunk c-1 (zero for c == 0): floats [2 kPW wave, 2 kPW (wave+1)) of my row
    const uint32_t ox = c > 0 ? ((uint32_t)my_r * cs_rs + (uint32_t)(c * a.state_ratio - 1) * cs_ks + (uint32_t)(2 * kPW * wave)) * 4u
                              : 0x80000000u;
#pragma unroll
    for (int k = 0; k < kPW / 2; ++k) px0[k] = __builtin_bit_cast(f32x4, buf_ld16(rs_cs, ox + 16 * k));
  };

  auto own_vec = [&](int slot, int blk) __attribute__((always_inline)) -> uint4 {   // this lane's row, 16-B block blk of the chunk
    return *reinterpret_cast<const uint4*>(rows + slot * CR::kBytes + CR::off(lane, blk));
  };

  const int nch = (L_ + kTC - 1) / kTC;
  prefetch(nch - 1);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)

  for (int c = nch - 1; c >= 0; --c) {
    const int l0 = c * kTC;
    // ---- stage the prefetched rows and quads, take the chunk-start state
#pragma unroll
    for (int k = 0; k < VPR; ++k) {
      const int j = lane + k * kRows;
      const int off = CR::off(j / VPR, rev ? VPR - 1 - j % VPR : j % VPR);   // reversed: mirrored block
      // mirrored blocks arrive in memory order: flip them here
      if (stage0) *reinterpret_cast<uint4*>(rows + slot0 * CR::kBytes + off) = rev ? reverse_elems<TI>(pf0[k]) : pf0[k];
      *reinterpret_cast<uint4*>(rows + slot1 * CR::kBytes + off) = rev ? reverse_elems<TI>(pf1[k]) : pf1[k];
    }
#pragma unroll
    for (int k = 0; k < kQPer; ++k) {
      const int q = tid + k * kWG;
      if ((k + 1) * kWG <= kQC || q < kQC) bql[q] = pq[k];
    }
    f32x2 x0r[kPW];
#pragma unroll
    for (int k = 0; k < kPW / 2; ++k) {
      const int n0 = 2 * kPW * wave + 4 * k;
      const f32x4 v = px0[k];
      x0r[2 * k] = f32x2{n0 < a.dstate ? v.x : 0.f, n0 + 1 < a.dstate ? v.y : 0.f};
      x0r[2 * k + 1] = f32x2{n0 + 2 < a.dstate ? v.z : 0.f, n0 + 3 < a.dstate ? v.w : 0.f};
    }
    lds_barrier();
    prefetch(c - 1);     // flies under this chunk's math

    const int nsub = min(kSub, (L_ - l0 + kTB - 1) / kTB);   // sub-tiles holding positions < L

    // per-position scalars of sub-tile s from the staged rows (positions >= L zeroed)
    auto sub_scalars = [&](int s, float (&dt)[kTB], float (&dtu)[kTB], float (&gy)[kTB], bool want_gy) {
      uint4 qu[kVT], qd[kVT], qz[kVT], qg[kVT];
#pragma unroll
      for (int k = 0; k < kVT; ++k) {
        qu[k] = own_vec(0, s * kVT + k);
        qd[k] = own_vec(1, s * kVT + k);
        if (want_gy) {
          qz[k] = own_vec(2, s * kVT + k);
          qg[k] = own_vec(3, s * kVT + k);
        }
      }
#pragma unroll
      for (int t = 0; t < kTB; ++t) {
        const bool tv = l0 + s * kTB + t < L_;
        const float uv = tv ? elem_f<TI>(qu[t / VI], t % VI) : 0.f;
        const float r = elem_f<TI>(qd[t / VI], t % VI) + biasv;
        float d = softplus ? softplus_f(r) : r;
        d = tv ? d : 0.f;
        dt[t] = d;
        // lanes mirroring a row past the group end: dtu = gy = 0 zeroes their dB / dC terms
        dtu[t] = my_ok ? d * uv : 0.f;
        if (want_gy) {
          const float go = tv ? elem_f<TI>(qg[t / VI], t % VI) : 0.f;
          float gyv = go;
          if (hasZ) {
            const float zv = tv ? elem_f<TI>(qz[t / VI], t % VI) : 0.f;
            gyv = go * zv * sigmoid_f(zv);   // dout * silu(z)
          }
          gy[t] = my_ok ? gyv : 0.f;
        }
      }
    };

    // ---- recompute the states at the starts of sub-tiles 1 .. nsub-1 (own pairs) -> LDS
    {
      f32x2 x[kPW];
#pragma unroll
      for (int pl = 0; pl < kPW; ++pl) x[pl] = x0r[pl];
#pragma unroll 1
      for (int s = 0; s + 1 < nsub; ++s) {
        float dt[kTB], dtu[kTB], gy[kTB];
        sub_scalars(s, dt, dtu, gy, false);
#pragma unroll
        for (int t = 0; t < kTB; ++t) {
          if (t % 2 == 0) __builtin_amdgcn_sched_barrier(0);   // bounded hoisting: 2 positions x kPW pairs
#pragma unroll
          for (int pl = 0; pl < kPW; ++pl) {
            const f32x2 bb = reinterpret_cast<const f32x2*>(bql + (s * kTB + t) * kP + wave * kPW + pl)[0];
            const f32x2 arg = A2[pl] * dt[t];
            const f32x2 aa = {fast_exp2(arg.x), fast_exp2(arg.y)};
            x[pl] = aa * x[pl] + bb * dtu[t];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pl = 0; pl < kPW; ++pl) st[(s * kPW + pl) * kRows + lane] = x[pl];
      }
    }

    // ---- sub-tiles in reverse
#pragma unroll 1
    for (int s = nsub - 1; s >= 0; --s) {
      float dt[kTB], dtu[kTB], gy[kTB];
      sub_scalars(s, dt, dtu, gy, true);
      float Sa[kTB], Qa[kTB], Ya[kTB];      // per-position sums over this wave's pairs
#pragma unroll
      for (int t = 0; t < kTB; ++t) { Sa[t] = Qa[t] = Ya[t] = 0.f; }

#pragma unroll
      for (int pl = 0; pl < kPW; ++pl) {
        __builtin_amdgcn_sched_barrier(0);      // one pair at a time: bounded register live ranges
        const int p = wave * kPW + pl;
        // Pin the program order of the pairs: empty volatile asm statements keep their
        // order, and this pair's inputs / last pair's outputs pass through them, so the
        // instruction-selection DAG cannot run all forward sweeps ahead of the reverse
        // sweeps (that interleaving keeps every pair's xs / as live at once).
        f32x2 a2p = A2[pl];
        asm volatile("" : "+v"(a2p));
        const f32x2 x0p = s == 0 ? x0r[pl] : st[((s - 1) * kPW + pl) * kRows + lane];
        // forward sweep: states and decays of this pair over the sub-tile (B halves only)
        f32x2 xs[kTB], as[kTB];
        // the decays first (independent of the state chain), then the chain itself
#pragma unroll
        for (int t = 0; t < kTB; ++t) {
          const f32x2 arg = a2p * dt[t];
          as[t] = f32x2{fast_exp2(arg.x), fast_exp2(arg.y)};
        }
        f32x2 x = x0p;
#pragma unroll
        for (int t = 0; t < kTB; ++t) {
          const f32x2 bb = reinterpret_cast<const f32x2*>(bql + (s * kTB + t) * kP + p)[0];
          x = as[t] * x + bb * dtu[t];
          xs[t] = x;
        }
        __builtin_amdgcn_sched_barrier(0);
        // dC_t,n = sum over the wave's channels of gy_t x_t,n
        {
          float red[2 * kTB];
#pragma unroll
          for (int t = 0; t < kTB; ++t) {
            const f32x2 v = xs[t] * gy[t];
            red[2 * t] = v.x;
            red[2 * t + 1] = v.y;
          }
          const float tot = wave_transpose_reduce<2 * kTB>(red, lane);
          const int j = lane / (64 / (2 * kTB));
          if ((lane & (64 / (2 * kTB) - 1)) == 0) dbc[((j >> 1) * 2 + 1) * kN + 2 * p + (j & 1)] = tot;
        }
        __builtin_amdgcn_sched_barrier(0);
        // reverse sweep: adjoint of the state (+ y_t = sum_n C x for dz)
        f32x2 h = hcar[pl];
        f32x2 dAp = dA2[pl];
        float red[2 * kTB];
        // quads read one position ahead of their use (LDS latency under the chain)
        f32x4 qn = bql[(s * kTB + kTB - 1) * kP + p];
#pragma unroll
        for (int t = kTB - 1; t >= 0; --t) {
          const f32x4 q = qn;
          if (t > 0) qn = bql[(s * kTB + t - 1) * kP + p];
          Ya[t] = fmaf(q.hi.x, xs[t].x, fmaf(q.hi.y, xs[t].y, Ya[t]));
          h = q.hi * gy[t] + h;                     // + C_t gy_t
          Sa[t] = fmaf(h.x, q.lo.x, fmaf(h.y, q.lo.y, Sa[t]));
          const f32x2 vb = h * dtu[t];
          red[2 * t] = vb.x;
          red[2 * t + 1] = vb.y;
          const f32x2 ha = h * as[t];
          const f32x2 hax = ha * (t > 0 ? xs[t - 1] : x0p);
          const f32x2 qa = hax * a2p;
          Qa[t] += qa.x + qa.y;
          dAp = hax * dt[t] + dAp;
          h = ha;
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(h), "+v"(dAp));
#pragma unroll
        for (int t = 0; t < kTB; ++t) asm volatile("" : "+v"(Sa[t]), "+v"(Qa[t]), "+v"(Ya[t]));
        hcar[pl] = h;
        dA2[pl] = dAp;
        {
          const float tot = wave_transpose_reduce<2 * kTB>(red, lane);
          const int j = lane / (64 / (2 * kTB));
          if ((lane & (64 / (2 * kTB) - 1)) == 0) dbc[((j >> 1) * 2 + 0) * kN + 2 * p + (j & 1)] = tot;
        }
      }
      __builtin_amdgcn_sched_barrier(0);

      // ---- exchange partial sums, then each wave finishes half of the sub-tile's positions.
      // The wave index is made a compile-time constant here so that every register
      // array (Sa / Qa / Ya / dt) is indexed statically (a runtime index would
      // demote them to scratch).
      auto exchange_and_finish = [&](auto wc) __attribute__((always_inline)) {
        constexpr int W = decltype(wc)::value;
        {   // the other wave finishes positions [kEH*(1-W), +kEH): give it my partial sums
          constexpr int t0 = kEH * (1 - W);
          float* xo = xch + (W * kRows + lane) * 3 * kEH;
          f32x4 sv, qv, yv;
#pragma unroll
          for (int e = 0; e < kEH; ++e) { sv[e] = Sa[t0 + e]; qv[e] = Qa[t0 + e]; yv[e] = Ya[t0 + e]; }
          reinterpret_cast<f32x4*>(xo)[0] = sv;
          reinterpret_cast<f32x4*>(xo)[1] = qv;
          reinterpret_cast<f32x4*>(xo)[2] = yv;
        }
        lds_barrier();
        // my positions t = kEH*W + e: du, ddelta, dz written over the consumed rows
        constexpr int t0 = kEH * W;
        const float* xi = xch + ((1 - W) * kRows + lane) * 3 * kEH;
        const f32x4 so = reinterpret_cast<const f32x4*>(xi)[0];
        const f32x4 qo = reinterpret_cast<const f32x4*>(xi)[1];
        const f32x4 yo = reinterpret_cast<const f32x4*>(xi)[2];
        const int blk = s * kVT + t0 / VI;            // 16-B block holding my positions
        constexpr int eo = t0 % VI;                   // first element of mine inside it
        const uint4 qu = own_vec(0, blk), qd = own_vec(1, blk), qz = own_vec(2, blk), qg = own_vec(3, blk);
        float o_du[kEH], o_dd[kEH], o_dz[kEH];
#pragma unroll
        for (int e = 0; e < kEH; ++e) {
          const int t = t0 + e;
          const bool tv = l0 + s * kTB + t < L_;
          const float uv = tv ? elem_f<TI>(qu, eo + e) : 0.f;
          const float r = elem_f<TI>(qd, eo + e) + biasv;
          const float go = tv ? elem_f<TI>(qg, eo + e) : 0.f;
          const float S = Sa[t] + so[e];
          const float Q = (Qa[t] + qo[e]) * kLn2;   // A2 carries log2(e)
          const float Y = Ya[t] + yo[e];
          const float sg = softplus ? (r > 20.f ? 1.f : sigmoid_f(r)) : 1.f;
          float gyv = go, gz = 0.f;
          if (hasZ) {
            const float zv = tv ? elem_f<TI>(qz, eo + e) : 0.f;
            const float sgz = sigmoid_f(zv);
            gyv = go * zv * sgz;
            gz = go * sgz * (1.f + zv * (1.f - sgz));
          }
          o_dz[e] = gz * fmaf(Dv, uv, Y);             // dout * silu'(z) * (y + D u)
          o_du[e] = fmaf(Dv, gyv, dt[t] * S);
          const float dr = fmaf(uv, S, Q) * sg;
          o_dd[e] = dr;
          if (tv && my_ok) {
            dDacc = fmaf(gyv, uv, dDacc);
            dbacc += dr;
          }
        }
        // write over the consumed row bytes (read above by this lane only)
        auto put = [&](int slot, const float (&v)[kEH]) {
          char* dst = rows + slot * CR::kBytes + CR::off(lane, blk) + eo * (int)sizeof(TI);
          if constexpr (sizeof(TI) == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
            *reinterpret_cast<uint2*>(dst) = make_uint2(bits16<TI>(v[0]) | (bits16<TI>(v[1]) << 16),
                                                        bits16<TI>(v[2]) | (bits16<TI>(v[3]) << 16));
          }
        };
        put(0, o_du);
        put(1, o_dd);
        if (hasZ) put(2, o_dz);
      };
      if (wave == 0) exchange_and_finish(std::integral_constant<int, 0>());
      else exchange_and_finish(std::integral_constant<int, 1>());
      // ---- the sub-tile's dB / dC sums -> this workgroup's slab (positions past L dropped)
      if (wave == 0) {
        constexpr int kF = kTB * 2 * kN;   // floats
#pragma unroll
        for (int k = 0; k < (kF + 4 * kRows - 1) / (4 * kRows); ++k) {
          const int f = 4 * (lane + k * kRows);
          if (f < kF) {
            const uint4 v = *reinterpret_cast<const uint4*>(dbc + f);
            buf_st16(rs_slab, (uint32_t)(((l0 + s * kTB) * 2 * kN + f) * 4), v);
          }
        }
      }
      lds_barrier();
    }

    // ---- the chunk's du / ddelta (wave 0) and dz (wave 1): coalesced 16-B stores
    {
      const int nst = wave == 0 ? 2 : (hasZ ? 1 : 0);
      for (int sidx = 0; sidx < nst; ++sidx) {
        const int slot = wave == 0 ? sidx : 2;
        TI* base;
        int64_t ds;
        if (slot == 0) { base = reinterpret_cast<TI*>(a.du) + (int64_t)b * a.du_bs + (int64_t)dbase * a.du_ds; ds = a.du_ds; }
        else if (slot == 1) { base = reinterpret_cast<TI*>(a.ddelta) + (int64_t)b * a.ddt_bs + (int64_t)dbase * a.ddt_ds; ds = a.ddt_ds; }
        else { base = reinterpret_cast<TI*>(a.dz) + (int64_t)b * a.dz_bs + (int64_t)dbase * a.dz_ds; ds = a.dz_ds; }
        const __amdgpu_buffer_rsrc_t rso = make_rsrc(base, span(ds));
#pragma unroll
        for (int k = 0; k < VPR; ++k) {
          const int j = lane + k * kRows;
          const int r = j / VPR, cc = j % VPR;
          const int cl = rev ? VPR - 1 - cc : cc;     // LDS block of this lane's vector
          const int col0 = l0 + cc * VI;
          const int cm = L_ - l0 - kTC + cc * VI;      // (reversed) ascending mirrored position
          if (r < nrows && l0 + cl * VI < L_) {
            const uint4 v = *reinterpret_cast<const uint4*>(rows + slot * CR::kBytes + CR::off(r, cl));
            const int nv = min(VI, L_ - (l0 + cl * VI));
            if constexpr (kAligned) {
              const uint32_t o = (uint32_t)(r * ds + (rev ? cm : col0)) * (uint32_t)sizeof(TI);
              if (nv == VI) buf_st16(rso, o, rev ? reverse_elems<TI>(v) : v);
              else buf_st16_masked<TI>(rso, o, v, nv);   // (never with rev: seqlen % VI == 0)
            } else if (rev) {
              st16_rev(base + (int64_t)r * ds, cm, v, nv);
            } else {
              st16_masked(base + (int64_t)r * ds + col0, v, nv);
            }
          }
        }
      }
    }
    lds_barrier();    // rows are free for the next chunk's staging
  }

  // ---- per-channel parameter gradients: dA (each wave its pairs), dD / dbias (both waves' halves)
  if (my_ok) {
#pragma unroll
    for (int pl = 0; pl < kPW; ++pl) {
      const int n0 = 2 * (wave * kPW + pl);
      a.slab_a[((int64_t)b * kN + n0) * a.dim + my_d] = dA2[pl].x;
      a.slab_a[((int64_t)b * kN + n0 + 1) * a.dim + my_d] = dA2[pl].y;
    }
  }
  if (wave == 1) { xch[2 * lane] = dDacc; xch[2 * lane + 1] = dbacc; }
  lds_barrier();
  if (wave == 0 && my_ok) {
    a.slab_d[(int64_t)b * a.dim + my_d] = dDacc + xch[2 * lane];
    a.slab_bias[(int64_t)b * a.dim + my_d] = dbacc + xch[2 * lane + 1];
  }
}

// B/C as the backward consumes them: fp32 quads {B_n, B_n+1, C_n, C_n+1} per
// (b, g, l, pair), states >= dstate zero.  One thread per quad.
template <typename TW, int kN>
__global__ __launch_bounds__(256) void bc_quad_kernel(const TW* __restrict__ B, const TW* __restrict__ C,
                                                      int64_t B_bs, int64_t B_gs, int64_t B_ns, int64_t C_bs,
                                                      int64_t C_gs, int64_t C_ns, int batch, int G, int L, int dstate,
                                                      int rev, f32x4* __restrict__ out) {
  constexpr int kP = kN / 2;
  const int64_t total = (int64_t)batch * G * L * kP;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % kP);
    const int64_t rest = i / kP;
    const int l = (int)(rest % L);
    const int64_t bg = rest / L;
    const int gg = (int)(bg % G), bb = (int)(bg / G);
    const int ls = ((rev >> gg) & 1) ? L - 1 - l : l;   // reversed groups: mirrored positions
    const TW* bs = B + (int64_t)bb * B_bs + (int64_t)gg * B_gs + ls;
    const TW* cs = C + (int64_t)bb * C_bs + (int64_t)gg * C_gs + ls;
    const int n0 = 2 * p;
    f32x4 v;
    v.x = n0 < dstate ? to_f(bs[(int64_t)n0 * B_ns]) : 0.f;
    v.y = n0 + 1 < dstate ? to_f(bs[(int64_t)(n0 + 1) * B_ns]) : 0.f;
    v.z = n0 < dstate ? to_f(cs[(int64_t)n0 * C_ns]) : 0.f;
    v.w = n0 + 1 < dstate ? to_f(cs[(int64_t)(n0 + 1) * C_ns]) : 0.f;
    out[i] = v;
  }
}

static hipError_t launch_bc_quads(const mc_scan_bwd_params* p, f32x4* out, hipStream_t s) {
  const int np = padded_dstate(p->dstate);
  const int64_t total = (int64_t)p->batch * p->n_groups * p->seqlen * (np / 2);
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
  MC_DISPATCH_T(p->wtype, MC_DISPATCH_NP(np, hipLaunchKernelGGL(
      (bc_quad_kernel<T, kN>), grid, 256, 0, s, reinterpret_cast<const T*>(p->B), reinterpret_cast<const T*>(p->C),
      p->B_batch_stride, p->B_group_stride, p->B_dstate_stride, p->C_batch_stride, p->C_group_stride,
      p->C_dstate_stride, p->batch, p->n_groups, p->seqlen, p->dstate, p->reverse_groups, out)));
  return hipGetLastError();
}

// dB / dC: sum the per-workgroup slabs; dA / dD / dbias: sum the per-batch slabs.
struct BcOutStrides {
  int64_t s[2][3];
};
template <typename TW, int kN>
__global__ __launch_bounds__(256) void scan_bwd_reduce_bc(const float* __restrict__ slab, int batch, int G, int nblk,
                                                           int dstate, int L, int rev, TW* __restrict__ dB,
                                                           TW* __restrict__ dC, BcOutStrides os) {
  // thread -> (b*G+g, l, which, n), n fastest: the slab reads are coalesced
  const int64_t total = (int64_t)batch * G * L * 2 * kN;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i % kN);
    int64_t r = i / kN;
    const int which = (int)(r % 2);
    r /= 2;
    const int l = (int)(r % L);
    const int64_t bgi = r / L;
    if (n >= dstate) continue;
    // the slab rows of one output are L * 2kN floats apart: keep 8 loads in flight
    // (the sum order stays k = 0, 1, 2, ...: deterministic, as before)
    const float* sp = slab + (bgi * nblk * L + l) * (2 * kN) + which * kN + n;
    const int64_t kst = (int64_t)L * (2 * kN);
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < nblk; ++k) s += sp[k * kst];
    TW* dst = which ? dC : dB;
    const int g = (int)(bgi % G);
    const int lo = ((rev >> g) & 1) ? L - 1 - l : l;
    const int64_t* st = os.s[which];
    dst[(bgi / G) * st[0] + g * st[1] + n * st[2] + lo] = from_f<TW>(s);
  }
}

// Column sums over the batch: out[c] = sum_b in[b][c] (row stride ld).  A
// block = 32 columns x 8 batch lanes; the 8 partials meet in LDS in a fixed
// order (deterministic).  Used for dD and dbias (cols = d).
__global__ __launch_bounds__(256) void scan_bwd_colsum(const float* __restrict__ in0, const float* __restrict__ in1,
                                                       int batch, int cols, int64_t ld, float* __restrict__ out0,
                                                       float* __restrict__ out1) {
  // blockIdx.y selects the (slab, output) pair: dD and dbias in one launch
  const float* __restrict__ in = blockIdx.y ? in1 : in0;
  float* __restrict__ out = blockIdx.y ? out1 : out0;
  __shared__ float part[8][33];
  const int cx = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  float s = 0.f;
  if (c < cols)
#pragma unroll 8   // loads in flight; the summation order is unchanged
    for (int bb = q; bb < batch; bb += 8) s += in[(int64_t)bb * ld + c];
  part[q][cx] = s;
  __syncthreads();
  if (q == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += part[k][cx];
    out[c] = t;
  }
}

// dA[d][n] = sum_b slab[b][n][d] (slab row stride ld): columns c = n * dim + d
// (coalesced along d), output transposed to (dim, dstate).  Fixed-order sums.
__global__ __launch_bounds__(256) void scan_bwd_colsum_nd(const float* __restrict__ in, int batch, int dim,
                                                          int dstate, int64_t ld, float* __restrict__ out) {
  __shared__ float part[8][33];
  const int cx = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  const int cols = dim * dstate;
  float s = 0.f;
  if (c < cols)
#pragma unroll 8   // loads in flight; the summation order is unchanged
    for (int bb = q; bb < batch; bb += 8) s += in[(int64_t)bb * ld + c];
  part[q][cx] = s;
  __syncthreads();
  if (q == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += part[k][cx];
    const int n = c / dim, d = c % dim;
    out[(int64_t)d * dstate + n] = t;
  }
}

struct BwdWs {
  size_t bq, slab_bc, slab_a, slab_d, slab_bias, total;
};
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
static BwdWs bwd_ws_layout(int batch, int dim, int seqlen, int dstate, int G) {
  const int np = padded_dstate(dstate);
  const int nblk = (dim / G + kRows - 1) / kRows;
  BwdWs w;
  size_t o = 0;
  w.bq = o; o += align256((size_t)batch * G * seqlen * (np / 2) * 16);
  w.slab_bc = o; o += align256((size_t)batch * G * nblk * np * 2 * seqlen * 4);
  w.slab_a = o; o += align256((size_t)batch * dim * np * 4);
  w.slab_d = o; o += align256((size_t)batch * dim * 4);
  w.slab_bias = o; o += align256((size_t)batch * dim * 4);
  w.total = o;
  return w;
}

template <typename TI, int kN>
static size_t bwd_lds_bytes() {
  constexpr int kP = kN / 2, kPW = kP / 2;
  return 4 * (size_t)ChunkRows<TI>::kBytes + (size_t)2 * (kSub - 1) * kPW * kRows * 8 + (size_t)kTC * kP * 16 +
         (size_t)2 * kRows * 3 * (kTB / 2) * 4 + (size_t)kTB * 2 * kN * 4;
}

// scan_bwd_pair.hip: the lane-pair kernel for 16-bit rows with dstate 16 (the text towers); it reads 16-bit
// B / C rows directly (no quad relayout)
void launch_bwd_pair(const mc_scan_bwd_params* p, const BwdSlabs& w, hipStream_t s);

// Everything mc_scan_bwd does for a call, decided in one place; mc_scan_bwd_kernel reads the same plan.
struct BwdPlan {
  int family = MC_SCAN_KERNEL_NONE;   // MC_SCAN_KERNEL_*; NONE: nothing to launch
  bool aligned = false;               // general kernel: 16-B vector rows
  f32x4* bq = nullptr;                // workspace: the general kernel's B / C quads
  int rows = kRows;                   // channels per workgroup of the chosen kernel
  BwdSlabs slabs{};                   // workspace: partial sums, one dB / dC slab per `rows` channels
  BwdArgs a{};                        // general kernel
};

// The choice: what a call with these params runs.  It reads shapes, strides and pointer alignment only,
// reports no error and touches nothing else, so mc_scan_bwd_kernel answers from it for any params.
static void choose_bwd(const mc_scan_bwd_params* p, BwdPlan& pl) {
  pl = BwdPlan{};
  const bool empty = p->batch == 0 || p->seqlen == 0, dirs = has_dirs(p->reverse_groups, p->u_groups);
  const int ib = elem_bytes(p->itype);
  const Rows rows[] = {{p->u, p->u_batch_stride, p->u_dim_stride},
                       {p->delta, p->delta_batch_stride, p->delta_dim_stride},
                       {p->z, p->z_batch_stride, p->z_dim_stride},
                       {p->dout, p->dout_batch_stride, p->dout_dim_stride},
                       {p->du, p->du_batch_stride, p->du_dim_stride},
                       {p->ddelta, p->ddelta_batch_stride, p->ddelta_dim_stride},
                       {p->dz, p->dz_batch_stride, p->dz_dim_stride}};
  const bool vec = all_vec_ok(rows, ib);
  // the pair kernel also addresses its workgroup's saved states with 32-bit byte offsets
  const bool pair = pair_shape_ok(p, kQN) && vec && all_span32(rows, kQCh * kQW, p->seqlen, ib) &&
                    (int64_t)kQCh * kQW * mc_scan_n_states(p->seqlen, p->state_interval) * kQN * 4 < ((int64_t)1 << 31);
  pl.family = empty ? MC_SCAN_KERNEL_NONE
                    : dirs ? MC_SCAN_KERNEL_DIRS : pair ? MC_SCAN_KERNEL_PAIR : MC_SCAN_KERNEL_GENERIC;
  pl.rows = pair ? kQCh * kQW : kRows;
  // the vector path addresses a workgroup's 64 rows with 32-bit byte offsets; mirrored blocks stay aligned
  pl.aligned = !pair && vec && all_span32(rows, kRows, (int64_t)p->seqlen + kTC, ib) && dirs_vec_ok(dirs, p->seqlen, ib);
}

// The checks of a call, in the ABI's order, around the choice; then the workspace carving and the args.
static int plan_bwd(const mc_scan_bwd_params* p, BwdPlan& pl) {
  MC_CHECK(p != nullptr, MC_ERR_INVALID, "mc_scan_bwd: null params");
  choose_bwd(p, pl);
  MC_TRY(validate_common(p->batch, p->dim, p->seqlen, p->dstate, p->n_groups, p->itype, p->wtype, "mc_scan_bwd"));
  const bool dirs = pl.family == MC_SCAN_KERNEL_DIRS;
  const int np = padded_dstate(p->dstate);
  MC_CHECK(p->A && p->dA, MC_ERR_INVALID, "mc_scan_bwd: A and dA must be non-null");
  MC_CHECK(!p->D || p->dD, MC_ERR_INVALID, "mc_scan_bwd: dD required when D is given");
  MC_CHECK(!p->delta_bias || p->ddelta_bias, MC_ERR_INVALID, "mc_scan_bwd: ddelta_bias required with delta_bias");
  if (pl.family == MC_SCAN_KERNEL_NONE) return MC_OK;
  MC_CHECK(p->u && p->delta && p->B && p->C && p->dout && p->du && p->ddelta && p->dB && p->dC, MC_ERR_INVALID,
           "mc_scan_bwd: u, delta, B, C, dout and du, ddelta, dB, dC must be non-null");
  MC_CHECK(!p->z || p->dz, MC_ERR_INVALID, "mc_scan_bwd: dz required when z is given");
  MC_CHECK((int64_t)kRows * mc_scan_n_chunks(p->seqlen) * p->dstate * 4 < ((int64_t)1 << 31) &&
               (int64_t)p->seqlen * (np / 2) * 16 < ((int64_t)1 << 31) &&
               (int64_t)p->seqlen * 2 * np * 4 < ((int64_t)1 << 31),
           MC_ERR_INVALID, "mc_scan_bwd: seqlen %d too long for 32-bit offsets", p->seqlen);
  MC_CHECK(p->chunk_states, MC_ERR_INVALID, "mc_scan_bwd: chunk_states (from the training forward) required");
  const int S = p->state_interval > 0 ? p->state_interval : kS;
  MC_CHECK(S == kS || (S == kFineS && p->seqlen % kFineS == 0), MC_ERR_SHAPE,
           "mc_scan_bwd: state_interval %d: 0 / %d, or %d with seqlen %% %d == 0 (the forward's interval)",
           p->state_interval, kS, kFineS, kFineS);
  // a workgroup's saved states, either kernel's
  MC_CHECK((int64_t)kRows * mc_scan_n_states(p->seqlen, S) * p->dstate * 4 < ((int64_t)1 << 31) &&
               (int64_t)kQCh * kQW * mc_scan_n_states(p->seqlen, S) * kQN * 4 < ((int64_t)1 << 31),
           MC_ERR_INVALID, "mc_scan_bwd: seqlen %d too long for 32-bit state offsets", p->seqlen);
  MC_TRY(check_dirs(p, "mc_scan_bwd"));
  const BwdWs w = bwd_ws_layout(p->batch, p->dim, p->seqlen, p->dstate, p->n_groups);
  MC_CHECK(p->workspace && p->workspace_bytes >= w.total && (reinterpret_cast<uintptr_t>(p->workspace) & 255) == 0,
           MC_ERR_WORKSPACE, "mc_scan_bwd: workspace must be >= %zu bytes and 256-B aligned (got %zu)", w.total,
           p->workspace_bytes);

  char* ws = reinterpret_cast<char*>(p->workspace);
  pl.bq = reinterpret_cast<f32x4*>(ws + w.bq);
  pl.slabs = BwdSlabs{reinterpret_cast<float*>(ws + w.slab_bc), reinterpret_cast<float*>(ws + w.slab_a),
                      reinterpret_cast<float*>(ws + w.slab_d), reinterpret_cast<float*>(ws + w.slab_bias)};
  if (pl.family == MC_SCAN_KERNEL_PAIR) return MC_OK;   // scan_bwd_pair.hip fills its own args
  fill_bwd_args(pl.a, p, pl.slabs, pl.rows);
  pl.a.dstate = p->dstate;
  pl.a.softplus = p->delta_softplus;
  pl.a.bq = reinterpret_cast<const float*>(pl.bq);
  pl.a.rev_groups = dirs ? p->reverse_groups : 0; pl.a.u_groups = dirs ? p->u_groups : 0;
  return MC_OK;
}

static int launch_bwd_generic(const BwdPlan& pl, int itype, hipStream_t s) {
  const BwdArgs& a = pl.a;
  const dim3 grid(a.total_blocks), block(kWG);
  MC_DISPATCH_T(itype, MC_DISPATCH_NP(padded_dstate(a.dstate), MC_DISPATCH_BOOL(pl.aligned, kAl, MC_DISPATCH_BOOL(
      a.softplus != 0, kSP, MC_DISPATCH_BOOL(a.rev_groups || a.u_groups, kDirs, hipLaunchKernelGGL(
          (scan_bwd_kernel<T, kN, kAl, kSP, kDirs>), grid, block, (bwd_lds_bytes<T, kN>()), s, a))))));
  return check_launch("mc_scan_bwd");
}

// dB / dC: sum the slabs of the workgroups (`rows` channels each) into the outputs, whose strides come from
// the params (all zero: contiguous (batch, G, dstate, seqlen)); dA / dD / dbias: sum the per-batch slabs.
static int launch_reduce(const mc_scan_bwd_params* p, const BwdSlabs& w, int rows, hipStream_t s) {
  const int np = padded_dstate(p->dstate), nblk = (p->dim / p->n_groups + rows - 1) / rows;
  BcOutStrides os = {{{p->dB_batch_stride, p->dB_group_stride, p->dB_dstate_stride},
                      {p->dC_batch_stride, p->dC_group_stride, p->dC_dstate_stride}}};
  for (auto& st : os.s)
    if (st[0] == 0 && st[1] == 0 && st[2] == 0) {
      st[0] = (int64_t)p->n_groups * p->dstate * p->seqlen; st[1] = (int64_t)p->dstate * p->seqlen; st[2] = p->seqlen;
    }
  const int64_t total = (int64_t)p->batch * p->n_groups * np * 2 * p->seqlen;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
  MC_DISPATCH_T(p->wtype, MC_DISPATCH_NP(np, hipLaunchKernelGGL(
      (scan_bwd_reduce_bc<T, kN>), dim3(grid), dim3(256), 0, s, w.bc, p->batch, p->n_groups, nblk, p->dstate,
      p->seqlen, p->reverse_groups, reinterpret_cast<T*>(p->dB), reinterpret_cast<T*>(p->dC), os)));
  // slab_a is [b][n][d]: column c = n * dim + d -> dA[d][n] (transposed on output)
  const int ca = p->dim * p->dstate;
  hipLaunchKernelGGL(scan_bwd_colsum_nd, dim3((ca + 31) / 32), dim3(256), 0, s, w.a, p->batch, p->dim, p->dstate,
                     (int64_t)p->dim * np, p->dA);
  float* dD = p->dD; float* dbias = p->ddelta_bias;
  if (dD && dbias)
    hipLaunchKernelGGL(scan_bwd_colsum, dim3((p->dim + 31) / 32, 2), dim3(256), 0, s, w.d, w.bias, p->batch, p->dim,
                       (int64_t)p->dim, dD, dbias);
  else if (dD || dbias)
    hipLaunchKernelGGL(scan_bwd_colsum, dim3((p->dim + 31) / 32), dim3(256), 0, s, dD ? w.d : w.bias, nullptr,
                       p->batch, p->dim, (int64_t)p->dim, dD ? dD : dbias, nullptr);
  const hipError_t e = hipGetLastError();
  MC_CHECK(e == hipSuccess, MC_ERR_LAUNCH, "mc_scan_bwd: reduce launch failed: %s", hipGetErrorString(e));
  return MC_OK;
}

}  // namespace scan
}  // namespace mc

using namespace mc;
using namespace mc::scan;

extern "C" size_t mc_scan_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate,
                                              int32_t n_groups) {
  if (batch <= 0 || dim <= 0 || seqlen <= 0 || dstate <= 0 || n_groups <= 0 || dim % n_groups) return 0;
  return bwd_ws_layout(batch, dim, seqlen, dstate, n_groups).total;
}

extern "C" int32_t mc_scan_bwd_kernel(const mc_scan_bwd_params* p) {
  BwdPlan pl;
  if (p) choose_bwd(p, pl);
  return pl.family;
}

extern "C" int mc_scan_bwd(const mc_scan_bwd_params* p, void* stream) {
  BwdPlan pl;
  MC_TRY(plan_bwd(p, pl));
  hipStream_t s = (hipStream_t)stream;
  if (pl.family == MC_SCAN_KERNEL_NONE) {
    // no positions: parameter gradients are zero, per-position gradients are empty
    (void)hipMemsetAsync(p->dA, 0, (size_t)p->dim * p->dstate * 4, s);
    if (p->dD) (void)hipMemsetAsync(p->dD, 0, (size_t)p->dim * 4, s);
    if (p->ddelta_bias) (void)hipMemsetAsync(p->ddelta_bias, 0, (size_t)p->dim * 4, s);
    return MC_OK;
  }
  if (pl.family == MC_SCAN_KERNEL_PAIR) {
    launch_bwd_pair(p, pl.slabs, s);
    MC_TRY(check_launch("mc_scan_bwd"));
  } else {
    const hipError_t e = launch_bc_quads(p, pl.bq, s);
    MC_CHECK(e == hipSuccess, MC_ERR_LAUNCH, "mc_scan_bwd: B/C quad relayout launch failed: %s", hipGetErrorString(e));
    MC_TRY(launch_bwd_generic(pl, p->itype, s));
  }
  return launch_reduce(p, pl.slabs, pl.rows, s);
}
