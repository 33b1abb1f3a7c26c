// scan_fwd.hip -- selective-scan forward for MI355X (gfx950, CDNA4).
//
// Computes (reference semantics: /root/reference/src/mamba_clip/model.py:83-169,
// the op behind mamba_ssm's selective_scan_fn called at model.py:539-550):
//   dt   = softplus(delta + delta_bias[d])                  (optional softplus / bias)
//   x_t  = exp(dt_t * A[d,n]) * x_{t-1} + dt_t * B[b,g,n,t] * u_t
//   y_t  = sum_n C[b,g,n,t] * x_t[n]  (+ D[d] * u_t)  (* silu(z_t))
//
// Design (DESIGN.md "scan_fwd"):
//  * One lane owns one (b, d) channel and keeps its dstate states in VGPRs,
//    walking the sequence in chunks of kT = 32 positions: the work-optimal
//    form of the recurrence (no parallel-prefix overhead).  B*D channels give
//    thousands of waves at the benchmark shapes.
//  * A workgroup is ONE wave = 64 channels of one (batch, group): no
//    inter-wave barriers, fine-grained grid (no tail), XCD-aware ordering so
//    the waves of one batch share an XCD's L2.
//  * B_t / C_t are wave-uniform: a pre-pass re-lays them out as fp32
//    [b][g][l][2N]; each chunk's slice is staged in LDS and read with
//    broadcast ds_read_b128 (one address for all lanes).
//  * u / delta tiles move HBM -> registers (next chunk, prefetched under the
//    current chunk's recurrence) -> LDS with fully coalesced 16-B loads along
//    the sequence; each lane then reads back its own row (conflict-free).
//    y (+D u) is written back over the consumed row in fp32, and a
//    cooperative pass applies the z gate with coalesced z loads / out stores.
//  * exp(dt*A) = exp2(dt * A*log2e) on v_exp_f32.
#include <cstdlib>

#include "scan_common.h"

namespace mc {
namespace scan {

// FwdArgs, the row checks and the dispatch macros: scan_common.h
int launch_fwd_pair(const FwdArgs& a, int itype, hipStream_t s);   // scan_fwd_pair.hip

// B/C as the recurrence consumes them: fp32, position-major, [b][g][l][2*kNp]
// (B states 0..kNp-1 then C states; states >= dstate are zero).  Every lane of
// a wave reads the same position, so one chunk of it is a contiguous block
// that is staged in LDS once per wave and broadcast-read.
static size_t bct_bytes(int batch, int seqlen, int dstate, int n_groups) {
  return (size_t)batch * n_groups * seqlen * 2 * padded_dstate(dstate) * sizeof(float);
}

// Re-lay B/C (any strides along b/g/n, unit stride along l) into the fp32
// position-major buffer.  One thread per (b, g, l, j<2kNp).
template <typename TW, int kNp>
__global__ __launch_bounds__(256) void bc_relayout_kernel(const TW* __restrict__ B, const TW* __restrict__ C,
                                                         int64_t B_bs, int64_t B_gs, int64_t B_ns, int64_t C_bs,
                                                         int64_t C_gs, int64_t C_ns, int batch, int G, int L,
                                                         int dstate, int rev, float* __restrict__ out) {
  const int64_t total = (int64_t)batch * G * L * 2 * kNp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % (2 * kNp));
    const int64_t rest = i / (2 * kNp);
    const int l = (int)(rest % L);
    const int64_t bg = rest / L;
    const int g = (int)(bg % G), b = (int)(bg / G);
    const bool isC = j >= kNp;
    const int n = isC ? j - kNp : j;
    float v = 0.f;
    if (n < dstate) {
      const TW* src = isC ? C + (int64_t)b * C_bs + (int64_t)g * C_gs + (int64_t)n * C_ns
                          : B + (int64_t)b * B_bs + (int64_t)g * B_gs + (int64_t)n * B_ns;
      v = to_f(src[((rev >> g) & 1) ? L - 1 - l : l]);   // reversed groups: mirrored positions
    }
    out[i] = v;
  }
}

// Vector form for 16-bit B/C with 16-B aligned rows, L % 8 == 0 and no reversed groups (every
// long-sequence call): one thread per (b, g, 8-position block, B|C half) reads kNp 16-B row
// vectors and writes its half of 8 position rows as float4s (the element-wise kernel above
// moves 2-B loads and 4-B stores: 31 us at C4).
template <typename TW, int kNp>
__global__ __launch_bounds__(256) void bc_relayout_vec_kernel(const TW* __restrict__ B, const TW* __restrict__ C,
                                                             int64_t B_bs, int64_t B_gs, int64_t B_ns, int64_t C_bs,
                                                             int64_t C_gs, int64_t C_ns, int batch, int G, int L,
                                                             int dstate, float* __restrict__ out) {
  const int nblk = L / 8;
  const int64_t total = (int64_t)batch * G * nblk * 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int half = (int)(i & 1);
    const int64_t rest = i >> 1;
    const int lb = (int)(rest % nblk);
    const int64_t bg = rest / nblk;
    const int g = (int)(bg % G), b = (int)(bg / G);
    const TW* src = half ? C + (int64_t)b * C_bs + (int64_t)g * C_gs : B + (int64_t)b * B_bs + (int64_t)g * B_gs;
    const int64_t ns = half ? C_ns : B_ns;
    uint4 q[kNp];
#pragma unroll
    for (int n = 0; n < kNp; ++n)
      q[n] = n < dstate ? ld16(src + (int64_t)n * ns + 8 * lb) : make_uint4(0u, 0u, 0u, 0u);
    float* dst = out + ((bg * L + 8 * lb) * 2 + half) * kNp;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int n4 = 0; n4 < kNp / 4; ++n4)
        reinterpret_cast<float4*>(dst + e * 2 * kNp)[n4] =
            make_float4(elem_f<TW>(q[4 * n4], e), elem_f<TW>(q[4 * n4 + 1], e), elem_f<TW>(q[4 * n4 + 2], e),
                        elem_f<TW>(q[4 * n4 + 3], e));
  }
}

static hipError_t relayout_bc(const mc_scan_fwd_params* p, int rev, float* out, hipStream_t s) {
  const int np = padded_dstate(p->dstate), batch = p->batch, G = p->n_groups, L = p->seqlen, dstate = p->dstate;
  const int64_t B_bs = p->B_batch_stride, B_gs = p->B_group_stride, B_ns = p->B_dstate_stride;
  const int64_t C_bs = p->C_batch_stride, C_gs = p->C_group_stride, C_ns = p->C_dstate_stride;
  if (elem_bytes(p->wtype) == 2 && rev == 0 && L % 8 == 0 && vec_ok(p->B, B_bs, B_gs, B_ns, 2) &&
      vec_ok(p->C, C_bs, C_gs, C_ns, 2)) {
    const int64_t tv = (int64_t)batch * G * (L / 8) * 2;
    const int gv = (int)std::min<int64_t>((tv + 255) / 256, 16384);
    MC_DISPATCH_T16(p->wtype, MC_DISPATCH_NP(np, hipLaunchKernelGGL(
        (bc_relayout_vec_kernel<T, kN>), gv, 256, 0, s, reinterpret_cast<const T*>(p->B),
        reinterpret_cast<const T*>(p->C), B_bs, B_gs, B_ns, C_bs, C_gs, C_ns, batch, G, L, dstate, out)));
    return hipGetLastError();
  }
  const int64_t total = (int64_t)batch * G * L * 2 * np;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
  MC_DISPATCH_T(p->wtype, MC_DISPATCH_NP(np, hipLaunchKernelGGL(
      (bc_relayout_kernel<T, kN>), grid, 256, 0, s, reinterpret_cast<const T*>(p->B),
      reinterpret_cast<const T*>(p->C), B_bs, B_gs, B_ns, C_bs, C_gs, C_ns, batch, G, L, dstate, rev, out)));
  return hipGetLastError();
}

// LDS row of one channel for one chunk: kT / VI blocks; block k = {u vector k
// (16 B = VI steps), delta vector k (16 B)}.  After consuming block k the
// thread writes y for those VI steps (fp32, 4*VI <= 32 B) over the block, so
// the y tile costs no extra LDS.  Row stride = data + 16 B: conflict-free
// ds_read_b128 when every lane reads its own row.
template <typename TI>
struct RowLayout {
  static constexpr int VI = ElemTraits<TI>::kVec;
  static constexpr int kBlock = 32;
  static constexpr int kBlocks = kT / VI;
  static constexpr int kBytes = kBlocks * kBlock;
  static constexpr int kStride = kBytes + 16;
};


// The long-sequence kernel: the recurrence runs in groups of kG = 4 steps whose u / delta are read
// from LDS together and whose four fp32 y values go back over exactly those bytes; the next chunk's
// u / delta vectors and B/C block are prefetched into registers under the current chunk's recurrence.
// 16-bit rows are sized for 2 waves per SIMD; fp32 rows double the prefetch registers, and one wave
// per SIMD keeps them out of scratch (the SS2D grids are a few hundred waves, occupancy buys nothing
// there).  At C4 (B=64, D=3072: 3072 one-wave workgroups on 1024 SIMDs) the kernel is
// VALU + v_exp issue bound (~33 SIMD cycles per wave per (t, n) step, measured
// the same at 1 and 2 waves per SIMD), not HBM bound.
// kAligned: 0 = element-wise rows, 1 = 16-B aligned rows, 2 = aligned and every chunk
// full (seqlen % kT == 0: no masked-load code at all, which keeps the register
// budget of the 3-waves-per-SIMD build free of spills)
// kSP: softplus on delta (a template flag: a runtime one is a uniform branch per position
// that splits the recurrence into small basic blocks)
constexpr int kG = 4;   // steps per recurrence group
template <typename TI, int kN, int kAligned, bool kSP>
__global__ __launch_bounds__(kRows, sizeof(TI) == 4 ? 1 : 2) void scan_fwd_kernel(const FwdArgs a) {
  using RL = RowLayout<TI>;
  constexpr int VI = RL::VI;                    // elements per 16-B vector
  constexpr int kVPR = kT / VI;                 // vectors per row segment per array

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* rowbuf = smem;
  float* bcl = reinterpret_cast<float*>(smem + kRows * RL::kStride);   // [kT][2kN] (mode 1)

  const int lane = threadIdx.x;
  const int lin = xcd_remap(blockIdx.x, a.total_blocks);
  const int dblk = lin % a.nblk;
  const int bg = lin / a.nblk;
  const int g = bg % a.n_groups, b = bg / a.n_groups;
  const int H = a.dim / a.n_groups;
  const int dbase = g * H + dblk * kRows;
  const int nrows = min(kRows, H - dblk * kRows);
  const int L_ = a.seqlen;
  const bool hasZ = a.z != nullptr;

  const TI* __restrict__ u = reinterpret_cast<const TI*>(a.u) + (int64_t)b * a.u_bs;
  // grouped directions: reversed groups walk mirrored positions; u_groups > 0 shares u blocks
  // (vector modes: the host guarantees seqlen % VI == 0, so a mirrored 16-B block is aligned)
  const bool rev = (a.rev_groups >> g) & 1;
  const int urow0 = a.u_groups ? (g % a.u_groups) * H + dblk * kRows : dbase;
  const TI* __restrict__ dl = reinterpret_cast<const TI*>(a.delta) + (int64_t)b * a.dt_bs;
  const TI* __restrict__ zp = reinterpret_cast<const TI*>(a.z) + (int64_t)b * a.z_bs;
  TI* __restrict__ out = reinterpret_cast<TI*>(a.out) + (int64_t)b * a.o_bs;
  // (whole-chunk mode) this wave's rows of u / delta / z / out as buffer ranges: 32-bit offsets
  auto rows_rsrc = [&](const void* base, int64_t ds, int row0 = -1) {
    return make_rsrc(reinterpret_cast<const TI*>(base) + (int64_t)(row0 < 0 ? dbase : row0) * ds,
                     (uint32_t)(((int64_t)(nrows - 1) * ds + L_) * (int64_t)sizeof(TI)));
  };
  const __amdgpu_buffer_rsrc_t rs_out = rows_rsrc(out, a.o_ds);
  const __amdgpu_buffer_rsrc_t rs_u = rows_rsrc(u, a.u_ds, urow0), rs_d = rows_rsrc(dl, a.dt_ds);
  const __amdgpu_buffer_rsrc_t rs_z = rows_rsrc(hasZ ? (const void*)zp : (const void*)u, hasZ ? a.z_ds : a.u_ds);
  const __amdgpu_buffer_rsrc_t rs_y =
      rows_rsrc(a.out_y ? (const void*)(reinterpret_cast<const TI*>(a.out_y) + (int64_t)b * a.y_bs) : (const void*)u,
                a.out_y ? a.y_ds : a.u_ds);

  // ---- per-channel constants
  const int my_d = dbase + lane;
  const bool my_ok = lane < nrows;
  // states are processed in pairs with packed fp32 math (v_pk_mul_f32 / v_pk_fma_f32)
  // unconditional loads (clamped row / state index), masked afterwards: no load behind a branch
  f32x2 A2[kN / 2];
  const int my_dc = dbase + min(lane, nrows - 1);
  {
    float av[kN];
#pragma unroll
    for (int n = 0; n < kN; ++n) av[n] = a.A[(int64_t)my_dc * a.dstate + min(n, a.dstate - 1)];
#pragma unroll
    for (int n = 0; n < kN; ++n) {
      const float v = (my_ok && n < a.dstate) ? av[n] * kLog2e : 0.f;
      if (n & 1) A2[n / 2].y = v; else A2[n / 2].x = v;
    }
  }
  const float Dv = (my_ok && a.D) ? a.D[my_dc] : 0.f;
  const float biasv = (my_ok && a.delta_bias) ? a.delta_bias[my_dc] : 0.f;

  f32x2 x[kN / 2];
#pragma unroll
  for (int n = 0; n < kN / 2; ++n) x[n] = f32x2{0.f, 0.f};

  // ---- register prefetch of the next chunk (issued before this chunk's
  // recurrence, consumed after it): u / delta vectors + the B/C chunk.
  constexpr int kBCVec = kT * 2 * kN / 4;                 // float4s in one B/C chunk
  constexpr int kBCPer = (kBCVec + kRows - 1) / kRows;
  uint4 pu[kVPR], pd[kVPR];
  float4 pbc[kBCPer];
  // (whole-chunk mode) this (batch, group)'s B/C rows as a buffer range: chunks past
  // the end read 0, so the prefetch needs no branch (a branch around loads makes the
  // compiler drain the stores issued after them before the loads may be consumed)
  const __amdgpu_buffer_rsrc_t rs_bc = make_rsrc(a.bct + (int64_t)bg * L_ * (2 * kN), (uint32_t)L_ * (2 * kN) * 4u);
  auto load_bc = [&](int l0, float4 (&dst)[kBCPer]) {
    if constexpr (kAligned == 2) {
#pragma unroll
      for (int k = 0; k < kBCPer; ++k) {
        const int v = lane + k * kRows;
        const uint32_t off = v < kBCVec ? (uint32_t)(l0 * (2 * kN) + 4 * v) * 4u : 0x80000000u;
        dst[k] = __builtin_bit_cast(float4, buf_ld16(rs_bc, off));
      }
      return;
    }
    const float4* src = reinterpret_cast<const float4*>(a.bct + ((int64_t)bg * L_ + l0) * (2 * kN));
    const int nvec = min(kT, L_ - l0) * (2 * kN) / 4;
#pragma unroll
    for (int k = 0; k < kBCPer; ++k) {
      const int v = lane + k * kRows;
      dst[k] = v < nvec ? src[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto load_regs = [&](int l0) {
    const bool full = kAligned == 2 || (kAligned == 1 && l0 + kT <= L_);
#pragma unroll
    for (int k = 0; k < kVPR; ++k) {
      const int j = lane + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      const int rr = min(r, nrows - 1);   // rows past the group end: load a valid row, never stored
      const int col0 = l0 + c * VI;
      if constexpr (kAligned == 2) {   // 32-bit offsets into the wave's row block (no 64-bit pointers)
        // reversed group: ascending mirrored block (mc_common.h ld16_rev; past the end it goes
        // negative -> wraps out of range for row 0, reads an unused neighbour otherwise: never consumed)
        const int cm = rev ? L_ - l0 - kT + c * VI : col0;
        // (element order is reversed at staging: touching the values here would wait for the loads)
        pu[k] = buf_ld16(rs_u, (uint32_t)(rr * a.u_ds + cm) * (uint32_t)sizeof(TI));
        pd[k] = buf_ld16(rs_d, (uint32_t)(rr * a.dt_ds + cm) * (uint32_t)sizeof(TI));
        continue;
      }
      if (rev) {
        const int nv = max(0, min(VI, L_ - (l0 + (kVPR - 1 - c) * VI)));   // steps < L of block kVPR-1-c
        const int cm = L_ - l0 - kT + c * VI;
        pu[k] = ld16_top(u + (int64_t)(urow0 + rr) * a.u_ds, cm, nv);   // flipped at staging
        pd[k] = ld16_top(dl + (int64_t)(dbase + rr) * a.dt_ds, cm, nv);
        continue;
      }
      const TI* su = u + (int64_t)(urow0 + rr) * a.u_ds + col0;
      const TI* sd = dl + (int64_t)(dbase + rr) * a.dt_ds + col0;
      if (full) {
        pu[k] = ld16(su);
        pd[k] = ld16(sd);
      } else {
        const int nv = max(0, min(VI, L_ - col0));
        pu[k] = ld16_masked(su, nv);
        pd[k] = ld16_masked(sd, nv);
      }
    }
    load_bc(l0, pbc);
  };

  load_regs(0);
  for (int ch = 0; ch < a.n_chunks; ++ch) {
    const int l0 = ch * kT;
    const bool full = kAligned == 2 || (kAligned == 1 && l0 + kT <= L_);

    // ---- stage u / delta (vector j = lane + k*64 -> row j / kVPR, col j % kVPR) and B/C
#pragma unroll
    for (int k = 0; k < kVPR; ++k) {
      const int j = lane + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      char* blk = rowbuf + r * RL::kStride + (rev ? kVPR - 1 - c : c) * RL::kBlock;   // reversed: mirrored block
      st16(blk, rev ? reverse_elems<TI>(pu[k]) : pu[k]);        // mirrored blocks arrive in memory order
      st16(blk + 16, rev ? reverse_elems<TI>(pd[k]) : pd[k]);
    }
    {
      float4 cur[kBCPer];
#pragma unroll
      for (int k = 0; k < kBCPer; ++k) cur[k] = pbc[k];
#pragma unroll
      for (int k = 0; k < kBCPer; ++k) {
        const int v = lane + k * kRows;
        if (v < kBCVec) reinterpret_cast<float4*>(bcl)[v] = cur[k];
      }
    }
    wave_lds_sync();
    if constexpr (kAligned == 2) load_regs(l0 + kT);   // past the end: out-of-range offsets read 0
    else if (ch + 1 < a.n_chunks) load_regs(l0 + kT);
    // this chunk's z vectors (gate pass mapping), loaded now so that they arrive
    // under the recurrence instead of stalling the gate pass
    uint4 cz[kVPR];
    if (hasZ) {
      const int ln = kAligned == 2 ? opaque_lane_id() : lane;   // rebuilt here, not held live
#pragma unroll
      for (int k = 0; k < kVPR; ++k) {
        const int j = ln + k * kRows;
        const int r = j / kVPR, c = j % kVPR;
        const int col0 = l0 + c * VI;
        if constexpr (kAligned == 2) {
          cz[k] = buf_ld16(rs_z, (uint32_t)(min(r, nrows - 1) * a.z_ds + col0) * (uint32_t)sizeof(TI));
        } else {
          const TI* zs = zp + (int64_t)(dbase + min(r, nrows - 1)) * a.z_ds + col0;
          cz[k] = full ? ld16(zs) : ld16_masked(zs, max(0, min(VI, L_ - col0)));
        }
      }
    }

    // ---- the recurrence over this chunk, one channel per lane.  Steps go
    // in groups of kG: read the group's u / delta (kG elements each), run
    // kG steps, write the kG fp32 y values back over exactly those bytes.
    {
      char* row = rowbuf + lane * RL::kStride;
#pragma unroll 1
      for (int t0 = 0; t0 < kT; t0 += kG) {
        char* pu = row + (t0 / VI) * RL::kBlock + (t0 % VI) * (int)sizeof(TI);
        char* pd = pu + 16;
        float uu[kG], dd[kG];
        {
          constexpr int kB = kG * (int)sizeof(TI);   // bytes of one array in this group
          uint4 qa, qb;
          if constexpr (kB == 16) { qa = ld16(pu); qb = ld16(pd); }
          else {
            static_assert(kB == 8, "a group is 16 B (fp32) or 8 B (16-bit) per array");
            const uint2 a2 = *reinterpret_cast<const uint2*>(pu), b2 = *reinterpret_cast<const uint2*>(pd);
            qa = make_uint4(a2.x, a2.y, 0u, 0u); qb = make_uint4(b2.x, b2.y, 0u, 0u);
          }
#pragma unroll
          for (int e = 0; e < kG; ++e) { uu[e] = elem_f<TI>(qa, e); dd[e] = elem_f<TI>(qb, e); }
        }
        float yv[kG];
#pragma unroll
        for (int e = 0; e < kG; ++e) {
          const int t = l0 + t0 + e;
          const float uv = uu[e];
          const float dr = dd[e] + biasv;
          float dt = kSP ? softplus_f(dr) : dr;
          if constexpr (kAligned != 2) dt = (t < L_) ? dt : 0.f;  // past the end: state frozen
          const float du = dt * uv;
          // every decay of this position first: each exp's result is consumed a
          // few pairs later, so no wait states sit between an exp and its use
          f32x2 dA[kN / 2];
#pragma unroll
          for (int p = 0; p < kN / 2; ++p) {
            const f32x2 arg = A2[p] * dt;                                   // v_pk_mul_f32
            dA[p] = f32x2{fast_exp2(arg.x), fast_exp2(arg.y)};
          }
          f32x2 y2 = {0.f, 0.f};
          {
            const f32x4* bc4 = reinterpret_cast<const f32x4*>(bcl + (t0 + e) * (2 * kN));
#pragma unroll
            for (int n4 = 0; n4 < kN / 4; ++n4) {
              const f32x4 bq = bc4[n4], cq = bc4[kN / 4 + n4];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const int p = 2 * n4 + h;
                const f32x2 bb = h ? bq.hi : bq.lo, cc = h ? cq.hi : cq.lo;
                x[p] = dA[p] * x[p] + bb * du;                              // v_pk_mul + v_pk_fma
                y2 = cc * x[p] + y2;                                        // v_pk_fma
              }
            }
          }
          yv[e] = fmaf(Dv, uv, y2.x + y2.y);
        }
        // y[0..kG/2) -> the u bytes, y[kG/2..kG) -> the delta bytes of this group
        if (a.chunk_states && my_ok && ((t0 + kG) % kS) == 0) {
          const int sc = (l0 + t0 + kG) / kS - 1;   // saved-state index: state after position sc*kS + kS - 1
          if (sc < a.n_states) {
            float* cs = a.chunk_states + (((int64_t)b * a.dim + my_d) * a.n_states + sc) * a.dstate;
            if ((a.dstate & 3) == 0) {
#pragma unroll
              for (int n4 = 0; n4 < kN / 4; ++n4)
                if (n4 * 4 < a.dstate)
                  reinterpret_cast<float4*>(cs)[n4] =
                      make_float4(x[2 * n4].x, x[2 * n4].y, x[2 * n4 + 1].x, x[2 * n4 + 1].y);
            } else {
#pragma unroll
              for (int n = 0; n < kN; ++n)
                if (n < a.dstate) cs[n] = (n & 1) ? x[n / 2].y : x[n / 2].x;
            }
          }
        }
        static_assert(kG == 4, "two y values over each array's bytes");
        *reinterpret_cast<float2*>(pu) = make_float2(yv[0], yv[1]);
        *reinterpret_cast<float2*>(pd) = make_float2(yv[2], yv[3]);
      }
    }
    wave_lds_sync();

    // ---- gate + store, coalesced along the sequence (same vector mapping)
    const int lg = kAligned == 2 ? opaque_lane_id() : lane;   // offsets rebuilt, not held live
#pragma unroll
    for (int k = 0; k < kVPR; ++k) {
      const int j = lg + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      const int cl = rev ? kVPR - 1 - c : c;          // LDS block of this lane's vector
      const int col0 = l0 + c * VI;
      const int cm = L_ - l0 - kT + c * VI;            // (reversed) ascending mirrored position
      const int nv = max(0, min(VI, L_ - (l0 + cl * VI)));
      float o[VI];
      // y of step s (within the chunk) lives in group s / kG: first half of the
      // group's y values at the u bytes, second half at the delta bytes.
#pragma unroll
      for (int e = 0; e < VI; ++e) {
        const int st = cl * VI + e;
        const int g0 = st - st % kG;
        const int ie = st % kG;
        const char* pu = rowbuf + r * RL::kStride + (g0 / VI) * RL::kBlock + (g0 % VI) * (int)sizeof(TI);
        o[e] = reinterpret_cast<const float*>(ie < kG / 2 ? pu : pu + 16)[ie % (kG / 2)];
      }
      if (hasZ) {
        if (a.out_y && r < nrows) {
          if constexpr (kAligned == 2) {
            buf_st16(rs_y, (uint32_t)(r * a.y_ds + col0) * (uint32_t)sizeof(TI), pack_f<TI>(o));
          } else {
            TI* ydst = reinterpret_cast<TI*>(a.out_y) + (int64_t)b * a.y_bs + (int64_t)(dbase + r) * a.y_ds + col0;
            const uint4 yq = pack_f<TI>(o);
            if (full) st16(ydst, yq);
            else st16_masked(ydst, yq, nv);
          }
        }
#pragma unroll
        for (int e = 0; e < VI; ++e) o[e] *= silu_f(elem_f<TI>(cz[k], e));
      }
      if constexpr (kAligned == 2) {
        // whole chunks: every lane stores (rows past the group end fall outside the
        // buffer range and are dropped), so the store count is static and the next
        // chunk's prefetch wait does not have to drain these stores
        const uint32_t off = r < nrows ? (uint32_t)(r * a.o_ds + (rev ? cm : col0)) * (uint32_t)sizeof(TI) : 0x80000000u;
        const uint4 ov = pack_f<TI>(o);
        buf_st16(rs_out, off, rev ? reverse_elems<TI>(ov) : ov);
      } else if (r < nrows) {
        const uint4 ov = pack_f<TI>(o);
        if (rev) {
          st16_rev(out + (int64_t)(dbase + r) * a.o_ds, cm, ov, nv);
        } else {
          TI* dst = out + (int64_t)(dbase + r) * a.o_ds + col0;
          if (full) st16(dst, ov);
          else st16_masked(dst, ov, nv);
        }
      }
    }
    wave_lds_sync();  // next chunk's staging overwrites the rows
  }

  if (a.last_state && my_ok) {
    float* ls = a.last_state + ((int64_t)b * a.dim + my_d) * a.dstate;
#pragma unroll
    for (int n = 0; n < kN; ++n)
      if (n < a.dstate) ls[n] = (n & 1) ? x[n / 2].y : x[n / 2].x;
  }
}

typedef __attribute__((address_space(4))) const f32x4 cf32x4;   // constant address space: scalar loads

// Row layout of the 16-position chunk kernel: per row {u vector, delta vector} blocks + 16-B pad.
template <typename TI>
struct RowLayoutP {
  static constexpr int kTP = 16;
  static constexpr int VI = ElemTraits<TI>::kVec;
  static constexpr int kBlock = 32;                 // {u vector, delta vector}
  static constexpr int kBlocks = kTP / VI;
  static constexpr int kStride = kBlocks * kBlock + 16;
};

// ------------------------------------------------------------------ short-sequence kernel
// One channel per lane like scan_fwd_kernel, but each position's B/C row is loaded once per wave
// into SGPRs (no LDS staging of B/C), chunks are 16 positions, and the budget is 3 waves per SIMD:
// with short sequences the grid is many short-lived waves and occupancy hides the latencies.
// u / delta / z of the next chunk are prefetched into registers during the current chunk (z too:
// the gate pass never waits on HBM).
template <typename TI, int kN, bool kAligned, bool kSP>
__global__ __launch_bounds__(kRows, 3) void scan_fwd_mc_kernel(const FwdArgs a) {
  // Channels per lane (row lane + 64 r of the wave's block).  Only 1 is built: 3 measured slower (table
  // above launch_fwd_n).  The loops over r stay: writing them out changes the code the compiler
  // generates for every instance (profiles/scan_cleanup/isa_identity.txt).
  constexpr int kR = 1;
  using RL = RowLayoutP<TI>;
  constexpr int kTP = RL::kTP;
  constexpr int VI = RL::VI;
  constexpr int kVPR = kTP / VI;                  // vectors per row per array
  constexpr int kQ = kN / 4;
  constexpr int kW = kRows * kR;                  // channels per wave
  constexpr int kVL = kR * kVPR;                  // staged vectors per lane per array
  static_assert(kS % kTP == 0, "saved states fall on chunk ends");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* rowbuf = smem;                            // [kW][RL::kStride]

  const int lane = threadIdx.x;
  const int lin = xcd_remap(blockIdx.x, a.total_blocks);
  const int dblk = lin % a.nblk;
  const int bg = lin / a.nblk;
  const int g = bg % a.n_groups, b = bg / a.n_groups;
  const int H = a.dim / a.n_groups;
  const int dbase = g * H + dblk * kW;
  const int nrows = min(kW, H - dblk * kW);
  const int L_ = a.seqlen;
  const bool hasZ = a.z != nullptr;
  const int n_chunks = (L_ + kTP - 1) / kTP;

  const TI* __restrict__ u = reinterpret_cast<const TI*>(a.u) + (int64_t)b * a.u_bs;
  const TI* __restrict__ dl = reinterpret_cast<const TI*>(a.delta) + (int64_t)b * a.dt_bs;
  const TI* __restrict__ zp = reinterpret_cast<const TI*>(a.z) + (int64_t)b * a.z_bs;
  TI* __restrict__ out = reinterpret_cast<TI*>(a.out) + (int64_t)b * a.o_bs;
  const cf32x4* bcs = (const cf32x4*)(a.bct + (int64_t)bg * L_ * (2 * kN));

  // channel r of this lane: row lane + 64 r of the wave's block
  f32x2 A2[kR][kN / 2], x[kR][kN / 2];
  float Dv[kR], biasv[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int row = lane + kRows * r;
    const bool ok = row < nrows;
    const int d = dbase + min(row, nrows - 1);
#pragma unroll
    for (int n = 0; n < kN; ++n) {
      const float v = (ok && n < a.dstate) ? a.A[(int64_t)d * a.dstate + n] * kLog2e : 0.f;
      if (n & 1) A2[r][n / 2].y = v; else A2[r][n / 2].x = v;
    }
    Dv[r] = (ok && a.D) ? a.D[d] : 0.f;
    biasv[r] = (ok && a.delta_bias) ? a.delta_bias[d] : 0.f;
#pragma unroll
    for (int p = 0; p < kN / 2; ++p) x[r][p] = f32x2{0.f, 0.f};
  }

  // staged vector k of this lane: j = lane + 64 k -> row j / kVPR, column block j % kVPR
  uint4 pu[kVL], pd[kVL], pz[kVL];
  auto load_regs = [&](int l0) {
    const bool full = kAligned && (l0 + kTP <= L_);
#pragma unroll
    for (int k = 0; k < kVL; ++k) {
      const int j = lane + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      const int rr = min(r, nrows - 1);
      const int col0 = l0 + c * VI;
      const TI* su = u + (int64_t)(dbase + rr) * a.u_ds + col0;
      const TI* sd = dl + (int64_t)(dbase + rr) * a.dt_ds + col0;
      const TI* sz = zp + (int64_t)(dbase + rr) * a.z_ds + col0;
      if (full) {
        pu[k] = ld16(su);
        pd[k] = ld16(sd);
        if (hasZ) pz[k] = ld16(sz);
      } else {
        const int nv = max(0, min(VI, L_ - col0));
        pu[k] = ld16_masked(su, nv);
        pd[k] = ld16_masked(sd, nv);
        if (hasZ) pz[k] = ld16_masked(sz, nv);
      }
    }
  };
  auto load_bc = [&](int t, f32x4 (&dst)[2 * kQ]) {
    const cf32x4* src = bcs + (int64_t)min(t, L_ - 1) * (2 * kQ);
#pragma unroll
    for (int k = 0; k < 2 * kQ; ++k) dst[k] = src[k];
  };

  f32x4 bcA[2 * kQ], bcB[2 * kQ];
  load_bc(0, bcA);
  load_regs(0);
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int l0 = ch * kTP;
    const bool full = kAligned && (l0 + kTP <= L_);
#pragma unroll
    for (int k = 0; k < kVL; ++k) {
      const int j = lane + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      char* blk = rowbuf + r * RL::kStride + c * RL::kBlock;
      st16(blk, pu[k]);
      st16(blk + 16, pd[k]);
    }
    uint4 cz[kVL];
#pragma unroll
    for (int k = 0; k < kVL; ++k) cz[k] = pz[k];
    wave_lds_sync();
    uint4 ru[kR][kVPR], rd[kR][kVPR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const char* rowp = rowbuf + (lane + kRows * r) * RL::kStride;
#pragma unroll
      for (int k = 0; k < kVPR; ++k) {
        ru[r][k] = ld16(rowp + k * RL::kBlock);
        rd[r][k] = ld16(rowp + k * RL::kBlock + 16);
      }
    }
    if (ch + 1 < n_chunks) load_regs(l0 + kTP);

    auto step = [&](int tt, const f32x4 (&cur)[2 * kQ], f32x4 (&nxt)[2 * kQ]) {
      const int t = l0 + tt;
      __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): cur (issued a position ago) is back
      __builtin_amdgcn_sched_barrier(0);
      load_bc(t + 1, nxt);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const float uv = elem_f<TI>(ru[r][tt / VI], tt % VI);
        const float dr = elem_f<TI>(rd[r][tt / VI], tt % VI) + biasv[r];
        float dt = kSP ? softplus_f(dr) : dr;   // template flag: no per-position branch
        dt = (t < L_) ? dt : 0.f;
        const float du = dt * uv;
        f32x2 ya = {0.f, 0.f}, yb = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const f32x4 bq = cur[q], cq = cur[kQ + q];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int p = 2 * q + h;
            const f32x2 bb = h ? bq.hi : bq.lo, cc = h ? cq.hi : cq.lo;
            const f32x2 arg = A2[r][p] * dt;
            const f32x2 dA = {fast_exp2(arg.x), fast_exp2(arg.y)};
            x[r][p] = dA * x[r][p] + bb * du;
            if (h) yb = cc * x[r][p] + yb;
            else ya = cc * x[r][p] + ya;
          }
        }
        const f32x2 ys = ya + yb;
        reinterpret_cast<float*>(rowbuf + (lane + kRows * r) * RL::kStride)[tt] = fmaf(Dv[r], uv, ys.x + ys.y);
      }
    };
#pragma unroll
    for (int tt = 0; tt < kTP; tt += 2) {
      step(tt, bcA, bcB);
      step(tt + 1, bcB, bcA);
    }
    // saved state after every kS positions and after the last chunk (positions
    // past L froze the state, so that one is the state after position L-1)
    if (a.chunk_states && (((l0 + kTP) % kS) == 0 || ch == n_chunks - 1)) {
      const int sc = (l0 + kTP + kS - 1) / kS - 1;
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int row = lane + kRows * r;
        if (row < nrows && sc < a.n_states) {
          float* cs = a.chunk_states + (((int64_t)b * a.dim + dbase + row) * a.n_states + sc) * a.dstate;
          if ((a.dstate & 3) == 0) {
#pragma unroll
            for (int n4 = 0; n4 < kN / 4; ++n4)
              if (n4 * 4 < a.dstate)
                reinterpret_cast<float4*>(cs)[n4] =
                    make_float4(x[r][2 * n4].x, x[r][2 * n4].y, x[r][2 * n4 + 1].x, x[r][2 * n4 + 1].y);
          } else {
#pragma unroll
            for (int n = 0; n < kN; ++n)
              if (n < a.dstate) cs[n] = (n & 1) ? x[r][n / 2].y : x[r][n / 2].x;
          }
        }
      }
    }
    wave_lds_sync();

    // ---- gate + store, coalesced along the sequence (z prefetched a chunk ago)
#pragma unroll
    for (int k = 0; k < kVL; ++k) {
      const int j = lane + k * kRows;
      const int r = j / kVPR, c = j % kVPR;
      const int col0 = l0 + c * VI;
      const int nv = max(0, min(VI, L_ - col0));
      float o[VI];
      const float4* yv = reinterpret_cast<const float4*>(rowbuf + r * RL::kStride + c * VI * 4);
#pragma unroll
      for (int e4 = 0; e4 < VI / 4; ++e4) {
        const float4 q = yv[e4];
        o[4 * e4] = q.x; o[4 * e4 + 1] = q.y; o[4 * e4 + 2] = q.z; o[4 * e4 + 3] = q.w;
      }
      if (hasZ) {
        if (a.out_y && r < nrows) {
          TI* ydst = reinterpret_cast<TI*>(a.out_y) + (int64_t)b * a.y_bs + (int64_t)(dbase + r) * a.y_ds + col0;
          const uint4 yq = pack_f<TI>(o);
          if (full) st16(ydst, yq);
          else st16_masked(ydst, yq, nv);
        }
#pragma unroll
        for (int e = 0; e < VI; ++e) o[e] *= silu_f(elem_f<TI>(cz[k], e));
      }
      if (r < nrows) {
        TI* dst = out + (int64_t)(dbase + r) * a.o_ds + col0;
        const uint4 ov = pack_f<TI>(o);
        if (full) st16(dst, ov);
        else st16_masked(dst, ov, nv);
      }
    }
    wave_lds_sync();
  }

#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int row = lane + kRows * r;
    if (a.last_state && row < nrows) {
      float* ls = a.last_state + ((int64_t)b * a.dim + dbase + row) * a.dstate;
#pragma unroll
      for (int n = 0; n < kN; ++n)
        if (n < a.dstate) ls[n] = (n & 1) ? x[r][n / 2].y : x[r][n / 2].x;
    }
  }
}

// ------------------------------------------------------------------ host: plan and dispatch
// Kernel choice, measured on MI355X (ms, bf16, z, softplus):
//                                         C4 64x3072x4096   C2 256x1536x80
//   scan_fwd_kernel (kG 4, LDS B/C, 2 w/SIMD)     3.17 (r01: 3.35) 0.204
//   scan_fwd_mc_kernel (SGPR B/C, 16-pos)         3.87             0.152
//   the same with 3 channels per lane (1 w/SIMD)  3.66             0.180
// Tried, slower (git history has the kernels): per-position LDS broadcast at 3 w/SIMD
// 3.96 / 0.188; two-wave state split with SGPR half-rows 6.41 / 0.266; two-wave
// state split with LDS-staged rows and LDS partial-y sums (no 2+1 tail: 6
// half-tasks per SIMD) 3.92 at C4 -- the per-position work both waves repeat
// (row reads, softplus, y hand-off) costs more than the tail it removes;
// vector-load B/C rings spill at the occupancy they need.  With short
// sequences the grid is many short-lived waves and the SGPR-fed kernel wins;
// with long ones the LDS-staged kernel's deeper prefetch wins.  Grouped directions
// (per-group addressing) live in the LDS-staged kernel only.
//
// Everything mc_scan_fwd does for a call, decided in one place; the queries read the same plan.
struct FwdPlan {
  int family = MC_SCAN_KERNEL_NONE;   // MC_SCAN_KERNEL_*; NONE: nothing to launch
  bool mc = false;                    // general kernels: scan_fwd_mc_kernel (else the LDS-staged scan_fwd_kernel)
  int aligned = 0;                    // general kernels: row mode 0 / 1 / 2 (scan_fwd_mc_kernel: 0 / 1)
  int state_interval = kS;            // the interval the call saves states with
  FwdArgs a;
};
static_assert(kS == kT, "the pair kernel saves its default states at the ends of the forward's tiles");

// FwdArgs of a planned call; `rows`: channels per workgroup of the chosen kernel.  The workspace is the
// relaid B / C of the general kernels (the pair kernel reads the rows as given).
static void fill_fwd_args(const mc_scan_fwd_params* p, const FwdPlan& pl, int rows, FwdArgs& a) {
  const bool dirs = has_dirs(p->reverse_groups, p->u_groups);
  a.batch = p->batch; a.dim = p->dim; a.seqlen = p->seqlen; a.dstate = p->dstate; a.n_groups = p->n_groups;
  a.n_chunks = (p->seqlen + kT - 1) / kT;
  a.n_states = mc_scan_n_states(p->seqlen, pl.state_interval);
  a.nblk = (int)(((int64_t)p->dim / p->n_groups + rows - 1) / rows);   // 64-bit: no trap on unvalidated params
  a.total_blocks = p->batch * p->n_groups * a.nblk;
  a.softplus = p->delta_softplus;
  a.u_bs = p->u_batch_stride; a.u_ds = p->u_dim_stride;
  a.dt_bs = p->delta_batch_stride; a.dt_ds = p->delta_dim_stride;
  a.z_bs = p->z_batch_stride; a.z_ds = p->z_dim_stride;
  a.o_bs = p->out_batch_stride; a.o_ds = p->out_dim_stride;
  a.u = p->u; a.delta = p->delta; a.A = p->A; a.bct = reinterpret_cast<const float*>(p->workspace);
  a.D = p->D; a.z = p->z; a.delta_bias = p->delta_bias;
  a.out = p->out; a.chunk_states = p->chunk_states; a.last_state = p->last_state;
  a.out_y = p->z ? p->out_y : nullptr; a.y_bs = p->out_y_batch_stride; a.y_ds = p->out_y_dim_stride;
  a.rev_groups = dirs ? p->reverse_groups : 0; a.u_groups = dirs ? p->u_groups : 0;
  a.B = p->B; a.C = p->C;
  a.B_bs = p->B_batch_stride; a.B_gs = p->B_group_stride; a.B_ns = p->B_dstate_stride;
  a.C_bs = p->C_batch_stride; a.C_gs = p->C_group_stride; a.C_ns = p->C_dstate_stride;
  a.state_interval = pl.state_interval;
}

// The choice: what a call with these params runs.  It reads shapes, strides and pointer alignment only,
// reports no error and touches nothing else, so the queries answer from it for any params, valid or not;
// n_groups == 0 (no channels per group to divide into) leaves the defaults, NONE / kS.
static void choose_fwd(const mc_scan_fwd_params* p, FwdPlan& pl) {
  pl = FwdPlan{};
  if (p->n_groups == 0) return;
  const bool empty = p->batch == 0 || p->seqlen == 0, dirs = has_dirs(p->reverse_groups, p->u_groups);
  const int ib = elem_bytes(p->itype);
  const Rows rows[] = {{p->u, p->u_batch_stride, p->u_dim_stride},
                       {p->delta, p->delta_batch_stride, p->delta_dim_stride},
                       {p->z, p->z_batch_stride, p->z_dim_stride},
                       {p->out, p->out_batch_stride, p->out_dim_stride},
                       {p->z ? p->out_y : nullptr, p->out_y_batch_stride, p->out_y_dim_stride}};
  const bool aligned = all_vec_ok(rows, ib);
  // 16-bit rows, N = 16: state-split lane pairs (scan_fwd_pair.hip; C4 2.78 vs 3.22 ms, C2 training
  // forward 0.166 vs 0.183 ms per layer).  It reads B / C rows itself: no relayout pre-pass.
  const bool pair = pair_shape_ok(p, kPN) && aligned && all_span32(rows, kPCh, p->seqlen, ib);
  pl.family = empty ? MC_SCAN_KERNEL_NONE
                    : dirs ? MC_SCAN_KERNEL_DIRS : pair ? MC_SCAN_KERNEL_PAIR : MC_SCAN_KERNEL_GENERIC;
  pl.state_interval = pair && p->state_interval == kFineS ? kFineS : kS;   // the others save every kS
  if (!pair) {
    pl.mc = p->seqlen <= 512 && !dirs;
    const bool whole = !pl.mc && p->seqlen % kT == 0 && all_span32(rows, kRows, p->seqlen, ib);
    pl.aligned = !(aligned && dirs_vec_ok(dirs, p->seqlen, ib)) ? 0 : whole ? 2 : 1;
  }
  fill_fwd_args(p, pl, pair ? kPCh : kRows, pl.a);
}

// The checks of a call, in the ABI's order, around the choice.
static int plan_fwd(const mc_scan_fwd_params* p, FwdPlan& pl) {
  MC_CHECK(p != nullptr, MC_ERR_INVALID, "mc_scan_fwd: null params");
  choose_fwd(p, pl);
  MC_TRY(validate_common(p->batch, p->dim, p->seqlen, p->dstate, p->n_groups, p->itype, p->wtype, "mc_scan_fwd"));
  if (pl.family == MC_SCAN_KERNEL_NONE) return MC_OK;   // nothing to scan
  MC_CHECK(p->u && p->delta && p->A && p->B && p->C && p->out, MC_ERR_INVALID,
           "mc_scan_fwd: u, delta, A, B, C and out must be non-null");
  const size_t need = bct_bytes(p->batch, p->seqlen, p->dstate, p->n_groups);
  MC_CHECK(p->workspace && p->workspace_bytes >= need && aligned16(p->workspace), MC_ERR_WORKSPACE,
           "mc_scan_fwd: workspace must be >= %zu bytes and 16-B aligned (got %zu)", need, p->workspace_bytes);
  MC_TRY(check_dirs(p, "mc_scan_fwd"));
  MC_CHECK(p->state_interval == 0 || p->state_interval == kS ||
               (p->state_interval == kFineS && pl.family == MC_SCAN_KERNEL_PAIR),
           MC_ERR_SHAPE,
           "mc_scan_fwd: state_interval %d: 0 / %d, or %d on the pair kernel's shapes (mc_scan_fwd_state_interval)",
           p->state_interval, kS, kFineS);
  return MC_OK;
}

static int launch_fwd_generic(const FwdPlan& pl, int itype, hipStream_t s) {
  const FwdArgs& a = pl.a;
  const dim3 grid(a.total_blocks), block(kRows);
  const int np = padded_dstate(a.dstate);
  if (pl.mc)
    MC_DISPATCH_T(itype, MC_DISPATCH_NP(np, MC_DISPATCH_BOOL(pl.aligned != 0, kAl, MC_DISPATCH_BOOL(
        a.softplus != 0, kSP, hipLaunchKernelGGL((scan_fwd_mc_kernel<T, kN, kAl, kSP>), grid, block,
                                                 (size_t)kRows * RowLayoutP<T>::kStride, s, a)))));
  else
    MC_DISPATCH_T(itype, MC_DISPATCH_NP(np, MC_DISPATCH_ALIGNED3(pl.aligned, MC_DISPATCH_BOOL(
        a.softplus != 0, kSP, hipLaunchKernelGGL((scan_fwd_kernel<T, kN, kAl, kSP>), grid, block,
                                                 (size_t)kRows * RowLayout<T>::kStride + (size_t)kT * 2 * kN * 4, s,
                                                 a)))));
  return check_launch("mc_scan_fwd");
}

int validate_common(int batch, int dim, int seqlen, int dstate, int n_groups, int itype, int wtype, const char* who) {
  MC_CHECK(batch >= 0 && dim > 0 && seqlen >= 0, MC_ERR_SHAPE, "%s: bad shape batch=%d dim=%d seqlen=%d", who,
           batch, dim, seqlen);
  MC_CHECK(dstate >= 1 && dstate <= MC_SCAN_MAX_DSTATE, MC_ERR_SHAPE, "%s: dstate=%d must be in [1, %d]", who,
           dstate, MC_SCAN_MAX_DSTATE);
  MC_CHECK(n_groups >= 1 && dim % n_groups == 0, MC_ERR_SHAPE, "%s: dim=%d not divisible by n_groups=%d", who,
           dim, n_groups);
  MC_CHECK(itype >= MC_DTYPE_F32 && itype <= MC_DTYPE_F16, MC_ERR_DTYPE, "%s: bad input dtype %d", who, itype);
  MC_CHECK(wtype >= MC_DTYPE_F32 && wtype <= MC_DTYPE_F16, MC_ERR_DTYPE, "%s: bad weight dtype %d", who, wtype);
  return MC_OK;
}

}  // namespace scan
}  // namespace mc

// ------------------------------------------------------------------ C ABI
using namespace mc;
using namespace mc::scan;

extern "C" int32_t mc_scan_n_chunks(int32_t seqlen) { return seqlen <= 0 ? 0 : (seqlen + kS - 1) / kS; }

extern "C" int32_t mc_scan_n_states(int32_t seqlen, int32_t state_interval) {
  const int S = state_interval > 0 ? state_interval : kS;
  return seqlen <= 0 ? 0 : (seqlen + S - 1) / S;
}

extern "C" size_t mc_scan_chunk_states_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate) {
  return (size_t)batch * dim * mc_scan_n_chunks(seqlen) * dstate * sizeof(float);
}

extern "C" size_t mc_scan_fwd_workspace_bytes(int32_t batch, int32_t seqlen, int32_t dstate, int32_t n_groups) {
  return bct_bytes(batch, seqlen, dstate, n_groups);
}

extern "C" int mc_scan_fwd(const mc_scan_fwd_params* p, void* stream) {
  FwdPlan pl;
  MC_TRY(plan_fwd(p, pl));
  hipStream_t s = (hipStream_t)stream;
  if (pl.family == MC_SCAN_KERNEL_NONE) {
    // a zero-length sequence leaves the state at zero
    if (p->last_state && p->batch > 0)
      (void)hipMemsetAsync(p->last_state, 0, (size_t)p->batch * p->dim * p->dstate * 4, s);
    return MC_OK;
  }
  if (pl.family == MC_SCAN_KERNEL_PAIR) return launch_fwd_pair(pl.a, p->itype, s);
  const hipError_t e = relayout_bc(p, pl.a.rev_groups, reinterpret_cast<float*>(p->workspace), s);
  MC_CHECK(e == hipSuccess, MC_ERR_LAUNCH, "mc_scan_fwd: B/C relayout launch failed: %s", hipGetErrorString(e));
  return launch_fwd_generic(pl, p->itype, s);
}

extern "C" int32_t mc_scan_fwd_kernel(const mc_scan_fwd_params* p) {
  FwdPlan pl;
  if (p) choose_fwd(p, pl);
  return pl.family;
}

extern "C" int32_t mc_scan_fwd_state_interval(const mc_scan_fwd_params* p) {
  FwdPlan pl;
  if (p) choose_fwd(p, pl);
  return pl.state_interval;
}
