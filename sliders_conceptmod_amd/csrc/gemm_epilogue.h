// The GEMM epilogue, written once (device code only; included by gemm.hip, gemm2.hip, gemm3.hip, gemm4.hip).
//
//   C[m][n] = round( acc + bias[n] + rowvec[m / rows_per_vec][n] + lora_scale * sum_q xa[m][q] * up[n][q] + res[m][n] )
//
// in that order, all in fp32, one rounding at the store (kernels.h, GemmParams).  Every kernel generation and the
// split-K finish build their epilogue from the functions below, which is why the tile autotuner may serve a launch with
// any of them: the arithmetic is the same by construction.  What stays with each kernel is the placement of its loads
// (which rows it requests ahead, what it keeps across rows) and its store path.
//
// W is the number of consecutive output columns of one row a lane holds: 8 (one MFMA fragment pair) or 4.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace smi {

template <typename T, int W> using EpiPack = std::conditional_t<W == 8, Pack8<T>, Pack4<T>>;

template <typename T, int W>
__device__ __forceinline__ EpiPack<T, W> epi_load(const T* src) {  // one 16-byte (W = 8) or 8-byte load
  EpiPack<T, W> b;
  b.u = *reinterpret_cast<const decltype(b.u)*>(src);
  return b;
}
// v[0..W) += values already loaded (a kernel that fetches rows ahead, or keeps the bias across rows)
template <typename T, int W, int VW>
__device__ __forceinline__ void epi_add(float (&v)[VW], const EpiPack<T, W>& b) {
  static_assert(W <= VW, "more columns than the lane holds");
#pragma unroll
  for (int j = 0; j < W; ++j) v[j] += to_f(b.e[j]);
}
// ... kept as fp32 across rows: b[0..W) = src[0..W)
template <typename T, int W>
__device__ __forceinline__ void epi_unpack(float (&b)[W], const T* src) {
  const EpiPack<T, W> t = epi_load<T, W>(src);
#pragma unroll
  for (int j = 0; j < W; ++j) b[j] = to_f(t.e[j]);
}
template <int W>
__device__ __forceinline__ void epi_add(float (&v)[W], const float (&b)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) v[j] += b[j];
}
// v[0..W) += src[0..W): bias, row vector and residual
template <typename T, int W, int VW>
__device__ __forceinline__ void epi_add(float (&v)[VW], const T* src) {
  epi_add<T, W>(v, epi_load<T, W>(src));
}
// 8 columns, or the first 4 of them (the half-valid group at N % 8 == 4, a lone fragment)
template <typename T>
__device__ __forceinline__ void epi_add(float (&v)[8], const T* src, bool full) {
  if (full) epi_add<T, 8>(v, src);
  else epi_add<T, 4>(v, src);
}

// element offset of row m's row vector
__device__ __forceinline__ int64_t epi_rowvec_offset(const GemmParams& p, int m) {
  return (int64_t)(m / p.rows_per_vec) * (p.ld_rowvec ? p.ld_rowvec : (int64_t)p.N);
}

// ---------------------------------------------------------------------------------------------------------------
// The rank-r delta on the VALU: per column the canonical chain of smi_common.h (ascending fmaf from zero, then one fmaf
// with lora_scale onto the running value).  Row m >= lora_row0, columns n .. n + ncols - 1 (ncols = W, or 4 of W = 8).
// Operand forms: forward up [N, r] (16-byte loads of xa and of each column's row of up), dX "up" = lora_down [r, K] read
// along K (16-byte loads across columns), and general strides / ranks (scalar loads).  VEC = false: scalar loads only
// (the register-staged kernel takes operands of any alignment); FWD_VEC = false: a kernel whose forward deltas go to the
// MFMA form below keeps no second vector path for them (registers).
// ---------------------------------------------------------------------------------------------------------------
template <int W, bool VEC = true, bool FWD_VEC = VEC>
__device__ __forceinline__ void epi_lora(float (&v)[W], const GemmParams& p, int m, int n, int ncols = W) {
  const float* xrow0 = p.lora_xa + (int64_t)(m - p.lora_row0) * p.ld_xa;
  if (FWD_VEC && p.up_sq == 1 && p.up_sn == p.lora_r && (p.lora_r & 3) == 0) {
    const float* xrow = xrow0 + (p.lora_seg ? (n / p.lora_seg) * p.lora_r : 0);
    float d[W];
#pragma unroll
    for (int j = 0; j < W; ++j) d[j] = 0.f;
    for (int r0 = 0; r0 < p.lora_r; r0 += 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xrow + r0);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        if (j < 4 || ncols == W) {
          const f32x4 uv = *reinterpret_cast<const f32x4*>(p.lora_up + (int64_t)(n + j) * p.lora_r + r0);
          d[j] = lora_fma4(d[j], xv, uv);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = __builtin_fmaf(d[j], p.lora_scale, v[j]);
  } else if (VEC && p.up_sn == 1 && (p.up_sq & 3) == 0) {
    const float* xrow = xrow0 + (p.lora_seg ? (n / p.lora_seg) * p.lora_r : 0);
    float d[W];
#pragma unroll
    for (int j = 0; j < W; ++j) d[j] = 0.f;
    for (int r = 0; r < p.lora_r; ++r) {
      const float xq = xrow[r];
      const float* ar = p.lora_up + (int64_t)r * p.up_sq + n;
      f32x4 a[W / 4];
#pragma unroll
      for (int h = 0; h < W / 4; ++h)
        a[h] = (h == 0 || ncols == W) ? *reinterpret_cast<const f32x4*>(ar + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < W / 4; ++h) d[4 * h + j] = __builtin_fmaf(xq, a[h][j], d[4 * h + j]);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = __builtin_fmaf(d[j], p.lora_scale, v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (j < 4 || ncols == W) {
        const float* xr = xrow0 + (p.lora_seg ? ((n + j) / p.lora_seg) * p.lora_r : 0);
        const float* up = p.lora_up + (int64_t)(n + j) * p.up_sn;
        float d = 0.f;
        for (int r = 0; r < p.lora_r; ++r) d = __builtin_fmaf(xr[r], up[r * p.up_sq], d);
        v[j] = __builtin_fmaf(d, p.lora_scale, v[j]);
      }
    }
  }
}

// The same chain for four columns with the rank R as a compile-time constant and every operand requested before the first
// fmaf (the split-K finish: the rolled loop with its run-time strides made 2 r dependent round trips per column, +18 us on
// a 2048 x 1280 launch).  (lora_seg is a multiple of 4: the four columns share one xa row.)
template <int R>
__device__ __forceinline__ void epi_lora4_unrolled(float (&v)[4], const GemmParams& p, int m, int n) {
  const float* xr = p.lora_xa + (int64_t)(m - p.lora_row0) * p.ld_xa + (p.lora_seg ? (n / p.lora_seg) * p.lora_r : 0);
  const float* up0 = p.lora_up + (int64_t)n * p.up_sn;
  float x[R], u[4][R];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = xr[r];
  const bool al = (reinterpret_cast<uintptr_t>(p.lora_up) & 15) == 0;
  if (al && p.up_sq == 1 && p.up_sn == R) {  // [N, r] rows: 16-byte pieces (a lane's dword loads at a 4 r-byte
    // stride touch 64 lines per wave-instruction: 16 of them per thread made the delta cost 17 of the finish's 24 us)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < R / 4; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(up0 + j * R + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) u[j][q * 4 + e] = t[e];
      }
  } else if (al && p.up_sn == 1 && (p.up_sq & 3) == 0) {  // [r, K] read transposed: four columns of one rank row
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(up0 + (int64_t)r * p.up_sq);
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j][r] = t[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) u[j][r] = up0[(int64_t)j * p.up_sn + (int64_t)r * p.up_sq];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) d = __builtin_fmaf(x[r], u[j][r], d);
    v[j] = __builtin_fmaf(d, p.lora_scale, v[j]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The rank-r delta on the fp32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, i.e. the canonical chain in the
// accumulators' own register layout):  D[16 columns x 16 rows] = up-fragment [16 x 4] * xa-fragment [4 x 16] + D per
// block of four ranks.  One dword load per operand and lane.  Lane l = (fr = l & 15, fq = l >> 4).
// ---------------------------------------------------------------------------------------------------------------
enum : int { EPI_MFMA_NONE = 0, EPI_MFMA_FWD = 1, EPI_MFMA_DX = 2 };
// which operand form the MFMA delta can take for tiles BN columns wide (a tile must lie inside one fused segment)
__device__ __forceinline__ int epi_lora_mfma_form(const GemmParams& p, int bn) {
  if (p.lora_r <= 0 || (p.lora_r & 3) != 0 || p.lora_r > 16 || (p.lora_seg != 0 && p.lora_seg % bn != 0)) return EPI_MFMA_NONE;
  if (p.up_sq == 1 && p.up_sn == p.lora_r) return EPI_MFMA_FWD;
  return p.up_sn == 1 ? EPI_MFMA_DX : EPI_MFMA_NONE;
}
// column, within a fragment pair's 32, that fragment row fr of the pair's MFMA nip holds (the W-row permutation that
// gives a lane 8 consecutive output columns after the two MFMAs of a pair)
__device__ __forceinline__ int epi_pair_col(int fr, int nip) { return 8 * (fr >> 2) + 4 * nip + (fr & 3); }
// A operand of rank block b: lane (fr, fq) holds up[col][4 b + fq], col = the output column of fragment row fr
__device__ __forceinline__ float epi_mfma_up(const GemmParams& p, bool fwd, int col, int b, int fq) {
  return fwd ? p.lora_up[(int64_t)col * p.lora_r + 4 * b + fq] : p.lora_up[(int64_t)(4 * b + fq) * p.up_sq + col];
}
// B operand: lane (fr, fq) holds xa[row m of fragment column fr][4 b + fq] = epi_mfma_xa(...)[4 b]; `on`: m carries a delta
__device__ __forceinline__ const float* epi_mfma_xa(const GemmParams& p, int m, bool on, int xoff, int fq) {
  return p.lora_xa + (int64_t)(on ? m - p.lora_row0 : 0) * p.ld_xa + xoff + fq;
}
// one rank block: d += up-fragment * xa-fragment (blocks in ascending order from d = 0 make the canonical chain)
__device__ __forceinline__ f32x4 epi_mfma_block(float au, float bx, f32x4 d) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(au, bx, d, 0, 0, 0);
}
// v[0..4) += lora_scale * d
__device__ __forceinline__ void epi_add_delta(float* v, f32x4 d, float scale) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(d[j], scale, v[j]);
}

// ---------------------------------------------------------------------------------------------------------------
// stores: the one rounding
// ---------------------------------------------------------------------------------------------------------------
template <int W, int VW>
__device__ __forceinline__ void epi_store_f32(float* dst, const float (&v)[VW]) {
#pragma unroll
  for (int h = 0; h < W / 4; ++h)
    *reinterpret_cast<f32x4*>(dst + 4 * h) = f32x4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
}
// W values rounded to T, one 16- or 8-byte store (global memory or the staged LDS tile)
template <typename T, int W, int VW>
__device__ __forceinline__ void epi_store(T* dst, const float (&v)[VW]) {
  EpiPack<T, W> o;
#pragma unroll
  for (int j = 0; j < W; ++j) o.e[j] = from_f<T>(v[j]);
  *reinterpret_cast<decltype(o.u)*>(dst) = o.u;
}

// fused GEGLU: both halves of the projection are rounded to 16 bits first, the gate is applied to the rounded values
// (bit-identical to projection + separate GEGLU kernel)
template <typename T>
__device__ __forceinline__ T geglu_gate(T hidden, T gate) {
  return from_f<T>(to_f(hidden) * gelu_f(to_f(gate)));
}
// GEGLU tile: local column nl of a BN-wide tile -> global column (first half hidden, second half their gates)
template <int BN>
__device__ __forceinline__ int geglu_col(int bn0, int nhalf, int nl) {
  return nl < BN / 2 ? (bn0 >> 1) + nl : nhalf + (bn0 >> 1) + nl - BN / 2;
}

// ---------------------------------------------------------------------------------------------------------------
// Write-out of a 16-bit output tile staged in LDS (rows of BN + 8 elements), by NT threads: whole rows, one wave store
// instruction covers 4 rows x 256 contiguous bytes instead of 16 rows x 64 bytes.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int BM, int BN, int NT>
__device__ __forceinline__ void stage_writeout(const GemmParams& p, const T* otile, int tid, int bm0, int bn0) {
  constexpr int OLD = BN + 8;
  constexpr int CH = BN / 8;  // 16-byte chunks per tile row
#pragma unroll
  for (int i = 0; i < (BM * CH) / NT; ++i) {
    const int idx = tid + i * NT;
    const int r = idx / CH, c = idx - r * CH;
    const int n = bn0 + c * 8;
    const int m = bm0 + r;
    if (m < p.M && n < p.N)
      *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n) =
          *reinterpret_cast<const u32x4*>(otile + r * OLD + c * 8);
  }
}
// fused GEGLU: hidden * gelu(gate) to geglu_out; the projection itself only for the rows that will be differentiated
template <typename T, int BM, int BN, int NT>
__device__ __forceinline__ void geglu_writeout(const GemmParams& p, const T* otile, int tid, int bm0, int bn0) {
  constexpr int OLD = BN + 8;
  const int nhalf = p.N >> 1;
  {  // BN/16 chunks of 8 output columns per row
    constexpr int CH = BN / 16;
    T* gout = reinterpret_cast<T*>(p.geglu_out);
#pragma unroll
    for (int i = 0; i < (BM * CH) / NT; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / CH, c = idx - r * CH;
      const int m = bm0 + r;
      if (m < p.M) {
        Pack8<T> h, g, o;
        h.u = *reinterpret_cast<const u32x4*>(otile + r * OLD + c * 8);
        g.u = *reinterpret_cast<const u32x4*>(otile + r * OLD + BN / 2 + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = geglu_gate<T>(h.e[e], g.e[e]);
        *reinterpret_cast<u32x4*>(gout + (int64_t)m * nhalf + (bn0 >> 1) + c * 8) = o.u;
      }
    }
  }
  if (bm0 + BM > p.geglu_row0) {
    constexpr int CH = BN / 8;
#pragma unroll
    for (int i = 0; i < (BM * CH) / NT; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / CH, c = idx - r * CH;
      const int n = geglu_col<BN>(bn0, nhalf, c * 8);
      const int m = bm0 + r;
      if (m < p.M && m >= p.geglu_row0)
        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(p.C) + (int64_t)m * p.ldc + n) =
            *reinterpret_cast<const u32x4*>(otile + r * OLD + c * 8);
    }
  }
}

}  // namespace smi
