// Causal self-attention backward for short sequences (the CLIP text towers: L = 77, head_dim 64), gfx950.
//
// One workgroup of four waves owns one (sample, head): with L <= 128 the whole problem sits in LDS, so there is one
// launch, no atomics and one fixed summation order -- two runs give the same bits, and a sample's result does not
// depend on which other samples share the batch.  The grid is tiny (24 - 40 workgroups at the real shapes): the kernel
// is latency-bound, and nothing here is tuned for occupancy.
//
// Arithmetic (key j is visible to query i iff j <= i):
//   P[i][j]  = exp(scale * <Q_i, K_j> - lse[i]) for visible cells, else 0        (lse from the causal forward)
//   delta[i] = sum_d dO[i][d] * O[i][d]                                          (fp32, from the 16-bit operands)
//   dS[i][j] = P[i][j] * (<dO_i, V_j> - delta[i])                                (P still in fp32)
//   dV = P^T dO,  dQ = scale * dS K,  dK = scale * dS^T Q                         (P, dS rounded to 16 bit first)
// All products are v_mfma_f32_32x32x16 with fp32 accumulation.  Rounding sites: P and dS once (to the storage type, as
// MFMA operands) and the three outputs once.
//
// MFMA 32x32x16 wants both operands with the contraction index contiguous per lane (smi_common.h), so every product
// reads two row-major LDS tiles whose ROW is the output index and whose COLUMN is the contraction index:
//   S  [i][j] : Q  [i][d], K  [j][d]          dP [i][j] : dO [i][d], V [j][d]           (natural tiles)
//   dV^T[d][j]: dOt[d][i], Pt [j][i]          dK^T[d][j]: Qt [d][i], dSt[j][i]          dQ^T[d][i]: Kt[d][j], dS[i][j]
// The outputs are formed transposed so that a lane owns one output row and four consecutive d per accumulator quad:
// 8-byte global stores.  The transposed operand copies Qt / Kt / dOt are written while the operands are staged; Pt, dS
// and dSt are written from the score tiles' accumulators and take over the LDS of the natural tiles, which are dead by
// then (the score tiles wait in registers across the barrier in between).
//
// Left for whoever profiles it: O and dO are read from global memory a second time for delta although dO is already staged
// (O is not), and the score tiles above the diagonal, which the mask zeroes entirely, still run both MFMA chains.
//
// LDS at LP = 128 (L rounded up to 32): 1 KB (lse, delta) + max(4 * LP * 72, 3 * LP * (LP + 8)) * 2 + 3 * 64 * (LP + 8) * 2
// = 157696 bytes of the 160 KB; at L = 77 (LP = 96) 98 KB.  Rows and columns L .. LP - 1 are zero-filled: they take part
// in every k-loop.
#include "kernels.h"

namespace smi {
namespace {

constexpr int CA_D = 64;         // head_dim
constexpr int CA_LMAX = 128;     // longest sequence
constexpr int CA_LDN = CA_D + 8; // row length of the natural [L][64] tiles

__host__ __device__ constexpr size_t ca_region_a_elems(int LP) {
  return (size_t)(4 * LP * CA_LDN > 3 * LP * (LP + 8) ? 4 * LP * CA_LDN : 3 * LP * (LP + 8));
}
__host__ __device__ constexpr size_t ca_smem_bytes(int LP) {
  return 2 * CA_LMAX * sizeof(float) + 2 * (ca_region_a_elems(LP) + (size_t)3 * CA_D * (LP + 8));
}
static_assert(ca_smem_bytes(CA_LMAX) <= 160 * 1024, "causal attention backward: LDS");

template <typename T>
__device__ __forceinline__ typename TT<T>::v8 frag(const T* tile, int ld, int row, int col) {
  Pack8<T> t;
  t.u = *reinterpret_cast<const u32x4*>(tile + row * ld + col);
  return t.v;
}

template <typename T>
__global__ __launch_bounds__(256) void attn_causal_bwd_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ca_smem[];
  const int L = p.Nq;
  const int LP = (L + 31) / 32 * 32, NT = LP / 32, LDP = LP + 8;
  float* lse_s = reinterpret_cast<float*>(ca_smem);
  float* delta_s = lse_s + CA_LMAX;
  T* A = reinterpret_cast<T*>(delta_s + CA_LMAX);
  T* Qn = A;
  T* Kn = Qn + LP * CA_LDN;
  T* Vn = Kn + LP * CA_LDN;
  T* Gn = Vn + LP * CA_LDN;
  T* Pt = A;                // [j][i]   (region A again, after the score phase)
  T* dSn = Pt + LP * LDP;   // [i][j]
  T* dSt = dSn + LP * LDP;  // [j][i]
  T* Qt = A + ca_region_a_elems(LP);  // [d][i]
  T* Kt = Qt + CA_D * LDP;            // [d][j]
  T* Gt = Kt + CA_D * LDP;            // [d][i]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, h2 = lane >> 5;
  const int head = blockIdx.x, b = blockIdx.y;
  const int col0 = head * CA_D;
  const int64_t row0 = (int64_t)b * L;

  // ---- stage Q, K, V, dO: natural rows (16-byte stores) and, for Q / K / dO, the transposed copy; rows >= L are zeros
  {
    const T* src[4] = {(const T*)p.Q, (const T*)p.K, (const T*)p.V, (const T*)p.dO};
    const int64_t ld[4] = {p.ldq, p.ldk, p.ldv, p.lddo};
    T* nat[4] = {Qn, Kn, Vn, Gn};
    T* tr[4] = {Qt, Kt, nullptr, Gt};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      for (int idx = tid; idx < LP * 8; idx += 256) {
        const int row = idx >> 3, ch = idx & 7;
        Pack8<T> v;
        v.u = u32x4{0u, 0u, 0u, 0u};
        if (row < L) v.u = *reinterpret_cast<const u32x4*>(src[o] + (row0 + row) * ld[o] + col0 + ch * 8);
        *reinterpret_cast<u32x4*>(nat[o] + row * CA_LDN + ch * 8) = v.u;
        if (tr[o]) {
#pragma unroll
          for (int e = 0; e < 8; ++e) tr[o][(ch * 8 + e) * LDP + row] = v.e[e];
        }
      }
    }
  }
  // ---- lse and delta[i] = sum_d dO[i][d] O[i][d]: two threads per row, 32 columns each, one exchange
  {
    const int row = tid >> 1, half = tid & 1;
    float acc = 0.f;
    if (row < L) {
      const T* o = (const T*)p.O + (row0 + row) * p.ldo + col0 + half * 32;
      const T* g = (const T*)p.dO + (row0 + row) * p.lddo + col0 + half * 32;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        Pack8<T> a, d;
        a.u = *reinterpret_cast<const u32x4*>(o + c * 8);
        d.u = *reinterpret_cast<const u32x4*>(g + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(to_f(a.e[e]), to_f(d.e[e]), acc);
      }
    }
    const float other = __shfl_xor(acc, 1);
    const float sum = half == 0 ? acc + other : other + acc;  // columns 0..31 first, on both lanes
    if (half == 0) {
      delta_s[row] = row < L ? sum : 0.f;
      lse_s[row] = row < L ? p.lse[((int64_t)b * p.H + head) * L + row] : 0.f;
    }
  }
  __syncthreads();

  // ---- score phase: wave w owns the 32 x 32 tiles w, w + 4, ... of the NT x NT grid; P and dS wait in registers
  Pack4<T> p16[4][4], s16[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tile = wave + 4 * t;
    if (tile < NT * NT) {
      const int it = tile / NT, jt = tile - it * NT;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
      for (int k = 0; k < CA_D / 16; ++k) {
        const int c = 16 * k + 8 * h2;
        s = TT<T>::mfma32(frag<T>(Qn, CA_LDN, it * 32 + ql, c), frag<T>(Kn, CA_LDN, jt * 32 + ql, c), s);
        dp = TT<T>::mfma32(frag<T>(Gn, CA_LDN, it * 32 + ql, c), frag<T>(Vn, CA_LDN, jt * 32 + ql, c), dp);
      }
      // register r: query i = it * 32 + (r & 3) + 8 (r >> 2) + 4 h2, key j = jt * 32 + ql
      const int j = jt * 32 + ql;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = it * 32 + (r & 3) + 8 * (r >> 2) + 4 * h2;
        const bool vis = j <= i && i < L;  // (j <= i < L: j < L too)
        const float pv = vis ? __expf(s[r] * p.scale - lse_s[i]) : 0.f;
        const float ds = vis ? pv * (dp[r] - delta_s[i]) : 0.f;
        p16[t][r >> 2].e[r & 3] = from_f<T>(pv);
        s16[t][r >> 2].e[r & 3] = from_f<T>(ds);
      }
    }
  }
  __syncthreads();  // every wave is done with the natural tiles: Pt / dS / dSt take their place
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tile = wave + 4 * t;
    if (tile < NT * NT) {
      const int it = tile / NT, jt = tile - it * NT;
      const int j = jt * 32 + ql;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i0 = it * 32 + 8 * g + 4 * h2;  // four consecutive queries
        *reinterpret_cast<u32x2*>(Pt + j * LDP + i0) = p16[t][g].u;
        *reinterpret_cast<u32x2*>(dSt + j * LDP + i0) = s16[t][g].u;
#pragma unroll
        for (int e = 0; e < 4; ++e) dSn[(i0 + e) * LDP + j] = s16[t][g].e[e];
      }
    }
  }
  __syncthreads();

  // ---- output phase: 3 outputs x NT row tiles x 2 column tiles of 32 d, dealt round-robin to the waves
  for (int job = wave; job < 3 * NT * 2; job += 4) {
    const int which = job / (NT * 2);  // 0: dV, 1: dK, 2: dQ
    const int rem = job - which * NT * 2;
    const int nt = rem >> 1, dt = rem & 1;
    const T* At = which == 0 ? Gt : (which == 1 ? Qt : Kt);   // [d][contraction]
    const T* Bt = which == 0 ? Pt : (which == 1 ? dSt : dSn);  // [output row][contraction]
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = 0; k < LP / 16; ++k) {
      const int c = 16 * k + 8 * h2;
      acc = TT<T>::mfma32(frag<T>(At, LDP, dt * 32 + ql, c), frag<T>(Bt, LDP, nt * 32 + ql, c), acc);
    }
    // register r: d = dt * 32 + (r & 3) + 8 (r >> 2) + 4 h2, output row n = nt * 32 + ql
    const int n = nt * 32 + ql;
    if (n < L) {
      T* out = which == 0 ? (T*)p.dV : (which == 1 ? (T*)p.dK : (T*)p.dQ);
      const int64_t ldo = which == 0 ? p.lddv : (which == 1 ? p.lddk : p.lddq);
      const float mul = which == 0 ? 1.f : p.scale;
      T* dst = out + (row0 + n) * ldo + col0 + dt * 32 + 4 * h2;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Pack4<T> v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v.e[e] = from_f<T>(acc[4 * g + e] * mul);
        *reinterpret_cast<u32x2*>(dst + 8 * g) = v.u;
      }
    }
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

int launch_attn_causal_bwd(const AttnParams& p, hipStream_t stream) {
  SMI_CHECK(p.dtype == DT_F16 || p.dtype == DT_BF16, "causal attention bwd: dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(p.causal, "causal attention bwd: called without the causal flag");
  SMI_CHECK(p.D == CA_D, "causal attention bwd: head_dim %d, the kernel takes head_dim %d only", p.D, CA_D);
  SMI_CHECK(p.Nq == p.Nk && p.Nq >= 1 && p.Nq <= CA_LMAX,
            "causal attention bwd: Nq %d, Nk %d -- the kernel takes self-attention with 1 <= Nq == Nk <= %d", p.Nq, p.Nk,
            CA_LMAX);
  SMI_CHECK(p.B >= 1 && p.B <= 65535 && p.H >= 1, "causal attention bwd: batch %d outside [1, 65535] or heads %d < 1", p.B, p.H);
  SMI_CHECK(p.Q && p.K && p.V && p.O && p.lse && p.dO && p.dQ && p.dK && p.dV,
            "causal attention bwd: Q, K, V, O, lse, dO, dQ, dK and dV are all required");
  const int64_t need = (int64_t)p.H * CA_D;
  SMI_CHECK(p.ldq >= need && p.ldk >= need && p.ldv >= need && p.ldo >= need && p.lddo >= need && p.lddq >= need &&
                p.lddk >= need && p.lddv >= need,
            "causal attention bwd: a leading dimension is below heads * head_dim = %lld", (long long)need);
  SMI_CHECK((p.ldq | p.ldk | p.ldv | p.ldo | p.lddo | p.lddq | p.lddk | p.lddv) % 8 == 0 && aligned16(p.Q) && aligned16(p.K) &&
                aligned16(p.V) && aligned16(p.O) && aligned16(p.dO) && aligned16(p.dQ) && aligned16(p.dK) && aligned16(p.dV),
            "causal attention bwd: operands must be 16-byte aligned with leading dimensions that are multiples of 8");
  const int LP = (p.Nq + 31) / 32 * 32;
  const size_t sm = ca_smem_bytes(LP);
  const dim3 grid(p.H, p.B);
  if (p.dtype == DT_F16) {
    static DynLdsOnce once;
    if (int rc = once.set((const void*)attn_causal_bwd_kernel<f16>, (int)ca_smem_bytes(CA_LMAX))) return rc;
    hipLaunchKernelGGL(attn_causal_bwd_kernel<f16>, grid, dim3(256), sm, stream, p);
  } else {
    static DynLdsOnce once;
    if (int rc = once.set((const void*)attn_causal_bwd_kernel<bf16>, (int)ca_smem_bytes(CA_LMAX))) return rc;
    hipLaunchKernelGGL(attn_causal_bwd_kernel<bf16>, grid, dim3(256), sm, stream, p);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
