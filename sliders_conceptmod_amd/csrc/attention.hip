// Fused (flash-style) attention forward + backward for gfx950, non-causal, no mask, head_dim D in {8..160}.  (The tiled
// forward also knows the causal mask and, as a compile-time variant, T5's additive relative-position bias: attn_fwd_kernel.)
//
// MFMA shape: v_mfma_f32_32x32x16_{f16,bf16}.  Scores are produced TRANSPOSED, S^T[key, q] = K . Q^T, so that a
// lane owns ONE query column (q = lane & 31) and 16 keys per 32x32 tile in its registers: the online-softmax
// max / sum are register reductions plus a single cross-half exchange, and the f32 accumulator tile, converted
// pairwise to 16-bit, is already the B operand of the next product (O^T = V^T . P^T) -- no LDS round trip for P
// (cdna_hip_programming.md section 3, "An accumulator tile as the next MFMA's operand").  The A operand of that
// product needs V with the key index contiguous: V (and K / Q / dO in the backward) is staged row-major with 16-byte
// stores and read TRANSPOSED by the gfx950 `ds_read_b64_tr_b16` instruction (4 keys x 16 columns per 16-lane group,
// delivered column-major) -- no scatter writes.  Row strides are chosen so that both the row reads (ds_read_b128,
// stride D+8 elements) and the transposed reads (stride = 64 or 192 bytes mod 256) are bank-conflict free.
//
// Backward (activations only: dQ, and dK/dV when a LoRA hangs off to_k/to_v) recomputes P from Q, K and the
// forward's log-sum-exp; it is split into a dQ kernel (one workgroup per 128 queries, sweeping keys) and a dK/dV
// kernel (one workgroup per 128 keys, sweeping queries): no atomics, bitwise reproducible.  Both bodies have a BIAS form, the
// backward of the forward's (the table is frozen).
#include <stdlib.h>

#include <type_traits>

#include "kernels.h"

namespace smi {
namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int TK = 64;   // keys (or queries) per staged tile
typedef short s16x4 __attribute__((ext_vector_type(4)));
// row length (elements) of tiles read with ds_read_b64_tr_b16: a 32-lane half reads 4 rows x 64 contiguous bytes, so
// the byte stride must be 64 or 192 (mod 256) for the four row segments to fall on disjoint banks
__host__ __device__ constexpr int tr_stride(int DP) { return ((DP * 2) % 128 == 64) ? DP : DP + 32; }

// XCD-aware workgroup order.  The dispatcher deals consecutive workgroups round-robin over the 8 XCDs, each with
// its own 4 MB L2: with the natural order the 8-32 query blocks that sweep the SAME K / V of one (batch, head) land on
// 8 different L2s and every one of them fetches that K / V (1 MB at 4096 keys) again -- 8x the fabric traffic, and at
// 16 samples the working set (336 MB) no longer fits the Infinity Cache: 606 TF/s against 737 TF/s at 4 samples.
// The bijective remap gives each XCD a contiguous range of (batch, head, block) triples, x fastest.
__device__ __forceinline__ void xcd_block(int& bx, int& by, int& bz) {
  const int nx = gridDim.x, ny = gridDim.y;
  const int total = nx * ny * gridDim.z;
  const int lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
  const int q = total >> 3, r = total & 7, xcd = lin & 7;
  const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
  bx = v % nx;
  const int t = v / nx;
  by = t % ny;
  bz = t / ny;
}

template <typename T, int DP>
struct Stage {
  static constexpr int LDN = DP + 8;   // row length of tiles read by rows (ds_read_b128)
  static constexpr int LDV = tr_stride(DP);  // row length of tiles read transposed (ds_read_b64_tr_b16)
  static constexpr int NIT = DP / 32;  // 16-byte chunks per thread per tile (64 * DP/8 / 256)
  static constexpr int CPR = DP / 8;   // chunks per row

  // loads one [64 x D] tile (rows row0.., head columns) into registers
  static __device__ __forceinline__ void load(u32x4 (&reg)[NIT], __amdgpu_buffer_rsrc_t r, int64_t row0, int nrows,
                                              int64_t ld, int col0, int D, int tid) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / CPR, ch = idx - row * CPR;
      const bool ok = (row0 + row < nrows) && (ch * 8 < D);
      const uint32_t off = ok ? (uint32_t)(((row0 + row) * ld + col0 + ch * 8) * 2) : OOB;
      reg[i] = buf_load16(r, off);
    }
  }
  static __device__ __forceinline__ void store_nat(const u32x4 (&reg)[NIT], T* dst, int tid) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / CPR, ch = idx - row * CPR;
      *reinterpret_cast<u32x4*>(dst + row * LDN + ch * 8) = reg[i];
    }
  }
  static __device__ __forceinline__ void store_ld(const u32x4 (&reg)[NIT], T* dst, int ld, int tid) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / CPR, ch = idx - row * CPR;
      *reinterpret_cast<u32x4*>(dst + row * ld + ch * 8) = reg[i];
    }
  }
};

template <typename T>
__device__ __forceinline__ typename TT<T>::v8 pack8(const f32x16& a, int s) {
  Pack8<T> t;
#pragma unroll
  for (int j = 0; j < 8; ++j) t.e[j] = from_f<T>(a[8 * s + j]);
  return t.v;
}
template <typename T>
__device__ __forceinline__ typename TT<T>::v8 ld_frag_nat(const T* tile, int ldn, int row, int col) {
  Pack8<T> t;
  t.u = *reinterpret_cast<const u32x4*>(tile + row * ldn + col);
  return t.v;
}
// A-operand fragment X^T[d = d0 + (lane & 31)][k] from a ROW-MAJOR tile X[idx][d] through the hardware transposed
// read: per 16-lane group, lane 4q+p supplies the address of row q, columns 4p..4p+3 of a 4 x 16 block and lane i
// receives column i (rows 0..3 in elements 0..3).  Elements j < 4 come from rows idx0 + j, j >= 4 from idx0 + 8 + (j-4)
// (the k order of an accumulator tile used as the other operand); idx0 already contains 4 * (lane >> 5).
template <typename T>
__device__ __forceinline__ typename TT<T>::v8 ld_frag_trhw(const T* tile, int ld, int idx0, int d0, int lane) {
  const T* a = tile + (idx0 + ((lane & 15) >> 2)) * ld + d0 + ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 8 * ld));
  union {
    s16x4 h[2];
    typename TT<T>::v8 v;
  } u;
  u.h[0] = lo;
  u.h[1] = hi;
  return u.v;
}

// Row sum of eight packed 16-bit probabilities on the matrix pipe: v_mfma_f32_4x4x4 (16 blocks of 4 lanes) with an
// all-ones A operand gives D[i][j] = sum_k B[k][j], i.e. every lane receives the sum of its OWN four B elements in all
// four result registers.  Two of them per 8-wide fragment replace eight v_add_f32 of a loop that is VALU-bound, and
// the normaliser becomes the sum of exactly the rounded values the P.V product consumes.
template <typename T> struct Sum4;
template <> struct Sum4<f16> {
  static __device__ __forceinline__ f32x4 add8(f16x8 pf, f32x4 acc) {
    const f16x4 one = {(f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f};
    const f16x4 lo = {pf[0], pf[1], pf[2], pf[3]}, hi = {pf[4], pf[5], pf[6], pf[7]};
    acc = __builtin_amdgcn_mfma_f32_4x4x4f16(one, lo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_4x4x4f16(one, hi, acc, 0, 0, 0);
  }
};
template <> struct Sum4<bf16> {
  typedef short s4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f32x4 add8(bf16x8 pf, f32x4 acc) {
    const s4 one = {0x3F80, 0x3F80, 0x3F80, 0x3F80};
    union { bf16x8 v; s4 h[2]; } u;
    u.v = pf;
    acc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(one, u.h[0], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(one, u.h[1], acc, 0, 0, 0);
  }
};
// Combine a value with the one the lane 32 away holds.  v_permlane32_swap exchanges the upper half of its first operand
// with the lower half of its second; fed two copies of x it leaves {x.lo in both halves} and {x.hi in both halves}:
// one VALU instruction and no LDS round trip (__shfl_xor(x, 32) compiles to ds_bpermute_b32).  Inline asm on purpose:
// with the SAME value in both operands hipcc (ROCm 7.2) treats the builtin's two results as one register
// (`v_add v1, v1, v1`); the asm's two read-write operands cannot be merged.  s_nop 1: VALU write -> permlane read.
__device__ __forceinline__ void halves_split(float x, float& lo, float& hi) {
  lo = x;
  hi = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(lo), "+v"(hi));
}
__device__ __forceinline__ float halves_max(float x) {
  float a, b;
  halves_split(x, a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float halves_sum(float x) {
  float a, b;
  halves_split(x, a, b);
  return a + b;
}
__device__ __forceinline__ int acc_row(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

// =============================================================================================================
// forward
// =============================================================================================================
// NSD > 0 ("EX"): the number of 16-wide k-steps of the head dimension is a compile-time constant -- head_dim == DP (SD-XL:
// 64 -> 4) or one of the SD-1.x widths inside a wider tile (40 -> 3 of the 64-wide tile, 80 -> 5 of the 96-wide one) -- with the run-time
// `s < nsd` test hipcc wraps every (ds_read, MFMA) pair of the QK^T product in its own branch and waits lgkmcnt(0) after
// each read: eight exposed LDS round trips per key tile and wave instead of eight reads in flight.
// BIAS (T5's relative-position bias; self-attention, Nq == Nk = L): s[q, k] = q.k * scale + p.bias[head][k - q + L - 1].  The
// head's 2L - 1 floats are staged in dynamic LDS once per workgroup; the score tile is turned into biased scores in fp32
// right after the MFMAs, so the mask, the tile maximum and the lazy rescale below all see what the softmax is over, and
// the rest of the loop runs with scale 1.  A lane's 32 table reads per tile are at k - q + L - 1 with q = the lane's query:
// consecutive lanes read consecutive (descending) words.  Lanes past Nq and keys past Nk exist in the ragged last blocks:
// their index is clamped into the table (their scores are masked or never stored).
template <typename T, int DP, int NSD, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnParams p) {
  using S = Stage<T, DP>;
  constexpr int NS = DP / 16, NB = DP / 32;
  constexpr bool EX = NSD > 0;  // the number of 16-wide k-steps is the compile-time NSD (0: run-time, from p.D)
  // two LDS stages: tile t + 1 is written while tile t is being read, so ONE barrier per key tile orders both the
  // "everyone is done with stage s" and the "stage s ^ 1 is complete" edges (it was two barriers on one stage)
  __shared__ __attribute__((aligned(16))) T Ks2[2][TK * S::LDN];
  __shared__ __attribute__((aligned(16))) T Vs2[2][TK * S::LDV];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, h2 = lane >> 5;
  int bx, head, b;
  xcd_block(bx, head, b);
  const int q_idx = bx * 128 + wave * 32 + ql;
  const int col0 = head * p.D;
  const int nsd = NSD > 0 ? NSD : (p.D + 15) / 16;

  const auto rQ = make_rsrc((const T*)p.Q + (int64_t)b * p.Nq * p.ldq, (uint32_t)((int64_t)p.Nq * p.ldq * 2));
  const auto rK = make_rsrc((const T*)p.K + (int64_t)b * p.Nk * p.ldk, (uint32_t)((int64_t)p.Nk * p.ldk * 2));
  const auto rV = make_rsrc((const T*)p.V + (int64_t)b * p.Nk * p.ldv, (uint32_t)((int64_t)p.Nk * p.ldv * 2));

  typename TT<T>::v8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int d = 16 * s + 8 * h2;
    const bool ok = (q_idx < p.Nq) && (d < p.D);
    Pack8<T> t;
    t.u = buf_load16(rQ, ok ? (uint32_t)(((int64_t)q_idx * p.ldq + col0 + d) * 2) : OOB);
    qf[s] = t.v;
  }
  const float scale = BIAS ? 1.f : p.scale;  // BIAS: the scores are scaled where the bias is added
  const float sl = scale * LOG2E;
  extern __shared__ __attribute__((aligned(16))) float bias_tab[];  // BIAS only: [2 Nk - 1]
  const int nb1 = 2 * p.Nk - 2;                                    // last index of the table
  if constexpr (BIAS) {
    const float* src = p.bias + (int64_t)head * p.bias_ld;
    for (int i = tid; i <= nb1; i += 256) bias_tab[i] = src[i];
  }

  f32x16 o[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -INFINITY;
  f32x4 l4 = {0.f, 0.f, 0.f, 0.f};  // running row sum (all four registers equal), see Sum4
  // bf16: lse from an fp32 sum of the UNROUNDED probabilities.  l4 adds the 16-bit values (the normaliser of exactly what
  // P.V consumes, so O is unchanged), and against the lazily rescaled reference the probability of a row's dominant key is
  // not 1 but a rounded number in [1, 256]: log(l4) is off by up to 2^-8 = 3.9e-3 when one key carries the row, above the
  // 2e-3 the backward's lse is held to.  fp16 (2^-11) stays on l4 alone: 32 VALU adds per tile in a VALU-bound loop.
  constexpr bool LSE_F32 = std::is_same<T, bf16>::value;
  float lx = 0.f;

  const int ntiles = (p.Nk + TK - 1) / TK;
  // K/V tiles are fetched one tile ahead into registers: the global-load latency hides under the MFMAs / softmax
  u32x4 rk[S::NIT], rv[S::NIT];
  S::load(rk, rK, 0, p.Nk, p.ldk, col0, p.D, tid);
  S::load(rv, rV, 0, p.Nk, p.ldv, col0, p.D, tid);
  S::store_nat(rk, Ks2[0], tid);
  S::store_ld(rv, Vs2[0], S::LDV, tid);
  if (ntiles > 1) {
    S::load(rk, rK, TK, p.Nk, p.ldk, col0, p.D, tid);
    S::load(rv, rV, TK, p.Nk, p.ldv, col0, p.D, tid);
  }
  __syncthreads();
  // one key tile; (xk, xv) = the registers that hold tile kt + 1 on entry
  auto tile_body = [&](int kt, auto& xk, auto& xv) {
    const int k0 = kt * TK;
    const T* Ks = Ks2[kt & 1];
    const T* Vs = Vs2[kt & 1];
    if (kt + 1 < ntiles) {  // tile kt + 1 (in registers since the previous tile) into the other stage, kt + 2 on its way
      S::store_nat(xk, Ks2[(kt + 1) & 1], tid);
      S::store_ld(xv, Vs2[(kt + 1) & 1], S::LDV, tid);
      if (kt + 2 < ntiles) {
        S::load(xk, rK, k0 + 2 * TK, p.Nk, p.ldk, col0, p.D, tid);
        S::load(xv, rV, k0 + 2 * TK, p.Nk, p.ldv, col0, p.D, tid);
      }
    }

    f32x16 st[2];
    if constexpr (EX && NSD <= 4) {
      // all K fragments of the tile in flight before the first MFMA (2 * NSD * 4 registers): hipcc otherwise recycles
      // two fragment registers and waits for every read right in front of the MFMA that consumes it
      typename TT<T>::v8 kfr[2][NSD > 0 ? NSD : 1];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int s = 0; s < NSD; ++s) kfr[sub][s] = ld_frag_nat<T>(Ks, S::LDN, sub * 32 + ql, 16 * s + 8 * h2);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[sub][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NSD; ++s) st[sub] = TT<T>::mfma32(kfr[sub][s], qf[s], st[sub]);
      }
    } else {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[sub][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < nsd) {
            const auto kf = ld_frag_nat<T>(Ks, S::LDN, sub * 32 + ql, 16 * s + 8 * h2);
            st[sub] = TT<T>::mfma32(kf, qf[s], st[sub]);
          }
        }
      }
    }
    if constexpr (BIAS) {
      const int base = k0 - q_idx + p.Nk - 1;  // index of key k0 for this lane's query
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = min(max(base + sub * 32 + acc_row(r, h2), 0), nb1);
          st[sub][r] = __builtin_fmaf(st[sub][r], p.scale, bias_tab[idx]);
        }
    }
    // mask keys beyond Nk (ragged last tile only) and, for causal attention, keys after the query; tile max
    if (k0 + TK > p.Nk || p.causal) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + sub * 32 + acc_row(r, h2);
          if (key >= p.Nk || (p.causal && key > q_idx)) st[sub][r] = -INFINITY;
        }
    }
    float mloc = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, st[sub][r]);
    mloc = halves_max(mloc);
    // Lazy rescale: the running reference m_run only moves when the tile maximum exceeds it by more than 2^8 in the
    // exponent domain; until then probabilities are formed against the stale reference (p <= 256: exact in fp32,
    // representable in fp16 / bf16) and O, l stay un-rescaled.  o / l is unchanged mathematically; it saves the
    // 16 NB accumulator multiplies and an exp per tile on all but the first tile or two -- the loop is VALU-bound.
    const bool need = (mloc - m_run) * sl > 8.f;  // both halves of a query agree (mloc is already combined)
    if (__builtin_amdgcn_ballot_w64(need)) {
      const float m_new = need ? mloc : m_run;
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sl);  // 1 for lanes that keep their reference
      m_run = m_new;
      l4 *= alpha;
      if constexpr (LSE_F32) lx *= alpha;
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
    }
    const float mb = m_run * sl;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[sub][r] = __builtin_amdgcn_exp2f(st[sub][r] * sl - mb);
    if constexpr (LSE_F32) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) lx += st[sub][r];
    }
    // O^T[d, q] += V^T[d, keys] . P^T[keys, q]
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const auto pf = pack8<T>(st[sub], s2);
        const int kb = sub * 32 + s2 * 16 + 4 * h2;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const auto vf = ld_frag_trhw<T>(Vs, S::LDV, kb, i * 32, lane);
          o[i] = TT<T>::mfma32(vf, pf, o[i]);
        }
        l4 = Sum4<T>::add8(pf, l4);
      }
    __syncthreads();  // every wave is done with stage kt & 1, and stage (kt + 1) & 1 is complete
  };
  for (int kt = 0; kt < ntiles; ++kt) tile_body(kt, rk, rv);

  const float l_tot = halves_sum(l4[0]);
  const float inv = 1.f / l_tot;
  float l_lse = l_tot;
  if constexpr (LSE_F32) l_lse = halves_sum(lx);
  if (q_idx < p.Nq) {
    T* orow = (T*)p.O + ((int64_t)b * p.Nq + q_idx) * p.ldo + col0;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = i * 32 + 8 * g + 4 * h2;
        if (d < p.D) {
          Pack4<T> t;
#pragma unroll
          for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(o[i][4 * g + j] * inv);
          *reinterpret_cast<u32x2*>(orow + d) = t.u;
        }
      }
    if (p.lse && h2 == 0)
      p.lse[((int64_t)b * p.H + head) * p.Nq + q_idx] =
          m_run * scale + __logf(l_lse);
  }
}

// =============================================================================================================
// backward: delta[b,h,q] = sum_d dO[q,d] * O[q,d]
// =============================================================================================================
template <typename T>
__global__ void attn_delta_kernel(AttnParams p) {
  const int64_t total = (int64_t)p.B * p.H * p.Nq;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int h = (int)(i % p.H);
    const int64_t tok = i / p.H;  // b*Nq + q
    const T* o = (const T*)p.O + tok * p.ldo + h * p.D;
    const T* g = (const T*)p.dO + tok * p.lddo + h * p.D;
    float acc = 0.f;
    for (int d = 0; d < p.D; d += 8) {
      Pack8<T> a, c;
      a.u = *reinterpret_cast<const u32x4*>(o + d);
      c.u = *reinterpret_cast<const u32x4*>(g + d);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += to_f(a.e[j]) * to_f(c.e[j]);
    }
    const int64_t bb = tok / p.Nq, q = tok - bb * p.Nq;
    p.delta[(bb * p.H + h) * p.Nq + q] = acc;
  }
}

// =============================================================================================================
// backward: dQ.  One workgroup = 128 queries (4 waves x 32), sweeping 64-key tiles.
//   S^T = K Q^T ; P^T = exp(scale*S^T - lse[q]) ; dP^T = V dO^T ; dS^T = P^T o (dP^T - delta[q])
//   dQ^T[d,q] += K^T[d,keys] dS^T[keys,q]
// =============================================================================================================
// REMAT: re-broadcast the two row constants in front of every chain (32 v_mov per 32-key sub-tile) instead of keeping
// two 16-register copies alive across the loop (0 VALU, +32 registers: 2 waves per SIMD instead of 3)
template <typename T, int DP>
constexpr size_t dq_smem() {  // K and V by rows + K again at the transposed-read stride
  return (size_t)(2 * TK * Stage<T, DP>::LDN + TK * Stage<T, DP>::LDV) * sizeof(T);
}
// body of the dQ workgroup (bx, head, b); `smem`: dq_smem<T, DP>() bytes
// BIAS (the backward of attn_fwd_kernel's BIAS form; Nq == Nk = L, p.lse the biased forward's): the probabilities are recomputed
// as exp(scale q.k + table[head][key - query + L - 1] - lse[query]); the head's 2 L - 1 floats are staged once in `btab`
// (LDS, behind the tiles) and ordered by the first tile's barriers.  The table is frozen: nothing is differentiated to it.
// A padded query or key (ragged blocks) reads a clamped entry, as in the forward.  No guard is needed here: a padded query
// is this lane's own column of every product -- with a large entry its p dP is exp(100) x 0 = NaN, which stays in that column
// and is never stored -- and a padded key's dS is ASSIGNED 0 below, whatever its probability was.
template <typename T, int DP, int NSD, bool REMAT, bool BIAS = false>
__device__ __forceinline__ void attn_bwd_dq_body(const AttnParams& p, int bx, int head, int b, unsigned char* smem,
                                                 float* btab = nullptr) {
  using S = Stage<T, DP>;
  constexpr int NS = DP / 16, NB = DP / 32;
  T* Ks = reinterpret_cast<T*>(smem);
  T* Vs = Ks + TK * S::LDN;
  T* Ks2 = Vs + TK * S::LDN;  // K again, at the transposed-read stride

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, h2 = lane >> 5;
  const int q_idx = bx * 128 + wave * 32 + ql;
  const int col0 = head * p.D;
  const int nsd = NSD > 0 ? NSD : (p.D + 15) / 16;

  const auto rQ = make_rsrc((const T*)p.Q + (int64_t)b * p.Nq * p.ldq, (uint32_t)((int64_t)p.Nq * p.ldq * 2));
  const auto rG = make_rsrc((const T*)p.dO + (int64_t)b * p.Nq * p.lddo, (uint32_t)((int64_t)p.Nq * p.lddo * 2));
  const auto rK = make_rsrc((const T*)p.K + (int64_t)b * p.Nk * p.ldk, (uint32_t)((int64_t)p.Nk * p.ldk * 2));
  const auto rV = make_rsrc((const T*)p.V + (int64_t)b * p.Nk * p.ldv, (uint32_t)((int64_t)p.Nk * p.ldv * 2));

  const auto rO = make_rsrc((const T*)p.O + (int64_t)b * p.Nq * p.ldo, (uint32_t)((int64_t)p.Nq * p.ldo * 2));
  typename TT<T>::v8 qf[NS], gf[NS];
  // delta[q] = sum_d dO[q, d] O[q, d] is formed here from the dO fragments this lane holds anyway (one extra read of
  // the O rows) and published for the dK / dV kernel that runs next -- no separate delta launch when dQ is wanted
  float dpart = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int d = 16 * s + 8 * h2;
    const bool ok = (q_idx < p.Nq) && (d < p.D);
    Pack8<T> t, u, w;
    t.u = buf_load16(rQ, ok ? (uint32_t)(((int64_t)q_idx * p.ldq + col0 + d) * 2) : OOB);
    u.u = buf_load16(rG, ok ? (uint32_t)(((int64_t)q_idx * p.lddo + col0 + d) * 2) : OOB);
    w.u = buf_load16(rO, ok ? (uint32_t)(((int64_t)q_idx * p.ldo + col0 + d) * 2) : OOB);
    qf[s] = t.v;
    gf[s] = u.v;
#pragma unroll
    for (int j = 0; j < 8; ++j) dpart += to_f(u.e[j]) * to_f(w.e[j]);
  }
  const bool qok = q_idx < p.Nq;
  const int64_t stat = ((int64_t)b * p.H + head) * p.Nq + (qok ? q_idx : 0);
  const float dlt = halves_sum(dpart);
  if (qok && h2 == 0) p.delta[stat] = dlt;
  const float sl = p.scale * LOG2E;
  const int nb1 = 2 * p.Nk - 2;  // BIAS: last index of the table
  if constexpr (BIAS) {
    const float* src = p.bias + (int64_t)head * p.bias_ld;
    for (int i = tid; i <= nb1; i += 256) btab[i] = src[i];
  }
  // Row constants as the INITIAL ACCUMULATORS of the two score products (the query is on the lane, so they are
  // lane constants): S' = K Q^T - lse / scale leaves its MFMA chain ready for p = exp2(sl * S'), dP' = V dO^T - delta
  // is the factor of dS -- no zero fill, no subtraction.  Rows of K / V past Nk are staged as zeros; their dS is
  // zeroed in the ragged last tile (below).  Padded queries (their Q / dO fragments are zero) keep both constants at 0.
  const float cl = qok ? -p.lse[stat] / p.scale : 0.f, cd = qok ? -dlt : 0.f;
  f32x16 c_lse, c_dlt;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    c_lse[r] = cl;
    c_dlt[r] = cd;
  }

  f32x16 dq[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;

  const int ntiles = (p.Nk + TK - 1) / TK;
  u32x4 rk[S::NIT], rv[S::NIT];  // one tile ahead (see forward)
  S::load(rk, rK, 0, p.Nk, p.ldk, col0, p.D, tid);
  S::load(rv, rV, 0, p.Nk, p.ldv, col0, p.D, tid);
  for (int kt = 0; kt < ntiles; ++kt) {
    const int k0 = kt * TK;
    __syncthreads();
    S::store_nat(rk, Ks, tid);
    S::store_ld(rk, Ks2, S::LDV, tid);
    S::store_nat(rv, Vs, tid);
    __syncthreads();
    if (kt + 1 < ntiles) {
      S::load(rk, rK, k0 + TK, p.Nk, p.ldk, col0, p.D, tid);
      S::load(rv, rV, k0 + TK, p.Nk, p.ldv, col0, p.D, tid);
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 st = c_lse, dp = c_dlt;
      if constexpr (REMAT) {
        float a = cl, c = cd;
        asm volatile("" : "+v"(a), "+v"(c));  // opaque per sub-tile: the broadcasts cannot be hoisted out of the loop
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[r] = a;
          dp[r] = c;
        }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s < nsd) {
          const auto kf = ld_frag_nat<T>(Ks, S::LDN, sub * 32 + ql, 16 * s + 8 * h2);
          st = TT<T>::mfma32(kf, qf[s], st);
          const auto vf = ld_frag_nat<T>(Vs, S::LDN, sub * 32 + ql, 16 * s + 8 * h2);
          dp = TT<T>::mfma32(vf, gf[s], dp);
        }
      }
      if constexpr (BIAS) {
        const int base = k0 + sub * 32 - q_idx + p.Nk - 1;  // table index of key k0 + 32 sub for this lane's query
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int idx = min(max(base + acc_row(r, h2), 0), nb1);
          st[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(btab[idx], LOG2E, st[r] * sl)) * dp[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] * sl) * dp[r];  // dS^T = P^T o (dP^T - delta)
      }
      // keys past Nk (ragged last tile only, wave-uniform test): their K / V rows are staged as zeros, so p = exp(-lse)
      // and dS = -p delta -- with a strongly negative log-sum-exp and a loss-scaled delta that leaves the fp16 range,
      // and inf x (the zero K row) = NaN would enter dQ.  dS of a key that does not exist is 0.
      if (k0 + TK > p.Nk) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + sub * 32 + acc_row(r, h2) >= p.Nk) st[r] = 0.f;
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const auto df = pack8<T>(st, s2);
        const int kb = sub * 32 + s2 * 16 + 4 * h2;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const auto kf = ld_frag_trhw<T>(Ks2, S::LDV, kb, i * 32, lane);
          dq[i] = TT<T>::mfma32(kf, df, dq[i]);
        }
      }
    }
  }
  if (qok) {
    T* row = (T*)p.dQ + ((int64_t)b * p.Nq + q_idx) * p.lddq + col0;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = i * 32 + 8 * g + 4 * h2;
        if (d < p.D) {
          Pack4<T> t;
#pragma unroll
          for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(dq[i][4 * g + j] * p.scale);
          *reinterpret_cast<u32x2*>(row + d) = t.u;
        }
      }
  }
}
template <typename T, int DP, int NSD, bool REMAT, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[dq_smem<T, DP>()];
  extern __shared__ __attribute__((aligned(16))) float dq_bias_tab[];  // BIAS only: [2 Nk - 1]
  int bx, head, b;
  xcd_block(bx, head, b);
  attn_bwd_dq_body<T, DP, NSD, REMAT, BIAS>(p, bx, head, b, smem, dq_bias_tab);
}

// =============================================================================================================
// backward: dK, dV.  One workgroup = 128 keys (4 waves x 32, key on the lane), sweeping 64-query tiles.
//   S[q,key] = Q K^T ; P = exp(scale*S - lse[q]) ; dP[q,key] = dO V^T ; dS = P o (dP - delta[q])
//   dV^T[d,key] += dO^T[d,q] P[q,key] ;  dK^T[d,key] += Q^T[d,q] dS[q,key]
// WHICH: 1 = dK only, 2 = dV only, 3 = both (register budget: both only fits for DP <= 96)
// =============================================================================================================
// OWN_DELTA: delta[q] = sum_d dO[q, d] O[q, d] of the staged queries is formed HERE (the O rows are fetched next to dO,
// eight-lane partial dots) instead of read from p.delta: the workgroup then depends on nothing the dQ workgroups write and
// both kinds can share one launch (attn_bwd_fused_kernel).  Needs a power-of-two chunk count per row (DP = 32 / 64).
// BIAS: as in attn_bwd_dq_body.  Here the KEY is on the lane and the queries run along the tile; the table index is still
// key - query + L - 1.  A padded query's row meets every key of the block, so its probability has to be finite whatever
// entry the clamp lands on: its row constant is -inf (p = 0), where the bias-free form may leave it at 0 (p = 1).
template <typename T, int DP, int WHICH, int NSD, bool OWN_DELTA, bool BIAS = false>
__device__ __forceinline__ void attn_bwd_dkv_body(const AttnParams& p, int bx, int head, int b, unsigned char* dyn_smem,
                                                  float* btab = nullptr) {
  using S = Stage<T, DP>;
  constexpr int NS = DP / 16, NB = DP / 32;
  constexpr bool DO_DK = (WHICH & 1) != 0, DO_DV = (WHICH & 2) != 0;
  static_assert(!OWN_DELTA || (S::CPR & (S::CPR - 1)) == 0, "OWN_DELTA: chunks per row must be a power of two");
  T* Qs = reinterpret_cast<T*>(dyn_smem);
  T* Gs = Qs + TK * S::LDN;
  T* Qs2 = Gs + TK * S::LDN;  // Q and dO again, at the transposed-read stride
  T* Gs2 = Qs2 + TK * S::LDV;
  float* lse_s = reinterpret_cast<float*>(Gs2 + TK * S::LDV);  // -lse / scale per staged query (see the dQ kernel)
  float* dlt_s = lse_s + TK;                                   // -delta

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kl = lane & 31, h2 = lane >> 5;
  const int k_idx = bx * 128 + wave * 32 + kl;
  const int col0 = head * p.D;
  const int nsd = NSD > 0 ? NSD : (p.D + 15) / 16;

  const auto rQ = make_rsrc((const T*)p.Q + (int64_t)b * p.Nq * p.ldq, (uint32_t)((int64_t)p.Nq * p.ldq * 2));
  const auto rG = make_rsrc((const T*)p.dO + (int64_t)b * p.Nq * p.lddo, (uint32_t)((int64_t)p.Nq * p.lddo * 2));
  const auto rK = make_rsrc((const T*)p.K + (int64_t)b * p.Nk * p.ldk, (uint32_t)((int64_t)p.Nk * p.ldk * 2));
  const auto rV = make_rsrc((const T*)p.V + (int64_t)b * p.Nk * p.ldv, (uint32_t)((int64_t)p.Nk * p.ldv * 2));

  typename TT<T>::v8 kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int d = 16 * s + 8 * h2;
    const bool ok = (k_idx < p.Nk) && (d < p.D);
    Pack8<T> t, u;
    t.u = buf_load16(rK, ok ? (uint32_t)(((int64_t)k_idx * p.ldk + col0 + d) * 2) : OOB);
    u.u = buf_load16(rV, ok ? (uint32_t)(((int64_t)k_idx * p.ldv + col0 + d) * 2) : OOB);
    kf[s] = t.v;
    vf[s] = u.v;
  }
  const float sl = p.scale * LOG2E, inv_scale = 1.f / p.scale;
  const int64_t stat0 = ((int64_t)b * p.H + head) * p.Nq;
  const int nb1 = 2 * p.Nk - 2;  // BIAS: last index of the table
  if constexpr (BIAS) {
    const float* src = p.bias + (int64_t)head * p.bias_ld;
    for (int i = tid; i <= nb1; i += 256) btab[i] = src[i];
  }

  f32x16 dk[DO_DK ? NB : 1], dv[DO_DV ? NB : 1];
#pragma unroll
  for (int i = 0; i < (DO_DK ? NB : 1); ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] = 0.f;
#pragma unroll
  for (int i = 0; i < (DO_DV ? NB : 1); ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dv[i][r] = 0.f;

  const int ntiles = (p.Nq + TK - 1) / TK;
  u32x4 rq[S::NIT], rg[S::NIT];  // Q / dO tiles one tile ahead in registers
  u32x4 ro[OWN_DELTA ? S::NIT : 1];  // OWN_DELTA: the O rows of the same tile
  const auto rO = make_rsrc((const T*)p.O + (int64_t)b * p.Nq * p.ldo, (uint32_t)((int64_t)p.Nq * p.ldo * 2));
  float lv = 0.f, dl = 0.f;
  auto fetch = [&](int q0) {
    S::load(rq, rQ, q0, p.Nq, p.ldq, col0, p.D, tid);
    S::load(rg, rG, q0, p.Nq, p.lddo, col0, p.D, tid);
    if constexpr (OWN_DELTA) S::load(ro, rO, q0, p.Nq, p.ldo, col0, p.D, tid);
    if (tid < TK) {
      const bool ok = q0 + tid < p.Nq;
      lv = ok ? -p.lse[stat0 + q0 + tid] * inv_scale : (BIAS ? -INFINITY : 0.f);  // padded queries: their Q / dO rows are zeros, any finite P does
      if constexpr (!OWN_DELTA) dl = ok ? -p.delta[stat0 + q0 + tid] : 0.f;
    }
  };
  fetch(0);
  for (int qt = 0; qt < ntiles; ++qt) {
    const int q0 = qt * TK;
    __syncthreads();
    S::store_nat(rq, Qs, tid);
    S::store_nat(rg, Gs, tid);
    if (DO_DK) S::store_ld(rq, Qs2, S::LDV, tid);
    if (DO_DV) S::store_ld(rg, Gs2, S::LDV, tid);
    if (tid < TK) {
      lse_s[tid] = lv;
      if constexpr (!OWN_DELTA) dlt_s[tid] = dl;
    }
    if constexpr (OWN_DELTA) {
      // chunk i of this thread is row (tid + 256 i) / CPR of the tile, the CPR lanes of a row are adjacent: partial dot of
      // the 8 elements, combined by butterflies inside the aligned CPR-lane group, stored (negated) by the group's first
      // lane; rows past Nq hold zeros (-> delta 0).  The same 16-bit dO / O values as the dQ workgroups use.
#pragma unroll
      for (int i = 0; i < S::NIT; ++i) {
        Pack8<T> g, o;
        g.u = rg[i];
        o.u = ro[i];
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += to_f(g.e[j]) * to_f(o.e[j]);
#pragma unroll
        for (int m = 1; m < S::CPR; m <<= 1) d += __shfl_xor(d, m);
        const int idx = tid + 256 * i;
        if (idx % S::CPR == 0) dlt_s[idx / S::CPR] = -d;
      }
    }
    __syncthreads();
    if (qt + 1 < ntiles) fetch(q0 + TK);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      // the row constants of the four consecutive queries a register quad covers come straight out of LDS as the
      // initial accumulators: S' = Q K^T - lse / scale, dP' = dO V^T - delta
      f32x16 st, dp;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 cl = *reinterpret_cast<const f32x4*>(lse_s + sub * 32 + 8 * g + 4 * h2);
        const f32x4 cd = *reinterpret_cast<const f32x4*>(dlt_s + sub * 32 + 8 * g + 4 * h2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          st[4 * g + j] = cl[j];
          dp[4 * g + j] = DO_DK ? cd[j] : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s < nsd) {
          const auto qa = ld_frag_nat<T>(Qs, S::LDN, sub * 32 + kl, 16 * s + 8 * h2);
          st = TT<T>::mfma32(qa, kf[s], st);
          if (DO_DK) {
            const auto ga = ld_frag_nat<T>(Gs, S::LDN, sub * 32 + kl, 16 * s + 8 * h2);
            dp = TT<T>::mfma32(ga, vf[s], dp);
          }
        }
      }
      const int base = k_idx - (q0 + sub * 32) + p.Nk - 1;  // BIAS: table index of query q0 + 32 sub for this lane's key
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (BIAS)
          st[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(btab[min(max(base - acc_row(r, h2), 0), nb1)], LOG2E, st[r] * sl));
        else
          st[r] = __builtin_amdgcn_exp2f(st[r] * sl);
        if (DO_DK) dp[r] *= st[r];
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int qb = sub * 32 + s2 * 16 + 4 * h2;
        if (DO_DV) {
          const auto pf = pack8<T>(st, s2);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const auto ga = ld_frag_trhw<T>(Gs2, S::LDV, qb, i * 32, lane);
            dv[i] = TT<T>::mfma32(ga, pf, dv[i]);
          }
        }
        if (DO_DK) {
          const auto df = pack8<T>(dp, s2);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const auto qa = ld_frag_trhw<T>(Qs2, S::LDV, qb, i * 32, lane);
            dk[i] = TT<T>::mfma32(qa, df, dk[i]);
          }
        }
      }
    }
  }
  if (k_idx < p.Nk) {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = i * 32 + 8 * g + 4 * h2;
        if (d < p.D) {
          if (DO_DK) {
            Pack4<T> t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(dk[i][4 * g + j] * p.scale);
            *reinterpret_cast<u32x2*>((T*)p.dK + ((int64_t)b * p.Nk + k_idx) * p.lddk + col0 + d) = t.u;
          }
          if (DO_DV) {
            Pack4<T> t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(dv[i][4 * g + j]);
            *reinterpret_cast<u32x2*>((T*)p.dV + ((int64_t)b * p.Nk + k_idx) * p.lddv + col0 + d) = t.u;
          }
        }
      }
  }
}

// =============================================================================================================
// Short key sequences (Nk <= 96: cross-attention on the 77 text tokens, T/train_lora.py:68 routes attn2 through the same
// fused attention).  The generic kernels above run these as two 64-key tiles of an online softmax -- 40 % padding, a
// barrier and a K / V staging round trip per tile, Q / O moved in 16-32-byte pieces per row -- at 171 TF/s, twice their
// HBM time (Q read + O write).  Here ALL keys of a head sit in LDS, staged once per workgroup: three 32-key sub-tiles,
// one-pass softmax (no running maximum, no rescale), and Q / dO / O / dQ tiles move in whole 16-byte chunks of contiguous rows
// through a per-wave LDS tile (8 lanes per 128-byte row) -- the kernel is HBM-bound by construction.
// A workgroup = 4 waves x 32 queries; a wave stages, reads and writes only ITS 32 rows of the tile, so the only
// workgroup barrier is the one after K / V.
// =============================================================================================================
constexpr int XS_KEYS = 96;  // 3 sub-tiles of 32 keys

// orders a wave's own LDS accesses (ds operations of one wave execute in order; this only stops the compiler from moving
// a read above a write of another lane to the same tile)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename T, int DP>
struct XsTile {
  static constexpr int LDN = DP + 8;
  static constexpr int CPR = DP / 8;     // 16-byte chunks per row
  static constexpr int TOT = 32 * CPR;   // chunks of a wave's 32-row tile, dealt to the lanes in row-major order
  static constexpr int NIT = TOT / 64;   // (DP = 64: 4 instructions of 8 rows x 128 B)
  static_assert(TOT % 64 == 0, "tile depth");
  // this lane's chunk i of the wave's 32-row tile: (row, first column)
  static __device__ __forceinline__ void rc(int lane, int i, int& row, int& col) {
    const int idx = lane + 64 * i;
    row = idx / CPR;
    col = (idx - row * CPR) * 8;
  }
  static __device__ __forceinline__ void load(u32x4 (&reg)[NIT], __amdgpu_buffer_rsrc_t r, int64_t row0, int nrows,
                                              int64_t ld, int col0, int D, int lane) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int row, col;
      rc(lane, i, row, col);
      const bool ok = (row0 + row < nrows) && (col < D);
      reg[i] = buf_load16(r, ok ? (uint32_t)(((row0 + row) * ld + col0 + col) * 2) : OOB);
    }
  }
  static __device__ __forceinline__ void to_lds(const u32x4 (&reg)[NIT], T* tile, int lane) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int row, col;
      rc(lane, i, row, col);
      *reinterpret_cast<u32x4*>(tile + row * LDN + col) = reg[i];
    }
  }
  // rows of the wave's tile back out as whole 16-byte chunks (rows >= nrows and columns >= D are dropped)
  static __device__ __forceinline__ void store_rows(const T* tile, __amdgpu_buffer_rsrc_t r, int64_t row0, int nrows,
                                                    int64_t ld, int col0, int D, int lane) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int row, col;
      rc(lane, i, row, col);
      const bool ok = (row0 + row < nrows) && (col < D);
      const u32x4 v = *reinterpret_cast<const u32x4*>(tile + row * LDN + col);
      buf_store16(r, ok ? (uint32_t)(((row0 + row) * ld + col0 + col) * 2) : OOB, v);
    }
  }
};

// K (row reads), optionally K again at the transposed-read stride, V (row reads or transposed reads): all 96 rows, zeros
// past Nk / D.  Every thread of the workgroup takes part; the caller barriers.
template <typename T, int DP>
__device__ __forceinline__ void xs_stage_kv(__amdgpu_buffer_rsrc_t rK, __amdgpu_buffer_rsrc_t rV, int Nk, int64_t ldk,
                                            int64_t ldv, int col0, int D, int tid, T* Kn, T* Ktr, T* Vn, T* Vtr) {
  constexpr int CPR = DP / 8, LDN = DP + 8, LDV = tr_stride(DP);
  constexpr int TOT = XS_KEYS * CPR, NITK = (TOT + 255) / 256;
  u32x4 rk[NITK], rv[NITK];
#pragma unroll
  for (int i = 0; i < NITK; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / CPR, ch = idx - row * CPR;
    const bool ok = (idx < TOT) && (row < Nk) && (ch * 8 < D);
    rk[i] = buf_load16(rK, ok ? (uint32_t)(((int64_t)row * ldk + col0 + ch * 8) * 2) : OOB);
    rv[i] = buf_load16(rV, ok ? (uint32_t)(((int64_t)row * ldv + col0 + ch * 8) * 2) : OOB);
  }
#pragma unroll
  for (int i = 0; i < NITK; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / CPR, ch = idx - row * CPR;
    if (idx < TOT) {
      if (Kn) *reinterpret_cast<u32x4*>(Kn + row * LDN + ch * 8) = rk[i];
      if (Ktr) *reinterpret_cast<u32x4*>(Ktr + row * LDV + ch * 8) = rk[i];
      if (Vn) *reinterpret_cast<u32x4*>(Vn + row * LDN + ch * 8) = rv[i];
      if (Vtr) *reinterpret_cast<u32x4*>(Vtr + row * LDV + ch * 8) = rv[i];
    }
  }
}

template <typename T, int DP>
constexpr size_t xs_fwd_smem() {
  return (size_t)(XS_KEYS * (DP + 8) + XS_KEYS * tr_stride(DP) + 128 * (DP + 8)) * sizeof(T);
}
template <typename T, int DP>
constexpr size_t xs_dq_smem() {
  return (size_t)(2 * XS_KEYS * (DP + 8) + XS_KEYS * tr_stride(DP) + 128 * (DP + 8)) * sizeof(T);
}

// forward.  grid = (query blocks per workgroup chain, H, B): workgroup x walks the 128-query blocks x, x + gridDim.x, ...
// of its (batch, head) with K / V staged once.
template <typename T, int DP, int NSD>
__global__ __launch_bounds__(256, DP <= 64 ? 3 : 1) void attn_xs_fwd_kernel(AttnParams p) {
  using X = XsTile<T, DP>;
  constexpr int NB = DP / 32, LDN = DP + 8, LDV = tr_stride(DP);
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  T* Ks = reinterpret_cast<T*>(dyn_smem);
  T* Vs = Ks + XS_KEYS * LDN;
  T* Ts = Vs + XS_KEYS * LDV;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, h2 = lane >> 5;
  int bx, head, b;
  xcd_block(bx, head, b);
  const int col0 = head * p.D;
  T* tile = Ts + wave * 32 * LDN;

  const auto rQ = make_rsrc((const T*)p.Q + (int64_t)b * p.Nq * p.ldq, (uint32_t)((int64_t)p.Nq * p.ldq * 2));
  const auto rO = make_rsrc((const T*)p.O + (int64_t)b * p.Nq * p.ldo, (uint32_t)((int64_t)p.Nq * p.ldo * 2));
  const auto rK = make_rsrc((const T*)p.K + (int64_t)b * p.Nk * p.ldk, (uint32_t)((int64_t)p.Nk * p.ldk * 2));
  const auto rV = make_rsrc((const T*)p.V + (int64_t)b * p.Nk * p.ldv, (uint32_t)((int64_t)p.Nk * p.ldv * 2));

  const int nqb = (p.Nq + 127) / 128;
  u32x4 rq[X::NIT];
  X::load(rq, rQ, (int64_t)bx * 128 + wave * 32, p.Nq, p.ldq, col0, p.D, lane);  // in flight under the K / V staging
  xs_stage_kv<T, DP>(rK, rV, p.Nk, p.ldk, p.ldv, col0, p.D, tid, Ks, nullptr, nullptr, Vs);
  __syncthreads();
  const float sl = p.scale * LOG2E;

  for (int qb = bx; qb < nqb; qb += gridDim.x) {
    const int q0 = qb * 128 + wave * 32;
    const int q_idx = q0 + ql;
    X::to_lds(rq, tile, lane);
    wave_lds_sync();
    typename TT<T>::v8 qf[NSD];
#pragma unroll
    for (int s = 0; s < NSD; ++s) qf[s] = ld_frag_nat<T>(tile, LDN, ql, 16 * s + 8 * h2);
    if (qb + (int)gridDim.x < nqb)  // the next block's rows, in flight under this block's arithmetic
      X::load(rq, rQ, (int64_t)(qb + gridDim.x) * 128 + wave * 32, p.Nq, p.ldq, col0, p.D, lane);

    // S^T[key, q] = K Q^T, all keys
    f32x16 st[3];
#pragma unroll
    for (int sub = 0; sub < 3; ++sub) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[sub][r] = 0.f;
#pragma unroll
      for (int s = 0; s < NSD; ++s) {
        const auto kf = ld_frag_nat<T>(Ks, LDN, sub * 32 + ql, 16 * s + 8 * h2);
        st[sub] = TT<T>::mfma32(kf, qf[s], st[sub]);
      }
    }
    // keys past Nk: only the sub-tiles that contain some (wave-uniform tests; one compare against a lane constant and one
    // select per register -- written branch-free over all 48 registers this cost more than the exponentials)
#pragma unroll
    for (int sub = 0; sub < 3; ++sub) {
      if (sub * 32 + 32 > p.Nk) {
        asm volatile("" ::: "memory");  // keeps the (scalar) branch: hipcc otherwise if-converts all three blocks into selects
        const int lim = p.Nk - sub * 32 - 4 * h2;  // register r holds key sub * 32 + 4 h2 + (r & 3) + 8 (r >> 2)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[sub][r] = ((r & 3) + 8 * (r >> 2) >= lim) ? -INFINITY : st[sub][r];
      }
    }
    if (p.causal) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int sub = 0; sub < 3; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (sub * 32 + acc_row(r, h2) > q_idx) st[sub][r] = -INFINITY;
    }
    float m = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 3; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, st[sub][r]);
    m = halves_max(m);  // key 0 is visible to every query (also under the causal mask): finite
    const float mb = m * sl;
    // keys 80..95 (registers 8..15 of the third sub-tile) do not exist for the 77 text tokens: their exponentials, their
    // P.V step and their row sums are skipped (wave-uniform)
    const bool tail16 = p.Nk > 80;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[sub][r] = __builtin_amdgcn_exp2f(st[sub][r] * sl - mb);
#pragma unroll
    for (int r = 0; r < 8; ++r) st[2][r] = __builtin_amdgcn_exp2f(st[2][r] * sl - mb);
    if (tail16) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int r = 8; r < 16; ++r) st[2][r] = __builtin_amdgcn_exp2f(st[2][r] * sl - mb);
    }
    // bf16: lse from the fp32 sum of the unrounded probabilities, as in attn_fwd_kernel (here the dominant probability is
    // exactly 1, but the roundings of the others still reach 2e-3 in log(l)); O keeps the sum of the rounded ones
    constexpr bool LSE_F32 = std::is_same<T, bf16>::value;
    float lx = 0.f;
    if constexpr (LSE_F32) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) lx += st[sub][r];
#pragma unroll
      for (int r = 0; r < 8; ++r) lx += st[2][r];
      if (tail16) {
#pragma unroll
        for (int r = 8; r < 16; ++r) lx += st[2][r];
      }
    }

    // O^T[d, q] = V^T[d, keys] P^T[keys, q]
    f32x16 o[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    f32x4 l4 = {0.f, 0.f, 0.f, 0.f};
    auto pv_step = [&](int sub, int s2) {
      const auto pf = pack8<T>(st[sub], s2);
      const int kb = sub * 32 + s2 * 16 + 4 * h2;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const auto vf = ld_frag_trhw<T>(Vs, LDV, kb, i * 32, lane);
        o[i] = TT<T>::mfma32(vf, pf, o[i]);
      }
      l4 = Sum4<T>::add8(pf, l4);
    };
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      pv_step(sub, 0);
      pv_step(sub, 1);
    }
    pv_step(2, 0);
    if (tail16) {
      asm volatile("" ::: "memory");
      pv_step(2, 1);
    }
    const float l_tot = halves_sum(l4[0]);
    const float inv = 1.f / l_tot;
    // O rows through the wave's tile (its Q rows are consumed): a lane holds 4 consecutive d of ITS query per quad
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Pack4<T> t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(o[i][4 * g + j] * inv);
        *reinterpret_cast<u32x2*>(tile + ql * LDN + i * 32 + 8 * g + 4 * h2) = t.u;
      }
    wave_lds_sync();
    X::store_rows(tile, rO, q0, p.Nq, p.ldo, col0, p.D, lane);
    float l_lse = l_tot;
    if constexpr (LSE_F32) l_lse = halves_sum(lx);
    if (p.lse && h2 == 0 && q_idx < p.Nq) p.lse[((int64_t)b * p.H + head) * p.Nq + q_idx] = m * p.scale + __logf(l_lse);
    wave_lds_sync();  // the stores' tile reads precede the next block's Q rows
  }
}

// backward dQ for short key sequences: S^T, dP^T and dS^T as in attn_bwd_dq_kernel, every key at once; publishes delta.
template <typename T, int DP, int NSD>
__global__ __launch_bounds__(256) void attn_xs_bwd_dq_kernel(AttnParams p) {
  using X = XsTile<T, DP>;
  constexpr int NB = DP / 32, LDN = DP + 8, LDV = tr_stride(DP);
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  T* Ks = reinterpret_cast<T*>(dyn_smem);
  T* Vs = Ks + XS_KEYS * LDN;
  T* Ks2 = Vs + XS_KEYS * LDN;
  T* Ts = Ks2 + XS_KEYS * LDV;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, h2 = lane >> 5;
  int bx, head, b;
  xcd_block(bx, head, b);
  const int col0 = head * p.D;
  T* tile = Ts + wave * 32 * LDN;

  const auto rQ = make_rsrc((const T*)p.Q + (int64_t)b * p.Nq * p.ldq, (uint32_t)((int64_t)p.Nq * p.ldq * 2));
  const auto rG = make_rsrc((const T*)p.dO + (int64_t)b * p.Nq * p.lddo, (uint32_t)((int64_t)p.Nq * p.lddo * 2));
  const auto rO = make_rsrc((const T*)p.O + (int64_t)b * p.Nq * p.ldo, (uint32_t)((int64_t)p.Nq * p.ldo * 2));
  const auto rD = make_rsrc((const T*)p.dQ + (int64_t)b * p.Nq * p.lddq, (uint32_t)((int64_t)p.Nq * p.lddq * 2));
  const auto rK = make_rsrc((const T*)p.K + (int64_t)b * p.Nk * p.ldk, (uint32_t)((int64_t)p.Nk * p.ldk * 2));
  const auto rV = make_rsrc((const T*)p.V + (int64_t)b * p.Nk * p.ldv, (uint32_t)((int64_t)p.Nk * p.ldv * 2));

  const int nqb = (p.Nq + 127) / 128;
  u32x4 rq[X::NIT], rg[X::NIT], ro[X::NIT];
  auto fetch = [&](int qb) {
    const int64_t r0 = (int64_t)qb * 128 + wave * 32;
    X::load(rq, rQ, r0, p.Nq, p.ldq, col0, p.D, lane);
    X::load(rg, rG, r0, p.Nq, p.lddo, col0, p.D, lane);
    X::load(ro, rO, r0, p.Nq, p.ldo, col0, p.D, lane);
  };
  fetch(bx);
  xs_stage_kv<T, DP>(rK, rV, p.Nk, p.ldk, p.ldv, col0, p.D, tid, Ks, Ks2, Vs, nullptr);
  __syncthreads();
  const float sl = p.scale * LOG2E;

  for (int qb = bx; qb < nqb; qb += gridDim.x) {
    const int q0 = qb * 128 + wave * 32;
    const int q_idx = q0 + ql;
    const bool qok = q_idx < p.Nq;
    const int64_t stat = ((int64_t)b * p.H + head) * p.Nq + (qok ? q_idx : 0);
    // Q, dO and O rows pass through the wave's tile one after the other (whole-row loads, fragment reads)
    typename TT<T>::v8 qf[NSD], gf[NSD];
    X::to_lds(rq, tile, lane);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < NSD; ++s) qf[s] = ld_frag_nat<T>(tile, LDN, ql, 16 * s + 8 * h2);
    wave_lds_sync();
    X::to_lds(rg, tile, lane);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < NSD; ++s) gf[s] = ld_frag_nat<T>(tile, LDN, ql, 16 * s + 8 * h2);
    wave_lds_sync();
    X::to_lds(ro, tile, lane);
    wave_lds_sync();
    // delta[q] = sum_d dO[q, d] O[q, d] from the fragments (published for the dK / dV kernel that may run next)
    float dpart = 0.f;
#pragma unroll
    for (int s = 0; s < NSD; ++s) {
      Pack8<T> g, o;
      g.v = gf[s];
      o.v = ld_frag_nat<T>(tile, LDN, ql, 16 * s + 8 * h2);
#pragma unroll
      for (int j = 0; j < 8; ++j) dpart += to_f(g.e[j]) * to_f(o.e[j]);
    }
    const float dlt = halves_sum(dpart);
    if (qb + (int)gridDim.x < nqb) fetch(qb + gridDim.x);
    if (qok && h2 == 0) p.delta[stat] = dlt;
    const float cl = qok ? -p.lse[stat] / p.scale : 0.f, cd = qok ? -dlt : 0.f;

    f32x16 dq[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;
#pragma unroll
    for (int sub = 0; sub < 3; ++sub) {
      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = cl;
        dp[r] = cd;
      }
#pragma unroll
      for (int s = 0; s < NSD; ++s) {
        const auto kf = ld_frag_nat<T>(Ks, LDN, sub * 32 + ql, 16 * s + 8 * h2);
        st = TT<T>::mfma32(kf, qf[s], st);
        const auto vf = ld_frag_nat<T>(Vs, LDN, sub * 32 + ql, 16 * s + 8 * h2);
        dp = TT<T>::mfma32(vf, gf[s], dp);
      }
      // keys 80..95 (registers 8..15 of the third sub-tile) do not exist for the 77 text tokens: skipped (wave-uniform)
      const bool half2 = sub < 2 || p.Nk > 80;
#pragma unroll
      for (int r = 0; r < 8; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] * sl) * dp[r];  // dS^T = P^T o (dP^T - delta)
      if (half2) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 8; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] * sl) * dp[r];
      }
      if (sub * 32 + 32 > p.Nk) {  // keys that do not exist: dS = 0 (their p = exp(-lse) can leave the fp16 range)
        asm volatile("" ::: "memory");  // keeps the scalar branch
        const int lim = p.Nk - sub * 32 - 4 * h2;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = ((r & 3) + 8 * (r >> 2) >= lim) ? 0.f : st[r];
      }
      auto dq_step = [&](int s2) {
        const auto df = pack8<T>(st, s2);
        const int kb = sub * 32 + s2 * 16 + 4 * h2;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const auto kf = ld_frag_trhw<T>(Ks2, LDV, kb, i * 32, lane);
          dq[i] = TT<T>::mfma32(kf, df, dq[i]);
        }
      };
      dq_step(0);
      if (half2) {
        asm volatile("" ::: "memory");
        dq_step(1);
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Pack4<T> t;
#pragma unroll
        for (int j = 0; j < 4; ++j) t.e[j] = from_f<T>(dq[i][4 * g + j] * p.scale);
        *reinterpret_cast<u32x2*>(tile + ql * LDN + i * 32 + 8 * g + 4 * h2) = t.u;
      }
    wave_lds_sync();
    X::store_rows(tile, rD, q0, p.Nq, p.lddq, col0, p.D, lane);
    wave_lds_sync();
  }
}

// query blocks chained per workgroup: enough workgroups to fill the chip a few times over, K / V staged once per chain
static int xs_grid_x(const AttnParams& p) {
  const int nqb = cdiv(p.Nq, 128);
  const int64_t heads = (int64_t)p.H * p.B;
  int chain = 1;
  // measured (tools/bench_attn.py --xs, chain-length sweep): chaining pays while >= 5 workgroups per CU remain
  while (chain < 4 && nqb % (2 * chain) == 0 && heads * (nqb / (2 * chain)) >= 1280) chain *= 2;
  return nqb / chain;
}

template <typename T, int DP, int NSD>
int xs_fwd_launch(const AttnParams& p, hipStream_t st) {
  constexpr size_t sm = xs_fwd_smem<T, DP>();
  if (sm > 65536) {
    static DynLdsOnce once;
    if (int rc = once.set((const void*)attn_xs_fwd_kernel<T, DP, NSD>, (int)sm)) return rc;
  }
  dim3 grid(xs_grid_x(p), p.H, p.B);
  hipLaunchKernelGGL((attn_xs_fwd_kernel<T, DP, NSD>), grid, dim3(256), sm, st, p);
  SMI_HIP(hipGetLastError());
  return 0;
}
template <typename T, int DP, int NSD>
int xs_dq_launch(const AttnParams& p, hipStream_t st) {
  constexpr size_t sm = xs_dq_smem<T, DP>();
  if (sm > 65536) {
    static DynLdsOnce once;
    if (int rc = once.set((const void*)attn_xs_bwd_dq_kernel<T, DP, NSD>, (int)sm)) return rc;
  }
  dim3 grid(xs_grid_x(p), p.H, p.B);
  hipLaunchKernelGGL((attn_xs_bwd_dq_kernel<T, DP, NSD>), grid, dim3(256), sm, st, p);
  SMI_HIP(hipGetLastError());
  return 0;
}
// Selection override of the parity tests (set_attn_select): -1 = the environment variable, 0 = off, 1 = on
static int g_sel_xs = -1, g_sel_fused = -1;
// what the last launch_attn_fwd / launch_attn_bwd of this thread launched (attn_last_ran); host side only
static thread_local AttnRan g_ran;
static void ran_begin(int dp, int form) {
  g_ran = AttnRan();
  g_ran.dp = dp;
  g_ran.form = form;
}
static void ran_add(int family, int chain = 0) {
  if (g_ran.n < 4) g_ran.family[g_ran.n] = family;
  ++g_ran.n;
  if (chain) g_ran.chain = chain;
}
static int xs_chain(const AttnParams& p) { return cdiv(p.Nq, 128) / xs_grid_x(p); }

// SMI_ATTN_BWD_FUSED=0: dQ and dK / dV always as two launches (A/B)
static bool fused_enabled() {
  static const bool on = []() { const char* e = getenv("SMI_ATTN_BWD_FUSED"); return !(e && e[0] == '0'); }();
  return g_sel_fused < 0 ? on : g_sel_fused != 0;
}
// SMI_ATTN_XS=0: short key sequences through the generic tiled kernels (A/B)
static bool xs_enabled() {
  static const bool on = []() { const char* e = getenv("SMI_ATTN_XS"); return !(e && e[0] == '0'); }();
  return g_sel_xs < 0 ? on : g_sel_xs != 0;
}

template <typename T, int DP>
constexpr size_t dkv_smem() {
  return (size_t)(2 * TK * Stage<T, DP>::LDN + 2 * TK * Stage<T, DP>::LDV) * sizeof(T) + 2 * TK * sizeof(float);
}
template <typename T, int DP, int WHICH, int NSD, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  int bx, head, b;
  xcd_block(bx, head, b);
  attn_bwd_dkv_body<T, DP, WHICH, NSD, false, BIAS>(p, bx, head, b, dyn_smem,
                                                    reinterpret_cast<float*>(dyn_smem + dkv_smem<T, DP>()));
}

// dQ and dK / dV of a self-attention layer in ONE launch.  Each kind alone is a grid of Nq / 128 x H x B workgroups: 640 at
// SD-XL level 2 with 4 adapted samples -- 1.25 rounds of the 512 workgroups the chip holds at two waves per SIMD, so each
// launch pays for two rounds; at level 1, 2.5 -> 3.  Together they are 1280 (2560) workgroups = 2.5 (5) rounds.  The
// workgroups of a (batch, head) are adjacent in the launch order -- its key blocks (the longer ones: four products) first,
// then its query blocks -- so the XCD that gets a contiguous range of them reads Q, K, V, dO once for both kinds.  The
// dK / dV workgroups form delta themselves (OWN_DELTA): no workgroup waits for another.
template <typename T, int DP>
constexpr size_t fused_smem() {
  return dkv_smem<T, DP>() > dq_smem<T, DP>() ? dkv_smem<T, DP>() : dq_smem<T, DP>();
}
template <typename T, int DP, int NSD, bool BIAS = false>
__global__ __launch_bounds__(256) void attn_bwd_fused_kernel(AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const int nkb = (p.Nk + 127) / 128, nqb = (p.Nq + 127) / 128, per = nkb + nqb;
  const int total = gridDim.x, lin = blockIdx.x;
  const int q = total >> 3, r = total & 7, xcd = lin & 7;
  const int v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);  // XCD-contiguous order
  const int bh = v / per, j = v - bh * per;
  const int head = bh % p.H, b = bh / p.H;
  float* btab = reinterpret_cast<float*>(dyn_smem + fused_smem<T, DP>());  // BIAS only
  if (j < nkb)
    attn_bwd_dkv_body<T, DP, 3, NSD, true, BIAS>(p, j, head, b, dyn_smem, btab);
  else
    attn_bwd_dq_body<T, DP, NSD, false, BIAS>(p, j - nkb, head, b, dyn_smem, btab);
}

int check_attn(const AttnParams& p) {
  SMI_CHECK(p.D % 8 == 0 && p.D >= 8 && p.D <= 160, "attention: head_dim %d unsupported (need D %% 8 == 0, <= 160)", p.D);
  // O leaves the tiled forward in 8-byte quads, but the single-pass forward stores it, and every backward kernel reads it,
  // in whole 16-byte chunks (buf_store16 / buf_load16, the u32x4 loads of attn_delta_kernel): 16 bytes like the others
  SMI_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.ldo % 8 == 0,
            "attention: row strides ldq %lld ldk %lld ldv %lld ldo %lld must be multiples of 8 elements (16 bytes)",
            (long long)p.ldq, (long long)p.ldk, (long long)p.ldv, (long long)p.ldo);
  SMI_CHECK(p.B > 0 && p.H > 0 && p.Nq > 0 && p.Nk > 0, "attention: empty shape");
  SMI_CHECK((int64_t)p.Nq * p.ldq * 2 < 0xFFFFFFF0ll && (int64_t)p.Nk * p.ldk * 2 < 0xFFFFFFF0ll, "attention: per-batch tensor larger than 4 GiB");
  return 0;
}

int check_attn_bias(const AttnParams& p) {
  SMI_CHECK(p.D == 64 && p.Nq == p.Nk && !p.causal,
            "attention with a relative-position bias: self-attention (Nq %d == Nk %d), head_dim 64 (got %d), no causal mask",
            p.Nq, p.Nk, p.D);
  SMI_CHECK(p.Nk <= ATTN_BIAS_MAX_L && p.bias_ld >= 2 * p.Nk - 1,
            "attention with a relative-position bias: L %d exceeds %d (the table is staged in LDS), or table rows of %lld < 2 L - 1",
            p.Nk, ATTN_BIAS_MAX_L, (long long)p.bias_ld);
  return 0;
}

// compile-time k-step counts offered for a tile depth DP: the full depth, and the SD-1.x head widths that sit inside a
// wider tile (40 -> 3 steps of DP = 64, 80 -> 5 steps of DP = 96); anything else takes the run-time form (0)
template <int DP> constexpr int alt_steps() { return DP == 64 ? 3 : (DP == 96 ? 5 : 0); }

template <typename T, int DP>
int fwd_t(const AttnParams& p, hipStream_t st) {
  dim3 grid(cdiv(p.Nq, 128), p.H, p.B);
  constexpr int NS = DP / 16, ALT = alt_steps<DP>();
  const int nsd = (p.D + 15) / 16;
  ran_begin(DP, nsd == NS ? 1 : (ALT > 0 && nsd == ALT ? 2 : 0));
  if (p.Nk <= XS_KEYS && xs_enabled() && g_ran.form != 0 && !p.bias) {  // all keys at once (cross-attention on the text tokens)
    ran_add(ATTN_RAN_XS_FWD, xs_chain(p));
    if (nsd == NS) return xs_fwd_launch<T, DP, NS>(p, st);
    return xs_fwd_launch<T, DP, (ALT > 0 ? ALT : NS)>(p, st);
  }
  ran_add(ATTN_RAN_FWD);
  if constexpr (DP == 64) {
    if (p.bias) {  // (launch_attn_fwd has checked the shape: head_dim 64, Nq == Nk, the table within LDS)
      hipLaunchKernelGGL((attn_fwd_kernel<T, DP, NS, true>), grid, dim3(256), (size_t)(2 * p.Nk - 1) * sizeof(float), st, p);
      SMI_HIP(hipGetLastError());
      return 0;
    }
  }
  if (nsd == NS)
    hipLaunchKernelGGL((attn_fwd_kernel<T, DP, NS>), grid, dim3(256), 0, st, p);
  else if (ALT > 0 && nsd == ALT)
    hipLaunchKernelGGL((attn_fwd_kernel<T, DP, (ALT > 0 ? ALT : NS)>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((attn_fwd_kernel<T, DP, 0>), grid, dim3(256), 0, st, p);
  SMI_HIP(hipGetLastError());
  return 0;
}

template <typename T, int DP, int WHICH, int NSD>
int dkv_launch(const AttnParams& p, dim3 grid, size_t sm, hipStream_t st) {
  if (sm > 65536) {
    static DynLdsOnce once;  // (per instantiation, per device)
    if (int rc = once.set((const void*)attn_bwd_dkv_kernel<T, DP, WHICH, NSD>, (int)sm)) return rc;
  }
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, DP, WHICH, NSD>), grid, dim3(256), sm, st, p);
  return 0;
}

// The backward of the BIAS forward (head_dim 64, Nq == Nk; launch_attn_bwd has checked the shape).  The delta launch of the
// dK / dV-only form has gone out already.  The fused launch by the grid rule of bwd_t, without its Nk > 96 clause (that one
// keeps the single-pass kernels, which know no bias, in charge of short keys); otherwise the two tiled launches.  The tiles'
// LDS and the table's 2 L - 1 floats stay below 64 KB for every L <= ATTN_BIAS_MAX_L.
template <typename T>
int bwd_bias(const AttnParams& p, hipStream_t st) {
  constexpr int DP = 64, NS = DP / 16;
  const size_t tab = (size_t)(2 * p.Nk - 1) * sizeof(float);
  static_assert(fused_smem<T, DP>() + (2 * ATTN_BIAS_MAX_L - 1) * sizeof(float) <= 65536, "bias table next to the tiles");
  if (fused_enabled() && p.dQ && p.dK && (int64_t)cdiv(p.Nq, 128) * p.H * p.B <= 1024) {
    ran_add(ATTN_RAN_BWD_FUSED);
    const int64_t total = (int64_t)(cdiv(p.Nk, 128) + cdiv(p.Nq, 128)) * p.H * p.B;
    const size_t sm = fused_smem<T, DP>() + tab;
    hipLaunchKernelGGL((attn_bwd_fused_kernel<T, DP, NS, true>), dim3((unsigned)total), dim3(256), sm, st, p);
    SMI_HIP(hipGetLastError());
    return 0;
  }
  if (p.dQ) {
    ran_add(ATTN_RAN_DQ);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<T, DP, NS, false, true>), dim3(cdiv(p.Nq, 128), p.H, p.B), dim3(256), tab, st, p);
  }
  if (p.dK) {
    ran_add(ATTN_RAN_DKV);
    const size_t sm = dkv_smem<T, DP>() + tab;
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, DP, 3, NS, true>), dim3(cdiv(p.Nk, 128), p.H, p.B), dim3(256), sm, st, p);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}

template <typename T, int DP>
int bwd_t(const AttnParams& p, hipStream_t st) {
  constexpr int NS = DP / 16, ALT = alt_steps<DP>();
  constexpr int ALTC = ALT > 0 ? ALT : NS;
  const int nsd = (p.D + 15) / 16;
  const int form = nsd == NS ? 1 : (ALT > 0 && nsd == ALT ? 2 : 0);  // 1: full depth, 2: the alternative, 0: run-time
  ran_begin(DP, form);
  if (!p.dQ) {  // dK / dV only: nobody else forms delta
    ran_add(ATTN_RAN_DELTA);
    const int64_t total = (int64_t)p.B * p.H * p.Nq;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(attn_delta_kernel<T>, dim3(grid), dim3(256), 0, st, p);
  }
  if constexpr (DP == 64) {
    if (p.bias) return bwd_bias<T>(p, st);
  }
  // self-attention with every gradient wanted: one launch for both kinds of workgroup (attn_bwd_fused_kernel)
  if constexpr (DP <= 64) {
    // by measurement (tools/bench_attn.py, SMI_ATTN_BWD_FUSED=0|1): it pays on the small grids -- 4 samples x 20 heads x
    // 1024^2: 116.8 -> 110.6 us -- and loses 3-5 % from 4096 keys on (the two kinds then fill whole rounds by themselves)
    // (Since the backward runs on the live half of the adapted samples alone, the headline's 4096-key level has 640
    // workgroups per kind and takes the fused launch as well: measured inside the step against the separate kernels there,
    // 153.56 vs 153.67 ms per step over three alternations -- no difference, so the rule stays a grid-size rule.)
    if (fused_enabled() && p.dQ && p.dK && p.dV && form != 0 && p.Nk > XS_KEYS &&
        (int64_t)cdiv(p.Nq, 128) * p.H * p.B <= 1024) {
      ran_add(ATTN_RAN_BWD_FUSED);
      constexpr size_t sm = fused_smem<T, DP>();
      const int64_t total = (int64_t)(cdiv(p.Nk, 128) + cdiv(p.Nq, 128)) * p.H * p.B;
      SMI_CHECK(total < (1ll << 31), "attention bwd: grid too large");
      if (form == 1) {
        if (sm > 65536) {
          static DynLdsOnce once;
          if (int rc = once.set((const void*)attn_bwd_fused_kernel<T, DP, NS>, (int)sm)) return rc;
        }
        hipLaunchKernelGGL((attn_bwd_fused_kernel<T, DP, NS>), dim3((unsigned)total), dim3(256), sm, st, p);
      } else {
        if (sm > 65536) {
          static DynLdsOnce once;
          if (int rc = once.set((const void*)attn_bwd_fused_kernel<T, DP, ALTC>, (int)sm)) return rc;
        }
        hipLaunchKernelGGL((attn_bwd_fused_kernel<T, DP, ALTC>), dim3((unsigned)total), dim3(256), sm, st, p);
      }
      SMI_HIP(hipGetLastError());
      return 0;
    }
  }
  if (p.dQ && p.Nk <= XS_KEYS && xs_enabled() && form != 0) {
    ran_add(ATTN_RAN_XS_DQ, xs_chain(p));
    if (form == 1) { if (xs_dq_launch<T, DP, NS>(p, st)) return -2; }
    else { if (xs_dq_launch<T, DP, ALTC>(p, st)) return -2; }
  } else if (p.dQ) {
    ran_add(ATTN_RAN_DQ);
    dim3 grid(cdiv(p.Nq, 128), p.H, p.B);
    if (form == 1)
      hipLaunchKernelGGL((attn_bwd_dq_kernel<T, DP, NS, false>), grid, dim3(256), 0, st, p);
    else if (form == 2)
      hipLaunchKernelGGL((attn_bwd_dq_kernel<T, DP, ALTC, false>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((attn_bwd_dq_kernel<T, DP, 0, true>), grid, dim3(256), 0, st, p);
  }
  if (p.dK || p.dV) {
    SMI_CHECK(p.dK && p.dV, "attention bwd: dK and dV must both be given");
    dim3 grid(cdiv(p.Nk, 128), p.H, p.B);
    const size_t sm = dkv_smem<T, DP>();
    ran_add(DP <= 96 ? ATTN_RAN_DKV : ATTN_RAN_DK_DV);
    if (DP <= 96) {
      if (form == 1) { if (dkv_launch<T, DP, 3, NS>(p, grid, sm, st)) return -2; }
      else if (form == 2) { if (dkv_launch<T, DP, 3, ALTC>(p, grid, sm, st)) return -2; }
      else { if (dkv_launch<T, DP, 3, 0>(p, grid, sm, st)) return -2; }
    } else {
      if (form == 1) {
        if (dkv_launch<T, DP, 1, NS>(p, grid, sm, st) || dkv_launch<T, DP, 2, NS>(p, grid, sm, st)) return -2;
      } else {
        if (dkv_launch<T, DP, 1, 0>(p, grid, sm, st) || dkv_launch<T, DP, 2, 0>(p, grid, sm, st)) return -2;
      }
    }
  }
  SMI_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int dispatch(const AttnParams& p, hipStream_t st, bool bwd) {
  if (p.D <= 32) return bwd ? bwd_t<T, 32>(p, st) : fwd_t<T, 32>(p, st);
  if (p.D <= 64) return bwd ? bwd_t<T, 64>(p, st) : fwd_t<T, 64>(p, st);
  if (p.D <= 96) return bwd ? bwd_t<T, 96>(p, st) : fwd_t<T, 96>(p, st);
  return bwd ? bwd_t<T, 160>(p, st) : fwd_t<T, 160>(p, st);
}

}  // namespace

void set_attn_select(int xs, int fused) {
  g_sel_xs = xs;
  g_sel_fused = fused;
}
AttnRan attn_last_ran() { return g_ran; }

int launch_attn_fwd(const AttnParams& p, hipStream_t stream) {
  g_ran = AttnRan();
  if (check_attn(p)) return -1;
  if (p.bias && check_attn_bias(p)) return -1;
  return p.dtype == DT_F16 ? dispatch<f16>(p, stream, false) : dispatch<bf16>(p, stream, false);
}
int launch_attn_bwd(const AttnParams& p, hipStream_t stream) {
  g_ran = AttnRan();
  if (p.bias) {  // (before the causal route: a bias and a mask are refused; before any launch: a refusal queues nothing)
    if (check_attn(p) || check_attn_bias(p)) return -1;
    SMI_CHECK(!p.dK == !p.dV, "attention bwd: dK and dV must both be given");
  }
  if (p.causal) return launch_attn_causal_bwd(p, stream);  // the kernels below know no mask
  if (check_attn(p)) return -1;
  SMI_CHECK(p.lse && p.delta && p.dO && p.O, "attention bwd: lse/delta/dO/O required");
  // dO rows are read, and dQ rows written by the single-pass kernel, in whole 16-byte chunks
  SMI_CHECK(p.lddo % 8 == 0 && (!p.dQ || p.lddq % 8 == 0) && (!p.dK || p.lddk % 8 == 0) && (!p.dV || p.lddv % 8 == 0),
            "attention bwd: row strides lddo %lld lddq %lld lddk %lld lddv %lld must be multiples of 8 elements (16 bytes)",
            (long long)p.lddo, (long long)p.lddq, (long long)p.lddk, (long long)p.lddv);
  return p.dtype == DT_F16 ? dispatch<f16>(p, stream, true) : dispatch<bf16>(p, stream, true);
}

}  // namespace smi
