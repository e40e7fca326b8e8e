// GroupNorm (+SiLU) and LayerNorm, forward and activation-gradient, on token-major [N, HW, C] tensors.
// HBM-bound: every pass reads/writes each element once with 16-byte lanes; statistics are two-stage and
// deterministic (per-chunk partials reduced in a fixed order -- no float atomics).
//
// GroupNorm forward:  partial(mean, M2 = sum (x - mean)^2 per (n, chunk, g)) -> apply: every workgroup first merges the
//                     (<= 64) chunk partials of its sample to mean / rstd in LDS (a few KB from L2; a separate "finalize" launch was
//                     25 us of pure latency, 736 times per step), then y = silu?(x*a + b) for its rows; the workgroup
//                     of chunk 0 also stores mean / rstd and the per-(n,c) affine a, b for the backward
// GroupNorm backward: z = x*a+b, dz = dy*silu'(z);  S1 = sum dz*gamma, S2 = sum dz*(z-beta)  per (n,g)
//                     dx = a*dz + c2*x + c3   with  c2 = -r^2*S2/cnt,  c3 = -r*S1/cnt - c2*mu
#include <stdlib.h>


#include "kernels.h"

namespace smi {
namespace {

// rows per chunk: at most 64 chunks per sample (the apply kernels re-reduce the chunk partials), at least 16 rows
// (the 32x32 maps then still give 64 workgroups per sample).  Depends on HW only, so a sample's arithmetic does not
// depend on the batch it travels in (the norms' own arithmetic; the split-K GEMMs' slice count does follow the batch,
// csrc/gemm.hip).
// Maps beyond 128 x 128 (the VAE encoder: 1024 x 1024 x 128 channels of ONE image) get 256-row chunks instead -- 64
// workgroups on 256 CUs ran those at 0.64 TB/s -- and their partials are folded down to 64 slots by gn_fold_kernel
// before the apply kernels re-reduce them.
constexpr int GN_MAX_SLOTS = 64;
__host__ __device__ inline int gn_rows_per_chunk(int HW) {
  if (HW > 16384) return 256;
  const int r = (HW + 63) / 64;
  return r < 16 ? 16 : (r + 15) / 16 * 16;
}

struct GnGeom {
  int cols8;  // C / 8
  int ncol;   // column vectors per thread (ceil(cols8 / 256))
  int rpar;   // rows processed in parallel by one block
};
__host__ __device__ inline GnGeom gn_geom(int C) {
  GnGeom g;
  g.cols8 = C / 8;
  g.ncol = (g.cols8 + 255) / 256;
  g.rpar = g.cols8 >= 256 ? 1 : 256 / g.cols8;
  return g;
}

// rows of a chunk of `nrows` rows that row lane `rs` of `rpar` walks (rs, rs + rpar, ...)
__host__ __device__ inline int gn_lane_rows(int nrows, int rs, int rpar) {
  return rs < nrows ? (nrows - rs + rpar - 1) / rpar : 0;
}

// MODE 0: forward stats.  MODE 1: backward stats (S1, S2), SILU selects dz = dy*silu'(z).
// The forward statistics never form sum x^2 - (sum x)^2 / n on the raw data (that loses rstd once |mean| / std passes
// ~30: 2 % at 300).  A thread sums (x - k) and (x - k)^2 with k = the first element it reads of that channel, so the
// cancellation is relative to the spread of its own few rows; its (mean, M2) and those of the other row lanes and
// channels of the group are then merged (Chan et al.: M2 = sum M2_i + sum n_i (mean_i - mean)^2, the last sum itself
// taken shifted by the first entry's mean, whose distance to the others is a fraction of the spread), and so are the chunk
// partials in the fold and in the apply head.  Counts follow from the geometry, so a partial stays two floats: (mean, M2).
template <typename T, int MODE, bool SILU>
__device__ __forceinline__ void gn_partial_body(float* red /* LDS [rpar][C][2] */, int n, int chunk,
                                                const T* __restrict__ x, const T* __restrict__ dy,
                                                const T* __restrict__ gamma, const T* __restrict__ beta,
                                                const float* __restrict__ aa, const float* __restrict__ bb,
                                                float* __restrict__ partial, int HW, int C, int G, int nchunk) {
  const GnGeom gg = gn_geom(C);
  const int tid = threadIdx.x;
  const int rsub = gg.cols8 >= 256 ? 0 : tid / gg.cols8;
  const int col_base = gg.cols8 >= 256 ? tid : tid - rsub * gg.cols8;
  const bool active = rsub < gg.rpar;
  const int row0 = chunk * gn_rows_per_chunk(HW);
  const int row1 = min(HW, row0 + gn_rows_per_chunk(HW));
  const float* an = aa + (int64_t)n * C;  // only dereferenced in MODE 1
  const float* bn = bb + (int64_t)n * C;

  for (int j = 0; j < gg.ncol; ++j) {
    const int col = col_base + 256 * j;
    const bool cok = active && col < gg.cols8;
    float s0[8], s1[8], av[8], bv[8], gv[8], be[8], kv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s0[e] = s1[e] = kv[e] = 0.f;
    if (cok && MODE == 1) {
      Pack8<T> g8, b8;
      g8.u = *reinterpret_cast<const u32x4*>(gamma + col * 8);
      b8.u = *reinterpret_cast<const u32x4*>(beta + col * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        av[e] = an[col * 8 + e];
        bv[e] = bn[col * 8 + e];
        gv[e] = to_f(g8.e[e]);
        be[e] = to_f(b8.e[e]);
      }
    }
    if (cok) {
      // 4 independent row loads in flight per thread (otherwise a chain of dependent HBM latencies)
      for (int r0 = row0 + rsub; r0 < row1; r0 += 4 * gg.rpar) {
        Pack8<T> xv4[4], dv4[4];
        bool ok4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = r0 + u * gg.rpar;
          ok4[u] = r < row1;
          const int64_t off = ((int64_t)n * HW + (ok4[u] ? r : row0)) * C + col * 8;
          xv4[u].u = *reinterpret_cast<const u32x4*>(x + off);
          if (MODE == 1) dv4[u].u = *reinterpret_cast<const u32x4*>(dy + off);
        }
        if (MODE == 0 && r0 == row0 + rsub) {  // k: the thread's first row (no load of its own)
#pragma unroll
          for (int e = 0; e < 8; ++e) kv[e] = to_f(xv4[0].e[e]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!ok4[u]) continue;
          if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float v = to_f(xv4[u].e[e]) - kv[e];
              s0[e] += v;
              s1[e] += v * v;
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float z = to_f(xv4[u].e[e]) * av[e] + bv[e];
              float dz = to_f(dv4[u].e[e]);
              if (SILU) dz *= dsilu_f(z);
              s0[e] += dz * gv[e];
              s1[e] += dz * (z - be[e]);
            }
          }
        }
      }
      if (MODE == 0) {  // this lane's (mean, M2) of each channel
        const int nr = gn_lane_rows(row1 - row0, rsub, gg.rpar);
        const float inv = nr ? 1.f / (float)nr : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = s0[e] * inv;
          s1[e] = fmaxf(s1[e] - s0[e] * d, 0.f);
          s0[e] = kv[e] + d;
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[((int64_t)rsub * C + col * 8 + e) * 2 + 0] = s0[e];
        red[((int64_t)rsub * C + col * 8 + e) * 2 + 1] = s1[e];
      }
    }
  }
  __syncthreads();
  // 8 lanes per group walk its [rpar][cpg] entries (lane l takes channels l, l + 8, ... of every row lane), xor tree: fixed
  // order.  MODE 0 merges the (mean, M2) entries in one pass, the means shifted by the first entry's (row lane 0 always has
  // a row; lanes with none carry weight 0):
  //   mean = mref + sum n_i d_i / n,  M2 = sum M2_i + sum n_i d_i^2 - (sum n_i d_i)^2 / n,  d_i = mean_i - mref
  const int cpg = C / G;
  for (int g = tid >> 3; g < G; g += 32) {
    float a0 = 0.f, a1 = 0.f, q = 0.f;
    const float mref = red[((int64_t)g * cpg) * 2];
    for (int rs = 0; rs < gg.rpar; ++rs) {
      const float nr = (float)gn_lane_rows(row1 - row0, rs, gg.rpar);
      for (int c = g * cpg + (tid & 7); c < (g + 1) * cpg; c += 8) {
        const float v0 = red[((int64_t)rs * C + c) * 2 + 0], v1 = red[((int64_t)rs * C + c) * 2 + 1];
        if (MODE == 0) {
          const float d = v0 - mref;
          a0 += nr * d;
          q += nr * d * d;
          a1 += v1;
        } else {
          a0 += v0;
          a1 += v1;
        }
      }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o);
      a1 += __shfl_xor(a1, o);
      if (MODE == 0) q += __shfl_xor(q, o);
    }
    if (tid & 7) continue;
    if (MODE == 0) {
      const float nn = (float)(row1 - row0) * (float)cpg;
      a1 += fmaxf(q - a0 * a0 / nn, 0.f);
      a0 = mref + a0 / nn;
    }
    float* out = partial + (((int64_t)n * nchunk + chunk) * G + g) * 2;
    out[0] = a0;
    out[1] = a1;
  }
}
template <typename T, int MODE, bool SILU>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                         const T* __restrict__ gamma, const T* __restrict__ beta,
                                                         const float* __restrict__ aa, const float* __restrict__ bb,
                                                         float* __restrict__ partial, int Nb, int HW, int C, int G,
                                                         int nchunk) {
  extern __shared__ float red[];  // [rpar][C][2]
  gn_partial_body<T, MODE, SILU>(red, blockIdx.y, blockIdx.x, x, dy, gamma, beta, aa, bb, partial, HW, C, G, nchunk);
}

// rows of slot s when every slot but the last holds R rows of the HW (0 for a slot past the end)
__host__ __device__ inline int gn_slot_rows(int HW, int R, int s) {  // s * R < 2 HW: no overflow
  const int r = HW - s * R;
  return r <= 0 ? 0 : (r < R ? r : R);
}

// partial [Nb][nchunk][G][2] -> folded [Nb][GN_MAX_SLOTS][G][2]: slot s = chunks [s per, (s + 1) per) in order; the
// backward's (S1, S2) are summed, the forward's (mean, M2) (STATS) merged around the slot's mean
template <bool STATS>
__global__ __launch_bounds__(256) void gn_fold_kernel(const float* __restrict__ partial, float* __restrict__ folded,
                                                      int nchunk, int G2, int HW, int cpg) {
  const int n = blockIdx.y, s = blockIdx.x;
  const int per = (nchunk + GN_MAX_SLOTS - 1) / GN_MAX_SLOTS;
  const int c0 = s * per, c1 = min(nchunk, c0 + per);
  if (STATS) {
    const int rpc = gn_rows_per_chunk(HW);
    for (int g = threadIdx.x; g < G2 / 2; g += 256) {
      float mean = 0.f, m2 = 0.f;
      if (c0 < c1) {
        const float mref = partial[((int64_t)n * nchunk + c0) * G2 + g * 2];
        float acc = 0.f, q = 0.f;
        for (int c = c0; c < c1; ++c) {
          const float* p = partial + ((int64_t)n * nchunk + c) * G2 + g * 2;
          const float rows = (float)gn_slot_rows(HW, rpc, c), d = p[0] - mref;
          acc += rows * d;
          q += rows * d * d;
          m2 += p[1];
        }
        const float nrows = (float)gn_slot_rows(HW, per * rpc, s);
        m2 += (float)cpg * fmaxf(q - acc * acc / nrows, 0.f);
        mean = mref + acc / nrows;
      }
      folded[((int64_t)n * GN_MAX_SLOTS + s) * G2 + g * 2] = mean;
      folded[((int64_t)n * GN_MAX_SLOTS + s) * G2 + g * 2 + 1] = m2;
    }
    return;
  }
  for (int t = threadIdx.x; t < G2; t += 256) {
    float a = 0.f;
    for (int c = c0; c < c1; ++c) a += partial[((int64_t)n * nchunk + c) * G2 + t];
    folded[((int64_t)n * GN_MAX_SLOTS + s) * G2 + t] = a;
  }
}

// The (mean, M2) slot partials of (n, g) -> mean and variance of the group; called by the 8 lanes that walk the slots of
// a group (lane8 = 0..7), the same result in each.  Fixed order.  nslot: the chunk count, or GN_MAX_SLOTS after a fold.
__device__ __forceinline__ void gn_merge_slots(const float* partial, int n, int g, int G, int nslot, int HW, int cpg,
                                               int lane8, float& mean, float& var) {
  const int rpc = gn_rows_per_chunk(HW);
  const int nch = (HW + rpc - 1) / rpc;
  const int R = (nslot < nch ? (nch + GN_MAX_SLOTS - 1) / GN_MAX_SLOTS : 1) * rpc;  // rows per slot
  const float* base = partial + ((int64_t)n * nslot * G + g) * 2;
  float pm[GN_MAX_SLOTS / 8], pq[GN_MAX_SLOTS / 8], rows[GN_MAX_SLOTS / 8];
#pragma unroll
  for (int i = 0; i < GN_MAX_SLOTS / 8; ++i) {  // every load in flight at once: one trip to L2, as the plain sums had
    const int ch = lane8 + 8 * i;
    const bool ok = ch < nslot;
    rows[i] = ok ? (float)gn_slot_rows(HW, R, ch) : 0.f;
    pm[i] = ok ? base[(int64_t)ch * G * 2] : 0.f;
    pq[i] = ok ? base[(int64_t)ch * G * 2 + 1] : 0.f;
  }
  const float mref = __shfl(pm[0], (threadIdx.x & 63) & ~7);  // slot 0's mean
  float acc = 0.f, q = 0.f, m2 = 0.f;
#pragma unroll
  for (int i = 0; i < GN_MAX_SLOTS / 8; ++i) {
    const float d = rows[i] != 0.f ? pm[i] - mref : 0.f;
    acc += rows[i] * d;
    q += rows[i] * d * d;
    m2 += pq[i];
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o);
    q += __shfl_xor(q, o);
    m2 += __shfl_xor(m2, o);
  }
  mean = mref + acc / (float)HW;
  m2 += (float)cpg * fmaxf(q - acc * acc / (float)HW, 0.f);
  var = m2 / ((float)HW * (float)cpg);
}

// MODE 0: y = silu?(x*a+b).   MODE 1: dx = a*dz + c2*x + c3 (+ add).
// Grid (chunk, n) as the partial kernel.  Head: the chunk partials of sample n -> per-group statistics in LDS
// (8 lanes per group walk the partials, xor tree: fixed order, deterministic), then the rows of this chunk.
template <typename T, int MODE, bool SILU>
__device__ __forceinline__ void gn_apply_body(float* st /* LDS [G][2]: MODE 0 (mean, rstd); MODE 1 (c2, c3) */, int n,
                                              int chunk, const T* __restrict__ x, const T* __restrict__ dy,
                                              const T* __restrict__ gamma, const T* __restrict__ beta,
                                              const float* partial, float* aa, float* bb, float* mean_rstd,
                                              const T* add, T* out, int HW, int C, int G, int nchunk, float eps) {
  // nchunk = slots of `partial` per sample (the grid's chunk count, or GN_MAX_SLOTS after a fold)
  const GnGeom gg = gn_geom(C);
  const int tid = threadIdx.x;
  const int cpg = C / G;
  const float cnt = (float)HW * (float)cpg;
  for (int g = tid >> 3; g < G; g += 32) {
    float s = 0.f, sq = 0.f;
    if (MODE == 0) {
      gn_merge_slots(partial, n, g, G, nchunk, HW, cpg, tid & 7, s, sq);  // (mean, variance)
    } else {
      for (int ch = tid & 7; ch < nchunk; ch += 8) {
        const float* p = partial + (((int64_t)n * nchunk + ch) * G + g) * 2;
        s += p[0];
        sq += p[1];
      }
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        sq += __shfl_xor(sq, o);
      }
    }
    if (tid & 7) continue;
    if (MODE == 0) {
      const float mean = s;
      const float rstd = rsqrtf(sq + eps);
      st[g * 2] = mean;
      st[g * 2 + 1] = rstd;
      if (chunk == 0) {
        mean_rstd[((int64_t)n * G + g) * 2] = mean;
        mean_rstd[((int64_t)n * G + g) * 2 + 1] = rstd;
      }
    } else {
      const float mu = mean_rstd[((int64_t)n * G + g) * 2];
      const float r = mean_rstd[((int64_t)n * G + g) * 2 + 1];
      const float c2 = -r * r * sq / cnt;  // (s, sq) = (S1, S2)
      st[g * 2] = c2;
      st[g * 2 + 1] = -r * s / cnt - c2 * mu;
    }
  }
  __syncthreads();
  const int rsub = gg.cols8 >= 256 ? 0 : tid / gg.cols8;
  const int col_base = gg.cols8 >= 256 ? tid : tid - rsub * gg.cols8;
  if (rsub >= gg.rpar) return;
  const int rpc = gn_rows_per_chunk(HW);
  const int row0 = chunk * rpc;
  const int row1 = min(HW, row0 + rpc);
  float* an = aa + (int64_t)n * C;
  float* bn = bb + (int64_t)n * C;
  for (int j = 0; j < gg.ncol; ++j) {
    const int col = col_base + 256 * j;
    if (col >= gg.cols8) break;
    float av[8], bv[8], c2[8], c3[8];
    if (MODE == 0) {
      Pack8<T> g8, b8;
      g8.u = *reinterpret_cast<const u32x4*>(gamma + col * 8);
      b8.u = *reinterpret_cast<const u32x4*>(beta + col * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int g = (col * 8 + e) / cpg;
        av[e] = st[g * 2 + 1] * to_f(g8.e[e]);
        bv[e] = to_f(b8.e[e]) - st[g * 2] * av[e];
      }
      if (chunk == 0 && rsub == 0) {  // the backward reads the affine back
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          an[col * 8 + e] = av[e];
          bn[col * 8 + e] = bv[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int g = (col * 8 + e) / cpg;
        av[e] = an[col * 8 + e];
        bv[e] = bn[col * 8 + e];
        c2[e] = st[g * 2];
        c3[e] = st[g * 2 + 1];
      }
    }
    for (int r0 = row0 + rsub; r0 < row1; r0 += 4 * gg.rpar) {
      Pack8<T> xv4[4], dv4[4], ad4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * gg.rpar;
        const int64_t off = ((int64_t)n * HW + (r < row1 ? r : row0)) * C + col * 8;
        xv4[u].u = *reinterpret_cast<const u32x4*>(x + off);
        if (MODE == 1) {
          dv4[u].u = *reinterpret_cast<const u32x4*>(dy + off);
          if (add) ad4[u].u = *reinterpret_cast<const u32x4*>(add + off);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = r0 + u * gg.rpar;
        if (r >= row1) continue;
        Pack8<T> o;
        if (MODE == 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float z = to_f(xv4[u].e[e]) * av[e] + bv[e];
            if (SILU) z = silu_f(z);
            o.e[e] = from_f<T>(z);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xe = to_f(xv4[u].e[e]);
            float dz = to_f(dv4[u].e[e]);
            if (SILU) dz *= dsilu_f(xe * av[e] + bv[e]);
            o.e[e] = from_f<T>(av[e] * dz + c2[e] * xe + c3[e] + (add ? to_f(ad4[u].e[e]) : 0.f));
          }
        }
        *reinterpret_cast<u32x4*>(out + ((int64_t)n * HW + r) * C + col * 8) = o.u;
      }
    }
  }
}
// statistics only (the VAE decoder's fused tail applies the norm itself): the slot partials of sample n -> mean / rstd
// per group with the apply kernels' head (same order), then the per-(n,c) affine a, b for all C channels
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ gamma, const T* __restrict__ beta,
                                                       const float* __restrict__ partial, float* __restrict__ aa,
                                                       float* __restrict__ bb, float* __restrict__ mean_rstd, int HW,
                                                       int C, int G, int nchunk, float eps) {
  extern __shared__ float st[];  // [G][2]
  const int n = blockIdx.x, tid = threadIdx.x;
  const int cpg = C / G;
  for (int g = tid >> 3; g < G; g += 32) {
    float mean, var;
    gn_merge_slots(partial, n, g, G, nchunk, HW, cpg, tid & 7, mean, var);
    if (tid & 7) continue;
    const float rstd = rsqrtf(var + eps);
    st[g * 2] = mean;
    st[g * 2 + 1] = rstd;
    mean_rstd[((int64_t)n * G + g) * 2] = mean;
    mean_rstd[((int64_t)n * G + g) * 2 + 1] = rstd;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int g = c / cpg;
    const float a = st[g * 2 + 1] * to_f(gamma[c]);
    aa[(int64_t)n * C + c] = a;
    bb[(int64_t)n * C + c] = to_f(beta[c]) - st[g * 2] * a;
  }
}
template <typename T, int MODE, bool SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                       const T* __restrict__ gamma, const T* __restrict__ beta,
                                                       const float* __restrict__ partial, float* __restrict__ aa,
                                                       float* __restrict__ bb, float* __restrict__ mean_rstd,
                                                       const T* add, T* out, int Nb,
                                                       int HW, int C, int G, int nchunk, float eps) {
  extern __shared__ float st[];
  gn_apply_body<T, MODE, SILU>(st, blockIdx.y, blockIdx.x, x, dy, gamma, beta, partial, aa, bb, mean_rstd, add, out, HW, C,
                               G, nchunk, eps);
}

// ---------------------------------------------------------------------------------------------------------
// GroupNorm forward in ONE launch for maps whose (sample, group) slice fits LDS (SD-1.x at batch 1-4, every pre-roll, the
// deeper levels of SD-XL): workgroup (g, n) reads its HW x (C / G) slice once in 4-byte pieces (two channels; the group
// width is even everywhere), keeps it in LDS, reduces the sum and then the squared deviations in a fixed order, applies the affine (+ SiLU)
// from LDS and writes.  The two-kernel form costs such maps two launches of 8-16 us that are pure latency (SD-1.4: 12 % of
// all kernel time is GroupNorm, ~7500 launches in a 22-step run).  Statistics, affine and mean / rstd are stored where
// the two-kernel form stores them (the backward reads them); the selection depends on (HW, C, G) only, so a sample's
// arithmetic does not depend on its batch.
// ---------------------------------------------------------------------------------------------------------
template <typename T, bool SILU>
__global__ __launch_bounds__(256) void gn_fused_fwd_kernel(const T* __restrict__ x, const T* __restrict__ gamma,
                                                           const T* __restrict__ beta, T* __restrict__ y,
                                                           float* __restrict__ aa, float* __restrict__ bb,
                                                           float* __restrict__ mean_rstd, int HW, int C, int G, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gn_smem[];
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G, dpr = cpg >> 1, total = HW * dpr;  // dpr: 4-byte pieces per row of the slice
  uint32_t* tile = reinterpret_cast<uint32_t*>(gn_smem);
  float* fl = reinterpret_cast<float*>(gn_smem + (((size_t)total * 4 + 15) & ~(size_t)15));
  float* red = fl;             // [2][4] per-wave partial sums: sum | sum of squared deviations
  float* af = fl + 8;          // [cpg]
  float* bf = af + cpg;        // [cpg]
  const T* xg = x + (int64_t)n * HW * C + (int64_t)g * cpg;
  T* yg = y + (int64_t)n * HW * C + (int64_t)g * cpg;
  const int drow = 256 / dpr, dd = 256 - drow * dpr;  // idx += 256  <=>  (row, d) += (drow, dd) with carry
  union W2 {
    uint32_t u;
    T e[2];
  };
  // the mean from the plain fp32 sum (16-bit values of one binade sum almost exactly: 0.3 of the statistics bar at
  // |mean| / std = 256), then sum (x - mean)^2 in a second pass over the LDS copy, which the error of the mean enters squared
  float s = 0.f, sq = 0.f;
  {
    int row = tid / dpr, d = tid - row * dpr;
    for (int idx = tid; idx < total; idx += 256) {
      W2 w;
      w.u = *reinterpret_cast<const uint32_t*>(xg + (int64_t)row * C + 2 * d);
      tile[idx] = w.u;
      s += to_f(w.e[0]) + to_f(w.e[1]);
      d += dd;
      row += drow;
      if (d >= dpr) {
        d -= dpr;
        ++row;
      }
    }
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float cnt = (float)HW * (float)cpg;
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / cnt;
  for (int idx = tid; idx < total; idx += 256) {  // the words this thread stored itself
    W2 w;
    w.u = tile[idx];
    const float d0 = to_f(w.e[0]) - mean, d1 = to_f(w.e[1]) - mean;
    sq += d0 * d0 + d1 * d1;
  }
  sq = wave_sum(sq);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = sq;
  __syncthreads();
  const float var = ((red[4] + red[5]) + (red[6] + red[7])) / cnt;
  const float rstd = rsqrtf(var + eps);
  if (tid == 0) {
    mean_rstd[((int64_t)n * G + g) * 2] = mean;
    mean_rstd[((int64_t)n * G + g) * 2 + 1] = rstd;
  }
  if (tid < cpg) {
    const int c = g * cpg + tid;
    const float a = rstd * to_f(gamma[c]);
    const float b = to_f(beta[c]) - mean * a;
    af[tid] = a;
    bf[tid] = b;
    aa[(int64_t)n * C + c] = a;  // the backward reads the affine back
    bb[(int64_t)n * C + c] = b;
  }
  __syncthreads();
  {
    int row = tid / dpr, d = tid - row * dpr;
    for (int idx = tid; idx < total; idx += 256) {
      W2 w, o;
      w.u = tile[idx];
      float z0 = to_f(w.e[0]) * af[2 * d] + bf[2 * d];
      float z1 = to_f(w.e[1]) * af[2 * d + 1] + bf[2 * d + 1];
      if (SILU) {
        z0 = silu_f(z0);
        z1 = silu_f(z1);
      }
      o.e[0] = from_f<T>(z0);
      o.e[1] = from_f<T>(z1);
      *reinterpret_cast<uint32_t*>(yg + (int64_t)row * C + 2 * d) = o.u;
      d += dd;
      row += drow;
      if (d >= dpr) {
        d -= dpr;
        ++row;
      }
    }
  }
}
// Selection override of the parity tests (set_gn_select): -1 = the environment variables, 0 = never the one-launch form,
// 1 = the one-launch form wherever its shape rules hold (the tuned limits SMI_GN_FUSED_HW / SMI_GN_FUSED_MAX lifted)
static int g_gn_sel = -1;
// what the last launch_groupnorm_* / launch_layernorm_* of this thread launched (gn_last_ran); host side only
static thread_local NormRan g_norm_ran;
static void ran_set(int form, int chunks, int slots, int nv, int r) {
  g_norm_ran.form = form;
  g_norm_ran.chunks = chunks;
  g_norm_ran.slots = slots;
  g_norm_ran.nv = nv;
  g_norm_ran.r = r;
}
static void ran_two_launch(int nchunk) {
  ran_set(nchunk > GN_MAX_SLOTS ? NORM_RAN_GN_FOLD : NORM_RAN_GN_TWO, nchunk, nchunk > GN_MAX_SLOTS ? GN_MAX_SLOTS : nchunk, 0, 0);
}

// largest (sample, group) slice the one-launch form takes, in bytes (SMI_GN_FUSED_MAX; 0 = never)
static size_t gn_fused_max() {
  static const size_t v = []() {
    const char* e = getenv("SMI_GN_FUSED_MAX");
    return e ? (size_t)atoll(e) : (size_t)98304;
  }();
  return v;
}
// Measured (tools/bench_norm.py, SMI_GN_FUSED_MAX = 0 | 98304): the one-launch form wins where the map is a handful of rows
// -- 2 x 256 x 1280: 16.0 -> 8.5 us, 2 x 256 x 2560: 27.9 -> 13.7, 2 x 64 x 1280: 15.7 -> 4.8, 8 x 64 x 2560: 27.6 -> 5.7 -- and
// loses from 1024 rows on (2 x 1024 x 1280: 18 -> 34 us, 2 x 4096 x 320: 17 -> 42: one workgroup then streams 80 KB in 4-byte
// pieces): taken for maps of at most 256 pixels (the 16 x 16 and 8 x 8 levels of SD-1.x, the deepest level of small SD-XL
// latents).  (Since the variance became a second, centred pass over the LDS copy the one-launch figures are 9.4, 15.9, 4.8
// and 6.4 us.)
static bool gn_fused_ok(int HW, int C, int G) {
  static const int max_hw = []() { const char* e = getenv("SMI_GN_FUSED_HW"); return e ? atoi(e) : 256; }();
  const int cpg = C / G;
  const size_t slice = (size_t)HW * cpg * 2;
  if (g_gn_sel == 0) return false;
  const bool tuned = g_gn_sel == 1 || (HW <= max_hw && slice <= gn_fused_max());
  return tuned && (cpg & 1) == 0 && cpg >= 2 && cpg <= 256 && slice + 16 + (8 + 2 * cpg) * 4 <= 160 * 1024;
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm: a wave owns R consecutive rows (C <= 8*64*LN_MAXV); NV = vectors of 8 elements per lane is a template
// parameter, so a 1280-wide row is 3 loads per lane with no dead registers; the loads of all R rows are issued up front
// and their reductions interleave.  The wave reduction runs on DPP within 16-lane rows (quad swaps, half mirror, mirror)
// and four v_readlane across them instead of six LDS-crossbar shuffles.
// ---------------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 4;  // C <= 2048

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// the same sum in every lane; fixed order
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror: every lane of a 16-lane row holds the row's sum
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

template <typename T, int MODE, int NV, int R>  // MODE 0 fwd, 1 bwd
__global__ __launch_bounds__(256) void ln_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                 const T* __restrict__ gamma, const T* beta, T* out,
                                                 float* __restrict__ mean_rstd, int M, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= M) return;
  const int nvec = C / 8;
  const float inv_c = 1.f / (float)C;
  float xv[R][NV][8];
  Pack8<T> dv[MODE == 1 ? R : 1][NV];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = min(row0 + r, M - 1);  // a tail row re-reads the last row; its stores are masked below
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      Pack8<T> t;
      if (v < nvec) {
        t.u = *reinterpret_cast<const u32x4*>(x + (int64_t)row * C + v * 8);
        if (MODE == 1) dv[r][j].u = *reinterpret_cast<const u32x4*>(dy + (int64_t)row * C + v * 8);
      } else {
        t.u = u32x4{0u, 0u, 0u, 0u};
        if (MODE == 1) dv[r][j].u = u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[r][j][e] = to_f(t.e[e]);
    }
  }
  if (MODE == 0) {
    float mean[R], rstd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += xv[r][j][e];
      mean[r] = s;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mean[r] = wave_sum_dpp(mean[r]) * inv_c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (lane + 64 * j < nvec) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = xv[r][j][e] - mean[r];
            sq += d * d;
          }
        }
      }
      rstd[r] = sq;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rstd[r] = rsqrtf(wave_sum_dpp(rstd[r]) * inv_c + eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
        Pack8<T> g8, b8;
        g8.u = *reinterpret_cast<const u32x4*>(gamma + v * 8);
        b8.u = *reinterpret_cast<const u32x4*>(beta + v * 8);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (row0 + r < M) {
            Pack8<T> o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              o.e[e] = from_f<T>((xv[r][j][e] - mean[r]) * rstd[r] * to_f(g8.e[e]) + to_f(b8.e[e]));
            *reinterpret_cast<u32x4*>(out + (int64_t)(row0 + r) * C + v * 8) = o.u;
          }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (row0 + r < M) {
          mean_rstd[(int64_t)(row0 + r) * 2] = mean[r];
          mean_rstd[(int64_t)(row0 + r) * 2 + 1] = rstd[r];
        }
    }
  } else {
    float dg[R][NV][8];
    float s1[R], s2[R], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = min(row0 + r, M - 1);
      const float mean = mean_rstd[(int64_t)row * 2];
      rs[r] = mean_rstd[(int64_t)row * 2 + 1];
      s1[r] = s2[r] = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int v = lane + 64 * j;
        if (v < nvec) {
          Pack8<T> g8;
          g8.u = *reinterpret_cast<const u32x4*>(gamma + v * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            xv[r][j][e] = (xv[r][j][e] - mean) * rs[r];  // xhat
            dg[r][j][e] = to_f(dv[r][j].e[e]) * to_f(g8.e[e]);
            s1[r] += dg[r][j][e];
            s2[r] += dg[r][j][e] * xv[r][j][e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) dg[r][j][e] = 0.f;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s1[r] = wave_sum_dpp(s1[r]) * inv_c;
      s2[r] = wave_sum_dpp(s2[r]) * inv_c;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r >= M) continue;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int v = lane + 64 * j;
        if (v < nvec) {
          Pack8<T> o, ad;
          if (beta) ad.u = *reinterpret_cast<const u32x4*>(beta + (int64_t)(row0 + r) * C + v * 8);  // bwd: beta = `add`
#pragma unroll
          for (int e = 0; e < 8; ++e)
            o.e[e] = from_f<T>(rs[r] * (dg[r][j][e] - s1[r] - xv[r][j][e] * s2[r]) + (beta ? to_f(ad.e[e]) : 0.f));
          *reinterpret_cast<u32x4*>(out + (int64_t)(row0 + r) * C + v * 8) = o.u;
        }
      }
    }
  }
}

// rows per wave: 2 once there are enough rows to fill the chip twice over (16 waves per SIMD), else 1
template <typename T, int MODE>
int ln_launch(const T* x, const T* dy, const T* gamma, const T* beta, T* out, float* mean_rstd, int M, int C, float eps,
              hipStream_t stream) {
  const int nv = (C / 8 + 63) / 64;
  static const int force_r = []() { const char* e = getenv("SMI_LN_ROWS"); return e ? atoi(e) : 0; }();
  const int R = force_r ? force_r : (MODE == 0 && M >= 16384 ? 2 : 1);
  ran_set(NORM_RAN_LN, 0, 0, nv > LN_MAXV ? LN_MAXV : nv, R == 2 ? 2 : 1);
#define LN_GO(NV_, R_)                                                                                              \
  hipLaunchKernelGGL((ln_kernel<T, MODE, NV_, R_>), dim3(cdiv(M, 4 * R_)), dim3(256), 0, stream, x, dy, gamma, beta, \
                     out, mean_rstd, M, C, eps)
  if (R == 2) {
    switch (nv) {
      case 1: LN_GO(1, 2); break;
      case 2: LN_GO(2, 2); break;
      case 3: LN_GO(3, 2); break;
      default: LN_GO(4, 2); break;
    }
  } else {
    switch (nv) {
      case 1: LN_GO(1, 1); break;
      case 2: LN_GO(2, 1); break;
      case 3: LN_GO(3, 1); break;
      default: LN_GO(4, 1); break;
    }
  }
#undef LN_GO
  SMI_HIP(hipGetLastError());
  return 0;
}

inline int ew_grid(int64_t n_threads) {
  int64_t g = (n_threads + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// more than GN_MAX_SLOTS chunks per sample: fold them into the slots behind the raw partials; returns what to re-reduce
// (stats: the forward's (mean, M2) partials, merged; otherwise the backward's sums)
inline const float* gn_fold(float* partial, int Nb, int nchunk, int G, bool stats, int HW, int cpg, hipStream_t st) {
  if (nchunk <= GN_MAX_SLOTS) return partial;
  float* folded = partial + (size_t)Nb * nchunk * G * 2;
  if (stats)
    hipLaunchKernelGGL(gn_fold_kernel<true>, dim3(GN_MAX_SLOTS, Nb), dim3(256), 0, st, partial, folded, nchunk, G * 2, HW, cpg);
  else
    hipLaunchKernelGGL(gn_fold_kernel<false>, dim3(GN_MAX_SLOTS, Nb), dim3(256), 0, st, partial, folded, nchunk, G * 2, HW, cpg);
  return folded;
}

template <typename T>
int gn_fwd_t(const void* x, const void* gamma, const void* beta, void* y, float* ab, float* mean_rstd, float* partial,
             int Nb, int HW, int C, int G, float eps, int silu, hipStream_t st) {
  if (gn_fused_ok(HW, C, G)) {
    const int cpg = C / G;
    const size_t smf = (((size_t)HW * (cpg >> 1) * 4 + 15) & ~(size_t)15) + (8 + 2 * cpg) * sizeof(float);
    if (silu) {
      if (smf > 65536) {
        static DynLdsOnce once;
        if (int rc = once.set((const void*)gn_fused_fwd_kernel<T, true>, (int)(160 * 1024))) return rc;
      }
      hipLaunchKernelGGL((gn_fused_fwd_kernel<T, true>), dim3(G, Nb), dim3(256), smf, st, (const T*)x, (const T*)gamma,
                         (const T*)beta, (T*)y, ab, ab + (size_t)Nb * C, mean_rstd, HW, C, G, eps);
    } else {
      if (smf > 65536) {
        static DynLdsOnce once;
        if (int rc = once.set((const void*)gn_fused_fwd_kernel<T, false>, (int)(160 * 1024))) return rc;
      }
      hipLaunchKernelGGL((gn_fused_fwd_kernel<T, false>), dim3(G, Nb), dim3(256), smf, st, (const T*)x, (const T*)gamma,
                         (const T*)beta, (T*)y, ab, ab + (size_t)Nb * C, mean_rstd, HW, C, G, eps);
    }
    SMI_HIP(hipGetLastError());
    ran_set(NORM_RAN_GN_ONE, 0, 0, 0, 0);
    return 0;
  }
  const int nchunk = gn_num_chunks(HW);
  ran_two_launch(nchunk);
  const GnGeom gg = gn_geom(C);
  const size_t sm = (size_t)gg.rpar * C * 2 * sizeof(float);
  const size_t sa = (size_t)G * 2 * sizeof(float);
  hipLaunchKernelGGL((gn_partial_kernel<T, 0, false>), dim3(nchunk, Nb), dim3(256), sm, st, (const T*)x, nullptr,
                     nullptr, nullptr, ab, ab, partial, Nb, HW, C, G, nchunk);
  const float* red = gn_fold(partial, Nb, nchunk, G, true, HW, C / G, st);
  const int nslot = nchunk > GN_MAX_SLOTS ? GN_MAX_SLOTS : nchunk;
  if (silu)
    hipLaunchKernelGGL((gn_apply_kernel<T, 0, true>), dim3(nchunk, Nb), dim3(256), sa, st, (const T*)x, nullptr,
                       (const T*)gamma, (const T*)beta, red, ab, ab + (size_t)Nb * C, mean_rstd, nullptr, (T*)y, Nb, HW, C, G, nslot, eps);
  else
    hipLaunchKernelGGL((gn_apply_kernel<T, 0, false>), dim3(nchunk, Nb), dim3(256), sa, st, (const T*)x, nullptr,
                       (const T*)gamma, (const T*)beta, red, ab, ab + (size_t)Nb * C, mean_rstd, nullptr, (T*)y, Nb, HW, C, G, nslot, eps);
  SMI_HIP(hipGetLastError());
  return 0;
}

// aa / bb: the forward's per-(n,c) affine of the Nb samples being differentiated ([Nb][C] each)
template <typename T>
int gn_bwd_t(const void* x, const void* dy, const void* gamma, const void* beta, const float* aa, const float* bb,
             const float* mean_rstd, const void* add, void* dx, float* partial, int Nb, int HW, int C, int G, int silu,
             hipStream_t st) {
  const int nchunk = gn_num_chunks(HW);
  ran_two_launch(nchunk);
  const GnGeom gg = gn_geom(C);
  const size_t sm = (size_t)gg.rpar * C * 2 * sizeof(float);
  if (silu)
    hipLaunchKernelGGL((gn_partial_kernel<T, 1, true>), dim3(nchunk, Nb), dim3(256), sm, st, (const T*)x,
                       (const T*)dy, (const T*)gamma, (const T*)beta, aa, bb, partial, Nb, HW, C, G, nchunk);
  else
    hipLaunchKernelGGL((gn_partial_kernel<T, 1, false>), dim3(nchunk, Nb), dim3(256), sm, st, (const T*)x,
                       (const T*)dy, (const T*)gamma, (const T*)beta, aa, bb, partial, Nb, HW, C, G, nchunk);
  const size_t sa = (size_t)G * 2 * sizeof(float);
  float* abp = const_cast<float*>(aa);
  float* bbp = const_cast<float*>(bb);
  float* mrp = const_cast<float*>(mean_rstd);
  const float* red = gn_fold(partial, Nb, nchunk, G, false, HW, C / G, st);
  const int nslot = nchunk > GN_MAX_SLOTS ? GN_MAX_SLOTS : nchunk;
  if (silu)
    hipLaunchKernelGGL((gn_apply_kernel<T, 1, true>), dim3(nchunk, Nb), dim3(256), sa, st, (const T*)x, (const T*)dy,
                       (const T*)gamma, (const T*)beta, red, abp, bbp, mrp, (const T*)add, (T*)dx, Nb, HW, C, G, nslot, 0.f);
  else
    hipLaunchKernelGGL((gn_apply_kernel<T, 1, false>), dim3(nchunk, Nb), dim3(256), sa, st, (const T*)x, (const T*)dy,
                       (const T*)gamma, (const T*)beta, red, abp, bbp, mrp, (const T*)add, (T*)dx, Nb, HW, C, G, nslot, 0.f);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace

void set_gn_select(int fused) { g_gn_sel = fused; }
NormRan gn_last_ran() { return g_norm_ran; }

int gn_num_chunks(int HW) { return (HW + gn_rows_per_chunk(HW) - 1) / gn_rows_per_chunk(HW); }
size_t gn_partial_floats(int Nb, int HW, int G) {
  const int nchunk = gn_num_chunks(HW);
  return (size_t)Nb * (nchunk + (nchunk > GN_MAX_SLOTS ? GN_MAX_SLOTS : 0)) * G * 2;
}

int launch_groupnorm_fwd(int dtype, const void* x, const void* gamma, const void* beta, void* y, float* ab,
                         float* mean_rstd, float* partial, int Nb, int HW, int C, int G, float eps, int silu,
                         hipStream_t stream) {
  g_norm_ran = NormRan();
  SMI_CHECK(C % 8 == 0 && C % G == 0, "groupnorm: C=%d must be a multiple of 8 and of G=%d", C, G);
  SMI_CHECK((size_t)gn_geom(C).rpar * C * 8 <= 65536, "groupnorm: C=%d too large for the LDS reduction (C <= 8192)", C);
  return dtype == DT_F16 ? gn_fwd_t<f16>(x, gamma, beta, y, ab, mean_rstd, partial, Nb, HW, C, G, eps, silu, stream)
                         : gn_fwd_t<bf16>(x, gamma, beta, y, ab, mean_rstd, partial, Nb, HW, C, G, eps, silu, stream);
}

int launch_groupnorm_stats(int dtype, const void* x, const void* gamma, const void* beta, float* ab, float* mean_rstd,
                           float* partial, int Nb, int HW, int C, int G, float eps, hipStream_t stream) {
  g_norm_ran = NormRan();
  SMI_CHECK(C % 8 == 0 && C % G == 0, "groupnorm stats: C=%d must be a multiple of 8 and of G=%d", C, G);
  SMI_CHECK((size_t)gn_geom(C).rpar * C * 8 <= 65536, "groupnorm stats: C=%d too large for the LDS reduction (C <= 8192)", C);
  const int nchunk = gn_num_chunks(HW);
  ran_two_launch(nchunk);
  const size_t sm = (size_t)gn_geom(C).rpar * C * 2 * sizeof(float);
  const size_t sa = (size_t)G * 2 * sizeof(float);
  const int nslot = nchunk > GN_MAX_SLOTS ? GN_MAX_SLOTS : nchunk;
  if (dtype == DT_F16) {
    hipLaunchKernelGGL((gn_partial_kernel<f16, 0, false>), dim3(nchunk, Nb), dim3(256), sm, stream, (const f16*)x, nullptr,
                       nullptr, nullptr, ab, ab, partial, Nb, HW, C, G, nchunk);
    const float* red = gn_fold(partial, Nb, nchunk, G, true, HW, C / G, stream);
    hipLaunchKernelGGL(gn_stats_kernel<f16>, dim3(Nb), dim3(256), sa, stream, (const f16*)gamma, (const f16*)beta, red, ab,
                       ab + (size_t)Nb * C, mean_rstd, HW, C, G, nslot, eps);
  } else {
    hipLaunchKernelGGL((gn_partial_kernel<bf16, 0, false>), dim3(nchunk, Nb), dim3(256), sm, stream, (const bf16*)x,
                       nullptr, nullptr, nullptr, ab, ab, partial, Nb, HW, C, G, nchunk);
    const float* red = gn_fold(partial, Nb, nchunk, G, true, HW, C / G, stream);
    hipLaunchKernelGGL(gn_stats_kernel<bf16>, dim3(Nb), dim3(256), sa, stream, (const bf16*)gamma, (const bf16*)beta, red,
                       ab, ab + (size_t)Nb * C, mean_rstd, HW, C, G, nslot, eps);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}

// `partial` must hold Nb*nchunk*G*2 floats.  `a`, `b`: the forward's affine of these Nb samples ([Nb][C] each).
int launch_groupnorm_bwd(int dtype, const void* x, const void* dy, const void* gamma, const void* beta,
                         const float* a, const float* b, const float* mean_rstd, const void* add, void* dx,
                         float* partial, int Nb, int HW, int C, int G, int silu, hipStream_t stream) {
  g_norm_ran = NormRan();
  SMI_CHECK(C % 8 == 0 && C % G == 0, "groupnorm bwd: C=%d must be a multiple of 8 and of G=%d", C, G);
  SMI_CHECK((size_t)gn_geom(C).rpar * C * 8 <= 65536, "groupnorm bwd: C=%d too large for the LDS reduction (C <= 8192)", C);
  return dtype == DT_F16
             ? gn_bwd_t<f16>(x, dy, gamma, beta, a, b, mean_rstd, add, dx, partial, Nb, HW, C, G, silu, stream)
             : gn_bwd_t<bf16>(x, dy, gamma, beta, a, b, mean_rstd, add, dx, partial, Nb, HW, C, G, silu, stream);
}

int launch_layernorm_fwd(int dtype, const void* x, const void* gamma, const void* beta, void* y, float* mean_rstd,
                         int M, int C, float eps, hipStream_t stream) {
  g_norm_ran = NormRan();
  SMI_CHECK(C % 8 == 0 && C <= 8 * 64 * LN_MAXV, "layernorm: C=%d must be a multiple of 8 and at most %d", C, 8 * 64 * LN_MAXV);
  if (dtype == DT_F16)
    return ln_launch<f16, 0>((const f16*)x, nullptr, (const f16*)gamma, (const f16*)beta, (f16*)y, mean_rstd, M, C, eps,
                             stream);
  return ln_launch<bf16, 0>((const bf16*)x, nullptr, (const bf16*)gamma, (const bf16*)beta, (bf16*)y, mean_rstd, M, C,
                            eps, stream);
}

int launch_layernorm_bwd(int dtype, const void* x, const void* dy, const void* gamma, const float* mean_rstd,
                         const void* add, void* dx, int M, int C, hipStream_t stream) {
  g_norm_ran = NormRan();
  SMI_CHECK(C % 8 == 0 && C <= 8 * 64 * LN_MAXV, "layernorm: C=%d must be a multiple of 8 and at most %d", C, 8 * 64 * LN_MAXV);
  if (dtype == DT_F16)
    return ln_launch<f16, 1>((const f16*)x, (const f16*)dy, (const f16*)gamma, (const f16*)add, (f16*)dx,
                             const_cast<float*>(mean_rstd), M, C, 0.f, stream);
  return ln_launch<bf16, 1>((const bf16*)x, (const bf16*)dy, (const bf16*)gamma, (const bf16*)add, (bf16*)dx,
                            const_cast<float*>(mean_rstd), M, C, 0.f, stream);
}

}  // namespace smi
