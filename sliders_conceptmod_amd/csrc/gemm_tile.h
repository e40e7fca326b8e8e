// Tile plumbing shared by the GEMM kernels (gemm.hip, gemm2.hip, gemm3.hip, gemm4.hip): LDS-DMA, the scheduling fence,
// the zero page, and the workgroup -> tile maps.  Device code only.
#pragma once
#include "smi_common.h"

namespace smi {

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// LDS-DMA (`global_load_lds_dwordx4`): 16 bytes per lane from a per-lane global address to the wave's lane-linear 1 KiB
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((gbl_void*)gsrc, (lds_void*)lds_dst, 16, 0, 0);
}

#define SMI_FENCE() __builtin_amdgcn_sched_barrier(0)

namespace {
// Source of an LDS-DMA whose row does not exist (M / N tails, conv padding): LDS-DMA has a per-lane address but no
// per-lane predicate.  Zero-initialised.  The library is built without relocatable device code, so every translation unit
// that stages through LDS-DMA gets its own copy of this one definition.
[[maybe_unused]] __device__ __attribute__((aligned(256))) unsigned char g_zero_page[256];
}  // namespace

// XCD-aware bijective remap of a linear workgroup (or virtual tile) id: ids that share an XCD (id % 8) get a contiguous
// range of tiles, so neighbouring tiles (same A rows / same W rows) hit the same L2.
__device__ __forceinline__ int xcd_remap(int id, int n) {
  const int q = n >> 3, r = n & 7, xcd = id & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// Grouped rasterisation: consecutive workgroups (= the ones co-resident on one XCD after xcd_remap) sweep a band of GW
// column tiles before moving down a row tile, so the 32-64 tiles sharing an L2 form a ~8x8 patch (8 + 8 operand panels
// per K-step instead of 1 + 64 for a wide-N GEMM walked row-major).  Returns the tile's (row, column) index.
__device__ __forceinline__ void grouped_raster(int wg, int nbm, int nbn, int GW, int& tm, int& tn) {
  const int grp = wg / (GW * nbm);
  const int gw = min(nbn - grp * GW, GW);
  const int lw = wg - grp * GW * nbm;
  tm = lw / gw;
  tn = grp * GW + lw % gw;
}
// band width that splits nbn column tiles into equal bands of at most 8
__device__ __forceinline__ int raster_band(int nbn) {
  const int ngrp = (nbn + 7) / 8;
  return (nbn + ngrp - 1) / ngrp;
}

}  // namespace smi
