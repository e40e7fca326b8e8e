// What the op core (engine.h) keeps out of line: the weight-packing kernels with their two launchers, and the create /
// plan path that the forward-only engines share.
#include "engine.h"

namespace {
// ------------------------------------------------------------------------------------------------------------
// weight packing kernels (run once at creation)
// ------------------------------------------------------------------------------------------------------------
// dst[c][col0 + r] = src[r][c] through a 64x64 LDS tile: coalesced reads and writes
template <typename T>
__global__ __launch_bounds__(256) void pack_transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, int R,
                                                             int C, int ldd, int col0) {
  __shared__ T tile[64][66];
  const int tilesC = (C + 63) / 64;
  const int tr = (blockIdx.x / tilesC) * 64, tc = (blockIdx.x % tilesC) * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = tr + i, c = tc + tx;
    if (r < R && c < C) tile[i][tx] = src[(int64_t)r * C + c];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = tc + i, r = tr + tx;
    if (r < R && c < C) dst[(int64_t)c * ldd + col0 + r] = tile[tx][i];
  }
}
// conv weight [Cout, Cin, 3, 3] -> forward pack  dst[co][(ky*3+kx)*Cin + ci]
//                               -> gradient pack dst[ci][(ty*3+tx)*Cout + co] = w[co][ci][ky][kx],
//                                  (ty,tx) = flip ? (2-ky, 2-kx) : (ky, kx)
template <typename T>
__global__ void pack_conv_kernel(const T* __restrict__ src, T* __restrict__ dst, int Cout, int Cin, int mode,
                                 int pad) {  // pad: padded inner channel count (Cin for mode 0, Cout otherwise)
  const int64_t total = (int64_t)Cout * Cin * 9;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % 9);
    const int ci = (int)((i / 9) % Cin);
    const int co = (int)(i / (9 * (int64_t)Cin));
    const int ky = t / 3, kx = t % 3;
    if (mode == 0) {
      dst[((int64_t)co * 9 + t) * pad + ci] = src[i];
    } else {
      const int tt = mode == 2 ? (2 - ky) * 3 + (2 - kx) : t;
      dst[((int64_t)ci * 9 + tt) * pad + co] = src[i];
    }
  }
}
// conv weight [Cout, Cin, 3, 3] of a nearest-2x up-sampler -> phase pack dst[2 a + b][co][(2 p + q) * Cin + ci]: on the 2x
// grid, output row 2 i + a sees low-res row i - 1 + a + p through the 3x3 rows {0} | {1, 2} (a = 0) or {0, 1} | {2} (a = 1)
// for p = 0 | 1; columns alike.  The up to four weights are summed in fp32 and rounded once.
template <typename T>
__global__ void pack_conv_phase_kernel(const T* __restrict__ src, T* __restrict__ dst, int Cout, int Cin) {
  const int64_t total = (int64_t)16 * Cout * Cin;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const int tap = (int)((i / Cin) % 4);
    const int co = (int)((i / (4 * (int64_t)Cin)) % Cout);
    const int ph = (int)(i / (4 * (int64_t)Cin * Cout));
    const int a = ph >> 1, b = ph & 1, p = tap >> 1, q = tap & 1;
    const int ky0 = p == 0 ? 0 : 1 + a, ky1 = p == 0 ? a : 2;
    const int kx0 = q == 0 ? 0 : 1 + b, kx1 = q == 0 ? b : 2;
    const T* w = src + ((int64_t)co * Cin + ci) * 9;
    float s = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) s += to_f(w[ky * 3 + kx]);
    dst[i] = from_f<T>(s);
  }
}
}  // namespace

int smi::launch_pack_conv_phase(int dtype, const void* src, void* dst, int Cout, int Cin, hipStream_t stream) {
  const int64_t total = (int64_t)16 * Cout * Cin;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(pack_conv_phase_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, (f16*)dst, Cout, Cin);
  else
    hipLaunchKernelGGL(pack_conv_phase_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, Cout, Cin);
  SMI_HIP(hipGetLastError());
  return 0;
}
void smi_engine::pack_conv_phase_into(const void* src, void* dst, int Cout, int Cin) {
  if (dry || err || !src) return;
  ++pack_launches;
  if (launch_pack_conv_phase(dtype, src, dst, Cout, Cin, stream) != 0) err = true;
}

void smi_engine::transpose_into(const void* src, void* dst, int R, int C, int ldd, int col0, bool packing) {
  if (dry || err || !src) return;
  const int grid = ((R + 63) / 64) * ((C + 63) / 64);
  if (packing) ++pack_launches;
  if (dtype == DT_F16)
    hipLaunchKernelGGL(pack_transpose_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, (f16*)dst, R, C, ldd, col0);
  else
    hipLaunchKernelGGL(pack_transpose_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, R, C, ldd, col0);
}
void smi_engine::pack_conv_into(const void* src, void* dst, int Cout, int Cin, int mode, int pad) {
  if (dry || err || !src) return;
  if (pad == 0) pad = mode == 0 ? Cin : Cout;
  else (void)hipMemsetAsync(dst, 0, (size_t)(mode == 0 ? Cout : Cin) * 9 * pad * esz(), stream);
  const int64_t total = (int64_t)Cout * Cin * 9;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
  ++pack_launches;
  if (dtype == DT_F16)
    hipLaunchKernelGGL(pack_conv_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, (f16*)dst, Cout, Cin, mode, pad);
  else
    hipLaunchKernelGGL(pack_conv_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, Cout, Cin, mode, pad);
}

int finish_create(smi_engine* e, const char* what, smi_engine** out) {
  if (!e->err) (void)hipStreamSynchronize(e->stream);
  if (e->err || hipGetLastError() != hipSuccess) {
    if (!e->err) set_error("HIP error while packing %s", what);
    delete e;
    return -1;
  }
  e->wmap.clear();
  *out = e;
  return 0;
}

// ---- the forward-only engines: one plan, one size, one create ---------------------------------------------------------
struct ForwardOnlyPlan {
  size_t wpack = 0, arena = 0;
  size_t bytes() const { return wpack + arena + 2 * 4096; }
};
static void build_model(smi_engine& e) {  // the model's layers, then what every forward-only engine packs after them
  e.model->build(e);
  e.gscale = (float*)e.pack_alloc(256 * sizeof(float));
  e.finish_lora();
}
static int plan_forward_only(const Setup& setup, ForwardOnlyPlan* p) {
  smi_engine e;
  e.dry = true;
  setup(&e);
  build_model(e);
  if (e.err) return -1;
  p->wpack = align_up(e.wpack.peak, 4096);
  e.model->dry_forward(e);
  p->arena = align_up(e.arena[0].peak, 4096);
  return e.err ? -1 : 0;
}
int workspace_bytes_forward_only(const Setup& setup, size_t* bytes) {
  SMI_CHECK(bytes != nullptr, "bad arguments");
  ForwardOnlyPlan p;
  if (plan_forward_only(setup, &p)) return -1;
  *bytes = p.bytes();
  return 0;
}
int create_forward_only(const Setup& setup, const char* what, const smi_weight* weights, int n_weights, void* workspace,
                        size_t workspace_bytes, void* stream, smi_engine** out) {
  SMI_CHECK(out && workspace && weights && n_weights > 0, "bad arguments");
  ForwardOnlyPlan p;
  if (plan_forward_only(setup, &p)) return -1;
  SMI_CHECK(p.bytes() <= workspace_bytes, "workspace too small: need %zu bytes, got %zu", p.bytes(), workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  setup(e);
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = p.wpack;
  e->arena[0].base = base + p.wpack;
  e->arena[0].cap = p.arena;
  build_model(*e);
  return finish_create(e, what, out);
}

extern "C" void smi_destroy(smi_engine* e) { delete e; }  // (NULL is fine)
