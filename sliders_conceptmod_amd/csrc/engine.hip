// What the op core (engine.h) keeps out of line: the weight-packing kernels with their two launchers, the saved pass and
// backward scaffold of the differentiated models, and the create / plan path that the forward-only engines share.
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
__global__ void set_floats_kernel(float* dst0, float* dst1, F64Args a, int n) {
  const int i = threadIdx.x;
  if (i < n) {
    dst0[i] = a.v[i];
    if (dst1) dst1[i] = a.v[i];
  }
}
}  // namespace

// ---- the saved pass and its backward: what every differentiated model shares ------------------------------------------
#undef SMI_ENG
#define SMI_ENG (*this)
int smi_engine::upload_floats(float* dst0, float* dst1, const float* host, int n, float divisor) {
  for (int i0 = 0; i0 < n; i0 += 64) {
    F64Args a;
    const int cnt = n - i0 < 64 ? n - i0 : 64;
    for (int i = 0; i < 64; ++i) a.v[i] = i < cnt ? host[i0 + i] / divisor : 0.f;
    hipLaunchKernelGGL(set_floats_kernel, dim3(1), dim3(64), 0, stream, dst0 + i0, dst1 ? dst1 + i0 : (float*)nullptr, a, cnt);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}
int smi_engine::set_sample_multipliers(const float* multipliers, int n, bool save, float* mref) {
  float m = 0.f;
  for (int i = 0; i < n; ++i) m = fmaxf(m, fabsf(multipliers[i]));
  *mref = m;
  return m != 0.f ? upload_floats(samp_mult_dev, save ? samp_mult_dev + MAXS : nullptr, multipliers, n, m) : 0;
}

void smi_engine::register_sites(const smi_lora_site* s, int n_sites) {
  sites.assign(s, s + n_sites);
  site_names.resize(n_sites);
  site_used.assign(n_sites, 0);
  for (int i = 0; i < n_sites; ++i) {
    site_names[i] = s[i].target;
    sites[i].target = site_names[i].c_str();
  }
  for (int i = 0; i < n_sites; ++i) smap[site_names[i]] = &sites[i];
}
int check_linear_lora_sites(const char* who, const smi_lora_site* sites, int n_sites, std::initializer_list<const char*> suffixes,
                            const char* where) {
  for (int i = 0; i < n_sites; ++i) {
    const std::string t = sites[i].target ? sites[i].target : "";
    SMI_CHECK(sites[i].off_dora < 0, "%s: DoRA site '%s' -- plain LoRA sites only", who, t.c_str());
    SMI_CHECK(sites[i].rank >= 1 && sites[i].rank <= 16, "%s: rank %d of '%s' outside [1, 16]", who, sites[i].rank, t.c_str());
    bool ok = false;
    for (const char* suf : suffixes) {
      const size_t m = strlen(suf);
      ok = ok || (t.size() > m && t.compare(t.size() - m, m, suf) == 0);
    }
    SMI_CHECK(ok, "%s: target '%s' -- sites sit on %s", who, t.c_str(), where);
  }
  return 0;
}

int smi_engine::begin_backward(const char* no_pass, float* dd, float* du, int n_live) {
  if (!saved.valid && !dry) {
    set_error("%s", no_pass);
    return -4;
  }
  cur = &arena[1];
  tens = &tens_[1];
  in_block = persist_next = false;
  saving = false;
  d_down = dd;
  d_up = du;
  n_ad = n_live;  // rows per sample of a gradient buffer = its rows / n_ad
  wjobs.clear();
  pinned.clear();
  bw_skip = saved.n - n_live;
  return 0;
}
void smi_engine::rebuild_saved_operands() {
  if (!prep_sites.empty() && bw_down && bw_up && bw_mult != 0.f)
    RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(dtype, prep_sites_dev, (int)prep_sites.size(), bw_down, bw_up, lora_shadow, stream));
  mult = bw_mult;
}
int smi_engine::run_tape_and_weight_grads() {
  for (auto it = tape.rbegin(); it != tape.rend(); ++it) (*it)();
  int rc = 0;
  if (!wjobs.empty() && !err) {
    wgrad_grouped_finish(wjobs);
    if (!dry) {
      const bool same = saved.uploaded.size() == wjobs.size() &&
                        memcmp(saved.uploaded.data(), wjobs.data(), wjobs.size() * sizeof(WgradJob)) == 0;
      if (wjobs.size() > saved.cap) {
        set_error("internal: %zu weight-gradient jobs exceed the table (%zu)", wjobs.size(), saved.cap);
        rc = -1;
      } else if (!same) {
        saved.uploaded = wjobs;
        if (hipMemcpyAsync(saved.dev, saved.uploaded.data(), wjobs.size() * sizeof(WgradJob), hipMemcpyHostToDevice, stream) !=
            hipSuccess) {
          set_error("hipMemcpyAsync (weight-gradient job table) failed");
          saved.uploaded.clear();  // (the device table holds nothing that a later backward may take for its own)
          rc = -1;
        }
      }
      if (rc == 0) {
        double bytes = 0.0, flops = 0.0;
        for (const auto& j : wjobs) {
          bytes += (double)(j.M - j.m_begin) * j.K * 2.0;
          flops += 2.0 * (j.M - j.m_begin) * j.K * j.r;
        }
        RUNP(SMI_PROF_LORA, flops, bytes, launch_lora_wgrad_grouped(dtype, wjobs, saved.dev, stream));
      }
    }
  }
  drop_tape();
  return rc;
}
#undef SMI_ENG
#define SMI_ENG e

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
// scratch: one of the two regions a model's blocks alternate between (smi_engine::begin_block); 0 for a model without blocks
struct ForwardOnlyPlan {
  size_t wpack = 0, arena = 0, scratch = 0;
  size_t bytes() const { return wpack + arena + 2 * scratch + 2 * 4096; }
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
  p->scratch = align_up(std::max(e.scr[0].peak, e.scr[1].peak), 4096);
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
  if (p.scratch) e->set_arena0_regions(p.arena, p.scratch);
  build_model(*e);
  return finish_create(e, what, out);
}

extern "C" void smi_destroy(smi_engine* e) { delete e; }  // (NULL is fine)
