// The op core of every engine: runs a model's forward -- and the activation/LoRA-gradient backward of the models that are
// differentiated (the UNet, the CLIP text tower with LoRA sites, the MMDiT), whose saved pass and backward scaffold is
// written once here -- as a stream of hand-written gfx950 kernels (gemm.hip, attention.hip, norm.hip, elementwise.hip, lora.hip).  It names no model: each
// (engine_unet.hip, engine_vae.hip, engine_clip.hip, engine_lpips.hip, engine_mmdit.hip, engine_flux.hip) is a `Model` with its
// config, layers and forward over these ops.
//
// Structure
//   * Activations are token-major [n*H*W, C] in the model dtype (fp16/bf16); accumulation is fp32 everywhere.
//   * Frozen weights are borrowed from the caller in torch layout ([out, in] is already the K-contiguous "NT" operand)
//     and complemented at creation by packed copies inside the workspace: transposed matrices for the dX GEMMs,
//     (ky,kx,ci)-ordered conv filters (+ flipped/transposed gradient filters), fused q|k|v and k|v projections.
//   * Memory: two bump arenas sized by a dry run of the same code (no reuse inside a pass -- 288 GB of HBM makes
//     that the simple and fast choice): arena 0 serves no-grad passes, arena 1 the pass that is differentiated and
//     its backward, so a frozen pass can never clobber saved activations.
//   * Autograd: every op pushes a closure on a tape when its output depends on an adapted layer; the backward pops
//     them in reverse.  Gradients exist only downstream of the first adapted layer; frozen weights get none.
//     Residual / skip fan-in is accumulated inside the producing kernel (GEMM `res` epilogue, norm `add` operand).
//   * 16-bit gradient range: d_eps is multiplied by a power-of-two loss scale chosen on the device from max|d_eps|;
//     the LoRA weight-gradient kernels divide it out (they accumulate in fp32).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>
#include <deque>

#include "../../include/smi.h"
#include "kernels.h"

namespace smi {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  bool overflow = false;
  void reset() { off = 0; }
  void* alloc(size_t bytes) {
    off = align_up(off, 256);
    void* p = base + off;
    off += bytes;
    if (off > peak) peak = off;
    if (off > cap) overflow = true;
    return p;
  }
};

// up to 64 floats handed over BY VALUE in the kernel arguments (copied into the kernarg segment at launch): host values
// reach the device without a host buffer that must outlive the call (smi_engine::upload_floats)
struct F64Args {
  float v[64];
};

struct Ten {
  void* p = nullptr;
  void* g = nullptr;
  int64_t rows = 0;
  int cols = 0;
  int n = 0, H = 0, W = 0;  // rows = n*H*W for image tensors
  // first row of the ADAPTED samples: a batched pass carries frozen samples first and the adapted (LoRA on,
  // differentiated) samples last; gradients `g` cover rows [arow0, rows) only
  int64_t arow0 = 0;
  // a tail backward (smi_unet_backward_tail) differentiates the last n_live adapted samples only: it moves arow0 up to their
  // first row in every tensor of the saved pass and notes the distance here, for the few buffers that hold the adapted rows
  // of the FORWARD only (xa)
  int64_t bskip = 0;
  bool ng = false;
  // phase-major output of an up-sampler conv: p holds four planes [n, H/2, W/2, cols], plane 2 a + b the pixels
  // (2 i + a, 2 j + b).  Only concat reads it (as its first part); g is in ordinary row order
  bool phase = false;
  bool f32g = false;  // the context of a pass that differentiates it: its gradient is summed in fp32 in the caller's buffer
  float gmul = 1.f;  // the stored gradient g is gmul x the (loss-scaled) gradient; a power of two, 1 but for row vectors
};

struct Lin {
  std::string name;
  const void* W = nullptr;   // [out, in]
  const void* Wt = nullptr;  // [in, out]
  const void* b = nullptr;
  int in = 0, out = 0;
  // LoRA (fused projections carry nseg adjacent sites)
  int nseg = 1;
  int nsite = 0;
  int rank = 0;
  float scale = 0.f;
  int64_t off_down = 0, off_up = 0;
  // 16-bit GEMM-operand copies of the LoRA matrices, refreshed once per adapted forward (lora.hip lora_prep_kernel)
  int rows_pad = 0;
  const void* sh_down = nullptr;  // [rows_pad, in]
  const void* sh_up = nullptr;    // [rows_pad, out] block-diagonal over the fused segments
  // DoRA (T/dora.py): the adapted rows get a second GEMM against dW = lscale * ((W + up down) g / ||.||_col - W)
  bool dora = false;
  int dora_idx = -1;  // into smi_engine::dora_sites
};
struct Conv {
  const void* Wp = nullptr;   // forward pack [Cout][9*Cin]
  const void* Wg = nullptr;   // gradient pack [Cin][9*Cout]
  const void* Wph = nullptr;  // mode 2 without an adaptor, where the model asks for it: phase pack [4][Cout][4*Cin]
  bool phase = false;         // ... and that it was packed (Wph itself may be offset 0 of a dry run)
  const void* b = nullptr;
  int Cin = 0, Cout = 0;
  int mode = 0;  // 0 stride 1, 1 stride-2 downsample, 2 nearest-2x upsample + conv
  int pad = 1;   // 0: the VAE encoder's downsampler (input padded (0,1,0,1), stride 2)
  // c3lier LoRA (T/lora.py:100-114): 3x3 down conv [r][Cin][3][3] with the layer's stride / padding, then 1x1 up [Cout][r]
  std::string name;
  int nsite = 0, rank = 0, rows_pad = 0;
  float scale = 0.f;
  int64_t off_down = 0, off_up = 0;
  const void* sh_down = nullptr;  // 16-bit [rows_pad][9*Cin], (ky,kx,ci)-ordered: filter of the xa conv
  const void* sh_up = nullptr;    // 16-bit [rows_pad][Cout] = up^T (dxa = dy * up)
  const void* sh_gw = nullptr;    // 16-bit [Cin][9*64]: gradient filter of the down conv, rank zero-padded to 64
};
struct Norm {
  const void* gamma = nullptr;
  const void* beta = nullptr;
  int C = 0;
  int groups = 0;  // GroupNorm; 0 for a LayerNorm
  float eps = 1e-5f;
};
struct Resnet {
  Norm n1, n2;
  Conv c1, c2;
  Lin temb, sc;  // temb: only where the model has a time embedding
  bool has_sc = false;
  int64_t temb_col = 0;  // column offset of this resnet's time_emb_proj inside the grouped projection
};

}  // namespace smi

using namespace smi;

// what an engine runs.  The two virtuals are called once per create or plan; the typed forwards are reached by the entry
// points after their kind check, by a static_cast.  A model lives on the heap behind smi_engine::model for the engine's
// lifetime: closures on the tape point at its layers, so nothing that holds layers may move or resize after build()
struct smi_engine;
struct Model {
  virtual ~Model() = default;
  virtual void build(smi_engine& e) = 0;        // layers from the engine's weight map, packed copies into wpack
  virtual void dry_forward(smi_engine& e) = 0;  // the largest no-grad pass: sizes arena 0
};

struct smi_engine {
  // which model the engine holds: set once, by hold(); every entry point accepts one kind and refuses the others
  enum Kind { UNET, VAE_ENCODER, VAE_DECODER, CLIP_TEXT, CLIP_VISION, LPIPS, MMDIT, FLUX, T5_ENCODER };
  Kind kind = UNET;
  std::unique_ptr<Model> model;  // (also keeps a lambda from copying an engine it names through a reference parameter)
  int dtype = 0;
  int max_n = 0;  // largest batch of a pass: every entry point checks against it
  void hold(Kind k, Model* m, int dt, int batch) {
    kind = k;
    model.reset(m);
    dtype = dt;
    max_n = batch;
  }
  hipStream_t stream = nullptr;
  // LoRA weight gradients are DEFERRED: every adapted Linear appends its rank-r reductions to `wjobs` while the
  // backward runs and one grouped launch at the end does them all (lora.hip).  The arenas never recycle memory inside a
  // backward, so x, xa and dxa are still there; the one operand at risk is dY, which can live on as another tensor's
  // gradient (accumulate() aliases it) and would then be added to IN PLACE: such buffers are `pinned`, and a write
  // that would land on a pinned buffer goes to a fresh one instead (grad_slot / accumulate).
  std::vector<WgradJob> wjobs;
  // per-sample adaptor multipliers (smi_unet_forward_multi): sigma_i = m_i / m_ref per ADAPTED sample, applied to the rows
  // of xa = x down^T (forward) and dxa = dy up (backward) -- every other use of the multiplier stays the scalar m_ref.
  // Slot 0 serves the pass in flight, slot 1 keeps the saved pass's values for its backward.
  float* samp_mult_dev = nullptr;  // [2][MAXS]
  bool samp_on = false, bw_samp_on = false;
  int n_conv_sites = 0;
  const float* samp_ptr(bool bwd) const {
    return (bwd ? bw_samp_on : samp_on) ? samp_mult_dev + (bwd ? MAXS + bw_skip : 0) : nullptr;
  }
  // slider composition (smi_unet_forward_compose): one multiplier per (adapted sample, rank column of the stacked adaptor),
  // applied to the columns of xa = x down^T -- table [n_adapted][col_ld] on the device, column c of a site's xa reads entry
  // c % col_period (a fused q|k|v lays xa out segment-major).  Forward only: a compose pass saves nothing and drops any
  // saved pass, so the table lives in the loss-scale block `gscale`, which only a backward writes and reads (it rewrites
  // the block before its first read): the workspace layout is what it was without composition.
  static constexpr int MAX_STACK_RANK = 64, MAX_SLIDERS = 16;  // (COL_TABLE_FLOATS: next to gscale, below)
  float* col_table() const { return gscale; }
  bool col_on = false;
  int col_ld = 0, col_period = 0;
  std::vector<int> lin_site_ranks;  // rank of every adapted Linear (fused group): a stack's must all be sum r_k
  std::vector<const void*> pinned;
  // X, P and M describe the rows the backward runs on; in a tail backward the job is still planned over the rows of all
  // adapted samples, so that its sums are those of the full job (WgradJob::m_begin)
  WgradJob& push_wjob(const void* X, int64_t ldx, const float* P, int64_t ldp, float* dW, int64_t so_r, int64_t so_k,
                      int M, int K, int rr, int seg_cols, int rows_per_sample, float alpha) {
    WgradJob j;
    memset(&j, 0, sizeof(j));  // padding too: the table is compared bytewise with the uploaded copy
    j.X = X;
    j.ldx = ldx;
    j.P = P;
    j.ldp = ldp;
    j.dW = dW;
    j.so_r = so_r;
    j.so_k = so_k;
    j.m_begin = bw_skip * rows_per_sample;
    j.M = j.m_begin + M;
    j.K = K;
    j.r = rr;
    j.seg_cols = seg_cols;
    j.rows_per_sample = rows_per_sample;
    j.row_scale = gscale + MAXS;
    j.alpha = alpha;
    j.conv_tap = -1;
    wgrad_job_plan(j);
    j.partial = alloc_f32(wgrad_job_scratch_floats(j));
    wjobs.push_back(j);
    return wjobs.back();
  }
  bool is_pinned(const void* g) const {
    for (const void* q : pinned)
      if (q == g) return true;
    return false;
  }
  bool dry = false;
  bool err = false;

  // workspace layout
  Arena wpack;    // packed weights + persistent small buffers
  Arena arena[2];  // 0: no-grad passes, 1: differentiated pass + backward
  Arena* cur = nullptr;
  // per-sample power-of-two loss scales: [0, MAXS) scale of adapted sample j, [MAXS, 2 MAXS) its inverse, then scratch
  static constexpr int MAXS = 1024;
  static constexpr int GSCALE_FLOATS = 3 * MAXS + 258;  // + [2 MAXS..): min, 1/min, min / scale_j (DoRA)
  static constexpr int COL_TABLE_FLOATS = 3 * MAXS;     // the compose table borrows the block
  static_assert(COL_TABLE_FLOATS <= GSCALE_FLOATS, "the compose table must fit the loss-scale block");
  float* gscale = nullptr;

  std::unordered_map<std::string, const smi_weight*> wmap;
  std::unordered_map<std::string, const smi_lora_site*> smap;
  std::vector<smi_lora_site> sites;
  std::vector<std::string> site_names;
  std::vector<char> site_used;

  // DoRA sites: delta weights [out, in] (+ their transposes for dX) and column norms, rebuilt per adapted forward
  std::vector<DoraSite> dora_sites;
  DoraSite* dora_sites_dev = nullptr;
  float bw_mult = 0.f;
  // what the delta-weight buffers currently hold: set by dora_prepare, so that the backward of a saved forward does not
  // rebuild what that forward built (nothing ran in between); `with_t`: the transposed copies for the dX GEMMs exist too
  const float* dora_ready_down = nullptr;
  const float* dora_ready_up = nullptr;
  float dora_ready_mult = 0.f;
  bool dora_ready_t = false;
  void dora_prepare(const float* down, const float* up, float m, bool with_t, bool reuse) {
    if (dora_sites.empty() || dry || err) return;
    const bool same = reuse && dora_ready_down == down && dora_ready_up == up && dora_ready_mult == m;
    if (!same) {
      if (launch_dora_prep(dtype, dora_sites_dev, dora_sites.data(), (int)dora_sites.size(), down, up, m, stream) != 0) {
        err = true;
        return;
      }
      dora_ready_down = down;
      dora_ready_up = up;
      dora_ready_mult = m;
      dora_ready_t = false;
    }
    if (with_t && !dora_ready_t) {  // a no-grad pass (pre-roll) never reads the transposed copies
      if (launch_dora_transpose(dtype, dora_sites_dev, dora_sites.data(), (int)dora_sites.size(), stream) != 0) {
        err = true;
        return;
      }
      dora_ready_t = true;
    }
  }
  // LoRA shadow operands
  std::vector<HostLoraPrepSite> prep_sites;
  void* prep_sites_dev = nullptr;
  char* lora_shadow = nullptr;
  size_t lora_shadow_elems = 0;
  // the fp32 sink of a tensor marked f32g (linear_bwd sums its gradient terms there, in the caller's buffer): the output
  // of the backward in flight, [adapted rows, cols]; d_ctx_written: a term is in it
  float* d_ctx = nullptr;
  bool d_ctx_written = false;

  // per-call state
  std::deque<Ten> tens_[2];  // per arena: a no-grad pass must not invalidate the tensors the tape refers to
  std::deque<Ten>* tens = &tens_[0];
  std::vector<std::function<void()>> tape;
  bool saving = false;
  // the forward in flight has passed a source of gradients: an adapted layer, or an attention whose k|v are differentiated.
  // (Downstream of the first one every tensor of the trunk takes a gradient; a model that also differentiates an input
  // which reaches the trunk EARLIER -- the UNet's pooled embedding -- asks this to tell what took one without it.)
  bool grad_src = false;
  int64_t pack_launches = 0;  // weight-packing kernels launched so far (creation only: a replan must not add any)
  const float* lora_down = nullptr;  // parameters of the forward in flight
  const float* lora_up = nullptr;
  const float* bw_down = nullptr;    // parameters of the saved (differentiated) forward, used by its backward
  const float* bw_up = nullptr;
  float mult = 0.f;
  float* d_down = nullptr;
  float* d_up = nullptr;
  int n_ad = 0;     // adapted samples of the pass in flight (the last n_ad of n)
  int bw_skip = 0;  // ... of which the backward in flight leaves out the first bw_skip (zero gradient: tail backward)
  // the saved (differentiated) pass of a model that has a backward, and the device table of the deferred weight-gradient
  // jobs with what it holds (bump allocation gives the same addresses every step of a plan: uploaded once, then reused)
  struct SavedPass {
    bool valid = false;
    int n = 0;  // adapted samples of the saved pass
    std::vector<WgradJob> uploaded;
    WgradJob* dev = nullptr;
    size_t cap = 0;
  } saved;
  void alloc_job_table(size_t cap) {  // at build time; the model knows how many jobs its sites can push
    saved.cap = cap;
    saved.dev = (WgradJob*)pack_alloc(cap * sizeof(WgradJob));
  }
  // a backward consumes the saved pass, also where it fails half way: a tail backward has moved the tensors' arow0
  void drop_tape() {
    pinned.clear();
    tape.clear();
    saved.valid = false;
    bw_skip = 0;
  }

  size_t esz() const { return 2; }

  // ---------------------------------------------------------------------------------------------------------
  // RUN / RUNP launch on the engine SMI_ENG: *this inside smi_engine, the parameter `e` in a model's methods (redefined
  // below the struct)
#define SMI_ENG (*this)
#define RUN(call)                          \
  do {                                     \
    if (!SMI_ENG.dry && !SMI_ENG.err) {    \
      if ((call) != 0) {                   \
        SMI_ENG.err = true;                \
      }                                    \
      SMI_ENG.bound_queue_depth();         \
    }                                      \
  } while (0)
  // same, attributing the launch (and its algorithmic FLOPs / HBM bytes) to a kernel class for smi_profile_*
#define RUNP(cat, flops, bytes, call)      \
  do {                                     \
    if (!SMI_ENG.dry && !SMI_ENG.err) {    \
      SMI_ENG.prof_begin(cat, flops, bytes); \
      if (SMI_ENG.trace_launches) SMI_ENG.trace_before(#call); \
      if ((call) != 0) {                   \
        SMI_ENG.err = true;                \
      }                                    \
      if (SMI_ENG.trace_launches) SMI_ENG.trace_after(); \
      SMI_ENG.prof_end();                  \
      SMI_ENG.bound_queue_depth();         \
    }                                      \
  } while (0)
  // SMI_TRACE_LAUNCH=1 (debugging a hang): names every launch on stderr and waits for it, so the last line printed is the
  // launch that never came back
  bool trace_launches = getenv("SMI_TRACE_LAUNCH") != nullptr;
  // SMI_SYNC_EVERY=N: wait for the stream after every N launches, i.e. never more than N (x 3 with the profiling events)
  // AQL packets of ours outstanding.  For `rocprofv3 --pmc` runs: counter collection serialises dispatches behind its own
  // start / stop / read packets, the HIP runtime's queue backs up at our launch rate, and with some hundred packets
  // outstanding the profiler's intercept queue aborted once on a packet it had not finished rewriting
  int sync_every = getenv("SMI_SYNC_EVERY") ? atoi(getenv("SMI_SYNC_EVERY")) : 0;
  int launches_since_sync = 0;
  void bound_queue_depth() {
    if (sync_every > 0 && ++launches_since_sync >= sync_every) {
      launches_since_sync = 0;
      (void)hipStreamSynchronize(stream);
    }
  }
  void trace_before(const char* what) {
    fprintf(stderr, "[smi launch] %.110s ...", what);
    fflush(stderr);
  }
  void trace_after() {
    const hipError_t e = hipStreamSynchronize(stream);
    fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
    fflush(stderr);
  }
  // RUNP for launch_gemm: `what` names the site in the trace line; `tagged` launches enter the per-shape table of
  // SMI_PROF_DUMP.  flops / bytes are the site's algorithmic counts (gemm_flops / gemm_bytes of p unless the launched
  // shape is padded)
  void run_gemm(int cat, const GemmParams& p, double flops, double bytes, bool tagged, const char* what) {
    if (dry || err) return;
    prof_begin(cat, flops, bytes);
    if (tagged && prof_on && prof_dump) next_tag = gemm_tag(p);
    if (trace_launches) trace_before(what);
    if (launch_gemm(p, stream) != 0) err = true;
    if (trace_launches) trace_after();
    prof_end();
    bound_queue_depth();
  }
  static double gemm_flops(const GemmParams& p) { return 2.0 * p.M * p.N * p.K; }
  static double gemm_bytes(const GemmParams& p) {
    return 2.0 * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * p.N);
  }

  // ---- per-kernel-class timing with HIP events on the engine's stream (profiling mode only)
  bool prof_on = false;
  struct ProfEv {
    int cat;
    hipEvent_t a, b;
    std::string tag;
    double flops;
  };
  // SMI_PROF_DUMP=1: per-shape table of the GEMM / conv launches of the profiled step on stderr (smi_profile_read)
  struct TagAcc {
    double ms = 0, flops = 0;
    int n = 0;
  };
  std::unordered_map<std::string, TagAcc> prof_tags;
  bool prof_dump = getenv("SMI_PROF_DUMP") != nullptr;
  std::string gemm_tag(const GemmParams& p) const {
    char b[160];
    snprintf(b, sizeof(b), "%s M=%d N=%d K=%d%s%s%s%s%s%s", p.conv ? "conv" : "gemm", p.M, p.N, p.K, p.bias ? " bias" : "",
             p.res ? " res" : "", p.lora_r ? " lora" : "", p.geglu_out ? " geglu" : "", p.rowvec ? " rowvec" : "",
             p.out_f32 ? " f32" : "");
    return b;
  }
  std::string next_tag;
  std::vector<ProfEv> prof_ev;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[SMI_PROF_NCAT] = {0};
  double prof_flops[SMI_PROF_NCAT] = {0};
  double prof_bytes[SMI_PROF_NCAT] = {0};
  int64_t prof_launches[SMI_PROF_NCAT] = {0};
  hipEvent_t prof_event() {
    if (!prof_pool.empty()) {
      hipEvent_t e = prof_pool.back();
      prof_pool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
  void prof_begin(int cat, double flops, double bytes) {
    if (!prof_on) return;
    ProfEv pe;
    pe.cat = cat;
    pe.a = prof_event();
    pe.b = prof_event();
    pe.flops = flops;
    (void)hipEventRecord(pe.a, stream);
    prof_ev.push_back(pe);
    prof_flops[cat] += flops;
    prof_bytes[cat] += bytes;
    prof_launches[cat] += 1;
  }
  void prof_end() {
    if (!prof_on) return;
    prof_ev.back().tag.swap(next_tag);  // set by run_gemm for a tagged launch
    next_tag.clear();
    (void)hipEventRecord(prof_ev.back().b, stream);
  }
  void prof_collect() {  // host-synchronising
    for (auto& pe : prof_ev) {
      (void)hipEventSynchronize(pe.b);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, pe.a, pe.b);
      prof_ms[pe.cat] += ms;
      if (prof_dump && !pe.tag.empty()) {
        TagAcc& t = prof_tags[pe.tag];
        t.ms += ms;
        t.flops += pe.flops;
        t.n += 1;
      }
      prof_pool.push_back(pe.a);
      prof_pool.push_back(pe.b);
    }
    prof_ev.clear();
  }

  // ---- liveness in NO-GRAD passes (arena 0: pre-roll forwards, frozen-only passes).  Nothing is saved there, so a tensor
  // is dead once the block after its producer has run.  Allocation inside a block (resnet [+ transformer], sampler conv,
  // the final norm + conv_out) comes from one of two scratch regions that alternate per block -- block k writes region
  // k & 1 while it reads block k - 1's output in the other one, and re-starts the region block k - 2 used -- except the
  // block's OUTPUT when the up path will read it again as a skip connection: that one tensor, and everything allocated
  // outside blocks (embeddings, grouped projections, conv_in), goes to the persistent bump region.  Arena 0 is then
  // persistent + 2 x the largest block instead of the sum of all tensors of a pass (SD-XL 1024^2, 16 samples: 80 -> ~10 GB);
  // the saved pass (arena 1) keeps every tensor: its backward reads them.
  Arena scr[2];
  int scr_i = 0;
  bool in_block = false, persist_next = false;
  void begin_block() {
    if (saving) return;
    scr_i ^= 1;
    scr[scr_i].reset();
    in_block = true;
  }
  void end_block() { in_block = false; persist_next = false; }
  void set_arena0_regions(size_t persistent, size_t scratch) {  // sizes from the dry run (plan)
    arena[0].cap = persistent;
    for (int k = 0; k < 2; ++k) {
      scr[k] = Arena();
      scr[k].base = arena[0].base + persistent + k * scratch;
      scr[k].cap = scratch;
    }
  }
  // the next tensor created is the current block's output and must outlive the scratch regions (a skip connection)
  void keep_next_output() { persist_next = in_block; }

  // the phase-major tensor (Ten::phase) no concat has read yet.  Every op creates its output through new_ten, so an op other
  // than that concat running while one is live is caught here instead of misreading the four planes as rows
  Ten* phase_live = nullptr;
  Ten* new_ten(int64_t rows, int cols, int n = 0, int H = 0, int W = 0, size_t elt = 0) {
    if (phase_live && !err) {
      set_error("a phase-major up-sampler output (%d x %d x %d) reached an op other than the concat of the next up block",
                phase_live->H, phase_live->W, phase_live->cols);
      err = true;
    }
    const bool keep = persist_next;
    persist_next = false;
    return borrowed(arena_alloc((size_t)rows * cols * (elt ? elt : esz()), keep), rows, cols, n, H, W);
  }
  // a tensor of the pass in flight over memory that is not allocated here: a buffer of the caller's, a view into another tensor
  Ten* borrowed(const void* p, int64_t rows, int cols, int n = 0, int H = 0, int W = 0) {
    tens->emplace_back();
    Ten* t = &tens->back();
    t->p = const_cast<void*>(p);
    t->rows = rows;
    t->cols = cols;
    t->n = n;
    t->H = H;
    t->W = W;
    t->arow0 = n > 0 ? (int64_t)(n - n_ad) * (rows / n) : 0;
    return t;
  }
  int64_t MA(const Ten* t) const { return t->rows - t->arow0; }  // adapted rows
  char* PA(const Ten* t) const { return (char*)t->p + (size_t)t->arow0 * t->cols * esz(); }
  void* arena_alloc(size_t bytes, bool persistent = false) {
    Arena* a = (in_block && !persistent) ? &scr[scr_i] : cur;
    void* p = a->alloc(bytes);
    if (!dry && a->overflow && !err) {  // never launch a kernel on memory we do not own
      set_error("workspace arena overflow (%zu > %zu bytes)", a->off, a->cap);
      err = true;
    }
    return p;
  }
  float* alloc_f32(size_t count) { return (float*)arena_alloc(count * sizeof(float)); }
  void* alloc_t(int64_t rows, int cols) { return arena_alloc((size_t)rows * cols * esz()); }

  // gradient slot of t: `out` is where the producer writes, `add` (may be null, may equal out) what is already
  // accumulated there and has to be added in the same pass.  Out of place when the old buffer is pinned.
  struct Slot {
    void* add;
    void* out;
  };
  Slot grad_slot(Ten* t) {
    Slot s;
    if (!t->g) {
      s.add = nullptr;
      s.out = t->g = alloc_t(MA(t), t->cols);
    } else if (is_pinned(t->g)) {
      s.add = t->g;
      s.out = t->g = alloc_t(MA(t), t->cols);
    } else {
      s.add = s.out = t->g;
    }
    return s;
  }
  void accumulate(Ten* t, void* g) {
    if (!t->g) {
      t->g = g;  // alias: g is dead after its producer's closure (unless pinned: then nobody writes to it)
    } else {
      Slot s = grad_slot(t);
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_add(dtype, s.add, g, s.out, MA(t) * t->cols, stream));
    }
  }
  // for a producer that cannot add in place: `produce(dst)` launches it into the [rows, cols] gradient slot gs -- straight
  // into gs.out, or, when the slot already holds a gradient, into a temporary that one launch_add then sums with it
  template <class F>
  void into_slot(const Slot& gs, int64_t rows, int cols, F produce) {
    void* const dst = gs.add ? alloc_t(rows, cols) : gs.out;
    produce(dst);
    if (gs.add) RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_add(dtype, gs.add, dst, gs.out, rows * cols, stream));
  }

  // ---------------------------------------------------------------------------------------------------------
  // model construction
  // ---------------------------------------------------------------------------------------------------------
  const smi_weight* W(const std::string& name, bool required = true) {
    auto it = wmap.find(name);
    if (it == wmap.end()) {
      if (required && !dry) {
        set_error("missing weight '%s'", name.c_str());
        err = true;
      }
      return nullptr;
    }
    return it->second;
  }
  const void* Wd(const std::string& name, bool required = true) {
    const smi_weight* w = W(name, required);
    return w ? w->data : nullptr;
  }
  void check_shape(const std::string& name, std::initializer_list<int64_t> shp) {
    if (dry) return;
    const smi_weight* w = W(name);
    if (!w) return;
    int64_t want = 1, have = 1;
    for (auto v : shp) want *= v;
    for (int i = 0; i < w->ndim; ++i) have *= w->shape[i];
    if (want != have) {
      set_error("weight '%s': expected %lld elements, got %lld", name.c_str(), (long long)want, (long long)have);
      err = true;
    }
  }
  void* pack_alloc(size_t bytes) { return wpack.alloc(bytes); }

  // (engine.hip, next to their kernels)
  void transpose_into(const void* src, void* dst, int R, int C, int ldd, int col0, bool packing = true);
  void pack_conv_into(const void* src, void* dst, int Cout, int Cin, int mode, int pad = 0);
  void pack_conv_phase_into(const void* src, void* dst, int Cout, int Cin);  // phase pack [4][Cout][4 * Cin] of a mode-2 layer

  void attach_lora(Lin& L, const std::vector<std::string>& targets) {
    // targets: the module paths fused into this GEMM (1, 2 (k|v) or 3 (q|k|v)); all adapted or none
    int found = 0;
    const smi_lora_site* first = nullptr;
    for (size_t i = 0; i < targets.size(); ++i) {
      auto it = smap.find(targets[i]);
      if (it == smap.end()) continue;
      ++found;
      const smi_lora_site* s = it->second;
      site_used[s - sites.data()] = 1;
      if (!first) first = s;
      if (i > 0 && found == (int)i + 1) {
        const int cs = L.out / (int)targets.size();
        if (s->rank != first->rank || s->scale != first->scale ||
            s->off_down != first->off_down + (int64_t)i * first->rank * L.in ||
            s->off_up != first->off_up + (int64_t)i * cs * first->rank) {
          set_error("LoRA sites fused into '%s' must be adjacent in the flat buffers with equal rank/scale",
                    L.name.c_str());
          err = true;
        }
      }
    }
    if (found == 0) return;
    if (found != (int)targets.size()) {
      set_error("LoRA must adapt all or none of the projections fused into '%s'", L.name.c_str());
      err = true;
      return;
    }
    L.nsite = found;
    L.rank = first->rank;
    lin_site_ranks.push_back(first->rank);
    L.scale = first->scale;
    L.off_down = first->off_down;
    L.off_up = first->off_up;
    if (first->off_dora >= 0) {  // DoRA site(s): all fused segments must be DoRA with adjacent scale vectors
      for (size_t i = 0; i < targets.size(); ++i) {
        const smi_lora_site* si = smap.find(targets[i])->second;
        if (si->off_dora != first->off_dora + (int64_t)i * L.in) {
          set_error("DoRA sites fused into '%s' must have adjacent dora_scale vectors", L.name.c_str());
          err = true;
          return;
        }
      }
      if (L.rank > 32) {
        set_error("DoRA rank %d > 32 on '%s'", L.rank, L.name.c_str());
        err = true;
        return;
      }
      L.dora = true;
      L.dora_idx = (int)dora_sites.size();
      DoraSite d{};
      d.W = L.W;
      d.off_down = L.off_down;
      d.off_up = L.off_up;
      d.off_dora = first->off_dora;
      d.r = L.rank;
      d.nseg = L.nseg;
      d.K = L.in;
      d.cs = L.out / L.nseg;
      d.scale = L.scale;
      d.dW = pack_alloc((size_t)L.out * L.in * esz());
      d.cnorm = (float*)pack_alloc((size_t)L.nseg * L.in * sizeof(float));
      d.dWt = pack_alloc((size_t)L.out * L.in * esz());
      dora_sites.push_back(d);
      return;  // no 16-bit shadow operands: the delta is a dense second GEMM
    }
    const int rtot = L.rank * L.nseg;
    L.rows_pad = (rtot + 15) / 16 * 16;
    prep_sites.push_back(prep_site(L, L.nseg, L.in, L.out / L.nseg, (size_t)L.rows_pad * L.in, (size_t)L.rows_pad * L.out));
  }
  // a Lin's or Conv's entry in the table of 16-bit shadow operands: reserves down_elems, then up_elems, in the shared block
  template <class Site>
  HostLoraPrepSite prep_site(Site& s, int nseg, int K, int cs, size_t down_elems, size_t up_elems) {
    HostLoraPrepSite ps{};
    ps.off_down = s.off_down;
    ps.off_up = s.off_up;
    ps.dst_down = (int64_t)lora_shadow_elems;
    lora_shadow_elems += down_elems;
    ps.dst_up = (int64_t)lora_shadow_elems;
    lora_shadow_elems += up_elems;
    ps.r = s.rank;
    ps.nseg = nseg;
    ps.K = K;
    ps.cs = cs;
    ps.rows_pad = s.rows_pad;
    s.sh_down = reinterpret_cast<const void*>((uintptr_t)ps.dst_down);  // offsets for now; rebased in finish_lora()
    s.sh_up = reinterpret_cast<const void*>((uintptr_t)ps.dst_up);
    return ps;
  }
  void attach_lora_conv(Conv& c) {
    auto it = smap.find(c.name);
    if (it == smap.end()) return;
    const smi_lora_site* s = it->second;
    site_used[s - sites.data()] = 1;
    ++n_conv_sites;
    c.nsite = 1;
    c.rank = s->rank;
    c.scale = s->scale;
    c.off_down = s->off_down;
    c.off_up = s->off_up;
    c.rows_pad = (c.rank + 15) / 16 * 16;
    if (c.rank > 64) {
      set_error("conv LoRA rank %d > 64 on '%s'", c.rank, c.name.c_str());
      err = true;
      return;
    }
    HostLoraPrepSite ps = prep_site(c, 1, c.Cin, c.Cout, (size_t)c.rows_pad * 9 * c.Cin, (size_t)c.rows_pad * c.Cout);
    ps.dst_gw = (int64_t)lora_shadow_elems;
    lora_shadow_elems += (size_t)c.Cin * 9 * 64;
    ps.conv = c.mode == 1 ? 2 : 1;  // 1: flipped taps in the gradient filter, 2: stride-2 (unflipped, transposed gather)
    prep_sites.push_back(ps);
    c.sh_gw = reinterpret_cast<const void*>((uintptr_t)ps.dst_gw);
  }
  void finish_lora() {  // after build(): all Lin objects are at their final addresses
    dora_sites_dev = (DoraSite*)pack_alloc(std::max<size_t>(dora_sites.size(), 1) * sizeof(DoraSite));
    if (!dry && !err && !dora_sites.empty())
      (void)hipMemcpyAsync(dora_sites_dev, dora_sites.data(), dora_sites.size() * sizeof(DoraSite), hipMemcpyHostToDevice,
                           stream);
    lora_shadow = (char*)pack_alloc(std::max<size_t>(lora_shadow_elems, 8) * esz());
    prep_sites_dev = pack_alloc(std::max<size_t>(prep_sites.size(), 1) * sizeof(HostLoraPrepSite));
    if (!dry && !err && !prep_sites.empty())
      (void)hipMemcpyAsync(prep_sites_dev, prep_sites.data(), prep_sites.size() * sizeof(HostLoraPrepSite),
                           hipMemcpyHostToDevice, stream);
  }
  const void* shadow_ptr(const void* off) const { return lora_shadow + (uintptr_t)off * 2; }

  // need_t: the layer lies on the gradient path (gets a transposed copy) and may carry a LoRA adaptor
  // attach_only: the layer may carry a LoRA adaptor although no gradient flows to its input (time_emb_proj)
  Lin make_lin(const std::string& name, int in, int out, bool bias, bool need_t = true, bool attach_only = false) {
    Lin L;
    L.name = name;
    L.in = in;
    L.out = out;
    L.W = Wd(name + ".weight");
    check_shape(name + ".weight", {out, in});
    L.b = bias ? Wd(name + ".bias") : nullptr;
    if (need_t) {
      void* t = pack_alloc((size_t)in * out * esz());
      transpose_into(L.W, t, out, in, out, 0);
      L.Wt = t;
      attach_lora(L, {name});
    } else if (attach_only) {
      attach_lora(L, {name});
    }
    return L;
  }
  // fused projection: rows of the parts concatenated ([sum out, in]); Wt [in, sum out]
  Lin make_fused(const std::string& base, const std::vector<std::string>& parts, int in, int out_each, bool need_t) {
    Lin L;
    L.name = base + ".{" + parts[0] + "..}";
    L.in = in;
    L.out = out_each * (int)parts.size();
    L.nseg = (int)parts.size();
    char* w = (char*)pack_alloc((size_t)L.out * in * esz());
    char* t = need_t ? (char*)pack_alloc((size_t)L.out * in * esz()) : nullptr;
    std::vector<std::string> targets;
    for (size_t i = 0; i < parts.size(); ++i) {
      const std::string nm = base + "." + parts[i];
      const void* src = Wd(nm + ".weight");
      check_shape(nm + ".weight", {out_each, in});
      if (!dry && !err && src)
        (void)hipMemcpyAsync(w + i * (size_t)out_each * in * esz(), src, (size_t)out_each * in * esz(),
                             hipMemcpyDeviceToDevice, stream);
      if (t) transpose_into(src, t, out_each, in, L.out, (int)i * out_each);
      targets.push_back(nm);
    }
    L.W = w;
    L.Wt = t;
    attach_lora(L, targets);
    return L;
  }
  // the bias that goes with make_fused: the parts' bias vectors copied one after the other into one packed block
  const void* fused_bias(const std::string& base, const std::vector<std::string>& parts, int out_each) {
    char* b = (char*)pack_alloc(parts.size() * (size_t)out_each * esz());
    for (size_t i = 0; i < parts.size(); ++i) {
      const void* src = Wd(base + "." + parts[i] + ".bias");
      if (!dry && !err && src)
        (void)hipMemcpyAsync(b + i * (size_t)out_each * esz(), src, (size_t)out_each * esz(), hipMemcpyDeviceToDevice,
                             stream);
    }
    return b;
  }
  // phase: a mode-2 layer whose output only a concat reads (the UNets' up-samplers) may run as four 2x2 phase convs
  Conv make_conv(const std::string& name, int Cin, int Cout, int mode, bool grad_pack, bool phase = false) {
    Conv c;
    c.Cin = Cin;
    c.Cout = Cout;
    c.mode = mode;
    c.b = Wd(name + ".bias");
    c.name = name;
    check_shape(name + ".weight", {Cout, Cin, 3, 3});
    attach_lora_conv(c);
    void* wp = pack_alloc((size_t)Cout * Cin * 9 * esz());
    pack_conv_into(Wd(name + ".weight"), wp, Cout, Cin, 0);
    c.Wp = wp;
    if (grad_pack) {
      void* wg = pack_alloc((size_t)Cout * Cin * 9 * esz());
      pack_conv_into(Wd(name + ".weight"), wg, Cout, Cin, mode == 1 ? 1 : 2);
      c.Wg = wg;
    }
    // an adaptor keeps the layer on the 3x3 form: its xa / delta / weight-gradient jobs are written for that one
    if (phase && mode == 2 && c.rank == 0 && upconv_phase_on()) {
      void* wph = pack_alloc((size_t)16 * Cout * Cin * esz());
      pack_conv_phase_into(Wd(name + ".weight"), wph, Cout, Cin);
      c.Wph = wph;
      c.phase = true;
    }
    return c;
  }
  // a model's first conv on the MFMA conv path: input channels zero-padded to 64 (one K step per filter tap)
  Conv make_conv_in(const std::string& name, int Cin, int Cout) {
    Conv c;
    c.Cin = 64;
    c.Cout = Cout;
    c.b = Wd(name + ".bias");
    check_shape(name + ".weight", {Cout, Cin, 3, 3});
    void* wp = pack_alloc((size_t)Cout * 9 * 64 * esz());
    pack_conv_into(Wd(name + ".weight"), wp, Cout, Cin, 0, 64);
    c.Wp = wp;
    return c;
  }
  Norm make_norm(const std::string& name, int C, float eps, int groups) {  // groups: 0 for a LayerNorm
    Norm n;
    n.C = C;
    n.groups = groups;
    n.eps = eps;
    n.gamma = Wd(name + ".weight");
    n.beta = Wd(name + ".bias");
    check_shape(name + ".weight", {C});
    return n;
  }
  // ted: width of the time embedding (0: the block has no time_emb_proj); grad: the block lies on a gradient path
  // (gradient filter packs, transposed shortcut); eps 1e-5 UNet / 1e-6 VAE
  Resnet make_resnet(const std::string& name, int Cin, int Cout, int groups, int ted, float eps = 1e-5f, bool grad = true) {
    Resnet r;
    r.n1 = make_norm(name + ".norm1", Cin, eps, groups);
    r.c1 = make_conv(name + ".conv1", Cin, Cout, 0, grad);
    if (ted > 0) r.temb = make_lin(name + ".time_emb_proj", ted, Cout, true, false, true);
    r.n2 = make_norm(name + ".norm2", Cout, eps, groups);
    r.c2 = make_conv(name + ".conv2", Cout, Cout, 0, grad);
    r.has_sc = Cin != Cout;
    if (r.has_sc) r.sc = make_lin(name + ".conv_shortcut", Cin, Cout, true, grad);
    return r;
  }

  // ---------------------------------------------------------------------------------------------------------
  // ops
  // ---------------------------------------------------------------------------------------------------------
  template <class Site>  // Lin or Conv
  bool lora_active(const Site& L) const { return L.nsite > 0 && (dry || (lora_down && lora_up && mult != 0.f)); }
  // first adapted sample / adapted samples of t, whose samples are `rows` rows each
  int ad_first(const Ten* t, int rows) const { return (int)(t->arow0 / rows); }
  int ad_samples(const Ten* t, int rows) const { return t->n - ad_first(t, rows); }
  // rows per adapted sample of a buffer that holds M rows of the adapted samples
  int rows_per_ad(int64_t M) const { return std::max(1, (int)(M / std::max(n_ad, 1))); }

  // out[M, R] (fp32, dense) = X[M, K] * S[R, K]^T against a 16-bit LoRA shadow S: xa = x down^T and dxa = dy up.  The skinny
  // kernel where it takes the shape, else a GEMM (+ the per-sample multipliers `row_mul` as a launch of their own)
  void skinny_product(const void* X, int64_t ldx, const void* S, float* out, int M, int R, int K, double flops,
                      const float* row_mul, bool tagged, const char* what, bool cols = false) {
    if (cols && !dry) {  // a slider stack's column table instead of row_mul: same two routes
      if (lora_skinny_supported(X, ldx, S, out, R, M, R, K)) {
        RUNP(SMI_PROF_LORA, flops, 0.0,
             launch_lora_skinny_cols(dtype, X, ldx, S, out, R, M, R, K, col_table(), col_ld, col_period, rows_per_ad(M), stream));
        return;
      }
      run_gemm(SMI_PROF_LORA, gemm_nt(dtype, X, ldx, S, out, R, M, R, K).f32_out(), flops, 0.0, tagged, what);
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_col_scale_f32(out, R, M, R, col_table(), col_ld, col_period, rows_per_ad(M), stream));
      return;
    }
    if (dry || lora_skinny_supported(X, ldx, S, out, R, M, R, K)) {
      RUNP(SMI_PROF_LORA, flops, 0.0,
           launch_lora_skinny(dtype, X, ldx, S, out, R, M, R, K, stream, row_mul, rows_per_ad(M)));
      return;
    }
    run_gemm(SMI_PROF_LORA, gemm_nt(dtype, X, ldx, S, out, R, M, R, K).f32_out(), flops, 0.0, tagged, what);
    if (row_mul) RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_row_scale_f32(out, R, M, R, row_mul, rows_per_ad(M), stream));
  }

  Ten* linear(Ten* x, const Lin& L, Ten* res = nullptr) {
    Ten* y = new_ten(x->rows, L.out, x->n, x->H, x->W);
    const bool lon = lora_active(L);
    const int rtot = L.rank * L.nseg;
    float* xa = nullptr;
    const float lscale = mult * L.scale;
    if (lon && !L.dora) {  // xa[M, rows_pad] = x * down^T as one MFMA GEMM on the 16-bit shadow copy (fp32 result)
      xa = alloc_f32((size_t)MA(x) * L.rows_pad);
      skinny_product(PA(x), x->cols, shadow_ptr(L.sh_down), xa, (int)MA(x), L.rows_pad, L.in,
                     2.0 * (int)MA(x) * rtot * L.in, samp_ptr(false), true, "linear xa", col_on);
    }
    GemmParams p = gemm_nt(dtype, x->p, x->cols, L.W, y->p, L.out, (int)x->rows, L.out, L.in).with_bias(L.b);
    if (res) p.with_res(res->p, res->cols);
    if (lon && !L.dora)
      p.with_lora(xa, L.rows_pad, lora_up + L.off_up, L.rank, L.nseg > 1 ? L.out / L.nseg : 0, lscale, (int)x->arow0);
    run_gemm(SMI_PROF_GEMM, p, gemm_flops(p), gemm_bytes(p), true, "linear");
    y->arow0 = x->arow0;
    if (lon) grad_src = true;
    if (lon && L.dora && MA(x) > 0) {  // adapted rows: y += x dW^T (dW holds lscale), accumulated onto the main result
      const GemmParams d = gemm_nt(dtype, PA(x), x->cols, dora_sites[L.dora_idx].dW, PA(y), L.out, (int)MA(x), L.out, L.in)
                               .with_res(PA(y), L.out);
      run_gemm(SMI_PROF_LORA, d, gemm_flops(d), 0.0, false, "dora forward");
    }
    y->ng = lon || x->ng || (res && res->ng);
    if (saving && y->ng) {
      const Lin* Lp = &L;
      tape.push_back([=]() { linear_bwd(x, Lp, res, y, xa, lon, lscale); });
    }
    return y;
  }
  void linear_bwd(Ten* x, const Lin* L, Ten* res, Ten* y, float* xa, bool lon, float lscale) {
    void* dy = y->g;
    if (!dy) return;
    if (res && res->ng) accumulate(res, dy);
    const int M = (int)MA(x);
    const int rtot = L->rank * L->nseg;
    float* dxa = nullptr;
    if (lon && L->dora) {
      // G = dY^T X (dense fp32 [out, in]) from transposed 16-bit copies; rows of different samples carry different
      // power-of-two loss scales, so dY is brought to the smallest one while it is transposed (min / scale_j <= 1)
      const DoraSite& ds = dora_sites[L->dora_idx];
      const int Mp = (M + 63) / 64 * 64;
      const int rps = rows_per_ad(M);
      void* dyT = alloc_t(L->out, Mp);
      void* xT = alloc_t(L->in, Mp);
      float* G = alloc_f32((size_t)L->out * L->in);
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_transpose_scaled(dtype, dy, L->out, dyT, M, L->out, Mp, gscale + 2 * MAXS + 2, rps, stream));
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_transpose_scaled(dtype, PA(x), x->cols, xT, M, L->in, Mp, nullptr, rps, stream));
      run_gemm(SMI_PROF_LORA, gemm_nt(dtype, dyT, Mp, xT, G, L->in, L->out, L->in, Mp).f32_out(),
               2.0 * L->out * L->in * M, 0.0, false, "dora G");
      // dW was built with lscale folded in: d(dW_unscaled) = lscale * G; the common loss scale (the minimum) divides out
      float* dscr = alloc_f32(dora_grad_scratch_floats(ds));
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_dora_grads(dtype, ds, G, bw_down, bw_up, d_down, d_up, lscale / y->gmul, gscale + 2 * MAXS + 1, dscr, stream));
    }
    if (lon && !L->dora) {
      const int cs = L->out / L->nseg;
      const int r = L->rank;
      const int rp = L->rows_pad;
      dxa = alloc_f32((size_t)M * rp);
      // dxa[M, rows_pad] = dy * upT^T : one MFMA GEMM against the block-diagonal 16-bit shadow of lora_up
      skinny_product(dy, L->out, shadow_ptr(L->sh_up), dxa, M, rp, L->out, 2.0 * M * rtot * cs, samp_ptr(true), true,
                     "linear dxa");
      // deferred (see `wjobs`): d(up)[n][q] += lscale/S * sum_m dy[m][n] * xa[m][seg(n)*r + q]  for all segments,
      //                         d(down)[q'][k] += lscale/S * sum_m dxa[m][q'] * x[m][k]       (q' over the r_tot rows)
      const int rps = rows_per_ad(M);
      const float alpha = lscale / y->gmul;  // y->gmul: power-of-two factor the stored gradient carries (1 but for row vectors)
      auto push = [&](const void* X, int64_t ldx, const float* P, float* dW, int64_t so_r, int64_t so_k, int K, int rr,
                      int seg_cols) {
        push_wjob(X, ldx, P, rp, dW, so_r, so_k, M, K, rr, seg_cols, rps, alpha);
      };
      push(dy, L->out, xa + x->bskip * rp, d_up ? d_up + L->off_up : nullptr, 1, r, L->out, r, L->nseg > 1 ? cs : 0);
      // all segments of a fused projection in one job only while their rank rows fit the 8-accumulator class; beyond that
      // one job per segment: x is read once per segment, but the reduction kernel keeps R x 8 fp32 accumulators per thread
      // and its speed falls with R -- rank 8 on q|k|v (24 rows -> the 32-row class, 256 accumulators) took 7.5 ms per step
      // (lora class 12.7 -> 5.9 ms split), rank 4 (12 rows -> the 16-row class) 5.1 -> 4.7 ms.  SMI_WGRAD_SEG_MAX overrides.
      static const int seg_max = []() { const char* e = getenv("SMI_WGRAD_SEG_MAX"); return e ? atoi(e) : 8; }();
      if (rtot <= seg_max) {
        push(PA(x), x->cols, dxa, d_down ? d_down + L->off_down : nullptr, L->in, 1, L->in, rtot, 0);
      } else {
        for (int sg = 0; sg < L->nseg; ++sg) {
          push(PA(x), x->cols, dxa + sg * r, d_down ? d_down + L->off_down + (int64_t)sg * r * L->in : nullptr, L->in, 1,
               L->in, r, 0);
        }
      }
      pinned.push_back(dy);
    }
    if (x->ng) {
      if (!L->Wt && !dry) {
        set_error("internal: no transposed weight for '%s'", L->name.c_str());
        err = true;
        return;
      }
      if (x->f32g) {  // the context: one term per cross-attention block, summed in fp32 in the caller's buffer
        if (!d_ctx) return;
        if (lon && L->dora && !dry) {
          set_error("context gradient through a DoRA site ('%s') is not implemented", L->name.c_str());
          err = true;
          return;
        }
        float* dst = d_ctx_written ? alloc_f32((size_t)M * L->in) : d_ctx;
        GemmParams p = gemm_nt(dtype, dy, L->out, L->Wt, dst, L->in, M, L->in, L->out).f32_out();
        if (lon) p.with_lora_dx(dxa, L->rows_pad, bw_down + L->off_down, rtot, lscale);
        run_gemm(SMI_PROF_GEMM, p, gemm_flops(p), gemm_bytes(p), true, "linear d_ctx");
        if (d_ctx_written) RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_axpby(d_ctx, dst, 1.f, 1.f, (int64_t)M * L->in, stream));
        d_ctx_written = true;
        return;
      }
      const Slot gs = grad_slot(x);
      GemmParams p = gemm_nt(dtype, dy, L->out, L->Wt, gs.out, L->in, M, L->in, L->out);
      if (gs.add) p.with_res(gs.add, L->in);
      // (down: A_cat [rtot, in] read as [in][rtot])
      if (lon && !L->dora) p.with_lora_dx(dxa, L->rows_pad, bw_down + L->off_down, rtot, lscale);
      run_gemm(SMI_PROF_GEMM, p, gemm_flops(p), gemm_bytes(p), true, "linear dX");
      if (lon && L->dora) {  // dX += dY dW (dW^T [in, out] is the K-contiguous operand), accumulated in place
        const GemmParams d = gemm_nt(dtype, dy, L->out, dora_sites[L->dora_idx].dWt, gs.out, L->in, M, L->in, L->out)
                                 .with_res(gs.out, L->in);
        run_gemm(SMI_PROF_LORA, d, gemm_flops(d), 0.0, false, "dora dX");
      }
    }
  }

  Ten* layernorm(Ten* x, const Norm& nm) {
    Ten* y = new_ten(x->rows, x->cols, x->n, x->H, x->W);
    float* st = alloc_f32((size_t)x->rows * 2);
    RUNP(SMI_PROF_NORM, 0.0, 4.0 * x->rows * x->cols, launch_layernorm_fwd(dtype, x->p, nm.gamma, nm.beta, y->p, st, (int)x->rows, x->cols, nm.eps, stream));
    y->ng = x->ng;
    if (saving && y->ng) {
      const Norm* np = &nm;
      tape.push_back([=]() {
        if (!y->g) return;
        const Slot gs = grad_slot(x);
        RUNP(SMI_PROF_NORM, 0.0, 6.0 * MA(x) * x->cols, launch_layernorm_bwd(dtype, PA(x), y->g, np->gamma, st + x->arow0 * 2, gs.add, gs.out, (int)MA(x), x->cols,
                                 stream));
      });
    }
    return y;
  }

  Ten* groupnorm(Ten* x, const Norm& nm, bool silu) {
    const int HW = x->H * x->W, G = nm.groups, C = x->cols;
    Ten* y = new_ten(x->rows, C, x->n, x->H, x->W);
    float* ab = alloc_f32((size_t)2 * x->n * C);
    float* mr = alloc_f32((size_t)x->n * G * 2);
    const size_t npart = gn_partial_floats(x->n, HW, G);
    float* part = alloc_f32(npart);
    RUNP(SMI_PROF_NORM, 0.0, 4.0 * x->rows * x->cols, launch_groupnorm_fwd(dtype, x->p, nm.gamma, nm.beta, y->p, ab, mr, part, x->n, HW, C, G, nm.eps, silu ? 1 : 0,
                             stream));
    y->ng = x->ng;
    if (saving && y->ng) {
      const Norm* np = &nm;
      tape.push_back([=]() {
        if (!y->g) return;
        const Slot gs = grad_slot(x);
        float* scr = alloc_f32(npart);
        const int n0 = ad_first(x, HW);
        RUNP(SMI_PROF_NORM, 0.0, 6.0 * MA(x) * x->cols, launch_groupnorm_bwd(dtype, PA(x), y->g, np->gamma, np->beta, ab + (size_t)n0 * C, ab + (size_t)(x->n + n0) * C, mr + (size_t)n0 * G * 2, gs.add, gs.out, scr, x->n - n0, HW,
                                 C, G, silu ? 1 : 0, stream));
      });
    }
    return y;
  }

  // ff.net.0 (GEGLU): proj = x W^T + b ; out = proj[:, :4C] * gelu(proj[:, 4C:]) as ONE GEMM whose epilogue applies the
  // gate; the projection is written only for the adapted rows (the backward's geglu_bwd needs it).
  Ten* linear_geglu(Ten* x, const Lin& L) {
    const bool need_proj = saving && x->ng;
    void* const probe = reinterpret_cast<void*>(16);  // placeholder output pointers for the capability query
    GemmParams p = gemm_nt(dtype, x->p, x->cols, L.W, probe, L.out, (int)x->rows, L.out, L.in).with_bias(L.b);
    if (lora_active(L) || !(dry || gemm_geglu_supported(p.with_geglu(probe, 0)))) return geglu(linear(x, L));  // generic path
    Ten* out = new_ten(x->rows, L.out / 2, x->n, x->H, x->W);
    // the projection buffer holds the adapted rows only; virtual base so that row m lands at (m - arow0)
    char* pbuf = (char*)arena_alloc((size_t)(need_proj ? MA(x) : 1) * L.out * esz());
    Ten* pj = borrowed(pbuf - (size_t)x->arow0 * L.out * esz(), x->rows, L.out, x->n, x->H, x->W);
    pj->arow0 = x->arow0;
    p.C = pj->p;
    p.with_geglu(out->p, need_proj ? (int)x->arow0 : p.M);
    run_gemm(SMI_PROF_GEMM, p, gemm_flops(p), 2.0 * ((double)p.M * p.K + (double)p.N * p.K + 0.5 * (double)p.M * p.N), true,
             "linear_geglu");
    out->ng = x->ng;
    pj->ng = x->ng;
    if (saving && out->ng) {
      const Lin* Lp = &L;
      const int C4 = L.out / 2;
      tape.push_back([=]() {  // linear backward (runs after the GEGLU backward below has produced pj->g)
        linear_bwd(x, Lp, nullptr, pj, nullptr, false, 0.f);
      });
      tape.push_back([=]() {
        if (!out->g) return;
        void* dp = grad_slot(pj).out;  // the projection has a single consumer: nothing accumulated yet
        RUNP(SMI_PROF_ELEM, 0.0, 10.0 * MA(pj) * C4, launch_geglu_bwd(dtype, PA(pj), out->g, dp, (int)MA(pj), C4, stream));
      });
    }
    return out;
  }

  Ten* geglu(Ten* pj) {
    const int C4 = pj->cols / 2;
    Ten* y = new_ten(pj->rows, C4, pj->n, pj->H, pj->W);
    RUNP(SMI_PROF_ELEM, 0.0, 6.0 * pj->rows * C4, launch_geglu_fwd(dtype, pj->p, y->p, (int)pj->rows, C4, stream));
    y->ng = pj->ng;
    if (saving && y->ng) {
      tape.push_back([=]() {
        if (!y->g) return;
        // (a slot that holds a gradient never happens in this graph: proj has a single consumer)
        into_slot(grad_slot(pj), MA(pj), pj->cols, [&](void* dp) {
          RUNP(SMI_PROF_ELEM, 0.0, 10.0 * MA(pj) * C4, launch_geglu_bwd(dtype, PA(pj), y->g, dp, (int)MA(pj), C4, stream));
        });
      });
    }
    return y;
  }

  // self-attention on a fused [M, 3C] q|k|v tensor, or cross-attention on q [M, C] and kv [n*L, 2C] -- or on k|v at
  // `kv_ext` (leading dimension ld_ext) inside a tensor of the caller's; kvg: that tensor, when it takes a gradient
  // dq_apart (with kvg): dK|dV by a launch of their own, as where q takes no gradient, and dQ by a second one -- the bits
  // of dK|dV then do not depend on whether dQ is wanted (a dQ kernel forms delta in another order than attn_delta_kernel)
  Ten* attention(Ten* qkv, Ten* q, Ten* kv, int heads, int C, int nbatch, int Nq, int Nk, bool causal,
                 const void* kv_ext = nullptr, int64_t ld_ext = 0, Ten* kvg = nullptr, bool dq_apart = false) {
    Ten* src_q = qkv ? qkv : q;
    Ten* o = new_ten(src_q->rows, C, src_q->n, src_q->H, src_q->W);
    float* lse = alloc_f32((size_t)nbatch * heads * Nq);
    AttnParams p;
    p.dtype = dtype;
    p.B = nbatch;
    p.H = heads;
    p.Nq = Nq;
    p.Nk = Nk;
    p.D = C / heads;
    p.scale = 1.f / sqrtf((float)p.D);
    p.causal = causal ? 1 : 0;
    if (qkv) {
      p.Q = qkv->p;
      p.K = (char*)qkv->p + (size_t)C * esz();
      p.V = (char*)qkv->p + (size_t)2 * C * esz();
      p.ldq = p.ldk = p.ldv = 3 * C;
    } else {
      p.Q = q->p;
      p.ldq = C;
      p.K = kv_ext ? kv_ext : kv->p;
      p.V = (const char*)p.K + (size_t)C * esz();
      p.ldk = p.ldv = kv_ext ? ld_ext : 2 * C;
    }
    p.O = o->p;
    p.ldo = C;
    p.lse = lse;
    RUNP(SMI_PROF_ATTN, 4.0 * nbatch * heads * (double)Nq * Nk * p.D, 0.0, launch_attn_fwd(p, stream));
    // external k|v with a gradient owner: dK|dV go to this block's columns of the owner's gradient
    o->ng = qkv ? qkv->ng : (q->ng || (kv && kv->ng) || kvg);
    if ((kv && kv->ng) || kvg) grad_src = true;
    if (saving && o->ng) {
      tape.push_back([=]() {
        if (!o->g) return;
        AttnParams b = p;
        const int b0 = ad_first(o, Nq);
        b.B = nbatch - b0;
        b.Q = (const char*)p.Q + (size_t)b0 * Nq * p.ldq * esz();
        b.K = (const char*)p.K + (size_t)b0 * Nk * p.ldk * esz();
        b.V = (const char*)p.V + (size_t)b0 * Nk * p.ldv * esz();
        b.O = PA(o);
        b.lse = p.lse + (size_t)b0 * heads * Nq;
        b.dO = o->g;
        b.lddo = C;
        b.delta = alloc_f32((size_t)b.B * heads * Nq);
        // q|k|v, q and kv tensors have a single consumer (this attention): their slots are fresh
        if (qkv) {
          char* g = (char*)grad_slot(qkv).out;
          b.dQ = g;
          b.dK = g + (size_t)C * esz();
          b.dV = g + (size_t)2 * C * esz();
          b.lddq = b.lddk = b.lddv = 3 * C;
        } else {
          if (q->ng) {
            b.dQ = grad_slot(q).out;
            b.lddq = C;
          }
          if (kv && kv->ng) {
            char* g = (char*)grad_slot(kv).out;
            b.dK = g;
            b.dV = g + (size_t)C * esz();
            b.lddk = b.lddv = 2 * C;
          }
          if (kvg) {
            if (!kvg->g) {  // every block writes its own columns; zeroed once in case a block's gradient never arrives
              kvg->g = alloc_t(MA(kvg), kvg->cols);
              if (!dry && !err) (void)hipMemsetAsync(kvg->g, 0, (size_t)MA(kvg) * kvg->cols * esz(), stream);
            }
            char* g = (char*)kvg->g + ((const char*)kv_ext - (const char*)kvg->p);
            b.dK = g;
            b.dV = g + (size_t)C * esz();
            b.lddk = b.lddv = ld_ext;
          }
        }
        // SMI_PROF_DUMP: the cross-attention backward launches that produce dK / dV get a line of their own in the table
        if (prof_on && prof_dump && !qkv && b.dK) {
          char tag[96];
          snprintf(tag, sizeof(tag), "attn_bwd dK|dV%s B=%d H=%d Nq=%d Nk=%d D=%d", b.dQ ? "" : " (no dQ)", b.B, heads, Nq, Nk, b.D);
          next_tag = tag;
        }
        if (dq_apart && kvg && b.dQ) {
          AttnParams kvp = b, qp = b;
          kvp.dQ = nullptr;
          qp.dK = qp.dV = nullptr;
          RUNP(SMI_PROF_ATTN, 6.0 * b.B * heads * (double)Nq * Nk * b.D, 0.0, launch_attn_bwd(kvp, stream));
          RUNP(SMI_PROF_ATTN, 6.0 * b.B * heads * (double)Nq * Nk * b.D, 0.0, launch_attn_bwd(qp, stream));
          return;
        }
        RUNP(SMI_PROF_ATTN, 10.0 * b.B * heads * (double)Nq * Nk * b.D, 0.0, launch_attn_bwd(b, stream));
      });
    }
    return o;
  }

  // the gradient of a row vector added to a map of HW pixels is stored x 2^-k, k = rowvec_shift(HW) ~ log2(HW) / 2
  static int rowvec_shift(int HW) {
    int k = 0;
    while ((1 << (2 * (k + 1))) <= HW) ++k;
    return k;
  }
  // 3x3 conv (pad 1): mode 0 stride 1, 1 stride 2, 2 nearest-2x upsample then stride 1
  // rvg: the tensor `rowvec` is a column block of (leading dimension ld_rowvec), when that tensor takes the gradient:
  // d(rowvec) lands in the block's columns of rvg->g, x the block's own 2^-k (whoever reads rvg->g divides it out per block)
  Ten* conv3x3(Ten* x, const Conv& c, Ten* rowvec, Ten* res, int64_t ld_rowvec = 0, Ten* rvg = nullptr) {
    const int Hin = x->H, Win = x->W;
    const int Hout = conv3x3_out(Hin, c.mode), Wout = conv3x3_out(Win, c.mode);
    Ten* y = new_ten((int64_t)x->n * Hout * Wout, c.Cout, x->n, Hout, Wout);
    GemmParams p = conv3x3_fwd(dtype, x->p, c.Wp, y->p, x->n, Hin, Win, c.Cin, c.Cout, c.mode, c.pad).with_bias(c.b);
    if (rowvec) p.with_rowvec(rowvec->p, Hout * Wout, ld_rowvec);
    if (res) p.with_res(res->p, res->cols);
    // c3lier adaptor: y += lscale * up(down_conv(x)) on the adapted samples.  xa = down_conv(x) is the same conv once more on
    // the adapted samples with the (16-row padded) shadow filter and fp32 output; the 1x1 up-projection rides in the main
    // epilogue.
    const bool lon = lora_active(c);
    const float lscale = mult * c.scale;
    float* xa = nullptr;
    if (lon) {
      grad_src = true;
      xa = alloc_f32((size_t)MA(y) * c.rows_pad);
      const GemmParams g = conv3x3_fwd(dtype, PA(x), shadow_ptr(c.sh_down), xa, ad_samples(x, Hin * Win), Hin, Win, c.Cin,
                                       c.rows_pad, c.mode, c.pad).f32_out();
      run_gemm(SMI_PROF_LORA, g, 2.0 * g.M * c.rank * g.K, 0.0, false, "conv3x3 xa");
      p.with_lora(xa, c.rows_pad, lora_up + c.off_up, c.rank, 0, lscale, (int)y->arow0);
    }
    if (c.phase && !rowvec && !res && upconv_phase_takes(Hin * Win)) {
      // four 2x2 phase convs on the low-res grid (4/9 of the FLOPs, which is what the profile is told), one output plane
      // each: y is phase-major and the next op -- the up path's concat -- puts the rows back in order as it copies them
      for (int ph = 0; ph < 4; ++ph) {
        const GemmParams q = conv2x2_phase(dtype, x->p, c.Wph, y->p, x->n, Hin, Win, c.Cin, c.Cout, ph).with_bias(c.b);
        run_gemm(SMI_PROF_CONV, q, gemm_flops(q), 2.0 * ((double)x->rows * c.Cin + (double)q.N * q.K + (double)q.M * q.N), true,
                 "conv3x3 phase");
      }
      y->phase = true;
      phase_live = y;
    } else {
      run_gemm(SMI_PROF_CONV, p, gemm_flops(p), 2.0 * ((double)x->rows * c.Cin + (double)p.N * p.K + (double)p.M * p.N), true,
               "conv3x3");
    }
    y->ng = lon || x->ng || (res && res->ng) || (rowvec && rowvec->ng);
    if (saving && y->ng) {
      const Conv* cp = &c;
      tape.push_back([=]() {
        void* dy = y->g;
        if (!dy) return;
        if (res && res->ng) accumulate(res, dy);
        const int nb_ad = ad_samples(x, Hin * Win);
        if (rowvec && rowvec->ng) {
          // d(rowvec)[n][c] = sum over the pixels of sample n of dy; stored x 2^-k (k ~ log2(HW) / 2) so that a coherent sum
          // cannot leave the fp16 range -- linear_bwd divides it out again (Ten::gmul)
          rowvec->gmul = exp2f((float)-rowvec_shift(Hout * Wout));
          if (rvg) {  // every block writes its own columns; zeroed once in case a block's gradient never arrives
            if (!rvg->g) {
              rvg->g = alloc_t(MA(rvg), rvg->cols);
              if (!dry && !err) (void)hipMemsetAsync(rvg->g, 0, (size_t)MA(rvg) * rvg->cols * esz(), stream);
            }
            rowvec->g = (char*)rvg->g + ((const char*)rowvec->p - (const char*)rvg->p);
          } else {
            rowvec->g = alloc_t(MA(rowvec), rowvec->cols);
          }
          float* cs_scratch = alloc_f32(colsum_scratch_floats(nb_ad, cp->Cout));
          RUNP(SMI_PROF_ELEM, 0.0, 0.0,
               launch_colsum(dtype, dy, rowvec->g, cs_scratch, nb_ad, Hout * Wout, cp->Cout, rowvec->gmul, stream,
                             rvg ? ld_rowvec : 0));
        }
        float* dxa = nullptr;
        if (lon) {
          const int M = (int)MA(y), rp = cp->rows_pad, r = cp->rank;
          dxa = alloc_f32((size_t)M * rp);
          // dxa[M, rows_pad] = dy * up
          skinny_product(dy, cp->Cout, shadow_ptr(cp->sh_up), dxa, M, rp, cp->Cout, 2.0 * M * r * cp->Cout, nullptr, false,
                         "conv3x3 dxa");
          const int rps = Hout * Wout;
          // d(up)[n][q] += lscale/S * sum_m dy[m][n] xa[m][q];  d(down)[q][ci][tap] += lscale/S * sum_m dxa[m][q] x[pixel(m, tap)][ci]
          push_wjob(dy, cp->Cout, xa + y->bskip * rp, rp, d_up ? d_up + cp->off_up : nullptr, 1, r, M, cp->Cout, r, 0, rps, lscale);
          for (int t = 0; t < 9; ++t) {
            WgradJob& j = push_wjob(PA(x), cp->Cin, dxa, rp, d_down ? d_down + cp->off_down + t : nullptr,
                                    (int64_t)9 * cp->Cin, 9, M, cp->Cin, r, 0, rps, lscale);
            j.conv_tap = t;
            j.Hin = Hin;
            j.Win = Win;
            j.Hout = Hout;
            j.Wout = Wout;
            j.conv_stride = cp->mode == 1 ? 2 : 1;
            j.conv_ups = cp->mode == 2 ? 1 : 0;
          }
          pinned.push_back(dy);
        }
        if (!x->ng) return;
        const Slot gs = grad_slot(x);
        // the adaptor's share of dX: the same gradient conv once more on dxa (fp32 -> 64-channel 16-bit image, x lscale)
        // with the down filter's gradient pack, accumulated onto the main result
        void* dxa16 = nullptr;
        if (lon) {
          dxa16 = alloc_t(MA(y), 64);
          RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_f32_to_padded(dtype, dxa, cp->rows_pad, cp->rank, dxa16, 64, MA(y), lscale, stream));
        }
        // mode 2 (upsample + conv): the gradient lands on the 2x grid and is sum-pooled 2x2 afterwards; else straight in dX
        void* const dst = cp->mode == 2 ? alloc_t(MA(y), cp->Cin) : gs.out;
        GemmParams b = conv3x3_grad(dtype, dy, cp->Wg, dst, nb_ad, Hin, Win, cp->Cin, cp->Cout, cp->mode);
        if (cp->mode != 2 && gs.add) b.with_res(gs.add, cp->Cin);
        run_gemm(SMI_PROF_CONV, b, gemm_flops(b), 0.0, true, "conv3x3 dX");
        if (lon) {  // the same gradient conv on dxa16, accumulated onto the main result
          const GemmParams a = conv3x3_grad(dtype, dxa16, shadow_ptr(cp->sh_gw), dst, nb_ad, Hin, Win, cp->Cin, 64, cp->mode)
                                   .with_res(dst, cp->Cin);
          run_gemm(SMI_PROF_LORA, a, 2.0 * a.M * a.N * 9 * cp->rank, 0.0, false, "conv3x3 lora dX");
        }
        if (cp->mode == 2)
          into_slot(gs, MA(x), cp->Cin, [&](void* dx) {
            RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_pool2x2_sum(dtype, dst, dx, nb_ad, Hin, Win, cp->Cin, stream));
          });
      });
    }
    return y;
  }

  Ten* concat(Ten* a, Ten* b) {
    if (a->phase && a == phase_live) phase_live = nullptr;  // the one reader of a phase-major tensor (new_ten checks)
    Ten* y = new_ten(a->rows, a->cols + b->cols, a->n, a->H, a->W);
    if (a->phase)
      RUNP(SMI_PROF_ELEM, 0.0, 0.0,
           launch_copy_cols_phase(dtype, a->p, y->p, y->cols, 0, a->n, a->H / 2, a->W / 2, a->cols, stream));
    else
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(dtype, a->p, a->cols, y->p, y->cols, 0, (int)a->rows, a->cols, stream));
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(dtype, b->p, b->cols, y->p, y->cols, a->cols, (int)a->rows, b->cols, stream));
    y->ng = a->ng || b->ng;
    if (saving && y->ng) {
      tape.push_back([=]() {
        if (!y->g) return;
        Ten* parts[2] = {a, b};
        int col0 = 0;
        for (int i = 0; i < 2; ++i) {
          Ten* t = parts[i];
          if (t->ng)
            into_slot(grad_slot(t), MA(t), t->cols, [&](void* dt) {
              RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(dtype, (char*)y->g + (size_t)col0 * esz(), y->cols, dt, t->cols, 0, (int)MA(t),
                                   t->cols, stream));
            });
          col0 += t->cols;
        }
      });
    }
    return y;
  }

  Ten* silu(Ten* x) {  // only used on the (gradient-free) time embedding path
    Ten* y = new_ten(x->rows, x->cols, x->n, x->H, x->W);
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_silu(dtype, x->p, y->p, x->rows * x->cols, stream));
    return y;
  }

  // the MLP activations: kind 0 quick_gelu, 1 erf-gelu (CLIP); 2 tanh-gelu (MMDiT feed-forward)
  Ten* act(Ten* x, int kind) {
    Ten* y = new_ten(x->rows, x->cols, x->n, x->H, x->W);
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_act(dtype, x->p, y->p, x->rows * x->cols, kind, stream));
    y->ng = x->ng;
    if (saving && y->ng) {
      tape.push_back([=]() {
        if (!y->g) return;
        into_slot(grad_slot(x), MA(x), x->cols, [&](void* dx) {
          RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_act_bwd(dtype, PA(x), y->g, dx, MA(x) * x->cols, kind, stream));
        });
      });
    }
    return y;
  }

  // t: the projected time embedding, one row per sample with leading dimension ldt (0: dense); null where there is none;
  // tg: the wider tensor t is a column block of, when it takes t's gradient (conv3x3's rvg)
  Ten* resnet(Ten* x, const Resnet& r, Ten* t, int64_t ldt, bool keep_out = false, Ten* tg = nullptr) {
    Ten* h = groupnorm(x, r.n1, true);
    h = conv3x3(h, r.c1, t, nullptr, ldt, tg);
    h = groupnorm(h, r.n2, true);
    Ten* sc = r.has_sc ? linear(x, r.sc) : x;
    if (keep_out) keep_next_output();  // (conv3x3 creates its output tensor first)
    return conv3x3(h, r.c2, nullptr, sc);
  }

  // ---- whole passes: how one begins and how every one ends
  // a pass whose last n_adapted samples run under the adaptor.  save: it goes to arena 1 with a fresh tape and every tensor
  // kept (no scratch alternation: begin_block does nothing while saving); else arena 0, and a saved pass stays as it is
  void begin_pass(int n_adapted, bool save) {
    n_ad = n_adapted;
    cur = &arena[save ? 1 : 0];
    cur->reset();
    tens = &tens_[save ? 1 : 0];
    tens->clear();
    in_block = persist_next = false;
    if (!save) {
      scr[0].reset();
      scr[1].reset();
      if (dry) scr[0].cap = scr[1].cap = (size_t)-1;
    } else {
      drop_tape();
    }
    saving = save;
  }
  // the end of a saving forward: what its backward needs of the adaptor's state (the model keeps its own output tensors)
  void keep_saved_pass(int n_adapted) {
    saved.n = n_adapted;
    bw_down = lora_down;
    bw_up = lora_up;
    bw_mult = mult;
    bw_samp_on = samp_on;
    saved.valid = true;
  }
  // (forward only: arena 0, nothing adapted, nothing saved)
  void begin_forward_only_pass() {
    n_ad = 0;
    cur = &arena[0];
    cur->reset();
    tens = &tens_[0];
    tens->clear();
    saving = false;
    lora_down = lora_up = nullptr;
    mult = 0.f;
  }
  // the return value of every pass; `what` names the pass (and its arena) in the message: "this call (", "the backward ("
  int end_pass(const char* what) {
    if (cur->overflow && !dry) {
      set_error("workspace too small for %sneeds %zu bytes, has %zu)", what, cur->peak, cur->cap);
      return -3;
    }
    return err ? -1 : 0;
  }

  // ---- the backward of a saved pass (engine.hip): a model's backward is begin_backward, its own loss scales,
  // rebuild_saved_operands, its own output gradient, run_tape_and_weight_grads, end_pass("the backward (")
  // the refusal (-4, `no_pass`: the model's message) when nothing is saved; else arena 1, the gradient buffers, the last
  // n_live adapted samples of the saved pass, empty job and pin lists
  int begin_backward(const char* no_pass, float* dd, float* du, int n_live);
  // the 16-bit LoRA operands belong to the SAVED forward: an adapted no-grad pass in between may have rebuilt them with
  // other parameters or another multiplier
  void rebuild_saved_operands();
  // the tape in reverse, then every LoRA weight gradient of the pass as one grouped launch per accumulator class off the
  // device job table.  Drops the tape; not 0: the table failed (message set)
  int run_tape_and_weight_grads();

  // host floats by kernel argument, 64 per launch, ordered on the stream: dst0[i] (and dst1[i] unless NULL) = host[i] / divisor
  int upload_floats(float* dst0, float* dst1, const float* host, int n, float divisor);
  // per-sample multipliers of the coming pass: *mref = max |m_i|, sigma_i = m_i / mref to slot 0 of samp_mult_dev and, for a
  // pass that will be saved, to slot 1.  All zero: *mref = 0 and nothing is uploaded
  int set_sample_multipliers(const float* multipliers, int n, bool save, float* mref);
  // the engine's own copy of the caller's site list (targets re-pointed at strings it owns) and the map by target
  void register_sites(const smi_lora_site* s, int n_sites);
};

// from here on (the models' methods) the engine is the parameter `e`
#undef SMI_ENG
#define SMI_ENG e

// (engine.hip)  the end of every create: wait for the packing kernels, turn a failure into a message (`what` names the weights in it),
// drop the weight table, which is only borrowed during creation
int finish_create(smi_engine* e, const char* what, smi_engine** out);
// (engine.hip)  a site list of plain Linear LoRA on attention projections: no DoRA, rank in [1, 16], every target ends with
// one of `suffixes`; `who` prefixes the messages, `where` completes the last one with the allowed targets
int check_linear_lora_sites(const char* who, const smi_lora_site* sites, int n_sites, std::initializer_list<const char*> suffixes,
                            const char* where);
// the forward-only engines (VAE encoder, VAE decoder, CLIP text and image towers): `setup` fills a fresh engine with its
// kind, dtype, largest batch and its model; the workspace is [packed weights | arena 0 (| two block scratch regions, for a
// model whose forward runs in begin_block / end_block pairs)]
using Setup = std::function<void(smi_engine*)>;
int workspace_bytes_forward_only(const Setup& setup, size_t* bytes);
int create_forward_only(const Setup& setup, const char* what, const smi_weight* weights, int n_weights, void* workspace,
                        size_t workspace_bytes, void* stream, smi_engine** out);
