// The LPIPS engine, forward only: `lpips.LPIPS(net='alex')` in eval mode (eval-scripts/lpip_score.py) on the op core
// (engine.h).  Every convolution is gemm_nt with the bias epilogue on an explicit patch matrix (lpips.hip); the GEMM
// stores the pre-activation and every reader applies max(0, .).  conv3x3 is not used for conv3-5: its gather reads the
// map as it is stored, and a ReLU there would be a change to an existing kernel.  No split-K scratch is lent to the GEMMs
// (smi_lpips_distance), as in the CLIP image tower: a pair gives the same bits alone or in a batch.
#include "engine.h"

namespace {

struct LLayer {
  int k, stride, pad;
  bool pool;  // 3 x 3 / stride 2 max-pool between this layer's tap and the next convolution
};
constexpr LLayer ALEX[5] = {{11, 4, 2, true}, {5, 1, 2, true}, {3, 1, 1, false}, {3, 1, 1, false}, {3, 1, 1, false}};
const char* const ALEX_NAME[5] = {"features.0", "features.3", "features.6", "features.8", "features.10"};
int padded_k(int k, int cin) { return (k * k * cin + 63) / 64 * 64; }

struct Lpips : Model {
  smi_lpips_config cfg{};
  int img_h = 0, img_w = 0;
  Lin conv[5];
  const void* lin[5] = {};
  Lpips(const smi_lpips_config& c, int h, int w) : cfg(c), img_h(h), img_w(w) {}

  void build(smi_engine& e) override {
    int cin = 3;
    for (int i = 0; i < 5; ++i) {
      const int k = ALEX[i].k, cout = cfg.channels[i], Kp = padded_k(k, cin);
      const std::string nm = ALEX_NAME[i];
      const void* src = e.Wd(nm + ".weight");
      e.check_shape(nm + ".weight", {cout, cin, k, k});
      e.check_shape(nm + ".bias", {cout});
      void* wp = e.pack_alloc((size_t)cout * Kp * e.esz());
      if (!e.dry && !e.err && src) {
        ++e.pack_launches;
        if (launch_lpips_pack_filter(e.dtype, src, wp, cout, cin, k, Kp, e.stream) != 0) e.err = true;
      }
      conv[i].name = nm;
      conv[i].in = Kp;
      conv[i].out = cout;
      conv[i].W = wp;
      conv[i].b = e.Wd(nm + ".bias");
      const std::string ln = "lin" + std::to_string(i) + ".weight";
      lin[i] = e.Wd(ln);
      e.check_shape(ln, {cout});
      cin = cout;
    }
  }
  void dry_forward(smi_engine& e) override {
    forward(e, e.max_n, nullptr, nullptr, nullptr, nullptr, (float*)16, (float*)16, nullptr);
  }

  int forward(smi_engine& e, int n, const uint8_t* rgb8_a, const uint8_t* rgb8_b, const float* img_a, const float* img_b,
              float* dist, float* per_layer, void* const* feats) {
    e.begin_forward_only_pass();
    const int N2 = 2 * n;
    LpipsHeadTaps taps{};
    Ten* x = nullptr;  // the map the next convolution reads (pre-activation)
    for (int i = 0; i < 5; ++i) {
      const LLayer& a = ALEX[i];
      const int Hin = i == 0 ? img_h : x->H, Win = i == 0 ? img_w : x->W;
      const int Ho = lpips_conv_out(Hin, a.k, a.stride, a.pad), Wo = lpips_conv_out(Win, a.k, a.stride, a.pad);
      const int Kp = conv[i].in;
      Ten* pm = e.new_ten((int64_t)N2 * Ho * Wo, Kp, N2, Ho, Wo);
      // (profile classes: the patch matrices count as "conv", the GEMMs as "gemm", pool / taps / head as "elementwise")
      if (i == 0)
        RUNP(SMI_PROF_CONV, 0.0, 2.0 * pm->rows * Kp,
             launch_lpips_stem(e.dtype, rgb8_a, rgb8_b, img_a, img_b, pm->p, n, img_h, img_w, Kp, e.stream));
      else
        RUNP(SMI_PROF_CONV, 0.0, 2.0 * pm->rows * Kp,
             launch_lpips_im2col(e.dtype, x->p, pm->p, N2, Hin, Win, x->cols, a.k, a.stride, a.pad, Kp, e.stream));
      Ten* y = e.linear(pm, conv[i]);
      taps.y[i] = y->p;
      taps.w[i] = lin[i];
      taps.HW[i] = Ho * Wo;
      taps.C[i] = y->cols;
      if (feats && !e.dry)
        RUNP(SMI_PROF_ELEM, 0.0, 4.0 * y->rows * y->cols,
             launch_lpips_relu(e.dtype, y->p, feats[i], y->rows * y->cols, e.stream));
      x = y;
      if (a.pool) {
        const int Hp = lpips_pool_out(Ho), Wp = lpips_pool_out(Wo);
        Ten* pl = e.new_ten((int64_t)N2 * Hp * Wp, y->cols, N2, Hp, Wp);
        RUNP(SMI_PROF_ELEM, 0.0, 2.0 * (y->rows + pl->rows) * y->cols,
             launch_lpips_maxpool(e.dtype, y->p, pl->p, N2, Ho, Wo, y->cols, e.stream));
        x = pl;
      }
    }
    lpips_head_plan(taps);
    float* partial = e.alloc_f32((size_t)n * taps.blk0[5]);
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_lpips_head(e.dtype, taps, n, partial, dist, per_layer, e.stream));
    return e.end_pass("this call (");
  }
};

int check_lpips_cfg(const smi_lpips_config* c, int max_pairs, int h, int w) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(h >= 31 && w >= 31, "LPIPS: image %d x %d is smaller than 31 x 31, the smallest the AlexNet tower takes", h, w);
  SMI_CHECK(max_pairs >= 1 && max_pairs <= 65535, "LPIPS: max_pairs %d outside [1, 65535]", max_pairs);
  for (int i = 0; i < 5; ++i)
    SMI_CHECK(c->channels[i] >= 8 && c->channels[i] % 8 == 0 && c->channels[i] <= 4096,
              "LPIPS config: channels[%d] = %d must be a multiple of 8 in [8, 4096]", i, c->channels[i]);
  // the GEMM addresses each operand with a 32-bit byte offset: the largest patch matrix must stay below 4 GiB
  int H = h, W = w, cin = 3;
  for (int i = 0; i < 5; ++i) {
    H = lpips_conv_out(H, ALEX[i].k, ALEX[i].stride, ALEX[i].pad);
    W = lpips_conv_out(W, ALEX[i].k, ALEX[i].stride, ALEX[i].pad);
    const int64_t rows = (int64_t)2 * max_pairs * H * W;
    const int64_t bytes = rows * std::max(padded_k(ALEX[i].k, cin), c->channels[i]) * 2;
    SMI_CHECK(rows < (1ll << 31) && bytes < 0xFFFFFFF0ll,
              "LPIPS: %d pairs at %d x %d cross the GEMM's 4 GiB operand limit in layer %d (%lld MiB)", max_pairs, h, w,
              i, (long long)(bytes >> 20));
    cin = c->channels[i];
    if (ALEX[i].pool) {
      H = lpips_pool_out(H);
      W = lpips_pool_out(W);
    }
  }
  return 0;
}
Setup lpips_setup(const smi_lpips_config* cfg, int max_pairs, int h, int w) {
  return [=](smi_engine* e) { e->hold(smi_engine::LPIPS, new Lpips(*cfg, h, w), cfg->dtype, max_pairs); };
}

}  // namespace

extern "C" {

int smi_lpips_workspace_bytes(const smi_lpips_config* cfg, int max_pairs, int h, int w, size_t* bytes) {
  if (check_lpips_cfg(cfg, max_pairs, h, w)) return -1;
  return workspace_bytes_forward_only(lpips_setup(cfg, max_pairs, h, w), bytes);
}

int smi_lpips_create(const smi_lpips_config* cfg, const smi_weight* weights, int n_weights, int max_pairs, int h, int w,
                     void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_lpips_cfg(cfg, max_pairs, h, w)) return -1;
  return create_forward_only(lpips_setup(cfg, max_pairs, h, w), "the LPIPS weights", weights, n_weights, workspace,
                             workspace_bytes, stream, out);
}

int smi_lpips_distance(smi_engine* e, int n, const uint8_t* rgb8_a, const uint8_t* rgb8_b, const float* img_a,
                       const float* img_b, float* dist, float* per_layer, void* const* feats) {
  SMI_CHECK(e && e->kind == smi_engine::LPIPS,
            "smi_lpips_distance: NULL or not an LPIPS engine (create it with smi_lpips_create)");
  SMI_CHECK((rgb8_a && rgb8_b && !img_a && !img_b) || (!rgb8_a && !rgb8_b && img_a && img_b),
            "smi_lpips_distance: exactly one input form (rgb8_a and rgb8_b, or img_a and img_b)");
  SMI_CHECK(dist != nullptr, "smi_lpips_distance: dist is NULL");
  SMI_CHECK(n >= 1 && n <= e->max_n, "%d pairs outside [1, %d] the engine was created for", n, e->max_n);
  if (feats)
    for (int i = 0; i < 5; ++i) SMI_CHECK(feats[i] != nullptr, "smi_lpips_distance: feats[%d] is NULL", i);
  e->err = false;
  // launch_gemm splits K only into a scratch of the calling thread's; its slice count follows the launch's row count, so
  // with one lent the bits would depend on the batch.  Every owner sets it per call (the UNet engine, the op tests)
  smi::set_gemm_scratch(nullptr, 0);
  return static_cast<Lpips*>(e->model.get())->forward(*e, n, rgb8_a, rgb8_b, img_a, img_b, dist, per_layer, feats);
}

}  // extern "C"
