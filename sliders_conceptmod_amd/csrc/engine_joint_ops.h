// The ops a joint-stream transformer adds to the op core (engine.h), shared by the SD3 MMDiT (engine_mmdit.hip) and the Flux
// transformer (engine_flux.hip): each allocates its output, launches one kernel of mmdit.hip and, in a saved pass, pushes its
// backward on the tape when its output depends on an adapted layer.  The modulation tensors depend on temb alone: they take
// no gradient.
#pragma once
#include "engine.h"

inline const void* mod_row(const smi_engine& e, const Ten* mod, const Ten* x) {  // mod's row of x's first adapted sample
  return (const char*)mod->p + (size_t)(x->n > 0 ? x->arow0 / (x->rows / x->n) : 0) * mod->cols * e.esz();
}

// ---- ops --------------------------------------------------------------------------------------------------------------
// LN(x) (1 + scale) + shift with scale / shift at columns off_scale / off_shift of mod [n, *]; rows / n rows per sample.
// mean_rstd is kept next to the output: the backward's input
inline Ten* adaln(smi_engine& e, Ten* x, Ten* mod, int off_scale, int off_shift) {
  Ten* y = e.new_ten(x->rows, x->cols, x->n, x->H, x->W);
  float* st = e.alloc_f32((size_t)x->rows * 2);
  RUNP(SMI_PROF_NORM, 0.0, 4.0 * x->rows * x->cols,
       launch_adaln_modulate(e.dtype, x->p, mod->p, y->p, st, (int)x->rows, x->cols, (int)(x->rows / x->n), mod->cols, off_scale,
                             off_shift, 1e-6f, e.stream));
  y->ng = x->ng;
  if (e.saving && y->ng) {
    smi_engine* ep = &e;
    e.tape.push_back([=]() {
      smi_engine& e = *ep;
      if (!y->g) return;
      // the stream's residual gradient, when it is already in x's slot, rides in the same launch (add may equal dx)
      const smi_engine::Slot gs = e.grad_slot(x);
      RUNP(SMI_PROF_NORM, 0.0, 6.0 * e.MA(x) * x->cols,
           launch_adaln_modulate_bwd(e.dtype, e.PA(x), y->g, mod_row(e, mod, x), st + x->arow0 * 2, gs.add, gs.out, (int)e.MA(x),
                                     x->cols, (int)(x->rows / x->n), mod->cols, off_scale, e.stream));
    });
  }
  return y;
}
// h + gate f, gate at column off_gate of mod
inline Ten* gate_residual(smi_engine& e, Ten* h, Ten* f, Ten* mod, int off_gate) {
  Ten* y = e.new_ten(h->rows, h->cols, h->n, h->H, h->W);
  RUNP(SMI_PROF_ELEM, 0.0, 6.0 * h->rows * h->cols,
       launch_gate_residual(e.dtype, h->p, f->p, mod->p, y->p, h->rows, h->cols, (int)(h->rows / h->n), mod->cols, off_gate,
                            e.stream));
  y->ng = h->ng || f->ng;
  if (e.saving && y->ng) {
    smi_engine* ep = &e;
    e.tape.push_back([=]() {
      smi_engine& e = *ep;
      if (!y->g) return;
      if (f->ng)
        e.into_slot(e.grad_slot(f), e.MA(f), f->cols, [&](void* df) {
          RUNP(SMI_PROF_ELEM, 0.0, 4.0 * e.MA(f) * f->cols,
               launch_gate_residual_bwd(e.dtype, y->g, mod_row(e, mod, f), df, e.MA(f), f->cols, (int)(f->rows / f->n), mod->cols,
                                        off_gate, e.stream));
        });
      if (h->ng) e.accumulate(h, y->g);  // dh is dy itself
    });
  }
  return y;
}
// per sample the rows of a (image stream), then the rows of b (context stream)
inline Ten* joint_pack(smi_engine& e, Ten* a, Ten* b) {
  const int n = a->n, Nx = (int)(a->rows / n), Nc = (int)(b->rows / n);
  Ten* j = e.new_ten(a->rows + b->rows, a->cols, n, Nx + Nc, 1);
  RUNP(SMI_PROF_ELEM, 0.0, 4.0 * j->rows * j->cols, launch_joint_rows_pack(e.dtype, a->p, b->p, j->p, n, Nx, Nc, a->cols, e.stream));
  j->ng = a->ng || b->ng;
  if (e.saving && j->ng) {
    smi_engine* ep = &e;
    e.tape.push_back([=]() {  // the split of the gradient; a and b have this one consumer: their slots are fresh
      smi_engine& e = *ep;
      if (!j->g) return;
      const int n0 = e.ad_first(j, Nx + Nc);
      void* ga = a->ng ? e.grad_slot(a).out : nullptr;  // (outside the launch macro: a dry run allocates them too)
      void* gb = b->ng ? e.grad_slot(b).out : nullptr;
      RUNP(SMI_PROF_ELEM, 0.0, 4.0 * e.MA(j) * j->cols,
           launch_joint_rows_split(e.dtype, j->g, ga, gb, n - n0, Nx, Nc, j->cols, e.stream));
    });
  }
  return j;
}
// the inverse; want_b false: the context rows are dropped (the last block)
inline void joint_split(smi_engine& e, Ten* j, int Nx, int Nc, Ten** a, Ten** b, bool want_b) {
  const int n = j->n;
  *a = e.new_ten((int64_t)n * Nx, j->cols, n, Nx, 1);
  *b = want_b ? e.new_ten((int64_t)n * Nc, j->cols, n, Nc, 1) : nullptr;
  RUNP(SMI_PROF_ELEM, 0.0, 4.0 * j->rows * j->cols,
       launch_joint_rows_split(e.dtype, j->p, (*a)->p, want_b ? (*b)->p : nullptr, n, Nx, Nc, j->cols, e.stream));
  (*a)->ng = j->ng;
  if (*b) (*b)->ng = j->ng;
  if (e.saving && j->ng) {
    smi_engine* ep = &e;
    Ten *ta = *a, *tb = *b;
    e.tape.push_back([=]() {  // the pack of the two gradients; a stream that was dropped, or that no gradient reached, packs zeros
      smi_engine& e = *ep;
      if (!ta->g && !(tb && tb->g)) return;
      const int n0 = e.ad_first(j, Nx + Nc);
      auto grad_or_zero = [&](Ten* t, int rows) -> void* {
        if (t && t->g) return t->g;
        void* z = e.alloc_t((int64_t)(n - n0) * rows, j->cols);
        if (!e.dry && !e.err) (void)hipMemsetAsync(z, 0, (size_t)(n - n0) * rows * j->cols * e.esz(), e.stream);
        return z;
      };
      void* ga = grad_or_zero(ta, Nx);
      void* gb = grad_or_zero(tb, Nc);
      e.into_slot(e.grad_slot(j), e.MA(j), j->cols, [&](void* dj) {
        RUNP(SMI_PROF_ELEM, 0.0, 4.0 * e.MA(j) * j->cols, launch_joint_rows_pack(e.dtype, ga, gb, dj, n - n0, Nx, Nc, j->cols, e.stream));
      });
    });
  }
}
