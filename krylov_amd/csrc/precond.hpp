// Factorised preconditioners (kry_precond, precond.hip) as the solver cores
// see them: a preconditioner slot M / Ml / Mr holds either a matrix (kry_csr,
// one SpMV with the fused epilogue) or a kry_precond (a short sequence of
// triangular solves and row scales), and apply_prec serves both.
#pragma once

#include <vector>

#include "solver_common.hpp"

struct kry_tri;
struct kry_bjacobi;

// A stage is a triangular solve (tri), a row scale by an (n,) device vector
// of the preconditioner's dtype (scale), or an approximate-inverse solve
// (isai_w): x = W y, then `sweeps` times x = x + W (y - T x), and x = scale * x
// folded into the last product's store when the stage carries a scale. The
// stages are borrowed: the caller keeps the kry_tri / kry_vec / kry_csr
// handles alive while the preconditioner is. A preconditioner holds solves
// and scales or approximate-inverse stages, never both. A block-Jacobi stage
// (bj: one batched block product, bjacobi.hip) is the only stage of its
// preconditioner.
struct kry_precond {
  struct Stage {
    const kry_tri *tri = nullptr;
    const void *scale = nullptr;
    const kry_csr *isai_w = nullptr, *isai_t = nullptr;  // isai_t: null without sweeps
    int sweeps = 0;
    const kry_bjacobi *bj = nullptr;
  };
  kry_ctx *ctx = nullptr;
  int64_t n = 0;
  int dtype = 0;
  std::vector<Stage> stages;
  // An SpMV cannot run in place: the blocks the approximate-inverse stages
  // write between the source and the destination (two that alternate and the
  // residual of a sweep), n x scratch_k each, allocated at the first apply of
  // a k larger than any before.
  mutable void *scratch[3] = {nullptr, nullptr, nullptr};
  mutable int scratch_k = 0;
  ~kry_precond();
  // The fused apply of a multicolour object (kry_precond_fuse; precond.hip
  // fuse_plan), one entry per stage. A scale stage with `folded` set launches
  // nothing: the next solve multiplies its right-hand side by it (`pre`). A
  // solve with `boundary` leaves its last level to one launch that also does
  // the first level of the solve `next` (and the scale `mid` between them),
  // which then starts at its second level (`skip_first`).
  struct Fuse {
    bool folded = false, skip_first = false, boundary = false;
    const void *pre = nullptr, *mid = nullptr;
    const kry_tri *next = nullptr;
  };
  bool fuse_allowed = true;  // KRY_PRECOND_FUSE, read at creation
  bool fused = false;
  std::vector<Fuse> fuse;    // empty: every stage is its own launches
};

namespace kry {

// tri.hip: kry_tri_solve on raw n x k blocks (k a power of two <= 64; x may alias y)
void tri_solve_raw(const kry_tri *T, int k, const void *y, void *x, const Ctrl *ctrl, int step, hipStream_t st);
void tri_shape(const kry_tri *T, int64_t *n, int *dtype);
// tri.hip, for a fused kry_precond. tri_solve_part: the solve without its
// first and / or last level, its right-hand side times the row scale `scale`
// when non-null. tri_boundary_match: T's last level is a launch of its own and
// holds exactly the rows of next's first level, which has no off-diagonal
// entry (both built under an elimination order). tri_boundary: that level of
// both solves, with the row scale between them when non-null, in one launch.
// tri_launches: the launches of tri_solve_part.
void tri_solve_part(const kry_tri *T, int k, const void *y, void *x, const void *scale, bool skip_first,
                    bool skip_last, const Ctrl *ctrl, int step, hipStream_t st);
bool tri_boundary_match(const kry_tri *T, const kry_tri *next);
void tri_boundary(const kry_tri *T, const kry_tri *next, int k, const void *y, void *x, const void *scale,
                  const Ctrl *ctrl, int step, hipStream_t st);
int tri_launches(const kry_tri *T, bool skip_first, bool skip_last);
// bjacobi.hip: y = B x on raw n x k blocks (k a power of two <= kMaxCols; y may alias x)
void bjacobi_apply_raw(const kry_bjacobi *B, int k, const void *x, void *y, const Ctrl *ctrl, int step,
                       hipStream_t st);
void bjacobi_shape(const kry_bjacobi *B, int64_t *n, int *dtype);
// precond.hip: dst = P src, stage by stage (the first stage reads src, the
// others work in place on dst; dst may alias src)
void precond_stages(const kry_precond *P, int k, const void *src, void *dst, const Ctrl *ctrl, int step,
                    hipStream_t st);
// the most columns an apply takes: kMaxCols for approximate-inverse stages
// (SpMVs) and for a block-Jacobi stage, 64 for triangular solves
int precond_max_cols(const kry_precond *P);
// what every set_precond of the cores checks
void precond_check(const kry_precond *P, const kry_csr *A, int64_t n, int k, int dtype);
// what every set_preconditioners of the cores checks of a matrix it is given
void precond_matrix_check(const kry_csr *op, const kry_csr *A, int64_t n, int dtype);

// A preconditioner slot of a solver. It converts to bool like the kry_csr
// pointer it replaces, so `!s->M` and `s->M ? a : b` see both kinds.
struct PrecSlot {
  kry_csr *mat = nullptr;
  const kry_precond *fac = nullptr;
  explicit operator bool() const { return mat != nullptr || fac != nullptr; }
  PrecSlot &operator=(kry_csr *m) {
    mat = m;
    fac = nullptr;
    return *this;
  }
  PrecSlot &operator=(const kry_precond *p) {
    mat = nullptr;
    fac = p;
    return *this;
  }
};

// the inner-product partials a fused epilogue would have written: <q, y>_w
template <typename V>
struct OpPrecDot {
  const V *q, *y;
  const double *w;
  int k;
  __device__ __forceinline__ void operator()(int64_t e, int64_t N, double (&acc)[Vec16<V>::W]) const {
    constexpr int W = Vec16<V>::W;
    V a[W], b[W];
    VIO<V>::load(q, e, N, a);
    VIO<V>::load(y, e, N, b);
#pragma unroll
    for (int v = 0; v < W; ++v)
      if (e + v < N)
        acc[v] += w ? dterm_w((double)a[v], w[(e + v) / k], (double)b[v]) : dterm((double)a[v], (double)b[v]);
  }
};

// out = x0 + out (EpiAddStore's sum)
template <typename V>
struct OpPrecAdd {
  V *out;
  const V *x0;
  __device__ __forceinline__ void operator()(int64_t e, int64_t N, double (&)[Vec16<V>::W]) const {
    constexpr int W = Vec16<V>::W;
    V a[W], b[W];
    VIO<V>::load(x0, e, N, a);
    VIO<V>::load(out, e, N, b);
#pragma unroll
    for (int v = 0; v < W; ++v) b[v] = a[v] + b[v];
    VIO<V>::store(out, e, N, b);
  }
};

// out = out - h0 * pold and <v, out>_w (EpiLanczos on a finished product)
template <typename V>
struct OpPrecLanczos {
  V *out;
  const V *v, *pold;
  const double *h0, *w;
  int k;
  __device__ __forceinline__ void operator()(int64_t e, int64_t N, double (&acc)[Vec16<V>::W]) const {
    constexpr int W = Vec16<V>::W;
    V o[W], vv[W], po[W];
    VIO<V>::load(out, e, N, o);
    VIO<V>::load(v, e, N, vv);
    if (pold) {
      VIO<V>::load(pold, e, N, po);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const V t = (V)h0[(e + c) & (k - 1)] * po[c];
        o[c] = o[c] - t;
      }
      VIO<V>::store(out, e, N, o);
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (e + c < N)
        acc[c] += w ? dterm_w((double)vv[c], w[(e + c) / k], (double)o[c]) : dterm((double)vv[c], (double)o[c]);
  }
};

// The factorised form of each epilogue the cores fuse into a preconditioner
// product: the stages run into the epilogue's destination, then one
// element-wise pass does what the epilogue adds (partials in the layout of
// elementwise_kernel, which the rho / norm kernels already read).
template <typename V>
void prec_factored(const kry_precond *P, int k, const V *src, const EpiStore<V> &epi, double *, int *grid_out,
                   const Ctrl *ctrl, int step, hipStream_t st) {
  precond_stages(P, k, src, epi.y, ctrl, step, st);
  if (grid_out) *grid_out = 0;
}
template <typename V>
void prec_factored(const kry_precond *P, int k, const V *src, const EpiStoreNorm<V> &epi, double *part, int *grid_out,
                   const Ctrl *ctrl, int step, hipStream_t st) {
  precond_stages(P, k, src, epi.y, ctrl, step, st);
  const int g = launch_elementwise<V>(P->n * (int64_t)k, k, OpPrecDot<V>{epi.y, epi.y, epi.w, k}, part, ctrl, step, st);
  if (grid_out) *grid_out = g;
}
template <typename V>
void prec_factored(const kry_precond *P, int k, const V *src, const EpiStoreDot<V> &epi, double *part, int *grid_out,
                   const Ctrl *ctrl, int step, hipStream_t st) {
  KRY_REQUIRE(epi.q != epi.y, KRY_EINVAL, "the factorised preconditioner's destination aliases the dot operand");
  precond_stages(P, k, src, epi.y, ctrl, step, st);
  const int g = launch_elementwise<V>(P->n * (int64_t)k, k, OpPrecDot<V>{epi.q, epi.y, epi.w, k}, part, ctrl, step, st);
  if (grid_out) *grid_out = g;
}
template <typename V>
void prec_factored(const kry_precond *P, int k, const V *src, const EpiAddStore<V> &epi, double *, int *grid_out,
                   const Ctrl *ctrl, int step, hipStream_t st) {
  KRY_REQUIRE(epi.x0 != epi.out, KRY_EINVAL, "the factorised preconditioner's destination aliases x0");
  precond_stages(P, k, src, epi.out, ctrl, step, st);
  if (epi.x0) launch_elementwise<V>(P->n * (int64_t)k, k, OpPrecAdd<V>{epi.out, epi.x0}, nullptr, ctrl, step, st);
  if (grid_out) *grid_out = 0;
}

template <typename V>
void prec_factored(const kry_precond *P, int k, const V *src, const EpiLanczos<V> &epi, double *part, int *grid_out,
                   const Ctrl *ctrl, int step, hipStream_t st) {
  KRY_REQUIRE(epi.v != epi.out && epi.pold != epi.out, KRY_EINVAL,
              "the factorised preconditioner's destination aliases a Lanczos vector");
  precond_stages(P, k, src, epi.out, ctrl, step, st);
  const int g = launch_elementwise<V>(P->n * (int64_t)k, k,
                                      OpPrecLanczos<V>{epi.out, epi.v, epi.pold, epi.h0, epi.w, k}, part, ctrl, step, st);
  if (grid_out) *grid_out = g;
}

// Every preconditioner product of the cores: a matrix slot makes exactly the
// SpMV call it always made, a factorised one runs its stages.
template <typename V, class Epi>
void apply_prec(const PrecSlot &S, int k, SrcPlain<V> src, Epi epi, double *part, int *grid_out, const Ctrl *ctrl,
                int step, hipStream_t st) {
  if (S.fac) return prec_factored<V>(S.fac, k, src.x, epi, part, grid_out, ctrl, step, st);
  launch_spmv_any<V>(S.mat, k, src, epi, part, grid_out, ctrl, step, st);
}

}  // namespace kry
