// Host side shared by the CG / GMRES / MINRES cores: the fields every core
// starts with (SolverCore), the argument checks and buffer rules of their
// create / start / set_criterion / attach_comm / set_preconditioners /
// set_precond entry points, the sharded step tail with its global-check
// kernel, and the operator and residual products. solver_common.hpp stays
// the device-helper header. A core derives its struct from SolverCore, keeps
// its kernels, run loop and extern "C" functions in its own .hip, and states
// which scratch buffers each of its preconditioner slots needs (SlotDesc).
#pragma once

#include "precond.hpp"
#include "solver_common.hpp"

namespace kry {

struct SolverCore {
  kry_ctx *ctx = nullptr;
  kry_csr *A = nullptr;
  int64_t n = 0;
  int k = 1;
  int dtype = 0;
  void *b = nullptr, *x0 = nullptr, *xk = nullptr, *rt = nullptr;
  double *w = nullptr;     // inner-product weights (null = Euclidean)
  double *part = nullptr;  // reduction partials
  double *scal = nullptr;  // scalar slots (x k each), the core's own enum
  double *hist = nullptr;  // chunk_cap x hist_cols
  Ctrl *ctrl = nullptr;
  int chunk_cap = 0;
  bool started = false;
  // RHS sharding (attach_comm): this solver's k columns are global columns
  // [col_offset, col_offset + k) of total_k; every step allreduces gbuf
  kry_comm *comm = nullptr;
  int col_offset = 0, total_k = 0;
  double *gbuf = nullptr;   // total_k norms, [the non-invariant count,] the fault count
  double *gcrit = nullptr;  // total_k
};

// elements / bytes of one n x k vector, padded to whole 16-element groups
inline size_t vec_elems(const SolverCore *s) { return padded_elems(s->n, s->k); }
inline size_t vec_bytes(const SolverCore *s) { return vec_elems(s) * dsize(s->dtype); }
// columns of a history row
inline int hist_cols(const SolverCore *s) { return s->comm ? s->total_k : s->k; }

inline void *alloc_zeroed(size_t bytes, hipStream_t st) {
  void *p = dev_alloc(bytes);
  KRY_HIP(hipMemsetAsync(p, 0, bytes, st));
  return p;
}

// --------------------------------------------------------------- create
inline void check_create(const kry_ctx *ctx, const kry_csr *A, const void *out, int k, int dtype) {
  KRY_REQUIRE(ctx && A && out, KRY_EINVAL, "null argument");
  KRY_REQUIRE(is_pow2(k) && k <= kMaxCols, KRY_EUNSUPPORTED, "k must be a power of two <= 256");
  KRY_REQUIRE(dtype == A->dtype || (dtype == KRY_F64 && A->dtype == KRY_F32), KRY_EINVAL,
              "vectors must have the operator dtype (or float64 over a float32 operator)");
}

inline void init_core(SolverCore *s, kry_ctx *ctx, kry_csr *A, int k, int dtype) {
  s->ctx = ctx;
  s->A = A;
  s->n = A->n;
  s->k = k;
  s->dtype = dtype;
}

// ---------------------------------------------------------------- start
inline void check_start(const SolverCore *s, const kry_vec *b, const kry_vec *x0, const kry_vec *w) {
  check_vec(b, s->n, s->k, s->dtype, "b");
  if (x0) check_vec(x0, s->n, s->k, s->dtype, "x0");
  check_weights(w, s->n);
}

// b, x0 and the weights arrive in the caller's numbering (load_in: into a
// renumbered operator's, a plain copy otherwise); x0 and w are reallocated,
// null when absent. Returns the solver's stream, its device current.
inline hipStream_t load_start(SolverCore *s, const kry_vec *b, const kry_vec *x0, const kry_vec *w) {
  KRY_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  load_in(s->A, b->d, s->b, s->k, dsize(s->dtype), st);
  dev_free(s->x0);
  s->x0 = nullptr;
  if (x0) {
    s->x0 = dev_alloc(vec_bytes(s));
    load_in(s->A, x0->d, s->x0, s->k, dsize(s->dtype), st);
  }
  dev_free(s->w);
  s->w = nullptr;
  if (w) {
    s->w = static_cast<double *>(dev_alloc(((size_t)s->n + 1) * 8));
    load_in(s->A, w->d, s->w, 1, 8, st);
  }
  return st;
}

// ------------------------------------------------------------- criterion
// crit_slot: the core's scalar slot; under a communicator all total_k
// columns, in rank order
inline void set_criterion(SolverCore *s, const double *criterion, int crit_slot) {
  KRY_REQUIRE(s && criterion, KRY_EINVAL, "null argument");
  hipStream_t st = s->ctx->stream;
  if (s->comm)
    KRY_HIP(hipMemcpyAsync(s->gcrit, criterion, s->total_k * 8, hipMemcpyHostToDevice, st));
  else
    KRY_HIP(hipMemcpyAsync(s->scal + crit_slot * s->k, criterion, s->k * 8, hipMemcpyHostToDevice, st));
  KRY_HIP(hipStreamSynchronize(st));
}

// -------------------------------------------------------------- sharding
// extra_slots: what gbuf carries past the total_k norms (1: the fault count;
// 2: the non-invariant count before it). unsupported: the core's reason to
// refuse, if it has one.
inline void attach_comm(SolverCore *s, kry_comm *c, int col_offset, int total_k, int extra_slots,
                        const char *unsupported = nullptr) {
  KRY_REQUIRE(s && c, KRY_EINVAL, "null argument");
  KRY_REQUIRE(col_offset >= 0 && total_k >= col_offset + s->k && total_k <= 4096, KRY_EINVAL, "bad column range");
  KRY_REQUIRE(!unsupported, KRY_EUNSUPPORTED, unsupported);
  KRY_HIP(hipSetDevice(s->ctx->device));
  dev_free(s->gbuf);
  dev_free(s->gcrit);
  s->gbuf = nullptr;
  s->gcrit = nullptr;
  s->gbuf = static_cast<double *>(dev_alloc(((size_t)total_k + extra_slots) * 8));
  s->gcrit = static_cast<double *>(dev_alloc((size_t)total_k * 8));
  dev_free(s->hist);
  s->hist = nullptr;
  s->hist = static_cast<double *>(dev_alloc((size_t)(s->chunk_cap > 0 ? s->chunk_cap : 1) * total_k * 8));
  s->comm = c;
  s->col_offset = col_offset;
  s->total_k = total_k;
}

// a run call longer than any before it: a larger history
inline void grow_hist(SolverCore *s, int max_steps) {
  if (max_steps <= s->chunk_cap) return;
  dev_free(s->hist);
  s->hist = nullptr;
  s->hist = static_cast<double *>(dev_alloc((size_t)max_steps * hist_cols(s) * 8));
  s->chunk_cap = max_steps;
}

// Sharded global step decision on the allreduced vector: the history row and
// the stop rule over ALL columns of all ranks; INV: slot total_k counts the
// ranks with a non-invariant column (none left = the Krylov space is
// invariant, arnoldi.py:187, 270-272). The last slot is the fault count
// (post_fault).
template <bool INV>
__global__ void global_check_kernel(const double *gbuf, const double *gcrit, int total_k, double *hist, Ctrl *ctrl,
                                    int step) {
  if (halted(ctrl, step)) return;
  if (peer_fault(gbuf, total_k + (INV ? 2 : 1), ctrl, step)) return;
  __shared__ int flag;
  for (int t = threadIdx.x; t < total_k; t += blockDim.x) hist[(int64_t)step * total_k + t] = gbuf[t];
  const bool inv = INV && gbuf[total_k] == 0.0;
  const bool conv = all_le(gbuf, gcrit, total_k, &flag);
  if (threadIdx.x == 0) {
    if (inv) ctrl->invariant = 1;
    if (inv || conv) ctrl->stop_at = step + 1;
  }
}

// The tail of a sharded step, after the kernel that posted this rank's share
// of gbuf: exactly one collective per iteration, then the one-block decision.
template <bool INV>
void global_step(SolverCore *s, int step) {
  hipStream_t st = s->ctx->stream;
  const int nslots = s->total_k + (INV ? 2 : 1);
  inject_peer_fault(s->gbuf, nslots, step, st);
  comm_allreduce(s->comm, s->gbuf, nslots, st);
  hipLaunchKernelGGL(global_check_kernel<INV>, dim3(1), dim3(kBlock), 0, st, (const double *)s->gbuf,
                     (const double *)s->gcrit, s->total_k, s->hist, s->ctrl, step);
  KRY_HIP(hipGetLastError());
}

// ------------------------------------------------------- preconditioners
// One preconditioner slot of a core and the scratch buffers it needs while
// it is filled (allocated zero-filled on first use, kept afterwards).
struct SlotDesc {
  PrecSlot *slot;
  struct {
    void **buf;
    size_t bytes;
  } need[3];
};

template <class Op>  // kry_csr * (null = identity) or const kry_precond *
void install_slot(SolverCore *s, const SlotDesc &d, Op op) {
  if (op)
    for (const auto &nd : d.need)
      if (nd.buf && !*nd.buf) *nd.buf = alloc_zeroed(nd.bytes, s->ctx->stream);
  *d.slot = op;
}

template <int NS>
void check_matrices(const SolverCore *s, kry_csr *const (&ops)[NS]) {
  for (const kry_csr *op : ops)
    if (op) precond_matrix_check(op, s->A, s->n, s->dtype);
}

// kry_*_set_preconditioners after its checks: every slot is assigned, so a
// null matrix also clears a factorised preconditioner; needs a new start.
template <int NS, class SlotOf>
void install_matrices(SolverCore *s, kry_csr *const (&ops)[NS], SlotOf slot_of) {
  KRY_HIP(hipSetDevice(s->ctx->device));
  for (int i = 0; i < NS; ++i) install_slot(s, slot_of(i), ops[i]);
  KRY_HIP(hipStreamSynchronize(s->ctx->stream));
  s->started = false;
}

// kry_*_set_precond: slot 0 = M, 1 = Ml[, 2 = Mr] takes a factorised
// preconditioner in place of its matrix
inline void check_factored(const SolverCore *s, int slot, int nslots, const kry_precond *P) {
  KRY_REQUIRE(s && P, KRY_EINVAL, "null argument");
  KRY_REQUIRE(slot >= 0 && slot < nslots, KRY_EINVAL,
              nslots == 2 ? "slot must be 0 (M) or 1 (Ml)" : "slot must be 0 (M), 1 (Ml) or 2 (Mr)");
  precond_check(P, s->A, s->n, s->k, s->dtype);
  KRY_REQUIRE(!s->comm, KRY_EUNSUPPORTED, "factorised preconditioners do not run on sharded solves");
}

inline void install_factored(SolverCore *s, const SlotDesc &d, const kry_precond *P) {
  KRY_HIP(hipSetDevice(s->ctx->device));
  install_slot(s, d, P);
  KRY_HIP(hipStreamSynchronize(s->ctx->stream));
  s->started = false;
}

// ------------------------------------------------- operator and residual
// w = Ml (A (Mr v)) (Product(Ml, A, Mr), gmres.py:139, minres.py:151), `epi`
// on the last product; the solver's t1 holds Mr v, t2 holds A Mr v.
template <typename V, typename MV, typename I, class Solver, class Epi>
void apply_op(Solver *s, const V *v, Epi epi, double *part, int *P, const Ctrl *ctrl, int step) {
  hipStream_t st = s->ctx->stream;
  const int k = s->k;
  const V *src = v;
  if (s->Mr) {
    V *t1 = static_cast<V *>(s->t1);
    apply_prec<V>(s->Mr, k, SrcPlain<V>{v, k}, EpiStore<V>{t1, k}, nullptr, nullptr, ctrl, step, st);
    src = t1;
  }
  if (s->Ml) {
    V *t2 = static_cast<V *>(s->t2);
    launch_spmv<V, MV, I>(s->A, k, SrcPlain<V>{src, k}, EpiStore<V>{t2, k}, nullptr, nullptr, ctrl, step, st);
    apply_prec<V>(s->Ml, k, SrcPlain<V>{t2, k}, epi, part, P, ctrl, step, st);
  } else {
    launch_spmv<V, MV, I>(s->A, k, SrcPlain<V>{src, k}, epi, part, P, ctrl, step, st);
  }
}

// Ml (b - A z) -> mlr, M Ml (b - A z) -> mz (with M), and the partials of
// <Ml r, M Ml r> (cg.py:70-90, gmres.py:111-118, minres.py:105-118, 131-136);
// returns the partial count. raw: where b - A z goes under Ml.
template <typename V, typename MV, typename I>
int residual_chain(SolverCore *s, const PrecSlot &Ml, const PrecSlot &M, const V *z, V *raw, V *mlr, V *mz) {
  hipStream_t st = s->ctx->stream;
  const int k = s->k;
  int P = 0;
  if (!Ml) raw = mlr;
  launch_spmv<V, MV, I>(s->A, k, SrcPlain<V>{z, k}, EpiResidual<V>{static_cast<const V *>(s->b), raw, s->w, k},
                        s->part, &P, nullptr, 0, st);
  if (Ml) apply_prec<V>(Ml, k, SrcPlain<V>{raw, k}, EpiStoreNorm<V>{mlr, s->w, k}, s->part, &P, nullptr, 0, st);
  if (M) apply_prec<V>(M, k, SrcPlain<V>{mlr, k}, EpiStoreDot<V>{mz, mlr, s->w, k}, s->part, &P, nullptr, 0, st);
  return P;
}

// the end of kry_*_residual: the chain's P partial rows summed into the
// core's scratch scalar slot, then out to the host
inline void residual_out(SolverCore *s, int P, int tmp_slot, double *norm2) {
  hipStream_t st = s->ctx->stream;
  double *out = s->scal + tmp_slot * s->k;
  hipLaunchKernelGGL(reduce_to_kernel<0>, dim3(1), dim3(kBlock), 0, st, s->part, P, s->k, out);
  KRY_HIP(hipGetLastError());
  KRY_HIP(hipMemcpyAsync(norm2, out, s->k * 8, hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
}

}  // namespace kry
