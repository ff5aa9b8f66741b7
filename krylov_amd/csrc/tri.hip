// Device sparse triangular solve x = T^-1 y (kry_tri): the hot path of the
// reference's gauss_seidel / sor / ssor (scipy spsolve_triangular,
// stationary.py:26-94; krylov_amd/stationary.py).
//
// The host analysis (host_image.hpp tri_plan) sorts the rows by dependency
// level and cuts every level into SELL-64-style slices that never straddle a
// level. Work item (slice s, row lane r, column c) computes
//   x[row, c] = (y[row, c] - sum_j T[row, j] x[j, c]) / T[row, row]
// with the sum taken one term at a time in the row's stored (ascending
// column) order and a true division, no FMA: the result depends on neither
// the launch plan, the grid nor k. Items are numbered with the k columns of a
// row on adjacent lanes; lane groups read consecutive slots of a slot column.
//
// Launches (TriPlan::launch): a run of consecutive levels that fits one
// workgroup is one launch of one workgroup with a workgroup barrier between
// its levels (the values cross levels through global memory: same CU,
// workgroup scope); a larger level is one launch over many workgroups. No
// kernel waits on another workgroup: stream order is the only cross-workgroup
// dependency.
//
// Under an elimination order (kry_tri_create_ordered) the plan and image are
// those of the explicitly permuted triangle, kept in the caller's numbering:
// the kernels are the same. For a multicolour kry_precond (precond.hip) two
// more forms exist, both bitwise the separate launches they replace:
//  - a solve that takes its right-hand side times a row scale,
//    num = (y * s[row]) - acc (the product rounded first), which saves the
//    scale pass in front of it;
//  - tri_boundary_kernel: the last level of one solve and the first level of
//    the next over the same rows, where the next solve has no off-diagonal
//    entry: t = (y - acc) / d1, u = t * s (with a scale between), z = u / d2.
#include "host_image.hpp"
#include "precond.hpp"
#include "prog.hpp"

using namespace kry;

struct kry_tri {
  kry_ctx *ctx = nullptr;
  int64_t n = 0, nnz = 0;
  int dtype = 0;
  bool lower = true;
  int64_t nlevels = 0, nslices = 0, nslots = 0, max_level_rows = 0;
  std::vector<int32_t> launch;  // level boundaries of the launches
  std::vector<int32_t> lslice;  // host copy (grid sizes)
  void *d_lslice = nullptr;     // int32, nlevels + 1
  void *d_sptr = nullptr;       // int64, nslices + 1
  void *d_swidth = nullptr;     // int32, nslices
  void *d_rows = nullptr;       // int32, 64 nslices (+1), -1 = padding
  void *d_diag = nullptr;       // dtype, 64 nslices (+1)
  void *d_col = nullptr;        // int32, nslots (+1), -1 = padding
  void *d_val = nullptr;        // dtype, nslots (+1)
  size_t image_bytes = 0;
  // under an elimination order: the rows of the first and of the last level
  // (host copies, for kry_precond's boundary fusion) and whether the first
  // level has no off-diagonal entry
  bool ordered = false, first_bare = false;
  std::vector<int32_t> first_rows, last_rows;
};

namespace {

template <typename V>
struct TriImg {
  const int32_t *lslice;
  const int64_t *sptr;
  const int32_t *swidth;
  const int32_t *rows;
  const V *diag;
  const int32_t *col;
  const V *val;
};

// one work item: row lane r of slice s, column c. x is read at rows of lower
// levels only (written by earlier launches, or before the last barrier).
// S: the right-hand side is y * sc[row], rounded before the subtraction.
template <typename V, bool S = false>
__device__ __forceinline__ void tri_item(const TriImg<V> &T, int64_t s, int r, int c, int kshift, const V *y, V *x,
                                         const V *sc = nullptr) {
  const int32_t row = T.rows[s * kSlice + r];
  if (row < 0) return;
  const int w = T.swidth[s];
  const int64_t base = T.sptr[s] + r;
  V acc = V(0);
  for (int j = 0; j < w; ++j) {
    const int32_t col = T.col[base + (int64_t)j * kSlice];
    if (col >= 0) {
      const V p = T.val[base + (int64_t)j * kSlice] * x[((int64_t)col << kshift) + c];
      acc = acc + p;
    }
  }
  const int64_t o = ((int64_t)row << kshift) + c;
  V rhs = y[o];
  if constexpr (S) rhs = rhs * sc[row];
  const V num = rhs - acc;
  x[o] = num / T.diag[s * kSlice + r];
}

// a level of its own: slices [s0, s1) over the grid
template <typename V, bool S = false>
__global__ __launch_bounds__(kBlock) void tri_level_kernel(TriImg<V> T, int s0, int s1, int kshift, const V *y, V *x,
                                                           const Ctrl *ctrl, int step, const V *sc = nullptr) {
  if (halted(ctrl, step)) return;
  const int64_t items = ((int64_t)(s1 - s0) * kSlice) << kshift;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= items) return;
  const int c = (int)(t & ((1 << kshift) - 1));
  const int64_t q = t >> kshift;
  tri_item<V, S>(T, s0 + (q >> 6), (int)(q & 63), c, kshift, y, x, sc);
}

// levels [l0, l1) in one workgroup, a barrier between them
template <typename V, bool S = false>
__global__ __launch_bounds__(kBlock) void tri_group_kernel(TriImg<V> T, int l0, int l1, int kshift, const V *y, V *x,
                                                           const Ctrl *ctrl, int step, const V *sc = nullptr) {
  if (halted(ctrl, step)) return;
  for (int l = l0; l < l1; ++l) {
    const int s0 = T.lslice[l], s1 = T.lslice[l + 1];
    const int64_t items = ((int64_t)(s1 - s0) * kSlice) << kshift;
    for (int64_t t = threadIdx.x; t < items; t += kBlock) {
      const int c = (int)(t & ((1 << kshift) - 1));
      const int64_t q = t >> kshift;
      tri_item<V, S>(T, s0 + (q >> 6), (int)(q & 63), c, kshift, y, x, sc);
    }
    if (l + 1 < l1) {
      __threadfence_block();
      __syncthreads();
    }
  }
}

// The last level of T over the grid, then the same rows as the first level of
// the next solve, which has no off-diagonal entry there: slice s0 + i of T
// holds the rows of slice i of the next image, whose diagonals are d2.
template <typename V, bool S>
__global__ __launch_bounds__(kBlock) void tri_boundary_kernel(TriImg<V> T, int s0, int s1, int kshift, const V *y, V *x,
                                                              const V *sc, const V *d2, const Ctrl *ctrl, int step) {
  if (halted(ctrl, step)) return;
  const int64_t items = ((int64_t)(s1 - s0) * kSlice) << kshift;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= items) return;
  const int c = (int)(t & ((1 << kshift) - 1));
  const int64_t q = t >> kshift;
  const int64_t s = s0 + (q >> 6);
  const int r = (int)(q & 63);
  const int32_t row = T.rows[s * kSlice + r];
  if (row < 0) return;
  const int w = T.swidth[s];
  const int64_t base = T.sptr[s] + r;
  V acc = V(0);
  for (int j = 0; j < w; ++j) {
    const int32_t col = T.col[base + (int64_t)j * kSlice];
    if (col >= 0) {
      const V p = T.val[base + (int64_t)j * kSlice] * x[((int64_t)col << kshift) + c];
      acc = acc + p;
    }
  }
  const int64_t o = ((int64_t)row << kshift) + c;
  const V num = y[o] - acc;
  V u = num / T.diag[s * kSlice + r];
  if constexpr (S) u = u * sc[row];
  x[o] = u / d2[(q >> 6) * kSlice + r];
}

template <typename V>
TriImg<V> tri_img(const kry_tri *T) {
  return TriImg<V>{static_cast<const int32_t *>(T->d_lslice), static_cast<const int64_t *>(T->d_sptr),
                   static_cast<const int32_t *>(T->d_swidth), static_cast<const int32_t *>(T->d_rows),
                   static_cast<const V *>(T->d_diag),         static_cast<const int32_t *>(T->d_col),
                   static_cast<const V *>(T->d_val)};
}

int64_t level_grid(const kry_tri *T, int l0, int l1, int ks) {
  const int64_t rows = (int64_t)(T->lslice[(size_t)l1] - T->lslice[(size_t)l0]) * kSlice;
  const int64_t grid = ((rows << ks) + kBlock - 1) / kBlock;
  KRY_REQUIRE(grid < (int64_t(1) << 31), KRY_EUNSUPPORTED, "a triangular level beyond the grid limit");
  return grid;
}

// Levels [first, last) of the solve (all of them for kry_tri_solve; a fused
// kry_precond leaves a boundary level to tri_boundary). A launch of the plan
// cut by `first` keeps its kind: a group stays one workgroup.
template <typename V, bool S = false>
void tri_launch(const kry_tri *T, const kry_vec *y, kry_vec *x, const Ctrl *ctrl, int step, hipStream_t st,
                const V *sc = nullptr, int first = 0, int last = INT32_MAX) {
  int ks = 0;
  while ((1 << ks) < x->k) ++ks;
  const TriImg<V> img = tri_img<V>(T);
  const V *yd = static_cast<const V *>(y->d);
  V *xd = static_cast<V *>(x->d);
  for (size_t q = 0; q + 1 < T->launch.size(); ++q) {
    const int l0 = std::max(T->launch[q], first), l1 = std::min(T->launch[q + 1], last);
    if (l0 >= l1) continue;
    const int64_t rows = (int64_t)(T->lslice[(size_t)l1] - T->lslice[(size_t)l0]) * kSlice;
    if (l1 == l0 + 1 && rows > kTriGroupRows) {
      const int64_t grid = level_grid(T, l0, l1, ks);
      hipLaunchKernelGGL((tri_level_kernel<V, S>), dim3((unsigned)grid), dim3(kBlock), 0, st, img,
                         T->lslice[(size_t)l0], T->lslice[(size_t)l1], ks, yd, xd, ctrl, step, sc);
    } else {
      hipLaunchKernelGGL((tri_group_kernel<V, S>), dim3(1), dim3(kBlock), 0, st, img, l0, l1, ks, yd, xd, ctrl, step,
                         sc);
    }
  }
  KRY_HIP(hipGetLastError());
}

template <typename V>
void boundary_launch(const kry_tri *T, const kry_tri *next, int k, const void *y, void *x, const void *sc,
                     const Ctrl *ctrl, int step, hipStream_t st) {
  int ks = 0;
  while ((1 << ks) < k) ++ks;
  const int l0 = (int)T->nlevels - 1, l1 = (int)T->nlevels;
  const int64_t grid = level_grid(T, l0, l1, ks);
  const V *d2 = static_cast<const V *>(next->d_diag);
  if (sc)
    hipLaunchKernelGGL((tri_boundary_kernel<V, true>), dim3((unsigned)grid), dim3(kBlock), 0, st, tri_img<V>(T),
                       T->lslice[(size_t)l0], T->lslice[(size_t)l1], ks, static_cast<const V *>(y),
                       static_cast<V *>(x), static_cast<const V *>(sc), d2, ctrl, step);
  else
    hipLaunchKernelGGL((tri_boundary_kernel<V, false>), dim3((unsigned)grid), dim3(kBlock), 0, st, tri_img<V>(T),
                       T->lslice[(size_t)l0], T->lslice[(size_t)l1], ks, static_cast<const V *>(y),
                       static_cast<V *>(x), static_cast<const V *>(nullptr), d2, ctrl, step);
  KRY_HIP(hipGetLastError());
}

void tri_check(const kry_tri *T, const kry_vec *y, const kry_vec *x) {
  KRY_REQUIRE(T && y && x, KRY_EINVAL, "null argument");
  KRY_REQUIRE(y->n == T->n && x->n == T->n && x->k == y->k && x->dtype == T->dtype && y->dtype == T->dtype, KRY_EINVAL,
              "shape/dtype mismatch with the triangular operator");
  KRY_REQUIRE(is_pow2(x->k) && x->k <= 64, KRY_EUNSUPPORTED, "the triangular solve handles up to 64 columns");
}

void tri_free(kry_tri *T) {
  for (void *b : {T->d_lslice, T->d_sptr, T->d_swidth, T->d_rows, T->d_diag, T->d_col, T->d_val}) dev_free(b);
}

template <typename T>
void *upload(const T *h, size_t count, hipStream_t st, size_t *total) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  void *d = dev_alloc(bytes);
  if (count) KRY_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, st));
  *total += count * sizeof(T);
  return d;
}

template <typename I, typename V>
void tri_build(kry_tri *T, int64_t n, int64_t nnz, const I *ip, const I *ix, const V *dv, const int32_t *rank) {
  TriPlan p;
  tri_plan(n, nnz, ip, ix, T->lower, p, rank);
  hvec<int32_t> rows, col;
  hvec<V> diag, val;
  tri_fill(p, ip, ix, dv, rows, diag, col, val);
  T->nlevels = p.nlevels;
  T->nslices = p.nslices;
  T->nslots = p.nslots;
  T->max_level_rows = p.max_level_rows;
  T->launch = p.launch;
  T->lslice = p.lslice;
  T->ordered = rank != nullptr;
  if (rank && p.nlevels) {
    const size_t nl = (size_t)p.nlevels;
    T->first_rows.assign(p.order.begin(), p.order.begin() + p.lrow[1]);
    T->last_rows.assign(p.order.begin() + p.lrow[nl - 1], p.order.end());
    T->first_bare = true;
    for (int32_t q = p.lslice[0]; q < p.lslice[1]; ++q) T->first_bare = T->first_bare && p.swidth[(size_t)q] == 0;
  }
  hipStream_t st = T->ctx->stream;
  size_t tot = 0;
  T->d_lslice = upload(p.lslice.data(), p.lslice.size(), st, &tot);
  T->d_sptr = upload(p.sptr.data(), p.sptr.size(), st, &tot);
  T->d_swidth = upload(p.swidth.data(), p.swidth.size(), st, &tot);
  T->d_rows = upload(rows.data(), rows.size(), st, &tot);
  T->d_diag = upload(diag.data(), diag.size(), st, &tot);
  T->d_col = upload(col.data(), col.size(), st, &tot);
  T->d_val = upload(val.data(), val.size(), st, &tot);
  T->image_bytes = tot;
  KRY_HIP(hipStreamSynchronize(st));
}

}  // namespace

namespace kry {

// the solve on raw n x k blocks of a solver core or a kry_precond stage (precond.hpp)
void tri_solve_raw(const kry_tri *T, int k, const void *y, void *x, const Ctrl *ctrl, int step, hipStream_t st) {
  kry_vec yv, xv;
  yv.n = xv.n = T->n;
  yv.k = xv.k = k;
  yv.dtype = xv.dtype = T->dtype;
  yv.d = const_cast<void *>(y);
  xv.d = x;
  tri_check(T, &yv, &xv);
  if (T->dtype == KRY_F64) tri_launch<double>(T, &yv, &xv, ctrl, step, st);
  else tri_launch<float>(T, &yv, &xv, ctrl, step, st);
}

bool tri_boundary_match(const kry_tri *T, const kry_tri *next) {
  return T->ordered && next->ordered && T->n == next->n && T->dtype == next->dtype && T->nlevels >= 1 &&
         next->nlevels >= 1 && T->launch[T->launch.size() - 2] == (int32_t)T->nlevels - 1 && next->first_bare &&
         T->last_rows == next->first_rows;
}

int tri_launches(const kry_tri *T, bool skip_first, bool skip_last) {
  const int first = skip_first ? 1 : 0, last = (int)T->nlevels - (skip_last ? 1 : 0);
  int count = 0;
  for (size_t q = 0; q + 1 < T->launch.size(); ++q)
    if (std::max(T->launch[q], first) < std::min(T->launch[q + 1], last)) ++count;
  return count;
}

void tri_solve_part(const kry_tri *T, int k, const void *y, void *x, const void *scale, bool skip_first,
                    bool skip_last, const Ctrl *ctrl, int step, hipStream_t st) {
  kry_vec yv, xv;
  yv.n = xv.n = T->n;
  yv.k = xv.k = k;
  yv.dtype = xv.dtype = T->dtype;
  yv.d = const_cast<void *>(y);
  xv.d = x;
  tri_check(T, &yv, &xv);
  const int first = skip_first ? 1 : 0, last = (int)T->nlevels - (skip_last ? 1 : 0);
  if (T->dtype == KRY_F64) {
    if (scale) tri_launch<double, true>(T, &yv, &xv, ctrl, step, st, static_cast<const double *>(scale), first, last);
    else tri_launch<double>(T, &yv, &xv, ctrl, step, st, nullptr, first, last);
  } else {
    if (scale) tri_launch<float, true>(T, &yv, &xv, ctrl, step, st, static_cast<const float *>(scale), first, last);
    else tri_launch<float>(T, &yv, &xv, ctrl, step, st, nullptr, first, last);
  }
}

void tri_boundary(const kry_tri *T, const kry_tri *next, int k, const void *y, void *x, const void *scale,
                  const Ctrl *ctrl, int step, hipStream_t st) {
  KRY_REQUIRE(tri_boundary_match(T, next) && is_pow2(k) && k <= 64, KRY_EINVAL, "not a fusable level boundary");
  if (T->dtype == KRY_F64) boundary_launch<double>(T, next, k, y, x, scale, ctrl, step, st);
  else boundary_launch<float>(T, next, k, y, x, scale, ctrl, step, st);
}

void tri_shape(const kry_tri *T, int64_t *n, int *dtype) {
  *n = T->n;
  *dtype = T->dtype;
}

}  // namespace kry

extern "C" {

int kry_tri_create_ordered(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices,
                           const void *data, int dtype, int itype, int lower, const int32_t *rank, kry_tri **out) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx && out && indptr && n >= 0 && nnz >= 0 && (nnz == 0 || (indices && data)), KRY_EINVAL,
              "bad argument");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32 || itype == KRY_I64, KRY_EINVAL, "itype must be i32 or i64");
  KRY_HIP(hipSetDevice(ctx->device));
  auto *T = new kry_tri();
  T->ctx = ctx;
  T->n = n;
  T->nnz = nnz;
  T->dtype = dtype;
  T->lower = lower != 0;
  try {
    const bool i32 = itype == KRY_I32, f64 = dtype == KRY_F64;
    if (i32 && f64)
      tri_build(T, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
                static_cast<const double *>(data), rank);
    else if (i32)
      tri_build(T, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
                static_cast<const float *>(data), rank);
    else if (f64)
      tri_build(T, n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices),
                static_cast<const double *>(data), rank);
    else
      tri_build(T, n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices),
                static_cast<const float *>(data), rank);
  } catch (...) {
    tri_free(T);
    delete T;
    throw;
  }
  *out = T;
  KRY_API_END
}

int kry_tri_create(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                   int dtype, int itype, int lower, kry_tri **out) {
  return kry_tri_create_ordered(ctx, n, nnz, indptr, indices, data, dtype, itype, lower, nullptr, out);
}

int kry_tri_destroy(kry_tri *T) {
  KRY_API_BEGIN
  if (!T) return KRY_OK;
  (void)hipSetDevice(T->ctx->device);
  (void)hipStreamSynchronize(T->ctx->stream);
  tri_free(T);
  delete T;
  KRY_API_END
}

int kry_tri_info(const kry_tri *T, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(T && info, KRY_EINVAL, "null argument");
  info[0] = T->nlevels;
  info[1] = (int64_t)T->launch.size() - 1;
  info[2] = T->nslices;
  info[3] = T->nslots;
  info[4] = T->max_level_rows;
  info[5] = (int64_t)T->image_bytes;
  KRY_API_END
}

int kry_tri_solve(kry_ctx *ctx, const kry_tri *T, const kry_vec *y, kry_vec *x) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx, KRY_EINVAL, "null argument");
  tri_check(T, y, x);
  KRY_HIP(hipSetDevice(ctx->device));
  if (T->dtype == KRY_F64) tri_launch<double>(T, y, x, nullptr, 0, ctx->stream);
  else tri_launch<float>(T, y, x, nullptr, 0, ctx->stream);
  KRY_API_END
}

int kry_prog_trisolve(kry_prog *p, const kry_tri *T, const kry_vec *y, kry_vec *x, int32_t step) {
  KRY_API_BEGIN
  KRY_REQUIRE(p, KRY_EINVAL, "null argument");
  tri_check(T, y, x);
  KRY_REQUIRE(x->k == p->k, KRY_EINVAL, "column count differs from the chain's");
  if (T->dtype == KRY_F64) tri_launch<double>(T, y, x, p->ctrl, step, p->ctx->stream);
  else tri_launch<float>(T, y, x, p->ctrl, step, p->ctx->stream);
  KRY_API_END
}

}  // extern "C"
