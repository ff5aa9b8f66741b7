// Block-Jacobi preconditioner (kry_bjacobi): the diagonal blocks of A inverted
// once on the device, an apply one batched dense block product in one launch.
//
// Partition: block i is rows and columns [starts[i], starts[i + 1]), 1 to 32
// rows (host_image.hpp bjacobi_plan). Block i of A is the dense b x b array of
// A's stored entries inside it, zeros elsewhere.
//
// Inverse, in place, in V scalars (bjacobi_factor_kernel):
//   for c = 0 .. b-1:
//     p = c; for r = c+1 .. b-1: if |M[r, c]| > |M[p, c]|: p = r
//     swap rows c and p; piv[c] = p
//     d = M[c, c]; d == 0 or not finite: the block is singular
//     M[c, c] = 1;  M[c, j] = M[c, j] / d for every j
//     for every r != c: f = M[r, c]; M[r, c] = 0; M[r, j] = M[r, j] - (f * M[c, j]) for every j
//   for c = b-1 .. 0: swap columns c and piv[c]
// (true divisions, the product rounded before the subtraction). Every element
// takes its updates in ascending c, one rounded product and one subtraction
// each, so the parallel evaluation below has the loop's bits. A block belongs
// to a group of G = 4, 8, 16 or 32 lanes, 64 / G blocks to a wavefront (one
// wavefront per workgroup); the kernel is a template on G and every loop over
// the block is unrolled, so the block lives in registers under static indices.
// Lane l of a group owns COLUMN l of its block: the pivot search of step c is
// a scan of lane c's own registers, a row swap exchanges two registers of
// every lane (the runtime row by a chain of selects), the pivot and the
// multipliers f come from lane c by __shfl, and the column swaps of the end
// only change which column a lane stores. Every shuffle sits outside the
// per-group predicates and every loop bound is static: the lanes are
// converged at each of them. Rows are gathered through LDS (lane l reads row
// l of the CSR and writes it transposed). The lane that sees a singular pivot
// records its block with one atomicMin.
//
// Storage of the inverses: column-major inside a block (X[r, j] at
// off[i] + j b + r), blocks back to back, off an int64 per block.
//
// Apply (bjacobi_apply_kernel): work item (row, column), the k columns of a
// row on adjacent lanes, consecutive rows on consecutive lane groups (as
// tri.hip). y[r, c] = sum_j (X[r - s, j] * x[s + j, c]) from 0 over j
// ascending, each product rounded before its addition, all b terms whatever
// their values: independent of k, the grid and the launch shape. For a fixed j
// the rows of a block read consecutive X; the x entries a block's rows share
// are plain loads of the same address (broadcast within the wavefront, the
// L1 otherwise). No kernel waits on another workgroup. An apply whose
// destination is its source works from a copy of the source.
#include <climits>

#include "host_image.hpp"
#include "precond.hpp"
#include "prog.hpp"

using namespace kry;

struct kry_bjacobi {
  kry_ctx *ctx = nullptr;
  int64_t n = 0, nblocks = 0, values = 0;
  int dtype = 0;
  int32_t min_block = 0, max_block = 0;
  std::vector<int32_t> starts;  // nblocks + 1 (host copy, n closing)
  std::vector<int64_t> off;     // nblocks + 1
  void *d_starts = nullptr;     // int32, nblocks + 1
  void *d_off = nullptr;        // int64, nblocks + 1
  void *d_rowblk = nullptr;     // int32, n: the block of a row
  void *d_val = nullptr;        // dtype, values
  double factor_us = 0.0;       // the factor kernel alone (HIP events)
  mutable void *copy = nullptr;  // the source of an in-place apply, n x copy_k
  mutable int copy_k = 0;
};

namespace {

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { dev_free(p); }
};

struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() { KRY_HIP(hipEventCreate(&e)); }
  ~DevEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

template <typename T>
void *upload(const T *h, size_t count, hipStream_t st) {
  void *d = dev_alloc(std::max<size_t>(count, 1) * sizeof(T));
  if (count) KRY_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}

template <typename V>
struct BjFactorImg {
  const int32_t *ip, *ix;  // A, canonical CSR
  const V *val;
  const int32_t *starts;     // nblocks + 1
  const int64_t *off;        // nblocks + 1
  const int32_t *blocklist;  // blocks by (g, block)
  const BjTask *tasks;
  V *out;        // the inverses, column-major per block
  int32_t *bad;  // smallest singular block (INT_MAX: none)
};

template <typename V>
__device__ __forceinline__ V bj_abs(V v) {
  return v < V(0) ? -v : v;  // -0 and NaN pass through: neither wins a strict comparison
}

// Step C of the elimination and, by recursion, the steps behind it: a template
// on C so that every register index is a constant whatever the unroller does.
template <typename V, int G, int C>
__device__ __forceinline__ void bj_steps(V (&col)[G], int (&piv)[G], int b, int l, int gbase, int32_t blk,
                                         int32_t *bad) {
  constexpr int c = C;
  const bool act = c < b;
  // lane c: the pivot row of column c among the rows r >= c
  int p = c;
  V best = bj_abs(col[c]);
#pragma unroll
  for (int r = c + 1; r < G; ++r) {
    const V a = bj_abs(col[r]);
    if (a > best) {  // a row past the block holds 0 or NaN: it never wins
      best = a;
      p = r;
    }
  }
  p = __shfl(p, gbase + c);
  piv[c] = p;
  // every lane: rows c and p of its column change places
  const V pc = col[c];
  V pp = pc;
#pragma unroll
  for (int r = c + 1; r < G; ++r) pp = r == p ? col[r] : pp;
#pragma unroll
  for (int r = c + 1; r < G; ++r) col[r] = r == p ? pc : col[r];
  col[c] = pp;
  const V d = __shfl(col[c], gbase + c);
  if (act && l == c) {
    if (d == V(0) || !isfinite(d)) atomicMin(bad, blk);
    col[c] = V(1);
  }
  if (act) col[c] = col[c] / d;
#pragma unroll
  for (int r = 0; r < G; ++r) {
    if (r == c) continue;
    const V f = __shfl(col[r], gbase + c);
    if (act) {  // rows past the block included: they stay 0 (or NaN) and nothing reads them
      if (l == c) col[r] = V(0);
      const V t = f * col[c];
      col[r] = col[r] - t;
    }
  }
  if constexpr (C + 1 < G) bj_steps<V, G, C + 1>(col, piv, b, l, gbase, blk, bad);
}

// One task per workgroup of one wavefront; tasks [t0, t0 + gridDim.x) all have
// groups of G lanes.
template <typename V, int G>
__global__ __launch_bounds__(kWave) void bjacobi_factor_kernel(BjFactorImg<V> A, int32_t t0) {
  __shared__ V tile[kWave * G];  // group q at q G G; M[r, j] at j G + r
  const BjTask task = A.tasks[t0 + (int32_t)blockIdx.x];
  const int lane = threadIdx.x;
  const int grp = lane / G, l = lane - grp * G, gbase = grp * G;
  const bool have = grp < task.count;
  const int32_t blk = have ? A.blocklist[task.first + grp] : 0;
  const int32_t s = have ? A.starts[blk] : 0;
  const int b = have ? A.starts[blk + 1] - s : 0;
  V *mine = tile + gbase * G;
#pragma unroll
  for (int r = 0; r < G; ++r) mine[l * G + r] = V(0);
  __syncthreads();
  if (l < b) {  // row s + l of A, its entries inside the block, transposed into the tile
    const int32_t e1 = A.ip[s + l + 1];
    int32_t lo = A.ip[s + l], hi = e1;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (A.ix[mid] < s) lo = mid + 1;
      else hi = mid;
    }
    for (int32_t e = lo; e < e1; ++e) {
      const int32_t j = A.ix[e] - s;
      if (j >= b) break;
      mine[j * G + l] = A.val[e];
    }
  }
  __syncthreads();
  V col[G];  // column l of the block
#pragma unroll
  for (int r = 0; r < G; ++r) col[r] = mine[l * G + r];
  int outcol = l;  // the column this lane's registers are after the column swaps
  int piv[G];
  bj_steps<V, G, 0>(col, piv, b, l, gbase, blk, A.bad);
#pragma unroll
  for (int c = G - 1; c >= 0; --c) {
    if (c < b) {
      const int p = piv[c];
      outcol = outcol == c ? p : (outcol == p ? c : outcol);
    }
  }
  if (l < b && outcol < b) {  // outcol < b always: a pivot row lies inside the block
    V *o = A.out + A.off[blk] + (int64_t)outcol * b;
#pragma unroll
    for (int r = 0; r < G; ++r)
      if (r < b) o[r] = col[r];
  }
}

template <typename V>
struct BjImg {
  const int32_t *starts, *rowblk;
  const int64_t *off;
  const V *val;
};

template <typename V>
__global__ __launch_bounds__(kBlock) void bjacobi_apply_kernel(BjImg<V> B, int64_t n, int kshift, const V *x, V *y,
                                                               const Ctrl *ctrl, int step) {
  if (halted(ctrl, step)) return;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (n << kshift)) return;
  const int c = (int)(t & ((1 << kshift) - 1));
  const int64_t row = t >> kshift;
  const int32_t blk = B.rowblk[row];
  const int32_t s = B.starts[blk];
  const int b = B.starts[blk + 1] - s;
  const V *X = B.val + B.off[blk] + (row - s);
  const V *xs = x + (((int64_t)s) << kshift) + c;
  V acc = V(0);
  for (int j = 0; j < b; ++j) {
    const V p = X[(int64_t)j * b] * xs[(int64_t)j << kshift];
    acc = acc + p;
  }
  y[t] = acc;
}

template <typename V>
void factor_run(kry_bjacobi *B, int64_t nnz, const int32_t *ip, const int32_t *ix, const V *dv, const BjPlan &p,
                int64_t *info) {
  hipStream_t st = B->ctx->stream;
  DevBuf dip, dix, dval, dlist, dtask, dbad;
  dip.p = upload(ip, (size_t)B->n + 1, st);
  dix.p = upload(ix, (size_t)nnz, st);
  dval.p = upload(dv, (size_t)nnz, st);
  dlist.p = upload(p.blocklist.data(), p.blocklist.size(), st);
  dtask.p = upload(p.tasks.data(), p.tasks.size(), st);
  const int32_t none = INT_MAX;
  dbad.p = upload(&none, 1, st);
  const BjFactorImg<V> img{static_cast<const int32_t *>(dip.p),      static_cast<const int32_t *>(dix.p),
                           static_cast<const V *>(dval.p),           static_cast<const int32_t *>(B->d_starts),
                           static_cast<const int64_t *>(B->d_off),   static_cast<const int32_t *>(dlist.p),
                           static_cast<const BjTask *>(dtask.p),     static_cast<V *>(B->d_val),
                           static_cast<int32_t *>(dbad.p)};
  DevEvent e0, e1;  // the kernels alone, apart from the copies around them
  KRY_HIP(hipEventRecord(e0.e, st));
  // the tasks are sorted by g: one launch per class that has tasks
  size_t q = 0;
  while (q < p.tasks.size()) {
    size_t e = q;
    while (e < p.tasks.size() && p.tasks[e].g == p.tasks[q].g) ++e;
    const dim3 grid((unsigned)(e - q)), block(kWave);
    const int32_t t0 = (int32_t)q;
    switch (p.tasks[q].g) {
      case 4: hipLaunchKernelGGL((bjacobi_factor_kernel<V, 4>), grid, block, 0, st, img, t0); break;
      case 8: hipLaunchKernelGGL((bjacobi_factor_kernel<V, 8>), grid, block, 0, st, img, t0); break;
      case 16: hipLaunchKernelGGL((bjacobi_factor_kernel<V, 16>), grid, block, 0, st, img, t0); break;
      default: hipLaunchKernelGGL((bjacobi_factor_kernel<V, 32>), grid, block, 0, st, img, t0); break;
    }
    KRY_HIP(hipGetLastError());
    q = e;
  }
  KRY_HIP(hipEventRecord(e1.e, st));
  int32_t bad = none;
  KRY_HIP(hipMemcpyAsync(&bad, dbad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  KRY_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
  B->factor_us = (double)ms * 1000.0;
  info[2] = (int64_t)B->factor_us;
  info[0] = bad == none ? -1 : bad;
  KRY_REQUIRE(bad == none, KRY_ESINGULAR,
              "singular matrix: a pivot of diagonal block " + std::to_string(bad) + " (from row " +
                  std::to_string(B->starts[(size_t)bad]) + ") is zero or not finite");
}

void bj_free(kry_bjacobi *B) {
  for (void *b : {B->d_starts, B->d_off, B->d_rowblk, B->d_val, B->copy}) dev_free(b);
}

void bj_check(const kry_bjacobi *B, const kry_vec *x, const kry_vec *y) {
  KRY_REQUIRE(B && x && y, KRY_EINVAL, "null argument");
  KRY_REQUIRE(x->n == B->n && y->n == B->n && x->k == y->k && x->dtype == B->dtype && y->dtype == B->dtype, KRY_EINVAL,
              "shape/dtype mismatch with the block-Jacobi object");
  KRY_REQUIRE(is_pow2(x->k) && x->k <= kMaxCols, KRY_EUNSUPPORTED, "block-Jacobi handles up to 256 columns");
}

template <typename V>
void apply_launch(const kry_bjacobi *B, int k, const V *x, V *y, const Ctrl *ctrl, int step, hipStream_t st) {
  if (B->n == 0) return;
  int ks = 0;
  while ((1 << ks) < k) ++ks;
  if (x == y) {  // a row's result would overwrite what the other rows of its block still read
    if (k > B->copy_k) {
      dev_free(B->copy);  // launches that still read it come first in stream order
      B->copy = nullptr;
      B->copy_k = 0;
      B->copy = dev_alloc(padded_elems(B->n, k) * sizeof(V));
      B->copy_k = k;
    }
    KRY_HIP(hipMemcpyAsync(B->copy, x, (size_t)B->n * k * sizeof(V), hipMemcpyDeviceToDevice, st));
    x = static_cast<const V *>(B->copy);
  }
  const int64_t grid = ((B->n << ks) + kBlock - 1) / kBlock;
  KRY_REQUIRE(grid < (int64_t(1) << 31), KRY_EUNSUPPORTED, "a block-Jacobi apply beyond the grid limit");
  const BjImg<V> img{static_cast<const int32_t *>(B->d_starts), static_cast<const int32_t *>(B->d_rowblk),
                     static_cast<const int64_t *>(B->d_off), static_cast<const V *>(B->d_val)};
  hipLaunchKernelGGL(bjacobi_apply_kernel<V>, dim3((unsigned)grid), dim3(kBlock), 0, st, img, B->n, ks, x, y, ctrl,
                     step);
  KRY_HIP(hipGetLastError());
}

}  // namespace

namespace kry {

void bjacobi_shape(const kry_bjacobi *B, int64_t *n, int *dtype) {
  *n = B->n;
  *dtype = B->dtype;
}

// the apply on raw n x k blocks of a solver core or a chain step (precond.hpp)
void bjacobi_apply_raw(const kry_bjacobi *B, int k, const void *x, void *y, const Ctrl *ctrl, int step,
                       hipStream_t st) {
  KRY_REQUIRE(is_pow2(k) && k <= kMaxCols, KRY_EUNSUPPORTED, "block-Jacobi handles up to 256 columns");
  if (B->dtype == KRY_F64) apply_launch<double>(B, k, static_cast<const double *>(x), static_cast<double *>(y), ctrl, step, st);
  else apply_launch<float>(B, k, static_cast<const float *>(x), static_cast<float *>(y), ctrl, step, st);
}

}  // namespace kry

extern "C" {

int kry_bjacobi_create(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                       int dtype, int itype, int64_t nblocks, const int32_t *starts, int64_t *info,
                       kry_bjacobi **out) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx && out && indptr && info && n >= 0 && nnz >= 0 && nblocks >= 0 && (nnz == 0 || (indices && data)) &&
                  (nblocks == 0 || starts),
              KRY_EINVAL, "bad argument");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32, KRY_EUNSUPPORTED, "block-Jacobi takes int32 indices");
  KRY_REQUIRE(nnz < INT32_MAX && n < INT32_MAX, KRY_EUNSUPPORTED, "block-Jacobi indexes entries in int32");
  info[0] = -1;
  info[1] = info[2] = 0;
  BjPlan p;
  bjacobi_plan(n, nblocks, starts, p);
  info[1] = p.max_block;
  const int32_t *ip = static_cast<const int32_t *>(indptr), *ix = static_cast<const int32_t *>(indices);
  KRY_REQUIRE(ip[0] == 0 && ip[n] == nnz, KRY_EINVAL, "indptr does not span the entries");
  for (int64_t i = 0; i < n; ++i) {
    KRY_REQUIRE(ip[i + 1] >= ip[i] && ip[i + 1] <= nnz, KRY_EINVAL, "indptr is not monotone");
    for (int64_t q = ip[i]; q < ip[i + 1]; ++q)
      KRY_REQUIRE(ix[q] >= 0 && ix[q] < n && (q == ip[i] || ix[q - 1] < ix[q]), KRY_EINVAL,
                  "row " + std::to_string(i) + " is not strictly sorted inside [0, n)");
  }
  KRY_HIP(hipSetDevice(ctx->device));
  auto *B = new kry_bjacobi();
  B->ctx = ctx;
  B->n = n;
  B->nblocks = nblocks;
  B->dtype = dtype;
  B->values = p.values;
  B->min_block = p.min_block;
  B->max_block = p.max_block;
  try {
    B->starts.assign(starts, starts + nblocks);
    B->starts.push_back((int32_t)n);
    B->off.assign((size_t)nblocks + 1, 0);
    std::vector<int32_t> rowblk((size_t)n);
    for (int64_t i = 0; i < nblocks; ++i) {
      const int64_t b = B->starts[(size_t)i + 1] - B->starts[(size_t)i];
      B->off[(size_t)i + 1] = B->off[(size_t)i] + b * b;
      for (int64_t r = B->starts[(size_t)i]; r < B->starts[(size_t)i + 1]; ++r) rowblk[(size_t)r] = (int32_t)i;
    }
    hipStream_t st = ctx->stream;
    B->d_starts = upload(B->starts.data(), B->starts.size(), st);
    B->d_off = upload(B->off.data(), B->off.size(), st);
    B->d_rowblk = upload(rowblk.data(), rowblk.size(), st);
    B->d_val = dev_alloc(std::max<size_t>((size_t)p.values, 1) * dsize(dtype));
    if (n > 0) {
      if (dtype == KRY_F64) factor_run<double>(B, nnz, ip, ix, static_cast<const double *>(data), p, info);
      else factor_run<float>(B, nnz, ip, ix, static_cast<const float *>(data), p, info);
    }
    KRY_HIP(hipStreamSynchronize(st));  // rowblk is the host's until its copy is done
  } catch (...) {
    (void)hipStreamSynchronize(ctx->stream);
    bj_free(B);
    delete B;
    throw;
  }
  *out = B;
  KRY_API_END
}

int kry_bjacobi_destroy(kry_bjacobi *B) {
  KRY_API_BEGIN
  if (!B) return KRY_OK;
  (void)hipSetDevice(B->ctx->device);
  (void)hipStreamSynchronize(B->ctx->stream);
  bj_free(B);
  delete B;
  KRY_API_END
}

int kry_bjacobi_info(const kry_bjacobi *B, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(B && info, KRY_EINVAL, "null argument");
  info[0] = B->nblocks;
  info[1] = B->min_block;
  info[2] = B->max_block;
  info[3] = B->values * (int64_t)dsize(B->dtype);
  info[4] = (int64_t)(B->n * 4 + (B->nblocks + 1) * 12);
  info[5] = (int64_t)B->factor_us;
  KRY_API_END
}

int kry_bjacobi_get(const kry_bjacobi *B, void *host) {
  KRY_API_BEGIN
  KRY_REQUIRE(B && (host || B->values == 0), KRY_EINVAL, "null argument");
  if (B->values == 0) return KRY_OK;
  KRY_HIP(hipSetDevice(B->ctx->device));
  const size_t es = dsize(B->dtype);
  std::vector<char> cm((size_t)B->values * es);
  KRY_HIP(hipMemcpyAsync(cm.data(), B->d_val, cm.size(), hipMemcpyDeviceToHost, B->ctx->stream));
  KRY_HIP(hipStreamSynchronize(B->ctx->stream));
  char *dst = static_cast<char *>(host);
  for (int64_t i = 0; i < B->nblocks; ++i) {  // column-major on the device, row-major for the caller
    const int64_t b = B->starts[(size_t)i + 1] - B->starts[(size_t)i], o = B->off[(size_t)i];
    for (int64_t r = 0; r < b; ++r)
      for (int64_t j = 0; j < b; ++j)
        std::copy_n(cm.data() + (size_t)(o + j * b + r) * es, es, dst + (size_t)(o + r * b + j) * es);
  }
  KRY_API_END
}

int kry_bjacobi_apply(kry_ctx *ctx, const kry_bjacobi *B, const kry_vec *x, kry_vec *y) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx, KRY_EINVAL, "null argument");
  bj_check(B, x, y);
  KRY_HIP(hipSetDevice(ctx->device));
  bjacobi_apply_raw(B, x->k, x->d, y->d, nullptr, 0, ctx->stream);
  KRY_API_END
}

}  // extern "C"
