// Factorised preconditioners: the ILU(0) factorisation kernel and the stage
// object kry_precond (triangular solves of tri.hip and row scales) that the
// solver cores and the scalar chain apply in a preconditioner slot.
//
// ILU(0), in place over a copy of A's values, rows i ascending:
//   for k in cols(i), k < i, ascending:
//     a_ik = a_ik / a_kk
//     for j in cols(i), j > k, with (k, j) stored: a_ij = a_ij - (a_ik * a_kj)
// (true division, the product rounded before the subtraction: no FMA). Row i
// needs the finished rows k < i of its own pattern, so the rows of one level
// of tri_plan(lower) over tril(A)'s pattern are independent (host_image.hpp
// ilu0_plan). One wavefront factorises a row: entry e of the row belongs to
// lane (e - first) mod 64, which alone reads and writes it, so every entry
// takes its updates in ascending k whatever the launch plan; the k loop is
// sequential, the owner of (i, k) divides, stores and broadcasts l_ik, and
// each lane looks (k, j) up by binary search in row k's sorted upper part.
//
// Launches follow tri.hip: a run of consecutive levels holding at most
// kTriGroupRows rows is one launch of one workgroup with a workgroup barrier
// between its levels; a larger level is a launch of its own over many
// workgroups. No kernel waits on another workgroup: stream order is the only
// cross-workgroup dependency.
//
// A multicolour kry_precond (kry_precond_fuse) applies its stages in fewer
// launches, bitwise the stage-by-stage apply: a row scale goes into the solve
// behind it, and where one solve's last level and the next solve's first are
// the same rows (two colours) they are one launch (tri.hip). KRY_PRECOND_FUSE=0
// turns both off.
#include <climits>
#include <cstdlib>
#include <string>

#include "host_image.hpp"
#include "precond.hpp"
#include "prog.hpp"

using namespace kry;

namespace {

constexpr int kWave = 64;
constexpr int kIluWaves = kBlock / kWave;  // rows a workgroup factorises at a time

template <typename V>
struct IluImg {
  const int32_t *ip;     // n + 1
  const int32_t *ix;     // nnz
  const int32_t *diag;   // n: position of (i, i)
  const int32_t *order;  // n: rows by (level, row)
  const int32_t *lrow;   // nlevels + 1: a level's rows in order
  V *val;                // nnz, factorised in place
  int32_t *bad;          // smallest row whose pivot came out 0 or non-finite (INT_MAX: none)
};

// one row by one whole wavefront (every lane calls it)
template <typename V>
__device__ __forceinline__ void ilu_row(const IluImg<V> &A, int32_t i, int lane) {
  const int32_t b = A.ip[i], dpos = A.diag[i], e1 = A.ip[i + 1];
  for (int32_t ek = b; ek < dpos; ++ek) {
    const int32_t kk = A.ix[ek];
    const int32_t kd = A.diag[kk];
    const int owner = (ek - b) & (kWave - 1);
    V l = V(0);
    if (lane == owner) {
      l = A.val[ek] / A.val[kd];
      A.val[ek] = l;
    }
    l = __shfl(l, owner);
    const int32_t u0 = kd + 1, u1 = A.ip[kk + 1];
    // this lane's entries behind (i, k)
    int32_t e = b + lane;
    if (e <= ek) e += ((ek - e) / kWave + 1) * kWave;
    for (; e < e1; e += kWave) {
      const int32_t j = A.ix[e];
      int32_t lo = u0, hi = u1;
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (A.ix[mid] < j) lo = mid + 1;
        else hi = mid;
      }
      if (lo < u1 && A.ix[lo] == j) {
        const V p = l * A.val[lo];
        A.val[e] = A.val[e] - p;
      }
    }
  }
  if (lane == ((dpos - b) & (kWave - 1))) {
    const V d = A.val[dpos];
    if (d == V(0) || !isfinite(d)) atomicMin(A.bad, i);
  }
}

// a level of its own: rows order[r0, r1) over the grid, one wavefront each
template <typename V>
__global__ __launch_bounds__(kBlock) void ilu_level_kernel(IluImg<V> A, int32_t r0, int32_t r1) {
  const int64_t q = (int64_t)r0 + (int64_t)blockIdx.x * kIluWaves + (threadIdx.x / kWave);
  if (q >= r1) return;  // uniform over the wavefront
  ilu_row<V>(A, A.order[q], threadIdx.x & (kWave - 1));
}

// levels [l0, l1) in one workgroup, a barrier between them
template <typename V>
__global__ __launch_bounds__(kBlock) void ilu_group_kernel(IluImg<V> A, int32_t l0, int32_t l1) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  for (int32_t l = l0; l < l1; ++l) {
    const int32_t r1 = A.lrow[l + 1];
    for (int32_t q = A.lrow[l] + wave; q < r1; q += kIluWaves) ilu_row<V>(A, A.order[q], lane);
    if (l + 1 < l1) {
      __threadfence_block();
      __syncthreads();
    }
  }
}

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { dev_free(p); }
};

template <typename T>
void put(DevBuf &b, const T *h, size_t count, hipStream_t st) {
  b.p = dev_alloc(std::max<size_t>(count, 1) * sizeof(T));
  if (count) KRY_HIP(hipMemcpyAsync(b.p, h, count * sizeof(T), hipMemcpyHostToDevice, st));
}

template <typename V>
void ilu0_run(kry_ctx *ctx, int64_t n, int64_t nnz, const int32_t *ip, const int32_t *ix, const V *dv, V *out,
              int64_t *info) {
  Ilu0Plan p;
  ilu0_plan(n, nnz, ip, ix, p);
  KRY_REQUIRE(nnz < INT32_MAX, KRY_EUNSUPPORTED, "the ILU(0) factorisation indexes entries in int32");
  std::vector<int32_t> diag(p.diag.begin(), p.diag.end());
  const TriPlan &t = p.tri;
  info[0] = t.nlevels;
  info[1] = (int64_t)t.launch.size() - 1;
  info[2] = t.max_level_rows;
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  DevBuf dip, dix, ddiag, dorder, dlrow, dval, dbad;
  put(dip, ip, (size_t)n + 1, st);
  put(dix, ix, (size_t)nnz, st);
  put(ddiag, diag.data(), diag.size(), st);
  put(dorder, t.order.data(), t.order.size(), st);
  put(dlrow, t.lrow.data(), t.lrow.size(), st);
  put(dval, dv, (size_t)nnz, st);
  const int32_t none = INT_MAX;
  put(dbad, &none, 1, st);
  const IluImg<V> img{static_cast<const int32_t *>(dip.p),   static_cast<const int32_t *>(dix.p),
                      static_cast<const int32_t *>(ddiag.p), static_cast<const int32_t *>(dorder.p),
                      static_cast<const int32_t *>(dlrow.p), static_cast<V *>(dval.p),
                      static_cast<int32_t *>(dbad.p)};
  for (size_t q = 0; q + 1 < t.launch.size(); ++q) {
    const int32_t l0 = t.launch[q], l1 = t.launch[q + 1];
    const int32_t r0 = t.lrow[(size_t)l0], r1 = t.lrow[(size_t)l1];
    if (l1 == l0 + 1 && r1 - r0 > kTriGroupRows) {
      const unsigned grid = (unsigned)((r1 - r0 + kIluWaves - 1) / kIluWaves);
      hipLaunchKernelGGL(ilu_level_kernel<V>, dim3(grid), dim3(kBlock), 0, st, img, r0, r1);
    } else {
      hipLaunchKernelGGL(ilu_group_kernel<V>, dim3(1), dim3(kBlock), 0, st, img, l0, l1);
    }
  }
  KRY_HIP(hipGetLastError());
  int32_t bad = none;
  KRY_HIP(hipMemcpyAsync(&bad, dbad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipMemcpyAsync(out, dval.p, (size_t)nnz * sizeof(V), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
  info[3] = bad == none ? -1 : bad;
  KRY_REQUIRE(bad == none, KRY_ESINGULAR,
              "singular matrix: the ILU(0) pivot of row " + std::to_string(bad) + " is zero or not finite");
}

// z = z * d, d an (n,) vector broadcast over the k = 1 << kshift columns
template <typename V>
struct OpPrecScale {
  V *z;
  const V *x, *d;
  int kshift;
  __device__ __forceinline__ void operator()(int64_t e, int64_t N, double (&)[Vec16<V>::W]) const {
    constexpr int W = Vec16<V>::W;
    V xv[W];
    VIO<V>::load(x, e, N, xv);
#pragma unroll
    for (int v = 0; v < W; ++v) {
      const V dv = e + v < N ? d[(e + v) >> kshift] : V(1);
      xv[v] = xv[v] * dv;
    }
    VIO<V>::store(z, e, N, xv);
  }
};

template <typename V>
void scale_launch(int64_t n, int k, const void *x, void *z, const void *d, const Ctrl *ctrl, int step, hipStream_t st) {
  int ks = 0;
  while ((1 << ks) < k) ++ks;
  launch_elementwise<V>(n * (int64_t)k, k,
                        OpPrecScale<V>{static_cast<V *>(z), static_cast<const V *>(x), static_cast<const V *>(d), ks},
                        nullptr, ctrl, step, st);
}

void vec_check(const kry_precond *P, const kry_vec *x, const kry_vec *y) {
  KRY_REQUIRE(P && x && y, KRY_EINVAL, "null argument");
  KRY_REQUIRE(x->n == P->n && y->n == P->n && x->k == y->k && x->dtype == P->dtype && y->dtype == P->dtype, KRY_EINVAL,
              "shape/dtype mismatch with the preconditioner");
  KRY_REQUIRE(is_pow2(x->k) && x->k <= 64, KRY_EUNSUPPORTED, "a factorised preconditioner handles up to 64 columns");
}

}  // namespace

namespace kry {

// The fused form of the stage list: every scale directly in front of a solve
// is folded into it, and a solve hands its last level to a boundary launch
// when the next solve (behind at most one scale) matches it, it takes no
// folded scale itself and keeps a level of its own.
static void fuse_plan(kry_precond *P) {
  const size_t ns = P->stages.size();
  P->fuse.assign(ns, kry_precond::Fuse());
  for (size_t i = 0; i < ns; ++i) {
    const kry_precond::Stage &s = P->stages[i];
    if (!s.tri) {
      if (i + 1 < ns && P->stages[i + 1].tri) {
        P->fuse[i].folded = true;
        P->fuse[i + 1].pre = s.scale;
      }
      continue;
    }
    const size_t j = (i + 1 < ns && !P->stages[i + 1].tri) ? i + 2 : i + 1;
    if (j >= ns || !P->stages[j].tri || P->fuse[i].pre) continue;
    if (!tri_boundary_match(s.tri, P->stages[j].tri)) continue;
    if (P->fuse[i].skip_first && tri_launches(s.tri, true, false) == 0) continue;  // its only level is taken
    P->fuse[i].boundary = true;
    P->fuse[i].next = P->stages[j].tri;
    P->fuse[i].mid = j == i + 2 ? P->stages[i + 1].scale : nullptr;
    P->fuse[j].skip_first = true;
  }
}

static int precond_launches(const kry_precond *P) {
  int count = 0;
  for (size_t i = 0; i < P->stages.size(); ++i) {
    const kry_precond::Stage &s = P->stages[i];
    if (P->fuse.empty()) {
      count += s.tri ? tri_launches(s.tri, false, false) : 1;
      continue;
    }
    const kry_precond::Fuse &f = P->fuse[i];
    if (s.tri) count += tri_launches(s.tri, f.skip_first, f.boundary) + (f.boundary ? 1 : 0);
    else if (!f.folded) ++count;
  }
  return count;
}

void precond_stages(const kry_precond *P, int k, const void *src, void *dst, const Ctrl *ctrl, int step,
                    hipStream_t st) {
  KRY_REQUIRE(!P->stages.empty(), KRY_EINVAL, "a preconditioner without stages");
  const void *in = src;
  if (!P->fuse.empty()) {
    KRY_REQUIRE(P->fuse.size() == P->stages.size(), KRY_EINVAL, "a stage was added after kry_precond_fuse");
    for (size_t i = 0; i < P->stages.size(); ++i) {
      const kry_precond::Stage &s = P->stages[i];
      const kry_precond::Fuse &f = P->fuse[i];
      if (s.tri) {
        tri_solve_part(s.tri, k, in, dst, f.pre, f.skip_first, f.boundary, ctrl, step, st);
        if (f.boundary) tri_boundary(s.tri, f.next, k, in, dst, f.mid, ctrl, step, st);
      } else if (f.folded) {
        continue;  // `in` stays: the next solve reads it times this scale
      } else if (P->dtype == KRY_F64) {
        scale_launch<double>(P->n, k, in, dst, s.scale, ctrl, step, st);
      } else {
        scale_launch<float>(P->n, k, in, dst, s.scale, ctrl, step, st);
      }
      in = dst;
    }
    return;
  }
  for (const kry_precond::Stage &s : P->stages) {
    if (s.tri) tri_solve_raw(s.tri, k, in, dst, ctrl, step, st);
    else if (P->dtype == KRY_F64) scale_launch<double>(P->n, k, in, dst, s.scale, ctrl, step, st);
    else scale_launch<float>(P->n, k, in, dst, s.scale, ctrl, step, st);
    in = dst;
  }
}

void precond_check(const kry_precond *P, const kry_csr *A, int64_t n, int k, int dtype) {
  KRY_REQUIRE(P->n == n, KRY_EINVAL, "preconditioner shape does not match the operator");
  KRY_REQUIRE(P->dtype == dtype, KRY_EINVAL, "a factorised preconditioner's dtype must be the vectors'");
  KRY_REQUIRE(!P->stages.empty(), KRY_EINVAL, "a preconditioner without stages");
  KRY_REQUIRE(is_pow2(k) && k <= 64, KRY_EUNSUPPORTED, "a factorised preconditioner handles up to 64 columns");
  KRY_REQUIRE(!A->renumbered, KRY_EUNSUPPORTED,
              "a factorised preconditioner works in the caller's numbering: the operator was renumbered at upload "
              "(KRY_RENUMBER=0 keeps the caller's numbering)");
}

void precond_matrix_check(const kry_csr *op, const kry_csr *A, int64_t n, int dtype) {
  KRY_REQUIRE(op->n == n, KRY_EINVAL, "preconditioner shape does not match the operator");
  KRY_REQUIRE(op->dtype == dtype || (dtype == KRY_F64 && op->dtype == KRY_F32), KRY_EINVAL,
              "preconditioner dtype must match the vectors (or be float32 under float64 vectors)");
  KRY_REQUIRE(op->renumbered == A->renumbered && op->perm_hash == A->perm_hash, KRY_EINVAL,
              "preconditioner renumbered differently from the operator (build it with kry_csr_create_like)");
}

}  // namespace kry

extern "C" {

int kry_ilu0_factor(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                    int dtype, int itype, void *values, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx && indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || (indices && data && values)), KRY_EINVAL,
              "bad argument");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32, KRY_EUNSUPPORTED, "the ILU(0) factorisation takes int32 indices");
  KRY_HIP(hipSetDevice(ctx->device));
  info[3] = -1;
  if (dtype == KRY_F64)
    ilu0_run<double>(ctx, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
                     static_cast<const double *>(data), static_cast<double *>(values), info);
  else
    ilu0_run<float>(ctx, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
                    static_cast<const float *>(data), static_cast<float *>(values), info);
  KRY_API_END
}

int kry_precond_create(kry_ctx *ctx, int64_t n, int dtype, kry_precond **out) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx && out && n >= 0, KRY_EINVAL, "bad argument");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  auto *P = new kry_precond();
  P->ctx = ctx;
  P->n = n;
  P->dtype = dtype;
  const char *fuse = getenv("KRY_PRECOND_FUSE");
  P->fuse_allowed = !(fuse && fuse[0] == '0' && fuse[1] == 0);
  *out = P;
  KRY_API_END
}

int kry_precond_fuse(kry_precond *P) {
  KRY_API_BEGIN
  KRY_REQUIRE(P, KRY_EINVAL, "null argument");
  KRY_REQUIRE(!P->stages.empty(), KRY_EINVAL, "a preconditioner without stages");
  P->fused = P->fuse_allowed;
  if (P->fused) fuse_plan(P);
  KRY_API_END
}

int kry_precond_info(const kry_precond *P, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(P && info, KRY_EINVAL, "null argument");
  info[0] = precond_launches(P);
  info[1] = P->fused ? 1 : 0;
  info[2] = (int64_t)P->stages.size();
  int64_t folded = 0, boundaries = 0;
  for (const kry_precond::Fuse &f : P->fuse) {
    folded += f.folded ? 1 : 0;
    boundaries += f.boundary ? 1 : 0;
  }
  info[3] = folded;
  info[4] = boundaries;
  KRY_API_END
}

int kry_precond_destroy(kry_precond *P) {
  KRY_API_BEGIN
  delete P;
  KRY_API_END
}

int kry_precond_add_tri(kry_precond *P, const kry_tri *T) {
  KRY_API_BEGIN
  KRY_REQUIRE(P && T, KRY_EINVAL, "null argument");
  int64_t n = 0;
  int dtype = 0;
  tri_shape(T, &n, &dtype);
  KRY_REQUIRE(n == P->n && dtype == P->dtype, KRY_EINVAL, "shape/dtype mismatch with the preconditioner");
  KRY_REQUIRE(P->stages.size() < 8, KRY_EINVAL, "at most 8 stages");
  kry_precond::Stage s;
  s.tri = T;
  P->stages.push_back(s);
  KRY_API_END
}

int kry_precond_add_scale(kry_precond *P, const kry_vec *d) {
  KRY_API_BEGIN
  KRY_REQUIRE(P && d, KRY_EINVAL, "null argument");
  KRY_REQUIRE(d->n == P->n && d->k == 1 && d->dtype == P->dtype, KRY_EINVAL,
              "the scale must be (n,) of the preconditioner's dtype");
  KRY_REQUIRE(P->stages.size() < 8, KRY_EINVAL, "at most 8 stages");
  kry_precond::Stage s;
  s.scale = d->d;
  P->stages.push_back(s);
  KRY_API_END
}

int kry_precond_apply(kry_ctx *ctx, const kry_precond *P, const kry_vec *x, kry_vec *y) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx, KRY_EINVAL, "null argument");
  vec_check(P, x, y);
  KRY_HIP(hipSetDevice(ctx->device));
  precond_stages(P, x->k, x->d, y->d, nullptr, 0, ctx->stream);
  KRY_API_END
}

int kry_prog_precond(kry_prog *p, const kry_precond *P, const kry_vec *x, kry_vec *y, int32_t step) {
  KRY_API_BEGIN
  KRY_REQUIRE(p, KRY_EINVAL, "null argument");
  vec_check(P, x, y);
  KRY_REQUIRE(x->k == p->k, KRY_EINVAL, "column count differs from the chain's");
  precond_stages(P, x->k, x->d, y->d, p->ctrl, step, p->ctx->stream);
  KRY_API_END
}

}  // extern "C"
