// Factorised preconditioners: the ILU(0) factorisation kernel, the
// approximate-inverse kernel (ISAI, below) and the stage object kry_precond
// (triangular solves of tri.hip and row scales, or approximate-inverse
// products, or the one block-Jacobi product of bjacobi.hip) that the solver
// cores and the scalar chain apply in a preconditioner slot.
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

// ------------------------------------------------------------------ ISAI
// The incomplete sparse approximate inverse of a lower triangle T: W on T's
// pattern with (W T) = I on that pattern. Row i with pattern J[0..m-1]
// (J[m-1] = i) is the back substitution on T(J, J)^T:
//   w[m-1] = 1 / t(i, i)
//   for p = m-2 .. 0:  s = 0
//     for q = p+1 .. m-1 ascending, t(J[q], J[p]) stored: s = s - (t(J[q], J[p]) * w[q])
//     w[p] = s / t(J[p], J[p])
// (true divisions, the product rounded before the subtraction). The rows are
// independent: one launch, no levels. A row of m entries belongs to a group of
// g = 4, 8, 16, 32 or 64 lanes (the smallest holding it; 64 for longer rows),
// 64 / g rows to a wavefront; entry q belongs to lane q mod g of the group,
// which alone computes, stores and re-reads w[q]. For one p the lanes look
// t(J[q], J[p]) up in parallel, by binary search in the sorted row J[q], and
// form their products; the sum then takes the stored terms one at a time in
// ascending q (the set bits of a ballot), every lane of the group the same
// sum. Every loop bound is the wavefront's, so the lanes stay converged at
// the shuffles.
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() { KRY_HIP(hipEventCreate(&e)); }
  ~DevEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

struct IsaiTask {
  int32_t first, count, g, maxm;  // rows rowlist[first, first + count), their group size and longest row
};

template <typename V>
struct IsaiImg {
  const int32_t *ip, *ix;
  const V *val;
  const int32_t *rowlist;
  const IsaiTask *tasks;
  V *out;
  int32_t *bad;  // smallest row whose diagonal is 0 or non-finite (INT_MAX: none)
};

template <typename V>
__global__ __launch_bounds__(kBlock) void isai_lower_kernel(IsaiImg<V> A, int32_t ntasks) {
  const int32_t t = (int32_t)blockIdx.x * (kBlock / kWave) + (int32_t)(threadIdx.x / kWave);
  if (t >= ntasks) return;  // uniform over the wavefront
  const IsaiTask task = A.tasks[t];
  const int lane = threadIdx.x & (kWave - 1);
  const int g = task.g, grp = lane / g, l = lane - grp * g, gbase = grp * g;
  const bool have = grp < task.count;
  const int32_t i = have ? A.rowlist[task.first + grp] : 0;
  const int32_t b = have ? A.ip[i] : 0;
  const int32_t m = have ? A.ip[i + 1] - b : 0;
  const bool single = task.maxm <= g;  // entry l of the row is this lane's only one
  const uint64_t gmask = g == kWave ? ~uint64_t(0) : ((uint64_t(1) << g) - 1);
  V wreg = V(0);
  if (have && l == (m - 1) % g) {
    const V d = A.val[b + m - 1];
    if (d == V(0) || !isfinite(d)) atomicMin(A.bad, i);
    wreg = V(1) / d;
    A.out[b + m - 1] = wreg;
  }
  for (int32_t p = task.maxm - 2; p >= 0; --p) {
    const bool act = p <= m - 2;
    const int32_t jp = act ? A.ix[b + p] : 0;
    V s = V(0);
    for (int32_t cb = (p + 1) / g * g; cb < task.maxm; cb += g) {
      const int32_t q = cb + l;
      bool has = false;
      V prod = V(0);
      if (act && q > p && q < m) {
        const int32_t r = A.ix[b + q];
        const int32_t u1 = A.ip[r + 1] - 1;  // row r's entries left of its diagonal
        int32_t lo = A.ip[r], hi = u1;
        while (lo < hi) {
          const int32_t mid = lo + ((hi - lo) >> 1);
          if (A.ix[mid] < jp) lo = mid + 1;
          else hi = mid;
        }
        if (lo < u1 && A.ix[lo] == jp) {
          has = true;
          prod = A.val[lo] * (single ? wreg : A.out[b + q]);
        }
      }
      uint64_t bits = (__ballot(has) >> gbase) & gmask;
      while (__ballot(bits != 0) != 0) {
        const int src = bits ? __builtin_ctzll(bits) : 0;
        const V v = __shfl(prod, gbase + src);
        if (bits) {
          s = s - v;
          bits &= bits - 1;
        }
      }
    }
    if (act && l == p % g) {
      wreg = s / A.val[A.ip[jp + 1] - 1];
      A.out[b + p] = wreg;
    }
  }
}

// The pattern a row must have, and the rows by group size (host).
void isai_plan(int64_t n, int64_t nnz, const int32_t *ip, const int32_t *ix, std::vector<int32_t> &rowlist,
               std::vector<IsaiTask> &tasks, int64_t *longest) {
  KRY_REQUIRE(ip[0] == 0 && ip[n] == nnz, KRY_EINVAL, "indptr does not span the entries");
  std::vector<int32_t> bucket[5];  // g = 4 << q
  *longest = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = ip[i], e = ip[i + 1];
    KRY_REQUIRE(e >= b && e <= nnz, KRY_EINVAL, "indptr is not monotone");
    KRY_REQUIRE(e > b && ix[e - 1] == i, KRY_EINVAL,
                "row " + std::to_string(i) + " of the triangle does not end in its diagonal entry");
    KRY_REQUIRE(ix[b] >= 0, KRY_EINVAL, "negative column index in row " + std::to_string(i));
    for (int64_t q = b + 1; q < e; ++q)
      KRY_REQUIRE(ix[q - 1] < ix[q], KRY_EINVAL, "row " + std::to_string(i) + " is not strictly sorted");
    const int64_t m = e - b;
    KRY_REQUIRE(m <= 1024, KRY_EUNSUPPORTED,
                "row " + std::to_string(i) + " of the triangle has " + std::to_string(m) +
                    " entries: the approximate inverse takes rows of at most 1024");
    *longest = std::max(*longest, m);
    int q = 0;
    while (q < 4 && (4 << q) < m) ++q;
    bucket[q].push_back((int32_t)i);
  }
  rowlist.clear();
  tasks.clear();
  for (int q = 0; q < 5; ++q) {
    const int g = 4 << q, per = kWave / g;
    for (size_t r = 0; r < bucket[q].size(); r += (size_t)per) {
      IsaiTask t{(int32_t)rowlist.size(), (int32_t)std::min<size_t>((size_t)per, bucket[q].size() - r), g, 0};
      for (int32_t c = 0; c < t.count; ++c) {
        const int32_t i = bucket[q][r + (size_t)c];
        t.maxm = std::max(t.maxm, ip[i + 1] - ip[i]);
        rowlist.push_back(i);
      }
      tasks.push_back(t);
    }
  }
}

template <typename V>
void isai_run(kry_ctx *ctx, int64_t n, int64_t nnz, const int32_t *ip, const int32_t *ix, const V *dv, V *out,
              int64_t *info) {
  KRY_REQUIRE(nnz < INT32_MAX && n < INT32_MAX, KRY_EUNSUPPORTED, "the approximate inverse indexes entries in int32");
  std::vector<int32_t> rowlist;
  std::vector<IsaiTask> tasks;
  isai_plan(n, nnz, ip, ix, rowlist, tasks, &info[1]);
  if (n == 0) return;
  hipStream_t st = ctx->stream;
  DevBuf dip, dix, dval, drow, dtask, dout, dbad;
  put(dip, ip, (size_t)n + 1, st);
  put(dix, ix, (size_t)nnz, st);
  put(dval, dv, (size_t)nnz, st);
  put(drow, rowlist.data(), rowlist.size(), st);
  put(dtask, tasks.data(), tasks.size(), st);
  dout.p = dev_alloc((size_t)nnz * sizeof(V));
  const int32_t none = INT_MAX;
  put(dbad, &none, 1, st);
  const IsaiImg<V> img{static_cast<const int32_t *>(dip.p),  static_cast<const int32_t *>(dix.p),
                       static_cast<const V *>(dval.p),       static_cast<const int32_t *>(drow.p),
                       static_cast<const IsaiTask *>(dtask.p), static_cast<V *>(dout.p),
                       static_cast<int32_t *>(dbad.p)};
  const int32_t ntasks = (int32_t)tasks.size();
  const unsigned grid = (unsigned)((ntasks + kIluWaves - 1) / kIluWaves);
  DevEvent e0, e1;  // the kernel alone (info[2]), apart from the copies around it
  KRY_HIP(hipEventRecord(e0.e, st));
  hipLaunchKernelGGL(isai_lower_kernel<V>, dim3(grid), dim3(kBlock), 0, st, img, ntasks);
  KRY_HIP(hipGetLastError());
  KRY_HIP(hipEventRecord(e1.e, st));
  int32_t bad = none;
  KRY_HIP(hipMemcpyAsync(&bad, dbad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipMemcpyAsync(out, dout.p, (size_t)nnz * sizeof(V), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  KRY_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
  info[2] = (int64_t)((double)ms * 1000.0);
  info[0] = bad == none ? -1 : bad;
  KRY_REQUIRE(bad == none, KRY_ESINGULAR,
              "singular matrix: the diagonal entry of row " + std::to_string(bad) + " is zero or not finite");
}

// y = s * (x0 + W x) (x0 null: y = s * (W x)), s an (n,) vector broadcast over
// the columns: the row scale of SSOR in the store of the product in front of
// it. The sum and the product are rounded one after the other.
template <typename V>
struct EpiScaleAddStore {
  V *out;
  const V *x0;
  const V *s;
  int k;
  __device__ __forceinline__ double operator()(int64_t i, int c, V sum, V xi) const {
    const V t = x0 ? x0[i * k + c] + sum : sum;
    out[i * k + c] = s[i] * t;
    return 0.0;
  }
  template <int C>
  __device__ __forceinline__ void row(int64_t i, int c0, const V (&sum)[C], const V (&xi)[C], double (&d)[C]) const {
    V o[C];
    if (x0) {
      vload_row<V, C>(x0 + i * k + c0, o);
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = o[c] + sum[c];
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = sum[c];
    }
    const V si = s[i];
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = si * o[c];
    vstore_row<V, C>(out + i * k + c0, o);
  }
  __device__ __forceinline__ double rows2(int64_t i, const V (&sum)[2], const V (&xi)[2]) const {
    V o[2] = {sum[0], sum[1]};
    if (x0) {
      pload<V>(x0 + i, o);
      o[0] = o[0] + sum[0];
      o[1] = o[1] + sum[1];
    }
    o[0] = s[i] * o[0];
    o[1] = s[i + 1] * o[1];
    pstore<V>(out + i, o);
    return 0.0;
  }
};

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
  KRY_REQUIRE(is_pow2(x->k) && x->k <= precond_max_cols(P), KRY_EUNSUPPORTED,
              "a factorised preconditioner handles up to 64 columns (256 with approximate-inverse solves or "
              "block-Jacobi)");
}

bool is_isai(const kry_precond *P) { return !P->stages.empty() && P->stages[0].isai_w != nullptr; }
bool is_bjacobi(const kry_precond *P) { return !P->stages.empty() && P->stages[0].bj != nullptr; }

// the blocks between the stages, grown to k columns
void isai_scratch(const kry_precond *P, int k) {
  if (k <= P->scratch_k) return;
  for (void *&b : P->scratch) {
    dev_free(b);  // launches that still read it come first in stream order: the pool retires it after a sync
    b = nullptr;
  }
  P->scratch_k = 0;
  for (void *&b : P->scratch) b = dev_alloc(padded_elems(P->n, k) * dsize(P->dtype));
  P->scratch_k = k;
}

// one stage: x = W y, sweeps times x = x + W (y - T x), the scale in the last store (x != y)
template <typename V>
void isai_stage(const kry_precond::Stage &s, int k, const V *y, V *x, V *r, const Ctrl *ctrl, int step,
                hipStream_t st) {
  const V *scale = static_cast<const V *>(s.scale);
  if (scale && s.sweeps == 0)
    launch_spmv_any<V>(s.isai_w, k, SrcPlain<V>{y, k}, EpiScaleAddStore<V>{x, nullptr, scale, k}, nullptr, nullptr,
                       ctrl, step, st);
  else
    launch_spmv_any<V>(s.isai_w, k, SrcPlain<V>{y, k}, EpiStore<V>{x, k}, nullptr, nullptr, ctrl, step, st);
  for (int sw = 0; sw < s.sweeps; ++sw) {
    launch_spmv_any<V>(s.isai_t, k, SrcPlain<V>{x, k}, EpiResidual<V>{y, r, nullptr, k}, nullptr, nullptr, ctrl, step,
                       st);
    if (scale && sw + 1 == s.sweeps)
      launch_spmv_any<V>(s.isai_w, k, SrcPlain<V>{r, k}, EpiScaleAddStore<V>{x, x, scale, k}, nullptr, nullptr, ctrl,
                         step, st);
    else
      launch_spmv_any<V>(s.isai_w, k, SrcPlain<V>{r, k}, EpiAddStore<V>{x, x, k}, nullptr, nullptr, ctrl, step, st);
  }
}

// Every stage writes a block of its own: the last one dst, the others the two
// scratch blocks in turn. A single stage whose dst is its src works from a copy.
template <typename V>
void isai_stages(const kry_precond *P, int k, const V *src, V *dst, const Ctrl *ctrl, int step, hipStream_t st) {
  isai_scratch(P, k);
  const size_t ns = P->stages.size();
  const V *in = src;
  if (ns == 1 && src == dst) {
    KRY_HIP(hipMemcpyAsync(P->scratch[0], src, (size_t)P->n * k * sizeof(V), hipMemcpyDeviceToDevice, st));
    in = static_cast<const V *>(P->scratch[0]);
  }
  for (size_t i = 0; i < ns; ++i) {
    V *out = i + 1 == ns ? dst : static_cast<V *>(P->scratch[i & 1]);
    isai_stage<V>(P->stages[i], k, in, out, static_cast<V *>(P->scratch[2]), ctrl, step, st);
    in = out;
  }
}

}  // namespace

kry_precond::~kry_precond() {
  for (void *b : scratch) dev_free(b);
}

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

int precond_max_cols(const kry_precond *P) { return is_isai(P) || is_bjacobi(P) ? kMaxCols : 64; }

static int precond_launches(const kry_precond *P) {
  int count = 0;
  for (size_t i = 0; i < P->stages.size(); ++i) {
    const kry_precond::Stage &s = P->stages[i];
    if (s.bj) {
      count += 1;  // the batched block product
      continue;
    }
    if (s.isai_w) {
      count += 1 + 2 * s.sweeps;  // the SpMVs
      continue;
    }
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
  if (is_bjacobi(P)) return bjacobi_apply_raw(P->stages[0].bj, k, src, dst, ctrl, step, st);
  if (is_isai(P)) {
    if (P->dtype == KRY_F64)
      isai_stages<double>(P, k, static_cast<const double *>(src), static_cast<double *>(dst), ctrl, step, st);
    else
      isai_stages<float>(P, k, static_cast<const float *>(src), static_cast<float *>(dst), ctrl, step, st);
    return;
  }
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
  if (is_bjacobi(P))
    KRY_REQUIRE(is_pow2(k) && k <= kMaxCols, KRY_EUNSUPPORTED, "a block-Jacobi preconditioner handles up to 256 columns");
  else if (is_isai(P))
    KRY_REQUIRE(is_pow2(k) && k <= kMaxCols, KRY_EUNSUPPORTED,
                "a factorised preconditioner with approximate-inverse solves handles up to 256 columns");
  else
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

int kry_isai_lower(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                   int dtype, int itype, void *values, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(ctx && indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || (indices && data && values)), KRY_EINVAL,
              "bad argument");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32, KRY_EUNSUPPORTED, "the approximate inverse takes int32 indices");
  KRY_HIP(hipSetDevice(ctx->device));
  info[0] = -1;
  info[1] = info[2] = 0;
  if (dtype == KRY_F64)
    isai_run<double>(ctx, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
                     static_cast<const double *>(data), static_cast<double *>(values), info);
  else
    isai_run<float>(ctx, n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices),
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
  // approximate-inverse stages and a block-Jacobi stage have no levels to fuse
  P->fused = P->fuse_allowed && !is_isai(P) && !is_bjacobi(P);
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
  KRY_REQUIRE(!is_isai(P), KRY_EINVAL, "a preconditioner of approximate-inverse stages takes no other stage");
  KRY_REQUIRE(!is_bjacobi(P), KRY_EINVAL, "a block-Jacobi preconditioner takes no other stage");
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
  KRY_REQUIRE(!is_isai(P), KRY_EINVAL, "a preconditioner of approximate-inverse stages takes no other stage");
  KRY_REQUIRE(!is_bjacobi(P), KRY_EINVAL, "a block-Jacobi preconditioner takes no other stage");
  kry_precond::Stage s;
  s.scale = d->d;
  P->stages.push_back(s);
  KRY_API_END
}

int kry_precond_add_isai(kry_precond *P, const kry_csr *W, const kry_csr *T, int32_t sweeps, const kry_vec *scale) {
  KRY_API_BEGIN
  KRY_REQUIRE(P && W, KRY_EINVAL, "null argument");
  KRY_REQUIRE(sweeps >= 0 && sweeps <= 64, KRY_EINVAL, "sweeps must be 0 to 64");
  KRY_REQUIRE((sweeps > 0) == (T != nullptr), KRY_EINVAL, "the triangle T goes with sweeps > 0, and only with them");
  for (const kry_csr *M : {W, T}) {
    if (!M) continue;
    KRY_REQUIRE(M->n == P->n && M->dtype == P->dtype, KRY_EINVAL, "shape/dtype mismatch with the preconditioner");
    KRY_REQUIRE(!M->renumbered, KRY_EINVAL,
                "the stages work in the caller's numbering: create W and T with kry_csr_create_ex(renumber = 0)");
  }
  KRY_REQUIRE(!scale || (scale->n == P->n && scale->k == 1 && scale->dtype == P->dtype), KRY_EINVAL,
              "the scale must be (n,) of the preconditioner's dtype");
  KRY_REQUIRE(P->stages.size() < 8, KRY_EINVAL, "at most 8 stages");
  KRY_REQUIRE(P->stages.empty() || is_isai(P), KRY_EINVAL,
              "a preconditioner of solves and scales takes no approximate-inverse stage");
  kry_precond::Stage s;
  s.isai_w = W;
  s.isai_t = T;
  s.sweeps = sweeps;
  s.scale = scale ? scale->d : nullptr;
  P->stages.push_back(s);
  KRY_API_END
}

int kry_precond_add_bjacobi(kry_precond *P, const kry_bjacobi *B) {
  KRY_API_BEGIN
  KRY_REQUIRE(P && B, KRY_EINVAL, "null argument");
  int64_t n = 0;
  int dtype = 0;
  bjacobi_shape(B, &n, &dtype);
  KRY_REQUIRE(n == P->n && dtype == P->dtype, KRY_EINVAL, "shape/dtype mismatch with the preconditioner");
  KRY_REQUIRE(P->stages.empty(), KRY_EINVAL, "a block-Jacobi stage is the only stage of its preconditioner");
  kry_precond::Stage s;
  s.bj = B;
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
