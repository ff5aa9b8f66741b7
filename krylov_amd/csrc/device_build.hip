// Operator images built on the device (round 5): kry_csr_create uploads the
// caller's CSR arrays once (indptr, indices, values: 1.8 GB at the metric,
// ~33 ms of H2D) and builds the SELL-64 image (with its compact uint16 column
// form) and the SELL-128 diagonal-offset image with kernels, instead of the
// threaded host passes (0.6-0.9 s at the metric, round 4). The images are
// byte for byte the host builders' (host_image.cpp sell_plan / sell_fill /
// compact_fill / dia_build stay the definition and the test oracle:
// kry_csr_compare, tests/test_gpu_device_build.py).
//
//   csr_check_kernel   one thread per row: indptr monotone, columns in
//                      [0, n), rows strictly sorted (DIA), rows sorted (the
//                      column-blocked test), entries far from the diagonal
//   sell_plan_kernel   one wave per 64-row slice: width (longest row) or
//                      irregular (-1), slots
//   sell_fill_kernel   one wave per slice: slot columns of indices and
//                      values, and per slot column the compact base (wave
//                      min) and deltas; a span over 65534 disables compact
//   dia_offsets_kernel one block per 128-row slice: the slice's column
//                      offsets sorted (bitonic, in LDS) and made unique
//   dia_fill_kernel    one block per slice: each entry's slot column by
//                      binary search, its lane-mask bit (LDS atomicOr), its
//                      value; then per slot column whether its present rows
//                      all store one bit pattern (dia_build's uniform flag)
//   dia_class_*_kernel the descriptor classes (dia_classes): a hash per
//                      slice's block, grouped on the host from one small D2H
//                      copy; the table gathered from each group's first
//                      slice; every slice verified against it byte for byte
// Slot pointers are exclusive scans of the per-slice slot counts
// (hipcub::DeviceScan). Vector atomics only.
#include <hipcub/hipcub.hpp>

#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "host_image.hpp"
#include "objects.hpp"

namespace kry {
namespace {

constexpr int kDb = 256;
constexpr int kDiaWMax = 64;       // offsets per slice kept between the two DIA passes
constexpr int kDiaLdsEnt = 8192;   // a slice's entries sorted in LDS (more: no DIA image)

enum : unsigned {
  F_INDPTR = 1u,      // indptr decreases
  F_RANGE = 2u,       // a column outside [0, n)
  F_UNSORTED = 4u,    // a row not strictly increasing (no DIA)
  F_UNSORTED_NS = 8u  // a row decreasing somewhere (no column-blocked image)
};

__global__ __launch_bounds__(kDb) void csr_check_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ ip,
                                                        const int32_t *__restrict__ ix, int64_t half, unsigned *flags,
                                                        unsigned long long *far) {
  unsigned f = 0;
  unsigned long long fa = 0;
  for (int64_t r = (int64_t)blockIdx.x * kDb + threadIdx.x; r < n; r += (int64_t)gridDim.x * kDb) {
    const int32_t e0 = ip[r], e1 = ip[r + 1];
    if (e1 < e0 || e0 < 0 || (int64_t)e1 > nnz) {  // never read outside indices[0, nnz)
      f |= F_INDPTR;
      continue;
    }
    int32_t prev = INT32_MIN;
    for (int32_t e = e0; e < e1; ++e) {
      const int32_t c = ix[e];
      if (c < 0 || (int64_t)c >= n) f |= F_RANGE;
      if (e > e0 && c <= prev) f |= F_UNSORTED;
      if (e > e0 && c < prev) f |= F_UNSORTED_NS;
      prev = c;
      const int64_t d = (int64_t)c - r;
      fa += (d > half || d < -half) ? 1u : 0u;
    }
  }
  if (f) atomicOr(flags, f);
  if (fa) atomicAdd(far, fa);
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

// SELL-64 plan (host_image.cpp sell_plan): one wave per slice
__global__ __launch_bounds__(kDb) void sell_plan_kernel(int64_t n, int64_t ns, const int32_t *__restrict__ ip,
                                                        int *width, long long *slots, unsigned long long *nirr,
                                                        int *maxw) {
  const int lane = threadIdx.x & 63;
  const int64_t s = ((int64_t)blockIdx.x * kDb + threadIdx.x) >> 6;
  if (s >= ns) return;
  const int64_t r = s * kSlice + lane;
  const int len = r < n ? ip[r + 1] - ip[r] : 0;
  const int w = wave_max_i(len);
  if (lane == 0) {
    const int64_t r0 = s * kSlice, r1 = r0 + kSlice < n ? r0 + kSlice : n;
    const int64_t snnz = (int64_t)ip[r1] - (int64_t)ip[r0];
    const bool irregular = (int64_t)kSlice * w > 2 * snnz + 1024 || w > (1 << 30);
    width[s] = irregular ? -1 : w;
    slots[s] = irregular ? 0 : (long long)kSlice * w;
    if (irregular) atomicAdd(nirr, 1ull);
    atomicMax(maxw, irregular ? -1 : w);
  }
}

// SELL-64 fill + compact image (sell_fill / compact_fill): one wave per slice
template <typename MV>
__global__ __launch_bounds__(kDb) void sell_fill_kernel(int64_t n, int64_t ns, const int32_t *__restrict__ ip,
                                                        const int32_t *__restrict__ ix, const MV *__restrict__ dv,
                                                        const long long *__restrict__ sptr, const int *__restrict__ width,
                                                        int32_t *sidx, MV *sval, uint16_t *sdelta, int32_t *scbase,
                                                        unsigned *nocompact) {
  const int lane = threadIdx.x & 63;
  const int64_t s = ((int64_t)blockIdx.x * kDb + threadIdx.x) >> 6;
  if (s >= ns) return;
  const int w = width[s];
  if (w <= 0) return;
  const int64_t base = sptr[s];
  const int64_t r = s * kSlice + lane;
  const int len = r < n ? ip[r + 1] - ip[r] : 0;
  const int64_t e0 = r < n ? ip[r] : 0;
  bool span_ok = true;
  for (int j = 0; j < w; ++j) {
    const bool valid = j < len;
    const int32_t c = valid ? ix[e0 + j] : -1;
    const int64_t q = base + (int64_t)j * kSlice + lane;
    sidx[q] = c;
    sval[q] = valid ? dv[e0 + j] : MV(0);
    int mn = wave_min_i(valid ? c : INT32_MAX);
    const int mx = wave_max_i(valid ? c : -1);
    if (mx < 0) mn = 0;
    if (mx - mn > 65534) span_ok = false;
    if (lane == 0) scbase[base / kSlice + j] = mn;
    sdelta[q] = valid ? (uint16_t)(c - mn) : (uint16_t)0xFFFF;
  }
  if (!span_ok && lane == 0) atomicOr(nocompact, 1u);
}

template <typename T>
__global__ __launch_bounds__(kDb) void fill_kernel(T *a, int64_t count, T v) {
  for (int64_t i = (int64_t)blockIdx.x * kDb + threadIdx.x; i < count; i += (int64_t)gridDim.x * kDb) a[i] = v;
}

// DIA pass 1 (dia_build): one block per 128-row slice; the slice's offsets
// col - row sorted and made unique in LDS
__global__ __launch_bounds__(kDb) void dia_offsets_kernel(int64_t n, int64_t ns, const int32_t *__restrict__ ip,
                                                          const int32_t *__restrict__ ix, int *width, int *offs,
                                                          long long *slots, unsigned *fail, int *maxw) {
  __shared__ int buf[kDiaLdsEnt];
  __shared__ int pre[kDb];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t r0 = s * kDiaSlice, r1 = r0 + kDiaSlice < n ? r0 + kDiaSlice : n;
  const int32_t b0 = ip[r0];
  const int snnz = ip[r1] - b0;
  if (snnz > kDiaLdsEnt) {  // beyond this kernel's LDS: the host builder decides
    if (t == 0) atomicOr(fail, 2u);
    return;
  }
  int m = 1;
  while (m < snnz) m <<= 1;
  for (int i = t; i < m; i += kDb) buf[i] = INT32_MAX;
  __syncthreads();
  for (int64_t r = r0 + t; r < r1; r += kDb)
    for (int32_t e = ip[r]; e < ip[r + 1]; ++e) buf[e - b0] = (int)((int64_t)ix[e] - r);
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1)  // bitonic sort, ascending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < m; i += kDb) {
        const int p = i ^ j;
        if (p > i) {
          const int a = buf[i], b = buf[p];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            buf[i] = b;
            buf[p] = a;
          }
        }
      }
      __syncthreads();
    }
  // unique: entry i starts a new offset when it differs from i - 1; ranks by
  // a block scan over chunks of kDb
  int total = 0;
  for (int c0 = 0; c0 < snnz; c0 += kDb) {
    const int i = c0 + t;
    const int head = (i < snnz && (i == 0 || buf[i] != buf[i - 1])) ? 1 : 0;
    pre[t] = head;
    __syncthreads();
    for (int d = 1; d < kDb; d <<= 1) {
      const int v = t >= d ? pre[t - d] : 0;
      __syncthreads();
      pre[t] += v;
      __syncthreads();
    }
    const int rank = total + pre[t] - head;
    if (head && rank < kDiaWMax) offs[s * kDiaWMax + rank] = buf[i];
    const int add = pre[kDb - 1];
    __syncthreads();
    total += add;
  }
  if (t == 0) {
    if ((int64_t)total * kDiaSlice > 2 * (int64_t)snnz + 2048) atomicOr(fail, 1u);  // dia_build's refusal
    else if (total > kDiaWMax) atomicOr(fail, 2u);  // fits dia_build, not this kernel: the host builder decides
    width[s] = total;
    slots[s] = (long long)kDiaSlice * total;
    atomicMax(maxw, total);
  }
}

// DIA pass 2: one block per slice: slot column by binary search, lane mask
// bits in LDS, values (holes stay 0 from the fill before). Then (uniform != 0)
// wave q takes slot columns q, q + 4, ...: lane l reads back the values of
// rows 2l and 2l + 1 the block has just stored and compares their bits with
// those of the column's lowest present row; a ballot decides, so the flag, the
// value and the count do not depend on any order of execution.
template <typename MV>
__global__ __launch_bounds__(kDb) void dia_fill_kernel(int64_t n, const int32_t *__restrict__ ip,
                                                       const int32_t *__restrict__ ix, const MV *__restrict__ dv,
                                                       const long long *__restrict__ sptr, const int *__restrict__ width,
                                                       const int *__restrict__ offs, int32_t *doff, uint64_t *dmask,
                                                       MV *dval, int uniform, int32_t *uflag, MV *uval,
                                                       unsigned long long *nuniform) {
  using Bits = typename std::conditional<sizeof(MV) == 8, unsigned long long, unsigned>::type;
  __shared__ int o[kDiaWMax];
  __shared__ unsigned long long msk[2 * kDiaWMax];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int w = width[s];
  const int64_t base = sptr[s];
  const int64_t c0 = base / kDiaSlice;
  if (t < w) o[t] = offs[s * kDiaWMax + t];
  if (t < 2 * kDiaWMax) msk[t] = 0ull;
  __syncthreads();
  const int64_t r0 = s * kDiaSlice;
  if (t < kDiaSlice && r0 + t < n) {
    const int64_t r = r0 + t;
    for (int32_t e = ip[r]; e < ip[r + 1]; ++e) {
      const int off = (int)((int64_t)ix[e] - r);
      int lo = 0, hi = w;  // first o[j] >= off (present: the list holds every offset of the slice)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (o[mid] < off) lo = mid + 1;
        else hi = mid;
      }
      atomicOr(&msk[2 * lo + (t & 1)], 1ull << (t >> 1));
      dval[base + (int64_t)lo * kDiaSlice + t] = dv[e];
    }
  }
  __syncthreads();
  if (t < w) {
    doff[c0 + t] = o[t];
    dmask[2 * (c0 + t)] = msk[2 * t];
    dmask[2 * (c0 + t) + 1] = msk[2 * t + 1];
  }
  if (!uniform) return;
  // the block's own stores to dval are visible to it after the barrier above
  const int lane = t & 63;
  unsigned nu = 0;
  for (int j = t >> 6; j < w; j += kDb / 64) {
    const unsigned long long me = msk[2 * j], md = msk[2 * j + 1];
    if ((me | md) == 0ull) continue;
    const int le = me ? __ffsll((long long)me) - 1 : 64, ld = md ? __ffsll((long long)md) - 1 : 64;
    const int first = le <= ld ? 2 * le : 2 * ld + 1;  // the lowest present row
    const MV *cv = dval + base + (int64_t)j * kDiaSlice;
    const MV refv = cv[first];
    const Bits ref = __builtin_bit_cast(Bits, refv);
    const bool differ = (((me >> lane) & 1ull) && __builtin_bit_cast(Bits, cv[2 * lane]) != ref) ||
                        (((md >> lane) & 1ull) && __builtin_bit_cast(Bits, cv[2 * lane + 1]) != ref);
    if (__ballot(differ) == 0ull) {
      if (lane == 0) {
        uflag[c0 + j] = 1;
        uval[c0 + j] = refv;
      }
      ++nu;
    }
  }
  if (lane == 0 && nu) atomicAdd(nuniform, (unsigned long long)nu);
}

// Descriptor classes (dia_classes): a 64-bit hash of every slice's descriptor
// block, one thread per slice. The hash only groups; dia_class_verify_kernel
// decides equality on the bytes.
template <typename MV>
__device__ inline uint64_t uval_bits(MV v) {
  if constexpr (sizeof(MV) == 8) return (uint64_t)__double_as_longlong(v);
  else return (uint64_t)__float_as_uint(v);
}
__device__ inline uint64_t hash_mix(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
template <typename MV>
__global__ __launch_bounds__(kDb) void dia_class_hash_kernel(int64_t ns, const long long *__restrict__ sptr,
                                                             const int *__restrict__ width,
                                                             const int32_t *__restrict__ off,
                                                             const uint64_t *__restrict__ mask,
                                                             const int32_t *__restrict__ uflag,
                                                             const MV *__restrict__ uval, uint64_t *__restrict__ hash) {
  const int64_t s = (int64_t)blockIdx.x * kDb + threadIdx.x;
  if (s >= ns) return;
  const int64_t c0 = sptr[s] / kDiaSlice;
  const int w = width[s];
  uint64_t h = hash_mix(0x2545F4914F6CDD1Dull, (uint64_t)w);
  for (int64_t j = c0; j < c0 + w; ++j) {
    h = hash_mix(h, (uint32_t)off[j] | (uint64_t)(uint32_t)uflag[j] << 32);
    h = hash_mix(h, mask[2 * j]);
    h = hash_mix(h, mask[2 * j + 1]);
    h = hash_mix(h, uval_bits(uval[j]));
  }
  hash[s] = h;
}

// The class table: class k's block copied from its first slice's columns
// (rep_c0[k] ...) to the table's columns first[k] ..., one thread per class.
template <typename MV>
__global__ __launch_bounds__(kDb) void dia_class_gather_kernel(
    int64_t ncls, const long long *__restrict__ rep_c0, const int32_t *__restrict__ first,
    const int32_t *__restrict__ cwidth, const int32_t *__restrict__ off, const uint64_t *__restrict__ mask,
    const int32_t *__restrict__ uflag, const MV *__restrict__ uval, int32_t *__restrict__ toff,
    uint64_t *__restrict__ tmask, int32_t *__restrict__ tuflag, MV *__restrict__ tuval) {
  const int64_t k = (int64_t)blockIdx.x * kDb + threadIdx.x;
  if (k >= ncls) return;
  const int64_t c0 = rep_c0[k], t0 = first[k];
  for (int j = 0; j < cwidth[k]; ++j) {
    toff[t0 + j] = off[c0 + j];
    tmask[2 * (t0 + j)] = mask[2 * (c0 + j)];
    tmask[2 * (t0 + j) + 1] = mask[2 * (c0 + j) + 1];
    tuflag[t0 + j] = uflag[c0 + j];
    tuval[t0 + j] = uval[c0 + j];
  }
}

// Every slice's block against its class's block in the table, byte for byte
// (one thread per slice); any difference sets *bad.
template <typename MV>
__global__ __launch_bounds__(kDb) void dia_class_verify_kernel(
    int64_t ns, const long long *__restrict__ sptr, const int *__restrict__ width, const int32_t *__restrict__ word,
    const int32_t *__restrict__ off, const uint64_t *__restrict__ mask, const int32_t *__restrict__ uflag,
    const MV *__restrict__ uval, const int32_t *__restrict__ toff, const uint64_t *__restrict__ tmask,
    const int32_t *__restrict__ tuflag, const MV *__restrict__ tuval, unsigned *bad) {
  const int64_t s = (int64_t)blockIdx.x * kDb + threadIdx.x;
  if (s >= ns) return;
  const int64_t c0 = sptr[s] / kDiaSlice, t0 = word[2 * s];
  const int w = width[s];
  bool ok = word[2 * s + 1] == w;
  for (int j = 0; j < w && ok; ++j)
    ok = off[c0 + j] == toff[t0 + j] && mask[2 * (c0 + j)] == tmask[2 * (t0 + j)] &&
         mask[2 * (c0 + j) + 1] == tmask[2 * (t0 + j) + 1] && uflag[c0 + j] == tuflag[t0 + j] &&
         uval_bits(uval[c0 + j]) == uval_bits(tuval[t0 + j]);
  if (!ok) atomicOr(bad, 1u);
}

int grid_for_n(int64_t items, int per_block) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, (items + per_block - 1) / per_block));
}

// exclusive scan of cnt[0, m) into out[0, m] (out[m] = total)
void exclusive_scan(const long long *cnt, long long *out, int64_t m, hipStream_t st) {
  size_t tb = 0;
  KRY_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, out, (int)(m + 1), st));
  void *tmp = dev_alloc(tb + 16);
  try {
    KRY_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, out, (int)(m + 1), st));
  } catch (...) {
    dev_free(tmp);
    throw;
  }
  dev_free(tmp);
}

struct Tmp {
  void *p = nullptr;
  explicit Tmp(size_t b) : p(dev_alloc(b)) {}
  ~Tmp() { dev_free(p); }
  Tmp(const Tmp &) = delete;
  Tmp &operator=(const Tmp &) = delete;
  template <class T>
  T *as() const {
    return static_cast<T *>(p);
  }
  void *release() {
    void *q = p;
    p = nullptr;
    return q;
  }
};

template <typename T>
T read1(const T *d, hipStream_t st) {
  T v;
  KRY_HIP(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
  return v;
}

// The descriptor classes of the image just built (A->dia_*), byte-equal to
// dia_classes': the slices are grouped by their blocks' hashes on the host
// (one D2H copy of 20 bytes per slice), each group's first slice is its
// representative, the table is gathered from the representatives, and every
// slice is then verified against its class in the table byte for byte. A
// mismatch (two different blocks with one hash) records no classes.
template <typename MV>
void device_dia_classes(kry_csr *A, hipStream_t st) {
  const int64_t ns = A->dia_nslices, cols = A->dia_nslots / kDiaSlice;
  if (ns == 0) return;
  const auto *sptr = static_cast<const long long *>(A->dia_sptr);
  const auto *width = static_cast<const int *>(A->dia_width);
  const auto *off = static_cast<const int32_t *>(A->dia_off);
  const auto *mask = static_cast<const uint64_t *>(A->dia_mask);
  const auto *uflag = static_cast<const int32_t *>(A->dia_uflag);
  const auto *uval = static_cast<const MV *>(A->dia_uval);
  Tmp dhash((size_t)ns * 8);
  hipLaunchKernelGGL(dia_class_hash_kernel<MV>, dim3(grid_for_n(ns, kDb)), dim3(kDb), 0, st, ns, sptr, width, off, mask,
                     uflag, uval, dhash.as<uint64_t>());
  KRY_HIP(hipGetLastError());
  std::vector<uint64_t> hash(ns);
  std::vector<long long> hsptr(ns + 1);
  std::vector<int32_t> hwidth(ns);
  KRY_HIP(hipMemcpyAsync(hash.data(), dhash.p, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
  KRY_HIP(hipMemcpyAsync(hsptr.data(), sptr, (size_t)(ns + 1) * 8, hipMemcpyDeviceToHost, st));
  KRY_HIP(hipMemcpyAsync(hwidth.data(), width, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
  KRY_HIP(hipStreamSynchronize(st));
  const int64_t col_bytes = dia_class_col_bytes(sizeof(MV));
  std::unordered_map<uint64_t, int32_t> cls_of;  // hash -> class
  std::vector<long long> rep_c0;
  std::vector<int32_t> first, cwidth, word(2 * ns);
  int64_t ccols = 0;
  for (int64_t s = 0; s < ns; ++s) {
    auto it = cls_of.find(hash[s]);
    if (it == cls_of.end()) {
      it = cls_of.emplace(hash[s], (int32_t)rep_c0.size()).first;
      rep_c0.push_back(hsptr[s] / kDiaSlice);
      first.push_back((int32_t)ccols);
      cwidth.push_back(hwidth[s]);
      ccols += hwidth[s];
      // as dia_classes refuses: not smaller than the per-slice descriptors, or past the L2 share
      if (ccols >= cols || ccols * col_bytes > kDiaClassMaxBytes) return;
    }
    word[2 * s] = first[it->second];
    word[2 * s + 1] = cwidth[it->second];
  }
  const int64_t ncls = (int64_t)rep_c0.size(), tc = ccols + kDiaPad;
  Tmp dword((size_t)ns * 8 + 16), toff((size_t)tc * 4), tmask((size_t)tc * 16), tuflag((size_t)tc * 4),
      tuval((size_t)tc * sizeof(MV)), drep((size_t)ncls * 8), dfirst((size_t)ncls * 4), dcw((size_t)ncls * 4), dbad(16);
  KRY_HIP(hipMemsetAsync(static_cast<char *>(dword.p) + (size_t)ns * 8, 0, 16, st));  // one word past the last slice
  KRY_HIP(hipMemsetAsync(toff.p, 0, (size_t)tc * 4, st));
  KRY_HIP(hipMemsetAsync(tmask.p, 0, (size_t)tc * 16, st));
  KRY_HIP(hipMemsetAsync(tuflag.p, 0, (size_t)tc * 4, st));
  KRY_HIP(hipMemsetAsync(tuval.p, 0, (size_t)tc * sizeof(MV), st));
  KRY_HIP(hipMemsetAsync(dbad.p, 0, 16, st));
  KRY_HIP(hipMemcpyAsync(dword.p, word.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st));
  KRY_HIP(hipMemcpyAsync(drep.p, rep_c0.data(), (size_t)ncls * 8, hipMemcpyHostToDevice, st));
  KRY_HIP(hipMemcpyAsync(dfirst.p, first.data(), (size_t)ncls * 4, hipMemcpyHostToDevice, st));
  KRY_HIP(hipMemcpyAsync(dcw.p, cwidth.data(), (size_t)ncls * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dia_class_gather_kernel<MV>, dim3(grid_for_n(ncls, kDb)), dim3(kDb), 0, st, ncls,
                     drep.as<const long long>(), dfirst.as<const int32_t>(), dcw.as<const int32_t>(), off, mask, uflag,
                     uval, toff.as<int32_t>(), tmask.as<uint64_t>(), tuflag.as<int32_t>(), tuval.as<MV>());
  hipLaunchKernelGGL(dia_class_verify_kernel<MV>, dim3(grid_for_n(ns, kDb)), dim3(kDb), 0, st, ns, sptr, width,
                     dword.as<const int32_t>(), off, mask, uflag, uval, toff.as<const int32_t>(),
                     tmask.as<const uint64_t>(), tuflag.as<const int32_t>(), tuval.as<const MV>(), dbad.as<unsigned>());
  KRY_HIP(hipGetLastError());
  if (read1(dbad.as<const unsigned>(), st) != 0) return;  // (the sync also keeps the host vectors alive long enough)
  A->dia_ncls = ncls;
  A->dia_cls_cols = ccols;
  A->dia_cls_word = dword.release();
  A->dia_cls_off = toff.release();
  A->dia_cls_mask = tmask.release();
  A->dia_cls_uflag = tuflag.release();
  A->dia_cls_uval = tuval.release();
}

}  // namespace

template <typename MV>
int device_image_build(kry_csr *A, const int32_t *ip, const int32_t *ix, const MV *dv, bool renumber_candidates,
                       DeviceCsrFlags *out) {
  hipStream_t st = A->ctx->stream;
  const int64_t n = A->n, nnz = A->nnz;
  KRY_REQUIRE(ip[0] == 0 && (int64_t)ip[n] == nnz, KRY_EINVAL, "indptr must start at 0 and end at nnz");
  // the caller's CSR, once
  Tmp dip((size_t)(n + 1) * 4 + 16), dix((size_t)nnz * 4 + 16), ddv((size_t)nnz * sizeof(MV) + 16);
  host_xfer(dip.p, ip, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st);
  host_xfer(dix.p, ix, (size_t)nnz * 4, hipMemcpyHostToDevice, st);
  host_xfer(ddv.p, dv, (size_t)nnz * sizeof(MV), hipMemcpyHostToDevice, st);
  Tmp small(256);
  KRY_HIP(hipMemsetAsync(small.p, 0, 256, st));
  unsigned *flags = small.as<unsigned>();
  unsigned long long *far = reinterpret_cast<unsigned long long *>(small.as<char>() + 16);
  const int64_t cols = std::max<int64_t>(int64_t(1) << 18, (n + 15) / 16);
  hipLaunchKernelGGL(csr_check_kernel, dim3(grid_for_n(n, kDb)), dim3(kDb), 0, st, n, nnz, dip.as<int32_t>(),
                     dix.as<int32_t>(), cols / 2, flags, far);
  KRY_HIP(hipGetLastError());
  const unsigned f = read1(flags, st);
  const unsigned long long nfar = read1(far, st);
  KRY_REQUIRE(!(f & F_INDPTR), KRY_EINVAL, "indptr must be non-decreasing");
  KRY_REQUIRE(!(f & F_RANGE), KRY_EINVAL, "column index out of range [0, n)");
  out->strictly_sorted = !(f & F_UNSORTED);
  out->sorted = !(f & F_UNSORTED_NS);
  out->scattered = n * 8 >= (int64_t(8) << 20) && nnz > 0 && (int64_t)nfar * 4 >= nnz;
  if (out->scattered && renumber_candidates) return 0;  // the renumbering path (host images)
  // ---- SELL-64 (+ compact)
  const int64_t ns = (n + kSlice - 1) / kSlice;
  Tmp cnt((size_t)(ns + 1) * 8 + 16);
  KRY_HIP(hipMemsetAsync(cnt.p, 0, (size_t)(ns + 1) * 8, st));
  void *swidth = dev_alloc((size_t)ns * 4 + 4);
  A->swidth = swidth;
  unsigned long long *nirr = reinterpret_cast<unsigned long long *>(small.as<char>() + 32);
  int *maxw = reinterpret_cast<int *>(small.as<char>() + 48);
  fill_kernel<int><<<1, 1, 0, st>>>(maxw, 1, -1);
  hipLaunchKernelGGL(sell_plan_kernel, dim3(grid_for_n(ns * 64, kDb)), dim3(kDb), 0, st, n, ns, dip.as<int32_t>(),
                     static_cast<int *>(swidth), cnt.as<long long>(), nirr, maxw);
  A->sptr = dev_alloc((size_t)(ns + 1) * 8);
  exclusive_scan(cnt.as<long long>(), static_cast<long long *>(A->sptr), ns, st);
  A->nslices = ns;
  A->nslots = read1(static_cast<const long long *>(A->sptr) + ns, st);
  A->nirregular = (int64_t)read1(nirr, st);
  A->max_width = read1(maxw, st);
  const int64_t slots = A->nslots;
  Tmp sidx((size_t)(slots + 256) * 4);
  A->sval = dev_alloc((size_t)(slots + 256) * sizeof(MV));
  Tmp sdelta((size_t)(slots + 256) * 2 + 16);
  Tmp scbase((size_t)(slots / kSlice + 16) * 4);
  fill_kernel<int32_t><<<grid_for_n(slots + 256, kDb), kDb, 0, st>>>(sidx.as<int32_t>(), slots + 256, -1);
  fill_kernel<MV><<<grid_for_n(slots + 256, kDb), kDb, 0, st>>>(static_cast<MV *>(A->sval), slots + 256, MV(0));
  fill_kernel<uint16_t><<<grid_for_n(slots + 256, kDb), kDb, 0, st>>>(sdelta.as<uint16_t>(), slots + 256, (uint16_t)0xFFFF);
  KRY_HIP(hipMemsetAsync(scbase.p, 0, (size_t)(slots / kSlice + 16) * 4, st));
  unsigned *nocompact = small.as<unsigned>() + 16;
  if (slots > 0)
    hipLaunchKernelGGL(sell_fill_kernel<MV>, dim3(grid_for_n(ns * 64, kDb)), dim3(kDb), 0, st, n, ns, dip.as<int32_t>(),
                       dix.as<int32_t>(), ddv.as<MV>(), static_cast<const long long *>(A->sptr),
                       static_cast<const int *>(swidth), sidx.as<int32_t>(), static_cast<MV *>(A->sval),
                       sdelta.as<uint16_t>(), scbase.as<int32_t>(), nocompact);
  KRY_HIP(hipGetLastError());
  const char *cenv = getenv("KRY_SELL_COMPACT");
  A->compact = !(cenv && atoi(cenv) == 0) && slots > 0 && read1(nocompact, st) == 0;
  if (A->compact) {
    A->sdelta = sdelta.release();
    A->scbase = scbase.release();
  } else {
    A->sidx = sidx.release();
  }
  // ---- SELL-128 diagonal-offset image
  const char *denv = getenv("KRY_SPMV_DIA");
  bool dia = out->strictly_sorted && !(denv && atoi(denv) == 0) && n > 0;
  bool host_dia = false;
  if (dia) {
    const int64_t dns = (n + kDiaSlice - 1) / kDiaSlice;
    unsigned *dfail = small.as<unsigned>() + 20;
    int *dmaxw = reinterpret_cast<int *>(small.as<char>() + 96);
    Tmp dcnt((size_t)(dns + 1) * 8 + 16), offs((size_t)dns * kDiaWMax * 4 + 16);
    KRY_HIP(hipMemsetAsync(dcnt.p, 0, (size_t)(dns + 1) * 8, st));
    Tmp dwidth((size_t)dns * 4 + 4);
    hipLaunchKernelGGL(dia_offsets_kernel, dim3((unsigned)dns), dim3(kDb), 0, st, n, dns, dip.as<int32_t>(),
                       dix.as<int32_t>(), dwidth.as<int>(), offs.as<int>(), dcnt.as<long long>(), dfail, dmaxw);
    KRY_HIP(hipGetLastError());
    const unsigned df = read1(dfail, st);
    if (df & 1u) dia = false;  // refused, as dia_build would
    if (!(df & 1u) && (df & 2u)) host_dia = true;
    if (df == 0) {
      Tmp dsptr((size_t)(dns + 1) * 8);
      exclusive_scan(dcnt.as<long long>(), dsptr.as<long long>(), dns, st);
      const int64_t dslots = read1(dsptr.as<long long>() + dns, st);
      const int dmw = read1(dmaxw, st);
      // the 128-row slices may hold up to one slice more padding than SELL-64's
      if (!(dslots * 4 > slots * 5 + (int64_t)4 * kDiaSlice * dmw)) {
        const int64_t dcols = dslots / kDiaSlice;
        Tmp doff((size_t)(dcols + kDiaPad) * 4), dmask((size_t)2 * (dcols + kDiaPad) * 8),
            dval((size_t)(dslots + 2 * kDiaSlice) * sizeof(MV)), duflag((size_t)(dcols + kDiaPad) * 4),
            duval((size_t)(dcols + kDiaPad) * sizeof(MV));
        unsigned long long *dnuni = reinterpret_cast<unsigned long long *>(small.as<char>() + 112);
        KRY_HIP(hipMemsetAsync(duflag.p, 0, (size_t)(dcols + kDiaPad) * 4, st));
        KRY_HIP(hipMemsetAsync(duval.p, 0, (size_t)(dcols + kDiaPad) * sizeof(MV), st));
        KRY_HIP(hipMemsetAsync(doff.p, 0, (size_t)(dcols + kDiaPad) * 4, st));
        KRY_HIP(hipMemsetAsync(dmask.p, 0, (size_t)2 * (dcols + kDiaPad) * 8, st));
        KRY_HIP(hipMemsetAsync(dval.p, 0, (size_t)(dslots + 2 * kDiaSlice) * sizeof(MV), st));
        hipLaunchKernelGGL(dia_fill_kernel<MV>, dim3((unsigned)dns), dim3(kDb), 0, st, n, dip.as<int32_t>(),
                           dix.as<int32_t>(), ddv.as<MV>(), dsptr.as<const long long>(), dwidth.as<const int>(),
                           offs.as<const int>(), doff.as<int32_t>(), dmask.as<uint64_t>(), dval.as<MV>(),
                           env_off("KRY_DIA_UNIFORM") ? 0 : 1, duflag.as<int32_t>(), duval.as<MV>(), dnuni);
        KRY_HIP(hipGetLastError());
        A->dia_nuniform = (int64_t)read1(dnuni, st);
        A->dia = true;
        A->dia_nslices = dns;
        A->dia_nslots = dslots;
        A->dia_max_width = dmw;
        A->dia_sptr = dsptr.release();
        A->dia_width = dwidth.release();
        A->dia_off = doff.release();
        A->dia_mask = dmask.release();
        A->dia_val = dval.release();
        A->dia_uflag = duflag.release();
        A->dia_uval = duval.release();
        device_dia_classes<MV>(A, st);
      }
    }
  }
  if (A->nirregular > 0) {  // the irregular slices walk the CSR arrays: keep them
    A->indptr = dip.release();
    A->indices = dix.release();
    A->data = ddv.release();
  }
  KRY_HIP(hipStreamSynchronize(st));
  return A->dia ? 1 : (host_dia ? 3 : 2);
}

template int device_image_build<double>(kry_csr *, const int32_t *, const int32_t *, const double *, bool,
                                        DeviceCsrFlags *);
template int device_image_build<float>(kry_csr *, const int32_t *, const int32_t *, const float *, bool,
                                       DeviceCsrFlags *);

}  // namespace kry
