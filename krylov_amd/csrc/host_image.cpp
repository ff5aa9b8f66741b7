// Host-side image builders and host-only plans (see host_image.hpp). Plain
// C++: the library links this translation unit, and `make sanitize` builds it
// alone with ASan + UBSan and with TSan (the builders run multi-threaded, and
// release_later frees staging memory on a detached thread).
#include "host_image.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <type_traits>
#include <unordered_map>

namespace kry {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

// A staging vector's pages are returned on a detached thread once its H2D
// copies have completed (the caller has synchronised the stream): unmapping
// ~1 GB takes ~0.1 s that kry_csr_create then does not wait for.
template <class T>
void release_later(hvec<T> &v) {
  if (v.capacity() < (size_t(64) << 20) / sizeof(T)) {
    hvec<T>().swap(v);
    return;
  }
  auto *h = new hvec<T>();
  h->swap(v);
  std::thread([h] { delete h; }).detach();
}

template <class T>
static void par_fill(hvec<T> &v, size_t n, T val) {
  v.resize(n);
  const unsigned nt = n < (size_t(1) << 20) ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (nt == 1) {
    std::fill(v.begin(), v.end(), val);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&, t] { std::fill(v.data() + n * t / nt, v.data() + n * (t + 1) / nt, val); });
  for (auto &x : th) x.join();
}

template <typename I>
void check_csr(int64_t n, int64_t nnz, const I *ip, const I *ix) {
  KRY_REQUIRE(n >= 0 && nnz >= 0 && ip, KRY_EINVAL, "bad CSR arguments");
  KRY_REQUIRE(ip[0] == 0 && (int64_t)ip[n] == nnz, KRY_EINVAL, "indptr must start at 0 and end at nnz");
  KRY_REQUIRE(nnz == 0 || ix, KRY_EINVAL, "null indices");
  const unsigned nt = n + nnz < (int64_t(1) << 20) ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::atomic<int> bad{0};  // 1: indptr decreases, 2: a column out of range
  auto work = [&](unsigned t) {
    const int64_t r0 = n * t / nt, r1 = n * (t + 1) / nt;
    for (int64_t r = r0; r < r1; ++r)
      if (ip[r + 1] < ip[r]) {
        bad = 1;
        return;
      }
    // the rows are monotone here; the entries of [r0, r1) are [ip[r0], ip[r1])
    const int64_t e0 = (int64_t)ip[r0], e1 = (int64_t)ip[r1];
    for (int64_t e = e0; e < e1; ++e)
      if (ix[e] < 0 || (int64_t)ix[e] >= n) {
        bad = 2;
        return;
      }
  };
  if (nt == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto &x : th) x.join();
  }
  KRY_REQUIRE(bad != 1, KRY_EINVAL, "indptr must be non-decreasing");
  KRY_REQUIRE(bad != 2, KRY_EINVAL, "column index out of range [0, n)");
}

// ---------------------------------------------------------- SELL-64 layout
// Host-side plan: slice s = rows [64 s, 64 s + 64); width = longest row;
// a slice is irregular (CSR walk) when 64 * width > 2 * nnz_slice + 1024.
template <typename I>
void sell_plan(int64_t n, const I *ip, std::vector<int64_t> *sptr, std::vector<int32_t> *width,
                      int64_t *nslices, int64_t *nslots, int64_t *nirr) {
  const int64_t ns = (n + kSlice - 1) / kSlice;
  if (sptr) sptr->assign(ns + 1, 0);
  if (width) width->assign(ns, 0);
  int64_t slots = 0, irr = 0;
  for (int64_t s = 0; s < ns; ++s) {
    const int64_t r0 = s * kSlice, r1 = std::min<int64_t>(n, r0 + kSlice);
    int64_t w = 0;
    for (int64_t r = r0; r < r1; ++r) w = std::max<int64_t>(w, (int64_t)ip[r + 1] - (int64_t)ip[r]);
    const int64_t snnz = (int64_t)ip[r1] - (int64_t)ip[r0];
    const bool irregular = kSlice * w > 2 * snnz + 1024 || w > (int64_t(1) << 30);
    if (irregular) ++irr;
    if (width) (*width)[s] = irregular ? -1 : (int32_t)w;
    if (!irregular) slots += kSlice * w;
    if (sptr) (*sptr)[s + 1] = slots;
  }
  *nslices = ns;
  *nslots = slots;
  *nirr = irr;
}

template <typename I, typename MV>
void sell_fill(int64_t n, const I *ip, const I *ix, const MV *dv, const std::vector<int64_t> &sptr,
                      const std::vector<int32_t> &width, hvec<I> &sidx, hvec<MV> &sval) {
  const int64_t ns = (int64_t)width.size();
  const int64_t slots = sptr[ns];
  par_fill(sidx, slots + 256, I(-1));
  par_fill(sval, slots + 256, MV(0));
  auto work = [&](int64_t sa, int64_t sb) {
    for (int64_t s = sa; s < sb; ++s) {
      if (width[s] < 0) continue;
      const int64_t base = sptr[s];
      const int64_t r0 = s * kSlice, r1 = std::min<int64_t>(n, r0 + kSlice);
      for (int64_t r = r0; r < r1; ++r) {
        const int64_t lane = r - r0;
        int64_t j = 0;
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e, ++j) {
          sidx[base + j * kSlice + lane] = ix[e];
          sval[base + j * kSlice + lane] = dv[e];
        }
      }
    }
  };
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (ns < 4096) nt = 1;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, ns * t / nt, ns * (t + 1) / nt);
  for (auto &x : th) x.join();
}
// Compact column image: for every slot column (slice s, column j) the base is
// the smallest column index among its lanes and every lane stores col - base
// as uint16 (0xFFFF = padding). Possible when each slot column spans at most
// 65534 columns (banded and stencil matrices); the gathers then read 2 B of
// index per nonzero instead of 4. Returns false (nothing built) otherwise.
template <typename I>
bool compact_fill(const std::vector<int64_t> &sptr, const std::vector<int32_t> &width,
                         const hvec<I> &sidx, hvec<uint16_t> &sdelta, std::vector<int32_t> &scbase) {
  const int64_t ns = (int64_t)width.size();
  const int64_t slots = sptr[ns];
  par_fill(sdelta, slots + 256, (uint16_t)0xFFFF);
  scbase.assign(slots / kSlice + 16, 0);
  std::atomic<bool> ok{true};
  auto work = [&](int64_t sa, int64_t sb) {
    for (int64_t s = sa; s < sb && ok.load(std::memory_order_relaxed); ++s) {
      const int64_t base = sptr[s];
      for (int64_t j = 0; j < width[s]; ++j) {
        const I *c = sidx.data() + base + j * kSlice;
        int64_t mn = INT64_MAX, mx = -1;
        for (int l = 0; l < kSlice; ++l)
          if (c[l] >= 0) {
            mn = std::min<int64_t>(mn, c[l]);
            mx = std::max<int64_t>(mx, c[l]);
          }
        if (mx < 0) mn = 0;
        if (mx - mn > 65534 || mn > INT32_MAX) {
          ok = false;
          return;
        }
        scbase[base / kSlice + j] = (int32_t)mn;
        uint16_t *d = sdelta.data() + base + j * kSlice;
        for (int l = 0; l < kSlice; ++l)
          if (c[l] >= 0) d[l] = (uint16_t)(c[l] - mn);
      }
    }
  };
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (ns < 4096) nt = 1;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, ns * t / nt, ns * (t + 1) / nt);
  for (auto &x : th) x.join();
  return ok.load();
}

// Diagonal-offset image (see kry_csr::dia_*). Pass 1 collects every slice's
// sorted offset list (col - row over its entries) and checks that each row is
// strictly sorted, so a row's entries occur in the slot order of their
// offsets: the per-row summation order stays the stored order (bitwise
// csr_matvec). Pass 2 places entry (row, col) in the slot column of offset
// col - row and sets the row's mask bit. Returns false (nothing built) for
// unsorted or duplicate entries, or when the image would hold more than
// 1.25x the SELL image's slots (offsets not shared across the slice's rows).
// With `uniform`, pass 2 also flags every slot column whose present rows (the
// mask bits; holes take no part) all store one bit pattern, and keeps that
// value beside the flag (kry_csr::dia_uflag / dia_uval): bits are compared,
// so -0.0 differs from +0.0 and NaNs compare by payload; a slot column with
// one present row is uniform. A column that is not flagged keeps value 0.

namespace {
template <typename MV>
inline uint64_t value_bits(MV v) {
  typename std::conditional<sizeof(MV) == 8, uint64_t, uint32_t>::type b;
  std::memcpy(&b, &v, sizeof(MV));
  return b;
}
}  // namespace

template <typename I, typename MV>
bool dia_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, DiaHost<MV> &d, bool uniform) {
  if (sizeof(I) != 4 || n == 0) return false;
  constexpr int H = kDiaSlice;
  const int64_t ns = (n + H - 1) / H;
  std::vector<std::vector<int32_t>> offs(ns);
  std::atomic<bool> ok{true};
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (ns < 2048) nt = 1;
  auto pass1 = [&](int64_t sa, int64_t sb) {
    std::vector<int32_t> o;
    for (int64_t s = sa; s < sb && ok.load(std::memory_order_relaxed); ++s) {
      const int64_t r0 = s * H, r1 = std::min<int64_t>(n, r0 + H);
      o.clear();
      for (int64_t r = r0; r < r1; ++r) {
        // a row whose offsets repeat the previous row's adds nothing new to
        // the list (stencil rows, away from the grid's faces): checked
        // against it entry by entry, not pushed
        const int64_t len = (int64_t)ip[r + 1] - (int64_t)ip[r];
        bool same = r > r0 && len == (int64_t)ip[r] - (int64_t)ip[r - 1];
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
          if (e > ip[r] && ix[e] <= ix[e - 1]) {  // unsorted or duplicate: stored order is not offset order
            ok = false;
            return;
          }
          same = same && (int64_t)ix[e] - r == (int64_t)ix[e - len] - (r - 1);
        }
        if (!same)
          for (int64_t e = ip[r]; e < ip[r + 1]; ++e) o.push_back((int32_t)((int64_t)ix[e] - r));
      }
      std::sort(o.begin(), o.end());
      o.erase(std::unique(o.begin(), o.end()), o.end());
      if ((int64_t)o.size() * H > 2 * ((int64_t)ip[r1] - (int64_t)ip[r0]) + 2048) {
        ok = false;  // offsets not shared across the slice's rows
        return;
      }
      offs[s] = o;
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(pass1, ns * t / nt, ns * (t + 1) / nt);
    for (auto &x : th) x.join();
  }
  if (!ok) return false;
  d.sptr.assign(ns + 1, 0);
  d.width.assign(ns, 0);
  for (int64_t s = 0; s < ns; ++s) {
    d.width[s] = (int32_t)offs[s].size();
    d.max_width = std::max(d.max_width, d.width[s]);
    d.sptr[s + 1] = d.sptr[s] + (int64_t)H * d.width[s];
  }
  const int64_t slots = d.sptr[ns];
  // the 128-row slices may hold up to one slice more padding than SELL-64's
  if (slots * 4 > sell_slots * 5 + (int64_t)4 * H * d.max_width) return false;
  const int64_t cols = slots / H;
  d.off.assign(cols + kDiaPad, 0);
  par_fill(d.mask, 2 * (cols + kDiaPad), (uint64_t)0);
  par_fill(d.val, slots + 2 * H, MV(0));
  d.uflag.assign(cols + kDiaPad, 0);
  d.uval.assign(cols + kDiaPad, MV(0));
  std::atomic<int64_t> nuniform{0};
  auto pass2 = [&](int64_t sa, int64_t sb) {
    int64_t nu = 0;
    for (int64_t s = sa; s < sb; ++s) {
      const std::vector<int32_t> &o = offs[s];
      const int64_t base = d.sptr[s], c0 = base / H;
      for (size_t j = 0; j < o.size(); ++j) d.off[c0 + j] = o[j];
      const int64_t r0 = s * H, r1 = std::min<int64_t>(n, r0 + H);
      for (int64_t r = r0; r < r1; ++r) {
        const int rl = (int)(r - r0);
        size_t j = 0;
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
          const int32_t off = (int32_t)((int64_t)ix[e] - r);
          while (o[j] != off) ++j;  // the row's offsets ascend, as the list's do
          d.mask[2 * (c0 + j) + (rl & 1)] |= uint64_t(1) << (rl >> 1);
          d.val[base + (int64_t)j * H + rl] = dv[e];
          ++j;
        }
      }
      if (!uniform) continue;
      for (size_t j = 0; j < o.size(); ++j) {
        const uint64_t m[2] = {d.mask[2 * (c0 + j)], d.mask[2 * (c0 + j) + 1]};
        const MV *v = d.val.data() + base + (int64_t)j * H;
        int first = -1;  // the lowest present row
        bool same = true;
        for (int rl = 0; rl < H && same; ++rl) {
          if (!((m[rl & 1] >> (rl >> 1)) & 1u)) continue;
          if (first < 0) first = rl;
          same = value_bits(v[rl]) == value_bits(v[first]);
        }
        if (first >= 0 && same) {
          d.uflag[c0 + j] = 1;
          d.uval[c0 + j] = v[first];
          ++nu;
        }
      }
    }
    nuniform += nu;
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(pass2, ns * t / nt, ns * (t + 1) / nt);
    for (auto &x : th) x.join();
  }
  d.nuniform = nuniform.load();
  return true;
}

// Descriptor classes (DiaClassHost): an exact map over the block bytes. A
// 64-bit hash per slice (threaded) only picks the bucket; within a bucket a
// block is compared field by field with every class already there, so two
// slices share a class exactly when their blocks are byte-equal.
template <typename MV>
bool dia_classes(const DiaHost<MV> &d, DiaClassHost<MV> &c) {
  c = DiaClassHost<MV>();
  const int64_t ns = (int64_t)d.width.size();
  if (ns == 0) return false;
  const int64_t cols = d.sptr[ns] / kDiaSlice;
  std::vector<uint64_t> hash(ns);
  auto mix = [](uint64_t h, uint64_t v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
  };
  auto hpass = [&](int64_t sa, int64_t sb) {
    for (int64_t s = sa; s < sb; ++s) {
      const int64_t c0 = d.sptr[s] / kDiaSlice;
      uint64_t h = mix(0x2545F4914F6CDD1Dull, (uint64_t)d.width[s]);
      for (int64_t j = c0; j < c0 + d.width[s]; ++j) {
        h = mix(h, (uint32_t)d.off[j] | (uint64_t)(uint32_t)d.uflag[j] << 32);
        h = mix(h, d.mask[2 * j]);
        h = mix(h, d.mask[2 * j + 1]);
        h = mix(h, value_bits(d.uval[j]));
      }
      hash[s] = h;
    }
  };
  {
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (ns < 2048) nt = 1;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(hpass, ns * t / nt, ns * (t + 1) / nt);
    for (auto &x : th) x.join();
  }
  auto same = [&](int64_t a, int64_t b) {  // slices a and b: byte-equal blocks
    const int w = d.width[a];
    if (w != d.width[b]) return false;
    const int64_t ca = d.sptr[a] / kDiaSlice, cb = d.sptr[b] / kDiaSlice;
    return std::memcmp(&d.off[ca], &d.off[cb], (size_t)w * 4) == 0 &&
           std::memcmp(&d.mask[2 * ca], &d.mask[2 * cb], (size_t)w * 16) == 0 &&
           std::memcmp(&d.uflag[ca], &d.uflag[cb], (size_t)w * 4) == 0 &&
           std::memcmp(&d.uval[ca], &d.uval[cb], (size_t)w * sizeof(MV)) == 0;
  };
  const int64_t col_bytes = dia_class_col_bytes(sizeof(MV));
  std::unordered_multimap<uint64_t, int32_t> bucket;  // hash -> class
  std::vector<int64_t> rep;                           // class -> its first slice
  std::vector<int32_t> first;                         // class -> its first column in the table
  std::vector<int32_t> cls(ns);
  int64_t ccols = 0;
  for (int64_t s = 0; s < ns; ++s) {
    int32_t k = -1;
    auto range = bucket.equal_range(hash[s]);
    for (auto it = range.first; it != range.second && k < 0; ++it)
      if (same(rep[it->second], s)) k = it->second;
    if (k < 0) {
      k = (int32_t)rep.size();
      rep.push_back(s);
      first.push_back((int32_t)ccols);
      bucket.emplace(hash[s], k);
      ccols += d.width[s];
      // not smaller than the per-slice descriptors, or past the L2 share: no classes
      if (ccols >= cols || ccols * col_bytes > kDiaClassMaxBytes) return false;
    }
    cls[s] = k;
  }
  if (ccols >= cols) return false;
  c.nclasses = (int64_t)rep.size();
  c.ncols = ccols;
  c.word.resize(2 * ns);
  for (int64_t s = 0; s < ns; ++s) {
    c.word[2 * s] = first[cls[s]];
    c.word[2 * s + 1] = d.width[s];
  }
  c.off.assign(ccols + kDiaPad, 0);
  c.mask.assign(2 * (ccols + kDiaPad), 0);
  c.uflag.assign(ccols + kDiaPad, 0);
  c.uval.assign(ccols + kDiaPad, MV(0));
  for (size_t k = 0; k < rep.size(); ++k) {
    const int64_t c0 = d.sptr[rep[k]] / kDiaSlice;
    const int w = d.width[rep[k]];
    std::copy_n(&d.off[c0], w, &c.off[first[k]]);
    std::copy_n(&d.mask[2 * c0], 2 * w, &c.mask[2 * (int64_t)first[k]]);
    std::copy_n(&d.uflag[c0], w, &c.uflag[first[k]]);
    std::copy_n(&d.uval[c0], w, &c.uval[first[k]]);
  }
  return true;
}


// ------------------------------------------- bandwidth-reducing renumbering
// A fork-join team for the level-synchronous passes: up to 16 threads that
// live for one rcm_order call and meet at a spin barrier per level (a few
// microseconds; a thread start per level would cost ~50 us each).
namespace {
struct Team {
  unsigned nt;
  std::vector<std::thread> th;
  std::atomic<unsigned> gen{0}, left{0};
  std::atomic<bool> quit{false};
  std::function<void(unsigned)> job;
  explicit Team(unsigned want) : nt(std::max(1u, want)) {
    for (unsigned t = 1; t < nt; ++t)
      th.emplace_back([this, t] {
        unsigned seen = 0;
        for (;;) {
          unsigned g;
          while ((g = gen.load(std::memory_order_acquire)) == seen) {
            if (quit.load(std::memory_order_acquire)) return;
            std::this_thread::yield();
          }
          seen = g;
          job(t);
          left.fetch_sub(1, std::memory_order_acq_rel);
        }
      });
  }
  void run(const std::function<void(unsigned)> &f) {
    if (nt == 1) {
      f(0);
      return;
    }
    job = f;
    left.store(nt - 1, std::memory_order_release);
    gen.fetch_add(1, std::memory_order_acq_rel);
    f(0);
    while (left.load(std::memory_order_acquire) != 0) std::this_thread::yield();
  }
  ~Team() {
    quit.store(true, std::memory_order_release);
    for (auto &x : th) x.join();
  }
};

// One BFS level step: level[] of the frontier's unvisited neighbours set to
// `next` (compare-and-swap: one owner each); returns them, in thread order.
template <typename I>
void bfs_expand(Team &tm, const I *ip, const I *ix, const int32_t *front, int64_t nf, int32_t next,
                std::atomic<int32_t> *level, std::vector<std::vector<int32_t>> &loc, std::vector<int32_t> &out) {
  tm.run([&](unsigned t) {
    auto &v = loc[t];
    v.clear();
    const int64_t a = nf * t / tm.nt, b = nf * (t + 1) / tm.nt;
    for (int64_t q = a; q < b; ++q) {
      const int32_t u = front[q];
      for (int64_t e = ip[u]; e < ip[u + 1]; ++e) {
        const int32_t w = (int32_t)ix[e];
        int32_t expect = -1;
        if (level[w].load(std::memory_order_relaxed) == -1 &&
            level[w].compare_exchange_strong(expect, next, std::memory_order_relaxed))
          v.push_back(w);
      }
    }
  });
  out.clear();
  for (auto &v : loc) out.insert(out.end(), v.begin(), v.end());
}
}  // namespace

template <typename I>
bool scattered(int64_t n, const I *ip, const I *ix) {
  if (n * 8 < (int64_t(8) << 20)) return false;
  const int64_t nnz = (int64_t)ip[n];
  if (nnz == 0) return false;
  const int64_t cols = std::max<int64_t>(int64_t(1) << 18, (n + 15) / 16);
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<int64_t> far(nt, 0);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      const int64_t r0 = n * t / nt, r1 = n * (t + 1) / nt;
      int64_t f = 0;
      for (int64_t r = r0; r < r1; ++r)
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
          const int64_t d = (int64_t)ix[e] - r;
          f += (d > cols / 2 || d < -cols / 2);
        }
      far[t] = f;
    });
  for (auto &x : th) x.join();
  int64_t nfar = 0;
  for (int64_t f : far) nfar += f;
  return nfar * 4 >= nnz;
}

template <typename I>
bool rcm_order(int64_t n, const I *ip, const I *ix, int64_t wlimit, std::vector<int32_t> &perm, int64_t *levels) {
  if (n <= 0 || n >= (int64_t(1) << 31) - 1) return false;
  const unsigned nt = n < (int64_t(1) << 16) ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  Team tm(nt);
  std::vector<std::vector<int32_t>> loc(nt);
  std::unique_ptr<std::atomic<int32_t>[]> level(new std::atomic<int32_t>[n]);
  auto deg = [&](int64_t v) { return (int64_t)ip[v + 1] - (int64_t)ip[v]; };
  auto clear_levels = [&] {
    tm.run([&](unsigned t) {
      for (int64_t v = n * t / tm.nt; v < n * (t + 1) / tm.nt; ++v) level[v].store(-1, std::memory_order_relaxed);
    });
  };
  // levels-only BFS from `root`: the level count, and the last level's
  // smallest-degree (lowest-index) node; -1 if a level exceeds wlimit
  std::vector<int32_t> front, next;
  auto sweep = [&](int32_t root, int32_t *far_node) -> int64_t {
    clear_levels();
    level[root].store(0, std::memory_order_relaxed);
    front.assign(1, root);
    int64_t nl = 1;
    for (;;) {
      bfs_expand(tm, ip, ix, front.data(), (int64_t)front.size(), (int32_t)nl, level.get(), loc, next);
      if (next.empty()) break;
      if ((int64_t)next.size() > wlimit) return -1;
      front.swap(next);
      ++nl;
    }
    int32_t best = front[0];
    for (int32_t v : front)
      if (deg(v) < deg(best) || (deg(v) == deg(best) && v < best)) best = v;
    *far_node = best;
    return nl;
  };
  int32_t root = 0;
  for (int64_t v = 1; v < n; ++v)
    if (deg(v) < deg(root)) root = (int32_t)v;
  int32_t cand = root;
  int64_t ecc = sweep(root, &cand);
  if (ecc < 0) return false;
  static const int max_sweeps = [] {  // tuning override: George-Liu sweeps after the first BFS
    const char *e = getenv("KRY_RCM_SWEEPS");
    return e ? std::max(0, atoi(e)) : 3;
  }();
  for (int it = 0; it < max_sweeps && cand != root; ++it) {
    int32_t c2 = cand;
    const int64_t e2 = sweep(cand, &c2);
    if (e2 < 0) return false;
    if (e2 <= ecc) break;
    root = cand;
    ecc = e2;
    cand = c2;
  }
  // Cuthill-McKee numbering, level by level
  clear_levels();
  std::vector<int32_t> cm;
  cm.reserve(n);
  std::vector<int32_t> key(n, INT32_MAX);  // smallest parent number, written under the per-level owner rule below
  std::unique_ptr<std::atomic<int32_t>[]> akey(new std::atomic<int32_t>[n]);
  tm.run([&](unsigned t) {
    for (int64_t v = n * t / tm.nt; v < n * (t + 1) / tm.nt; ++v) akey[v].store(INT32_MAX, std::memory_order_relaxed);
  });
  int64_t scan = 0;  // lowest index that may still be unnumbered (new components)
  int64_t nlev = 0;
  std::vector<int64_t> cnt;
  while ((int64_t)cm.size() < n) {
    if (cm.empty()) {
      level[root].store(0, std::memory_order_relaxed);
      cm.push_back(root);
    } else {
      while (level[scan].load(std::memory_order_relaxed) != -1) ++scan;
      level[scan].store(0, std::memory_order_relaxed);
      cm.push_back((int32_t)scan);
    }
    int64_t a = (int64_t)cm.size() - 1, b = (int64_t)cm.size();  // the current level: numbers [a, b)
    ++nlev;
    for (;;) {
      // children of the level: claim (level = 1) and the smallest parent number
      tm.run([&](unsigned t) {
        auto &v = loc[t];
        v.clear();
        const int64_t qa = a + (b - a) * t / tm.nt, qb = a + (b - a) * (t + 1) / tm.nt;
        for (int64_t q = qa; q < qb; ++q) {
          const int32_t u = cm[q];
          for (int64_t e = ip[u]; e < ip[u + 1]; ++e) {
            const int32_t w = (int32_t)ix[e];
            int32_t expect = -1;
            if (level[w].load(std::memory_order_relaxed) == -1 &&
                level[w].compare_exchange_strong(expect, 1, std::memory_order_relaxed))
              v.push_back(w);
            if (level[w].load(std::memory_order_relaxed) == 1) {
              int32_t k = akey[w].load(std::memory_order_relaxed);
              while ((int32_t)q < k && !akey[w].compare_exchange_weak(k, (int32_t)q, std::memory_order_relaxed)) {
              }
            }
          }
        }
      });
      next.clear();
      for (auto &v : loc) next.insert(next.end(), v.begin(), v.end());
      if (next.empty()) break;
      if ((int64_t)next.size() > wlimit) return false;
      // counting sort by parent number, then (degree, index) within a parent
      const int64_t span = b - a;
      cnt.assign(span + 1, 0);
      for (int32_t w : next) cnt[akey[w].load(std::memory_order_relaxed) - a + 1]++;
      for (int64_t i = 0; i < span; ++i) cnt[i + 1] += cnt[i];
      front.resize(next.size());
      for (int32_t w : next) front[cnt[akey[w].load(std::memory_order_relaxed) - a]++] = w;
      int64_t i0 = 0;
      while (i0 < (int64_t)front.size()) {
        const int32_t k0 = akey[front[i0]].load(std::memory_order_relaxed);
        int64_t i1 = i0 + 1;
        while (i1 < (int64_t)front.size() && akey[front[i1]].load(std::memory_order_relaxed) == k0) ++i1;
        std::sort(front.begin() + i0, front.begin() + i1, [&](int32_t x, int32_t y) {
          return deg(x) != deg(y) ? deg(x) < deg(y) : x < y;
        });
        i0 = i1;
      }
      for (int32_t w : front) level[w].store(2, std::memory_order_relaxed);  // numbered
      a = (int64_t)cm.size();
      cm.insert(cm.end(), front.begin(), front.end());
      b = (int64_t)cm.size();
      ++nlev;
    }
  }
  (void)key;
  perm.resize(n);
  for (int64_t r = 0; r < n; ++r) perm[r] = cm[n - 1 - r];
  if (levels) *levels = nlev;
  return true;
}

template <typename I, typename MV>
void renumber_csr(int64_t n, const I *ip, const I *ix, const MV *dv, const std::vector<int32_t> &perm,
                  hvec<I> &ip2, hvec<I> &ix2, hvec<MV> &dv2) {
  std::vector<int32_t> iperm(n);
  for (int64_t r = 0; r < n; ++r) iperm[perm[r]] = (int32_t)r;
  ip2.resize(n + 1);
  ip2[0] = 0;
  for (int64_t r = 0; r < n; ++r) ip2[r + 1] = ip2[r] + (ip[perm[r] + 1] - ip[perm[r]]);
  const int64_t nnz = (int64_t)ip[n];
  ix2.resize(nnz + 1);
  dv2.resize(nnz + 1);
  const unsigned nt = n < (int64_t(1) << 16) ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int64_t r = n * t / nt; r < n * (t + 1) / nt; ++r) {
        const int64_t o = perm[r];
        int64_t q = (int64_t)ip2[r];
        for (int64_t e = ip[o]; e < ip[o + 1]; ++e, ++q) {
          ix2[q] = (I)iperm[ix[e]];
          dv2[q] = dv[e];
        }
      }
    });
  for (auto &x : th) x.join();
}

template <typename I, typename MV>
bool rs_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, RsHost<MV> &p) {
  constexpr int H = kPairSlice;
  if (n == 0 || n >= (int64_t(1) << 28) - 1) return false;
  const int64_t ns = (n + H - 1) / H;
  p.width.assign(ns, 0);
  p.sptr.assign(ns + 1, 0);
  for (int64_t s = 0; s < ns; ++s) {
    int64_t w = 0;
    for (int64_t r = s * H; r < std::min<int64_t>(n, (s + 1) * H); ++r) w = std::max<int64_t>(w, ip[r + 1] - ip[r]);
    if (w > INT32_MAX / H) return false;
    p.width[s] = (int32_t)w;
    p.max_width = std::max(p.max_width, (int)w);
    p.sptr[s + 1] = p.sptr[s] + H * w;
  }
  const int64_t slots = p.sptr[ns];
  if (slots == 0 || slots * 4 > sell_slots * 5 + (int64_t)4 * H * p.max_width) return false;
  par_fill(p.colrank, slots + 2 * H, 0xFFFFFFFFu);
  par_fill(p.val, slots + 2 * H, MV(0));
  auto fill = [&](int64_t sa, int64_t sb) {
    std::vector<std::pair<int64_t, int>> run;  // (column, position in run)
    for (int64_t s = sa; s < sb; ++s) {
      const int64_t r0 = s * H, r1 = std::min<int64_t>(n, r0 + H), base = p.sptr[s];
      for (int64_t r = r0; r < r1; ++r) {
        const int64_t e0 = (int64_t)ip[r], len = (int64_t)ip[r + 1] - e0;
        for (int64_t c0 = 0; c0 < len; c0 += kRsChunk) {
          const int m = (int)std::min<int64_t>(kRsChunk, len - c0);
          run.clear();
          for (int k = 0; k < m; ++k) run.emplace_back((int64_t)ix[e0 + c0 + k], k);
          std::stable_sort(run.begin(), run.end(),
                           [](const std::pair<int64_t, int> &x, const std::pair<int64_t, int> &y) { return x.first < y.first; });
          for (int j = 0; j < m; ++j) {
            const int64_t q = base + (c0 + j) * H + (r - r0);
            p.colrank[q] = (uint32_t)run[j].first | ((uint32_t)run[j].second << 28);
            p.val[q] = dv[e0 + c0 + run[j].second];
          }
        }
      }
    }
  };
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (ns < 2048) nt = 1;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(fill, ns * t / nt, ns * (t + 1) / nt);
  for (auto &x : th) x.join();
  return true;
}

// Host-only view of the diagonal-offset plan (kry_dia_plan): the image
// kry_csr_create would build for these CSR arrays, without a device.
template <typename I>
static void dia_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, int64_t *info, int32_t *widths,
                          int32_t *offsets, uint64_t *masks) {
  check_csr(n, nnz, ip, ix);
  int64_t ns = 0, sell_slots = 0, irr = 0;
  sell_plan(n, ip, nullptr, nullptr, &ns, &sell_slots, &irr);
  hvec<double> zeros;
  par_fill(zeros, (size_t)std::max<int64_t>(nnz, 1), 0.0);
  DiaHost<double> d;
  const bool built = dia_build(n, ip, ix, zeros.data(), sell_slots, d);
  info[0] = built ? 1 : 0;
  info[1] = built ? (int64_t)d.width.size() : 0;
  info[2] = built ? d.sptr.back() : 0;
  info[3] = built ? d.max_width : 0;
  if (!built) return;
  if (widths) std::copy(d.width.begin(), d.width.end(), widths);
  const int64_t cols = d.sptr.back() / kDiaSlice;
  if (offsets) std::copy(d.off.begin(), d.off.begin() + cols, offsets);
  if (masks) std::copy(d.mask.begin(), d.mask.begin() + 2 * cols, masks);
}

// Host-only view of the uniform slot columns dia_build finds
// (kry_dia_uniform_plan): info = {built, slot columns, uniform ones}, then the
// flag and the value of every slot column.
template <typename I, typename MV>
static void dia_uniform_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, const MV *dv, int64_t *info,
                                  int32_t *flags, MV *values) {
  check_csr(n, nnz, ip, ix);
  int64_t ns = 0, sell_slots = 0, irr = 0;
  sell_plan(n, ip, nullptr, nullptr, &ns, &sell_slots, &irr);
  DiaHost<MV> d;
  const bool built = dia_build(n, ip, ix, dv, sell_slots, d);
  const int64_t cols = built ? d.sptr.back() / kDiaSlice : 0;
  info[0] = built ? 1 : 0;
  info[1] = cols;
  info[2] = built ? d.nuniform : 0;
  if (!built) return;
  if (flags) std::copy(d.uflag.begin(), d.uflag.begin() + cols, flags);
  if (values) std::memcpy(values, d.uval.data(), (size_t)cols * sizeof(MV));
}

// Host-only view of the descriptor classes dia_classes finds
// (kry_dia_class_plan): info = {built, slot columns, classes, class-table
// columns}; the last two are 0 when the image takes no classes.
template <typename I, typename MV>
static void dia_class_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, const MV *dv, int uniform,
                                int64_t *info) {
  check_csr(n, nnz, ip, ix);
  int64_t ns = 0, sell_slots = 0, irr = 0;
  sell_plan(n, ip, nullptr, nullptr, &ns, &sell_slots, &irr);
  DiaHost<MV> d;
  const bool built = dia_build(n, ip, ix, dv, sell_slots, d, uniform != 0);
  DiaClassHost<MV> c;
  const bool cls = built && dia_classes(d, c);
  info[0] = built ? 1 : 0;
  info[1] = built ? d.sptr.back() / kDiaSlice : 0;
  info[2] = cls ? c.nclasses : 0;
  info[3] = cls ? c.ncols : 0;
}

// Column-blocked image (see kry_csr::cb_*). Returns false when not useful or
// not possible: rows not sorted, x small enough to stay cache-resident, the
// columns not scattered (most entries within half a block of the diagonal),
// or a segment too long for uint16 offsets.

template <typename I, typename MV>
bool cb_build(int64_t n, const I *ip, const I *ix, const MV *dv, CbHost<MV> &cb) {
  if (sizeof(I) != 4 || n * 8 < (int64_t(8) << 20)) return false;
  const int64_t nnz = (int64_t)ip[n];
  const char *cenv = getenv("KRY_CB_COLS");  // tuning override: columns per block
  int64_t cols = cenv ? std::max<int64_t>(1024, atoll(cenv)) : std::max<int64_t>(int64_t(1) << 18, (n + 15) / 16);
  const int64_t nb = (n + cols - 1) / cols;
  if (nb < 2) return false;
  // sorted rows and scattered columns
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<int64_t> far(nt, 0);
  std::atomic<bool> sorted{true};
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        const int64_t r0 = n * t / nt, r1 = n * (t + 1) / nt;
        int64_t f = 0;
        for (int64_t r = r0; r < r1; ++r)
          for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
            if (e > ip[r] && ix[e] < ix[e - 1]) sorted = false;
            const int64_t d = (int64_t)ix[e] - r;
            f += (d > cols / 2 || d < -cols / 2);
          }
        far[t] = f;
      });
    for (auto &x : th) x.join();
  }
  int64_t nfar = 0;
  for (int64_t f : far) nfar += f;
  if (!sorted || nnz == 0 || nfar * 4 < nnz) return false;
  const int64_t ng = (n + kCbRows - 1) / kCbRows;
  // the SpMV takes one launch per 16,384 groups (1024 blocks x 16 owned
  // groups) with 1024 block partials each, at most kMaxGridBlk = 32768 rows
  if (ng > 32 * 16384) return false;
  // per (block, row) counts -> per (block, group) segment lengths
  hvec<uint16_t> roff;
  par_fill(roff, nb * n + 256, (uint16_t)0);
  std::vector<int64_t> seg(nb * ng, 0);
  std::atomic<bool> fits{true};
  auto pass1 = [&](int64_t g0, int64_t g1) {
    std::vector<int64_t> cnt(nb);
    for (int64_t g = g0; g < g1; ++g) {
      std::fill(cnt.begin(), cnt.end(), 0);
      const int64_t r0 = g * kCbRows, r1 = std::min<int64_t>(n, r0 + kCbRows);
      for (int64_t r = r0; r < r1; ++r) {
        for (int64_t b = 0; b < nb; ++b) {
          if (cnt[b] > 65535) fits = false;
          roff[b * n + r] = (uint16_t)cnt[b];
        }
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) cnt[ix[e] / cols]++;
      }
      for (int64_t b = 0; b < nb; ++b) {
        if (cnt[b] > 65535) fits = false;
        seg[b * ng + g] = cnt[b];
      }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(pass1, ng * t / nt, ng * (t + 1) / nt);
  for (auto &x : th) x.join();
  th.clear();
  if (!fits) return false;
  cb.gptr.assign(nb * ng + 1, 0);
  for (int64_t i = 0; i < nb * ng; ++i) cb.gptr[i + 1] = cb.gptr[i] + seg[i];
  par_fill(cb.col, nnz + 256, (int32_t)0);
  par_fill(cb.val, nnz + 256, MV(0));
  auto pass2 = [&](int64_t g0, int64_t g1) {
    std::vector<int64_t> pos(nb);
    for (int64_t g = g0; g < g1; ++g) {
      for (int64_t b = 0; b < nb; ++b) pos[b] = cb.gptr[b * ng + g];
      const int64_t r0 = g * kCbRows, r1 = std::min<int64_t>(n, r0 + kCbRows);
      for (int64_t r = r0; r < r1; ++r)
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
          const int64_t p = pos[ix[e] / cols]++;
          cb.col[p] = (int32_t)ix[e];
          cb.val[p] = dv[e];
        }
    }
  };
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(pass2, ng * t / nt, ng * (t + 1) / nt);
  for (auto &x : th) x.join();
  cb.nb = nb;
  cb.cols = cols;
  cb.ng = ng;
  cb.roff = std::move(roff);
  return true;
}

// Paired-row SELL-128 image (see kry_csr::sp_*). Pass 1: slice widths (the
// longest row of each 128 rows); pass 2: per slot column the smallest column
// as base and every entry's delta and value at row position r - 128 s.
// Returns false (nothing built) when a slot column spans more than 65534
// columns, a column does not fit int32, or the image would hold more than
// 1.25x the SELL-64 image's slots (very uneven rows).

template <typename I, typename MV>
bool pair_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, PairHost<MV> &p) {
  constexpr int H = kPairSlice;
  if (n == 0 || n >= (int64_t(1) << 31)) return false;
  const int64_t ns = (n + H - 1) / H;
  p.width.assign(ns, 0);
  p.sptr.assign(ns + 1, 0);
  for (int64_t s = 0; s < ns; ++s) {
    int64_t w = 0;
    for (int64_t r = s * H; r < std::min<int64_t>(n, (s + 1) * H); ++r) w = std::max<int64_t>(w, ip[r + 1] - ip[r]);
    if (w > INT32_MAX / H) return false;
    p.width[s] = (int32_t)w;
    p.max_width = std::max(p.max_width, (int)w);
    p.sptr[s + 1] = p.sptr[s] + H * w;
  }
  const int64_t slots = p.sptr[ns];
  if (slots == 0 || slots * 4 > sell_slots * 5 + (int64_t)4 * H * p.max_width) return false;
  p.cbase.assign(slots / H + kDiaPad, 0);
  par_fill(p.delta, slots + 2 * H, (uint16_t)0xFFFF);
  par_fill(p.val, slots + 2 * H, MV(0));
  std::atomic<bool> ok{true};
  auto fill = [&](int64_t sa, int64_t sb) {
    for (int64_t s = sa; s < sb && ok.load(std::memory_order_relaxed); ++s) {
      const int64_t r0 = s * H, r1 = std::min<int64_t>(n, r0 + H), base = p.sptr[s];
      for (int64_t j = 0; j < p.width[s]; ++j) {
        int64_t mn = INT64_MAX, mx = -1;
        for (int64_t r = r0; r < r1; ++r)
          if ((int64_t)ip[r] + j < (int64_t)ip[r + 1]) {
            const int64_t c = (int64_t)ix[ip[r] + j];
            mn = std::min(mn, c);
            mx = std::max(mx, c);
          }
        if (mx < 0) mn = 0;
        if (mx - mn > 65534 || mn > INT32_MAX) {
          ok = false;
          return;
        }
        p.cbase[base / H + j] = (int32_t)mn;
        for (int64_t r = r0; r < r1; ++r)
          if ((int64_t)ip[r] + j < (int64_t)ip[r + 1]) {
            const int64_t q = base + j * H + (r - r0);
            p.delta[q] = (uint16_t)((int64_t)ix[ip[r] + j] - mn);
            p.val[q] = dv[ip[r] + j];
          }
      }
    }
  };
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (ns < 2048) nt = 1;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(fill, ns * t / nt, ns * (t + 1) / nt);
  for (auto &x : th) x.join();
  return ok.load();
}

// Host-only view of the paired-row plan (kry_pair_plan): the image
// kry_csr_create would build for these CSR arrays when neither the DIA nor the
// column-blocked image is built, without a device.
template <typename I>
static void pair_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, int64_t *info, int32_t *widths,
                           int32_t *cbase, uint16_t *deltas) {
  check_csr(n, nnz, ip, ix);
  int64_t ns = 0, sell_slots = 0, irr = 0;
  sell_plan(n, ip, nullptr, nullptr, &ns, &sell_slots, &irr);
  hvec<double> zeros;
  par_fill(zeros, (size_t)std::max<int64_t>(nnz, 1), 0.0);
  PairHost<double> p;
  const bool built = pair_build(n, ip, ix, zeros.data(), sell_slots, p);
  info[0] = built ? 1 : 0;
  info[1] = built ? (int64_t)p.width.size() : 0;
  info[2] = built ? p.sptr.back() : 0;
  info[3] = built ? p.max_width : 0;
  if (!built) return;
  if (widths) std::copy(p.width.begin(), p.width.end(), widths);
  const int64_t slots = p.sptr.back();
  if (cbase) std::copy(p.cbase.begin(), p.cbase.begin() + slots / kPairSlice, cbase);
  if (deltas) std::copy(p.delta.begin(), p.delta.begin() + slots, deltas);
}


// Host-only view of the column-blocked plan (kry_cb_plan): the image
// kry_csr_create would build for these CSR arrays when the diagonal-offset
// image is not, without a device.
template <typename I>
static void cb_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, int64_t *info, int64_t *gptr) {
  check_csr(n, nnz, ip, ix);
  hvec<double> vals;
  par_fill(vals, (size_t)std::max<int64_t>(nnz, 1), 1.0);
  CbHost<double> cb;
  const bool built = cb_build(n, ip, ix, vals.data(), cb);
  info[0] = built ? 1 : 0;
  info[1] = built ? cb.nb : 0;
  info[2] = built ? cb.cols : 0;
  info[3] = built ? cb.ng : 0;
  if (built && gptr) std::copy(cb.gptr.begin(), cb.gptr.end(), gptr);
  release_later(cb.val);
  release_later(cb.col);
  release_later(cb.roff);
  release_later(vals);
}

// ------------------------------------------- sparse triangular solve plan
template <typename I>
void tri_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, bool lower, TriPlan &p, const int32_t *rank) {
  check_csr(n, nnz, ip, ix);
  KRY_REQUIRE(n < INT32_MAX - kSlice, KRY_EUNSUPPORTED, "the triangular image numbers rows in int32");
  p = TriPlan();
  p.n = n;
  p.level.assign((size_t)n, 0);
  // the elimination order: at[q] = the row at position q (the identity without a rank)
  std::vector<int32_t> at;
  if (rank) {
    at.assign((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = rank[i];
      KRY_REQUIRE(r >= 0 && r < n && at[(size_t)r] < 0, KRY_EINVAL, "rank must be a permutation of 0..n-1");
      at[(size_t)r] = (int32_t)i;
    }
    p.rank.assign(rank, rank + n);
  }
  auto pos = [&](int64_t i) { return rank ? (int64_t)rank[i] : i; };
  auto row_at = [&](int64_t q) { return rank ? (int64_t)at[(size_t)q] : q; };
  // levels: a lower triangle's rows depend on earlier rows, an upper one's on later rows
  int32_t nlev = 0;
  for (int64_t q = 0; q < n; ++q) {
    const int64_t i = row_at(lower ? q : n - 1 - q);
    int32_t lev = 1;
    bool diag = false;
    for (int64_t e = (int64_t)ip[i]; e < (int64_t)ip[i + 1]; ++e) {
      const int64_t j = (int64_t)ix[e];
      KRY_REQUIRE(e == (int64_t)ip[i] || (int64_t)ix[e - 1] < j, KRY_EINVAL,
                  "triangular rows must be sorted without duplicates");
      if (j == i) {
        diag = true;
        continue;
      }
      KRY_REQUIRE(lower ? pos(j) < pos(i) : pos(j) > pos(i), KRY_EINVAL, "an entry on the wrong side of the diagonal");
      lev = std::max(lev, p.level[(size_t)j] + 1);
    }
    KRY_REQUIRE(diag, KRY_ESINGULAR, "singular matrix: no diagonal entry in row " + std::to_string(i));
    p.level[(size_t)i] = lev;
    nlev = std::max(nlev, lev);
  }
  p.nlevels = nlev;
  // rows by (level, position in the elimination order): a counting sort
  p.lrow.assign((size_t)nlev + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++p.lrow[(size_t)p.level[(size_t)i]];
  for (int32_t l = 0; l < nlev; ++l) p.lrow[(size_t)l + 1] += p.lrow[(size_t)l];
  p.order.assign((size_t)n, 0);
  {
    std::vector<int32_t> next(p.lrow.begin(), p.lrow.end() - (nlev ? 1 : 0));
    for (int64_t q = 0; q < n; ++q) {
      const int64_t i = row_at(q);
      p.order[(size_t)next[(size_t)p.level[(size_t)i] - 1]++] = (int32_t)i;
    }
  }
  // slices of up to kSlice rows inside a level
  p.lslice.assign((size_t)nlev + 1, 0);
  for (int32_t l = 0; l < nlev; ++l) {
    const int64_t rows = p.lrow[(size_t)l + 1] - p.lrow[(size_t)l];
    p.max_level_rows = std::max(p.max_level_rows, rows);
    p.lslice[(size_t)l + 1] = p.lslice[(size_t)l] + (int32_t)((rows + kSlice - 1) / kSlice);
  }
  p.nslices = nlev ? p.lslice[(size_t)nlev] : 0;
  p.swidth.assign((size_t)p.nslices, 0);
  p.sptr.assign((size_t)p.nslices + 1, 0);
  for (int32_t l = 0; l < nlev; ++l)
    for (int32_t s = p.lslice[(size_t)l]; s < p.lslice[(size_t)l + 1]; ++s) {
      const int64_t a = p.lrow[(size_t)l] + (int64_t)kSlice * (s - p.lslice[(size_t)l]);
      const int64_t b = std::min<int64_t>(a + kSlice, p.lrow[(size_t)l + 1]);
      int64_t w = 0;
      for (int64_t q = a; q < b; ++q) {
        const int64_t i = p.order[(size_t)q];
        w = std::max<int64_t>(w, (int64_t)ip[i + 1] - (int64_t)ip[i] - 1);
      }
      p.swidth[(size_t)s] = (int32_t)w;
      p.sptr[(size_t)s + 1] = p.sptr[(size_t)s] + w * kSlice;
    }
  p.nslots = p.sptr[(size_t)p.nslices];
  // launches: runs of levels that fit one workgroup together, large levels alone
  p.launch.assign(1, 0);
  for (int32_t l = 0; l < nlev;) {
    int64_t tot = p.lrow[(size_t)l + 1] - p.lrow[(size_t)l];
    int32_t e = l + 1;
    if (tot <= kTriGroupRows)
      while (e < nlev && tot + (p.lrow[(size_t)e + 1] - p.lrow[(size_t)e]) <= kTriGroupRows) {
        tot += p.lrow[(size_t)e + 1] - p.lrow[(size_t)e];
        ++e;
      }
    p.launch.push_back(e);
    l = e;
  }
}

template <typename I, typename V>
void tri_fill(const TriPlan &p, const I *ip, const I *ix, const V *dv, hvec<int32_t> &rows, hvec<V> &diag,
              hvec<int32_t> &col, hvec<V> &val) {
  par_fill(rows, (size_t)p.nslices * kSlice + 1, (int32_t)-1);
  par_fill(diag, (size_t)p.nslices * kSlice + 1, V(1));
  par_fill(col, (size_t)p.nslots + 1, (int32_t)-1);
  par_fill(val, (size_t)p.nslots + 1, V(0));
  const int32_t *rank = p.rank.empty() ? nullptr : p.rank.data();
  std::vector<int64_t> ent;  // a row's off-diagonal entries in ascending rank
  for (int64_t l = 0; l < p.nlevels; ++l)
    for (int64_t s = p.lslice[(size_t)l]; s < p.lslice[(size_t)l + 1]; ++s) {
      const int64_t a = p.lrow[(size_t)l] + (int64_t)kSlice * (s - p.lslice[(size_t)l]);
      const int64_t b = std::min<int64_t>(a + kSlice, p.lrow[(size_t)l + 1]);
      for (int64_t q = a; q < b; ++q) {
        const int64_t i = p.order[(size_t)q], r = q - a;
        rows[(size_t)(s * kSlice + r)] = (int32_t)i;
        int64_t j = 0;
        ent.clear();
        for (int64_t e = (int64_t)ip[i]; e < (int64_t)ip[i + 1]; ++e) {
          if ((int64_t)ix[e] == i) {
            KRY_REQUIRE(dv[e] != V(0), KRY_ESINGULAR, "singular matrix: zero diagonal in row " + std::to_string(i));
            diag[(size_t)(s * kSlice + r)] = dv[e];
            continue;
          }
          if (rank) {
            ent.push_back(e);
            continue;
          }
          const size_t slot = (size_t)(p.sptr[(size_t)s] + j * kSlice + r);
          col[slot] = (int32_t)ix[e];
          val[slot] = dv[e];
          ++j;
        }
        if (rank) {
          std::sort(ent.begin(), ent.end(), [&](int64_t a, int64_t b) { return rank[ix[a]] < rank[ix[b]]; });
          for (const int64_t e : ent) {
            const size_t slot = (size_t)(p.sptr[(size_t)s] + j * kSlice + r);
            col[slot] = (int32_t)ix[e];
            val[slot] = dv[e];
            ++j;
          }
        }
      }
    }
}

// ------------------------------------------------------------ ILU(0) plan
template <typename I>
void ilu0_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, Ilu0Plan &p) {
  check_csr(n, nnz, ip, ix);
  p = Ilu0Plan();
  p.diag.assign((size_t)n, -1);
  // the pattern of tril(A): every row up to and including its diagonal
  std::vector<I> lp((size_t)n + 1, 0), lx;
  lx.reserve((size_t)nnz / 2 + (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t e = (int64_t)ip[i]; e < (int64_t)ip[i + 1]; ++e) {
      const int64_t j = (int64_t)ix[e];
      KRY_REQUIRE(e == (int64_t)ip[i] || (int64_t)ix[e - 1] < j, KRY_EINVAL,
                  "ILU(0) needs sorted rows without duplicates (row " + std::to_string(i) + ")");
      if (j <= i) lx.push_back(ix[e]);
      if (j == i) p.diag[(size_t)i] = e;
    }
    KRY_REQUIRE(p.diag[(size_t)i] >= 0, KRY_ESINGULAR, "singular matrix: no diagonal entry in row " + std::to_string(i));
    lp[(size_t)i + 1] = (I)lx.size();
  }
  tri_plan(n, (int64_t)lx.size(), lp.data(), lx.data(), true, p.tri);
}

// --------------------------------------------------- multicolour ordering
template <typename I>
void color_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, std::vector<int32_t> &color,
                std::vector<int32_t> &perm, int64_t *ncolors, int64_t *max_rows) {
  check_csr(n, nnz, ip, ix);
  KRY_REQUIRE(n < INT32_MAX, KRY_EUNSUPPORTED, "the colouring numbers rows in int32");
  // the transposed half of the graph: tx[tp[c] .. tp[c + 1]) = the rows j < c that store (j, c)
  std::vector<int64_t> tp((size_t)n + 1, 0);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t e = (int64_t)ip[j]; e < (int64_t)ip[j + 1]; ++e)
      if ((int64_t)ix[e] > j) ++tp[(size_t)ix[e] + 1];
  for (int64_t c = 0; c < n; ++c) tp[(size_t)c + 1] += tp[(size_t)c];
  std::vector<int32_t> tx((size_t)tp[(size_t)n]);
  {
    std::vector<int64_t> next(tp.begin(), tp.end() - 1);
    for (int64_t j = 0; j < n; ++j)
      for (int64_t e = (int64_t)ip[j]; e < (int64_t)ip[j + 1]; ++e)
        if ((int64_t)ix[e] > j) tx[(size_t)next[(size_t)ix[e]]++] = (int32_t)j;
  }
  color.assign((size_t)n, 0);
  std::vector<int64_t> seen;  // seen[c] = the last row with a neighbour of colour c, plus 1
  std::vector<int32_t> count;
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t e = (int64_t)ip[i]; e < (int64_t)ip[i + 1]; ++e)
      if ((int64_t)ix[e] < i) seen[(size_t)color[(size_t)ix[e]]] = i + 1;
    for (int64_t e = tp[(size_t)i]; e < tp[(size_t)i + 1]; ++e) seen[(size_t)color[(size_t)tx[(size_t)e]]] = i + 1;
    size_t c = 0;
    while (c < seen.size() && seen[c] == i + 1) ++c;
    if (c == seen.size()) {
      seen.push_back(0);
      count.push_back(0);
    }
    color[(size_t)i] = (int32_t)c;
    ++count[c];
  }
  *ncolors = (int64_t)count.size();
  *max_rows = 0;
  std::vector<int64_t> next(count.size() + 1, 0);
  for (size_t c = 0; c < count.size(); ++c) {
    *max_rows = std::max<int64_t>(*max_rows, count[c]);
    next[c + 1] = next[c] + count[c];
  }
  perm.assign((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) perm[(size_t)next[(size_t)color[(size_t)i]]++] = (int32_t)i;
}

void bjacobi_plan(int64_t n, int64_t nblocks, const int32_t *starts, BjPlan &p) {
  KRY_REQUIRE(n < INT32_MAX, KRY_EUNSUPPORTED, "the block partition indexes rows in int32");
  KRY_REQUIRE((nblocks == 0) == (n == 0), KRY_EINVAL,
              n == 0 ? "an empty matrix has no blocks" : "the partition has no blocks");
  p = BjPlan();
  p.n = n;
  p.nblocks = nblocks;
  if (nblocks == 0) return;
  KRY_REQUIRE(starts[0] == 0, KRY_EINVAL, "the first block must start at row 0, not " + std::to_string(starts[0]));
  std::vector<int32_t> bucket[4];  // g = 4 << q
  p.min_block = kBjMaxBlock;
  for (int64_t i = 0; i < nblocks; ++i) {
    const int64_t s = starts[i], e = i + 1 < nblocks ? (int64_t)starts[i + 1] : n;
    KRY_REQUIRE(s < n, KRY_EINVAL,
                "block " + std::to_string(i) + " starts at row " + std::to_string(s) + ", past the last row");
    KRY_REQUIRE(e > s, KRY_EINVAL,
                "the block starts must increase strictly: block " + std::to_string(i + 1) + " starts at row " +
                    std::to_string(e) + ", block " + std::to_string(i) + " at row " + std::to_string(s));
    const int64_t b = e - s;
    KRY_REQUIRE(b <= kBjMaxBlock, KRY_EUNSUPPORTED,
                "block " + std::to_string(i) + " (from row " + std::to_string(s) + ") has " + std::to_string(b) +
                    " rows: block-Jacobi takes blocks of at most " + std::to_string(kBjMaxBlock));
    p.min_block = std::min<int32_t>(p.min_block, (int32_t)b);
    p.max_block = std::max<int32_t>(p.max_block, (int32_t)b);
    p.values += b * b;
    int q = 0;
    while ((4 << q) < b) ++q;
    bucket[q].push_back((int32_t)i);
  }
  p.blocklist.reserve((size_t)nblocks);
  for (int q = 0; q < 4; ++q) {
    const int g = 4 << q;
    const size_t per = (size_t)(64 / g);
    for (size_t r = 0; r < bucket[q].size(); r += per) {
      const size_t count = std::min(per, bucket[q].size() - r);
      p.tasks.push_back(BjTask{(int32_t)p.blocklist.size(), (int32_t)count, g});
      p.blocklist.insert(p.blocklist.end(), bucket[q].begin() + (ptrdiff_t)r, bucket[q].begin() + (ptrdiff_t)(r + count));
    }
  }
}

// explicit instantiations: the combinations kry_csr_create dispatches
#define KRY_HOST_I(I)                                                                                             \
  template void check_csr<I>(int64_t, int64_t, const I *, const I *);                                            \
  template bool scattered<I>(int64_t, const I *, const I *);                                                     \
  template bool rcm_order<I>(int64_t, const I *, const I *, int64_t, std::vector<int32_t> &, int64_t *);          \
  template void tri_plan<I>(int64_t, int64_t, const I *, const I *, bool, TriPlan &, const int32_t *);           \
  template void color_plan<I>(int64_t, int64_t, const I *, const I *, std::vector<int32_t> &,                   \
                              std::vector<int32_t> &, int64_t *, int64_t *);                                     \
  template void ilu0_plan<I>(int64_t, int64_t, const I *, const I *, Ilu0Plan &);                               \
  template void sell_plan<I>(int64_t, const I *, std::vector<int64_t> *, std::vector<int32_t> *, int64_t *,     \
                             int64_t *, int64_t *);                                                              \
  template bool compact_fill<I>(const std::vector<int64_t> &, const std::vector<int32_t> &, const hvec<I> &,     \
                                hvec<uint16_t> &, std::vector<int32_t> &);
#define KRY_HOST_IM(I, MV)                                                                                         \
  template void sell_fill<I, MV>(int64_t, const I *, const I *, const MV *, const std::vector<int64_t> &,       \
                                 const std::vector<int32_t> &, hvec<I> &, hvec<MV> &);                          \
  template bool dia_build<I, MV>(int64_t, const I *, const I *, const MV *, int64_t, DiaHost<MV> &, bool);      \
  template bool cb_build<I, MV>(int64_t, const I *, const I *, const MV *, CbHost<MV> &);                       \
  template bool pair_build<I, MV>(int64_t, const I *, const I *, const MV *, int64_t, PairHost<MV> &);          \
  template void renumber_csr<I, MV>(int64_t, const I *, const I *, const MV *, const std::vector<int32_t> &,    \
                                    hvec<I> &, hvec<I> &, hvec<MV> &);                                          \
  template bool rs_build<I, MV>(int64_t, const I *, const I *, const MV *, int64_t, RsHost<MV> &);              \
  template void tri_fill<I, MV>(const TriPlan &, const I *, const I *, const MV *, hvec<int32_t> &, hvec<MV> &,  \
                                hvec<int32_t> &, hvec<MV> &);
KRY_HOST_I(int32_t)
KRY_HOST_I(int64_t)
KRY_HOST_IM(int32_t, float)
KRY_HOST_IM(int32_t, double)
KRY_HOST_IM(int64_t, float)
KRY_HOST_IM(int64_t, double)
template bool dia_classes<float>(const DiaHost<float> &, DiaClassHost<float> &);
template bool dia_classes<double>(const DiaHost<double> &, DiaClassHost<double> &);
template void release_later<int32_t>(hvec<int32_t> &);
template void release_later<int64_t>(hvec<int64_t> &);
template void release_later<float>(hvec<float> &);
template void release_later<double>(hvec<double> &);
template void release_later<uint16_t>(hvec<uint16_t> &);
template void release_later<uint64_t>(hvec<uint64_t> &);
template void release_later<uint32_t>(hvec<uint32_t> &);

}  // namespace kry

using namespace kry;

template <typename I>
static void rs_plan_host(int64_t n, int64_t nnz, const I *ip, const I *ix, int64_t *info, int32_t *widths,
                         uint32_t *colrank) {
  check_csr(n, nnz, ip, ix);
  int64_t ns = 0, sell_slots = 0, irr = 0;
  sell_plan(n, ip, nullptr, nullptr, &ns, &sell_slots, &irr);
  hvec<double> zeros;
  par_fill(zeros, (size_t)std::max<int64_t>(nnz, 1), 0.0);
  RsHost<double> r;
  const bool built = rs_build(n, ip, ix, zeros.data(), sell_slots, r);
  info[0] = built ? 1 : 0;
  info[1] = built ? (int64_t)r.width.size() : 0;
  info[2] = built ? r.sptr.back() : 0;
  info[3] = built ? r.max_width : 0;
  if (!built) return;
  if (widths) std::copy(r.width.begin(), r.width.end(), widths);
  if (colrank) std::copy(r.colrank.begin(), r.colrank.begin() + r.sptr.back(), colrank);
}

extern "C" {

const char *kry_last_error(void) { return kry::g_last_error.c_str(); }

int kry_csr_layout(int64_t n, const void *indptr, int itype, int64_t *nslices, int64_t *nslots,
                   int64_t *nirregular) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && nslices && nslots && nirregular && n >= 0, KRY_EINVAL, "bad layout arguments");
  if (itype == KRY_I32)
    sell_plan(n, static_cast<const int32_t *>(indptr), nullptr, nullptr, nslices, nslots, nirregular);
  else if (itype == KRY_I64)
    sell_plan(n, static_cast<const int64_t *>(indptr), nullptr, nullptr, nslices, nslots, nirregular);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  KRY_API_END
}

int kry_dia_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                 int32_t *widths, int32_t *offsets, uint64_t *masks) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  if (itype == KRY_I32)
    dia_plan_host(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), info, widths,
                  offsets, masks);
  else if (itype == KRY_I64)
    dia_plan_host(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), info, widths,
                  offsets, masks);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  KRY_API_END
}

int kry_dia_uniform_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data, int dtype,
                         int itype, int64_t *info, int32_t *flags, void *values) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || (indices && data)), KRY_EINVAL,
              "bad plan arguments");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32 || itype == KRY_I64, KRY_EINVAL, "bad itype");
  static const double zd = 0;
  const void *dv = nnz ? data : (const void *)&zd;
  auto go = [&](auto *ip, auto *ix) {
    if (dtype == KRY_F64)
      dia_uniform_plan_host(n, nnz, ip, ix, static_cast<const double *>(dv), info, flags, static_cast<double *>(values));
    else
      dia_uniform_plan_host(n, nnz, ip, ix, static_cast<const float *>(dv), info, flags, static_cast<float *>(values));
  };
  if (itype == KRY_I32)
    go(static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices));
  else
    go(static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices));
  KRY_API_END
}

int kry_dia_class_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data, int dtype,
                       int itype, int uniform, int64_t *info) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || (indices && data)), KRY_EINVAL,
              "bad plan arguments");
  KRY_REQUIRE(dtype == KRY_F32 || dtype == KRY_F64, KRY_EINVAL, "dtype must be f32 or f64");
  KRY_REQUIRE(itype == KRY_I32 || itype == KRY_I64, KRY_EINVAL, "bad itype");
  static const double zd = 0;
  const void *dv = nnz ? data : (const void *)&zd;
  auto go = [&](auto *ip, auto *ix) {
    if (dtype == KRY_F64) dia_class_plan_host(n, nnz, ip, ix, static_cast<const double *>(dv), uniform, info);
    else dia_class_plan_host(n, nnz, ip, ix, static_cast<const float *>(dv), uniform, info);
  };
  if (itype == KRY_I32)
    go(static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices));
  else
    go(static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices));
  KRY_API_END
}

int kry_pair_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                  int32_t *widths, int32_t *cbase, uint16_t *deltas) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  if (itype == KRY_I32)
    pair_plan_host(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), info, widths,
                   cbase, deltas);
  else if (itype == KRY_I64)
    pair_plan_host(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), info, widths,
                   cbase, deltas);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  KRY_API_END
}

int kry_cb_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                int64_t *gptr) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  if (itype == KRY_I32)
    cb_plan_host(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), info, gptr);
  else if (itype == KRY_I64)
    cb_plan_host(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), info, gptr);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  KRY_API_END
}

int kry_rcm_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t wlimit,
                 int64_t *info, int32_t *perm) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  const int64_t wl = wlimit > 0 ? wlimit : std::max<int64_t>(int64_t(1) << 16, n / 32);
  std::vector<int32_t> p;
  int64_t levels = 0;
  bool built = false;
  if (itype == KRY_I32) {
    check_csr(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices));
    built = rcm_order(n, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), wl, p, &levels);
  } else if (itype == KRY_I64) {
    check_csr(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices));
    built = rcm_order(n, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), wl, p, &levels);
  } else {
    throw Error{KRY_EINVAL, "bad itype"};
  }
  info[0] = built ? 1 : 0;
  info[1] = built ? levels : 0;
  if (built && perm) std::copy(p.begin(), p.end(), perm);
  KRY_API_END
}

int kry_rs_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                int32_t *widths, uint32_t *colrank) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  if (itype == KRY_I32)
    rs_plan_host(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), info, widths,
                 colrank);
  else if (itype == KRY_I64)
    rs_plan_host(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), info, widths,
                 colrank);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  KRY_API_END
}

int kry_tri_plan_ordered(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int lower,
                         const int32_t *rank, int64_t *info, int32_t *level, int32_t *order, int32_t *launch,
                         int32_t *widths) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  TriPlan p;
  if (itype == KRY_I32)
    tri_plan(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), lower != 0, p, rank);
  else if (itype == KRY_I64)
    tri_plan(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), lower != 0, p, rank);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  info[0] = p.nlevels;
  info[1] = (int64_t)p.launch.size() - 1;
  info[2] = p.nslices;
  info[3] = p.nslots;
  info[4] = p.max_level_rows;
  if (level) std::copy(p.level.begin(), p.level.end(), level);
  if (order) std::copy(p.order.begin(), p.order.end(), order);
  if (launch) std::copy(p.launch.begin(), p.launch.end(), launch);
  if (widths) std::copy(p.swidth.begin(), p.swidth.end(), widths);
  KRY_API_END
}

int kry_tri_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int lower, int64_t *info,
                 int32_t *level, int32_t *order, int32_t *launch, int32_t *widths) {
  return kry_tri_plan_ordered(n, nnz, indptr, indices, itype, lower, nullptr, info, level, order, launch, widths);
}

int kry_color_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                   int32_t *color, int32_t *perm) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  std::vector<int32_t> c, p;
  if (itype == KRY_I32)
    color_plan(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), c, p, &info[0],
               &info[1]);
  else if (itype == KRY_I64)
    color_plan(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), c, p, &info[0],
               &info[1]);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  if (color) std::copy(c.begin(), c.end(), color);
  if (perm) std::copy(p.begin(), p.end(), perm);
  KRY_API_END
}

int kry_ilu0_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                  int32_t *level, int32_t *order, int32_t *launch, int64_t *diag) {
  KRY_API_BEGIN
  KRY_REQUIRE(indptr && info && n >= 0 && nnz >= 0 && (nnz == 0 || indices), KRY_EINVAL, "bad plan arguments");
  Ilu0Plan p;
  if (itype == KRY_I32)
    ilu0_plan(n, nnz, static_cast<const int32_t *>(indptr), static_cast<const int32_t *>(indices), p);
  else if (itype == KRY_I64)
    ilu0_plan(n, nnz, static_cast<const int64_t *>(indptr), static_cast<const int64_t *>(indices), p);
  else
    throw Error{KRY_EINVAL, "bad itype"};
  info[0] = p.tri.nlevels;
  info[1] = (int64_t)p.tri.launch.size() - 1;
  info[2] = p.tri.max_level_rows;
  if (level) std::copy(p.tri.level.begin(), p.tri.level.end(), level);
  if (order) std::copy(p.tri.order.begin(), p.tri.order.end(), order);
  if (launch) std::copy(p.tri.launch.begin(), p.tri.launch.end(), launch);
  if (diag) std::copy(p.diag.begin(), p.diag.end(), diag);
  KRY_API_END
}

int kry_bjacobi_plan(int64_t n, int64_t nblocks, const int32_t *starts, int64_t *info, int32_t *tasks,
                     int32_t *blocklist) {
  KRY_API_BEGIN
  KRY_REQUIRE(info && n >= 0 && nblocks >= 0 && (nblocks == 0 || starts), KRY_EINVAL, "bad plan arguments");
  BjPlan p;
  bjacobi_plan(n, nblocks, starts, p);
  info[0] = (int64_t)p.tasks.size();
  info[1] = p.max_block;
  info[2] = p.min_block;
  info[3] = p.values;
  if (tasks)
    for (size_t t = 0; t < p.tasks.size(); ++t) {
      tasks[3 * t] = p.tasks[t].first;
      tasks[3 * t + 1] = p.tasks[t].count;
      tasks[3 * t + 2] = p.tasks[t].g;
    }
  if (blocklist) std::copy(p.blocklist.begin(), p.blocklist.end(), blocklist);
  KRY_API_END
}

}  // extern "C"
