// Stand-alone driver of the sparse triangular solve's host analysis
// (kry_tri_plan, kry::tri_plan / kry::tri_fill in krylov_amd/csrc/
// host_image.cpp), meant to be built with the host sanitizers and run
// directly (tests/test_tri_plan.py):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       tools/tri_plan_check.cpp krylov_amd/csrc/host_image.cpp -o tri_plan_check
//   ./tri_plan_check matrix.bin ...
//
// A matrix file holds int64 {n, nnz, index bytes (4 | 8), lower (0 | 1)}, then
// indptr[n + 1] and indices[nnz] in that index type. For every file the
// program runs the plan through the C entry point (sizing call, then the full
// call), checks it (levels against the rows' dependencies, the order a
// permutation sorted by (level, row), launches covering the levels), builds
// the image with unit values and checks that it holds every entry once, and
// prints "<file> levels launches slices slots largest".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "../krylov_amd/csrc/host_image.hpp"

namespace {

[[noreturn]] void fail(const std::string &what) {
  std::cerr << "tri_plan_check: " << what << "\n";
  std::exit(1);
}

template <typename I>
void run(const char *path, std::ifstream &f, int64_t n, int64_t nnz, bool lower) {
  std::vector<I> ip((size_t)n + 1), ix((size_t)std::max<int64_t>(nnz, 1));
  f.read(reinterpret_cast<char *>(ip.data()), (std::streamsize)(ip.size() * sizeof(I)));
  f.read(reinterpret_cast<char *>(ix.data()), (std::streamsize)((size_t)nnz * sizeof(I)));
  if (!f) fail(std::string("short file ") + path);
  const int itype = sizeof(I) == 4 ? KRY_I32 : KRY_I64;
  int64_t info[5] = {0, 0, 0, 0, 0};
  if (kry_tri_plan(n, nnz, ip.data(), ix.data(), itype, lower ? 1 : 0, info, nullptr, nullptr, nullptr, nullptr) !=
      KRY_OK)
    fail(std::string("kry_tri_plan: ") + kry_last_error());
  std::vector<int32_t> level((size_t)n), order((size_t)n), launch((size_t)info[1] + 1), widths((size_t)info[2]);
  if (kry_tri_plan(n, nnz, ip.data(), ix.data(), itype, lower ? 1 : 0, info, level.data(), order.data(), launch.data(),
                   widths.data()) != KRY_OK)
    fail(std::string("kry_tri_plan: ") + kry_last_error());
  for (int64_t i = 0; i < n; ++i) {
    int32_t want = 1;
    for (int64_t e = (int64_t)ip[(size_t)i]; e < (int64_t)ip[(size_t)i + 1]; ++e)
      if ((int64_t)ix[(size_t)e] != i) want = std::max(want, level[(size_t)ix[(size_t)e]] + 1);
    if (level[(size_t)i] != want) fail("level of row " + std::to_string(i));
  }
  std::vector<char> seen((size_t)n, 0);
  for (int64_t q = 0; q < n; ++q) {
    const int32_t r = order[(size_t)q];
    if (r < 0 || r >= n || seen[(size_t)r]) fail("order is not a permutation");
    seen[(size_t)r] = 1;
    if (q > 0) {
      const int32_t p = order[(size_t)q - 1];
      if (level[(size_t)p] > level[(size_t)r] || (level[(size_t)p] == level[(size_t)r] && p >= r))
        fail("order is not sorted by (level, row)");
    }
  }
  if (launch.front() != 0 || launch.back() != info[0]) fail("launches do not cover the levels");
  for (size_t q = 0; q + 1 < launch.size(); ++q)
    if (launch[q] >= launch[q + 1]) fail("empty launch");
  // the image, with unit values
  kry::TriPlan p;
  kry::tri_plan(n, nnz, ip.data(), ix.data(), lower, p);
  std::vector<double> ones((size_t)std::max<int64_t>(nnz, 1), 1.0);
  kry::hvec<int32_t> rows, col;
  kry::hvec<double> diag, val;
  kry::tri_fill(p, ip.data(), ix.data(), ones.data(), rows, diag, col, val);
  int64_t stored = 0, live = 0;
  for (int64_t s = 0; s < p.nslots; ++s) stored += col[(size_t)s] >= 0;
  for (int64_t s = 0; s < p.nslices * kry::kSlice; ++s) live += rows[(size_t)s] >= 0;
  if (stored != nnz - n || live != n) fail("the image does not hold every entry once");
  if (p.nslices != info[2] || p.nslots != info[3]) fail("plan and entry point disagree");
  std::printf("%s %lld %lld %lld %lld %lld\n", path, (long long)info[0], (long long)info[1], (long long)info[2],
              (long long)info[3], (long long)info[4]);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) fail("usage: tri_plan_check matrix.bin ...");
  for (int a = 1; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    int64_t head[4];
    f.read(reinterpret_cast<char *>(head), sizeof(head));
    if (!f) fail(std::string("cannot read ") + argv[a]);
    try {
      if (head[2] == 4) run<int32_t>(argv[a], f, head[0], head[1], head[3] != 0);
      else if (head[2] == 8) run<int64_t>(argv[a], f, head[0], head[1], head[3] != 0);
      else fail("bad index size");
    } catch (const kry::Error &e) {
      fail(e.msg);
    }
  }
  return 0;
}
