// Stand-alone driver of the uniform-slot-column detection of the SELL-128/DIA
// image (kry_dia_uniform_plan, kry::dia_build in krylov_amd/csrc/
// host_image.cpp), meant to be built with the host sanitizers and run
// directly (tests/test_dia_uniform_plan.py):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       tools/dia_uniform_check.cpp krylov_amd/csrc/host_image.cpp -o dia_uniform_check
//   ./dia_uniform_check matrix.bin ...
//
// A matrix file holds int64 {n, nnz, value bytes (4 | 8)}, then int32
// indptr[n + 1], int32 indices[nnz] and values[nnz]. For every file the
// program runs the plan through the C entry point (sizing call, then the full
// call), builds the image itself, recomputes every slot column's flag from the
// image's masks and values (byte comparison), checks that the flags, the
// values and the count agree and that detection turned off flags nothing, and
// prints "<file> columns uniform".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "../krylov_amd/csrc/host_image.hpp"

namespace {

[[noreturn]] void fail(const std::string &what) {
  std::cerr << "dia_uniform_check: " << what << "\n";
  std::exit(1);
}

template <typename MV>
void run(const char *path, std::ifstream &f, int64_t n, int64_t nnz) {
  std::vector<int32_t> ip((size_t)n + 1), ix((size_t)std::max<int64_t>(nnz, 1));
  std::vector<MV> dv((size_t)std::max<int64_t>(nnz, 1));
  f.read(reinterpret_cast<char *>(ip.data()), (std::streamsize)(ip.size() * 4));
  f.read(reinterpret_cast<char *>(ix.data()), (std::streamsize)((size_t)nnz * 4));
  f.read(reinterpret_cast<char *>(dv.data()), (std::streamsize)((size_t)nnz * sizeof(MV)));
  if (!f) fail(std::string("short file ") + path);
  const int dtype = sizeof(MV) == 8 ? KRY_F64 : KRY_F32;
  int64_t info[3] = {0, 0, 0};
  if (kry_dia_uniform_plan(n, nnz, ip.data(), ix.data(), dv.data(), dtype, KRY_I32, info, nullptr, nullptr) != KRY_OK)
    fail(std::string("kry_dia_uniform_plan: ") + kry_last_error());
  if (!info[0]) fail(std::string("no diagonal-offset image for ") + path);
  std::vector<int32_t> flags((size_t)info[1]);
  std::vector<MV> values((size_t)info[1]);
  if (kry_dia_uniform_plan(n, nnz, ip.data(), ix.data(), dv.data(), dtype, KRY_I32, info, flags.data(),
                           values.data()) != KRY_OK)
    fail(std::string("kry_dia_uniform_plan: ") + kry_last_error());
  // the image itself
  int64_t ns = 0, sell_slots = 0, irr = 0;
  kry::sell_plan(n, ip.data(), (std::vector<int64_t> *)nullptr, (std::vector<int32_t> *)nullptr, &ns, &sell_slots,
                 &irr);
  kry::DiaHost<MV> d, off;
  if (!kry::dia_build(n, ip.data(), ix.data(), dv.data(), sell_slots, d, true)) fail("dia_build refused");
  if (!kry::dia_build(n, ip.data(), ix.data(), dv.data(), sell_slots, off, false)) fail("dia_build refused");
  const int64_t cols = d.sptr.back() / kry::kDiaSlice;
  if (cols != info[1] || d.nuniform != info[2]) fail("plan and builder disagree");
  if ((int64_t)d.uflag.size() != cols + kry::kDiaPad || (int64_t)d.uval.size() != cols + kry::kDiaPad)
    fail("descriptor arrays are not padded");
  int64_t count = 0;
  const MV zero = MV(0);
  for (int64_t c = 0; c < cols + kry::kDiaPad; ++c) {
    bool same = false;
    const MV *first = nullptr;
    if (c < cols) {
      same = true;
      for (int rl = 0; rl < kry::kDiaSlice && same; ++rl) {
        if (!((d.mask[(size_t)(2 * c + (rl & 1))] >> (rl >> 1)) & 1u)) continue;
        const MV *v = &d.val[(size_t)(c * kry::kDiaSlice + rl)];
        if (!first) first = v;
        same = std::memcmp(v, first, sizeof(MV)) == 0;
      }
      same = same && first != nullptr;
    }
    if (d.uflag[(size_t)c] != (same ? 1 : 0)) fail("flag of slot column " + std::to_string(c));
    if (std::memcmp(&d.uval[(size_t)c], same ? first : &zero, sizeof(MV)) != 0)
      fail("value of slot column " + std::to_string(c));
    if (c < cols && (flags[(size_t)c] != d.uflag[(size_t)c] || std::memcmp(&values[(size_t)c], &d.uval[(size_t)c], sizeof(MV)) != 0))
      fail("entry point and builder disagree at slot column " + std::to_string(c));
    if (off.uflag[(size_t)c] != 0 || std::memcmp(&off.uval[(size_t)c], &zero, sizeof(MV)) != 0)
      fail("detection off still flags slot column " + std::to_string(c));
    count += same;
  }
  if (count != d.nuniform || off.nuniform != 0) fail("uniform count");
  if (d.off != off.off || d.val.size() != off.val.size() ||
      std::memcmp(d.val.data(), off.val.data(), d.val.size() * sizeof(MV)) != 0)
    fail("detection changed the image");
  std::printf("%s %lld %lld\n", path, (long long)cols, (long long)d.nuniform);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) fail("usage: dia_uniform_check matrix.bin ...");
  for (int a = 1; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    int64_t head[3];
    f.read(reinterpret_cast<char *>(head), sizeof(head));
    if (!f) fail(std::string("cannot read ") + argv[a]);
    try {
      if (head[2] == 8) run<double>(argv[a], f, head[0], head[1]);
      else if (head[2] == 4) run<float>(argv[a], f, head[0], head[1]);
      else fail("bad value size");
    } catch (const kry::Error &e) {
      fail(e.msg);
    }
  }
  return 0;
}
