// Host-only plumbing shared by the HIP translation units and the plain C++
// one (host_image.cpp, which the sanitizer builds compile on their own):
// image geometry constants, the error type, KRY_REQUIRE and the
// KRY_API_BEGIN / KRY_API_END frame of the exported functions.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <exception>
#include <string>

#include "../../include/krylov_hip.h"

namespace kry {

constexpr int kSlice = 64;           // SELL slice height = one wavefront
// diagonal-offset image (kry_csr::dia_*): slices of kDiaSlice rows, lane l
// of the wave owns rows 2l and 2l + 1 of its slice
constexpr int kDiaSlice = 128;
constexpr int kDiaPad = 32;  // slot-column descriptors past the last one (unconditional reads of a round)
// descriptor classes (kry_csr::dia_cls_*): the class table may take a quarter
// of one XCD's 4 MiB L2; a column of it holds an int32 offset, two uint64
// masks, an int32 flag and a value
constexpr int64_t kDiaClassMaxBytes = int64_t(1) << 20;
constexpr int64_t dia_class_col_bytes(size_t value_size) { return 4 + 16 + 4 + (int64_t)value_size; }
// paired-row SELL-128 image (kry_csr::sp_*): lane l owns rows 2l, 2l + 1
constexpr int kPairSlice = 128;
constexpr int kCbRows = 256;         // rows per column-blocked segment (one per thread)
// rank-sorted SELL-128 image (kry_csr::rs_*): runs of stored entries sorted by column
constexpr int kRsChunk = 16;
// sparse triangular solve (kry_tri): consecutive dependency levels holding at
// most kTriGroupRows rows together run as one launch of one workgroup (each of
// its kBlock threads takes up to kTriGroupRows / kBlock rows of a level);
// a level above it gets a launch of its own over many workgroups
constexpr int kTriGroupRows = 1024;

// ---------------------------------------------------------------- errors
void set_error(const std::string &msg);

struct Error {
  int code;
  std::string msg;
};

#define KRY_REQUIRE(cond, code, msg)                                           \
  do {                                                                         \
    if (!(cond)) throw ::kry::Error{(code), (msg)};                            \
  } while (0)

}  // namespace kry

// The body of every extern "C" entry point sits between these two: an Error
// becomes its code and message (kry_last_error), anything else KRY_EDEVICE.
#define KRY_API_BEGIN try {
#define KRY_API_END                  \
  return KRY_OK;                     \
  }                                  \
  catch (const kry::Error &e) {      \
    kry::set_error(e.msg);           \
    return e.code;                   \
  }                                  \
  catch (const std::exception &e) {  \
    kry::set_error(e.what());        \
    return KRY_EDEVICE;              \
  }
