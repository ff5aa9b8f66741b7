// Host-side image builders of kry_csr_create (kry_csr::sptr / dia_* /
// cb_* / sp_*) and the host-only plans the C-ABI exposes (kry_csr_layout,
// kry_dia_plan, kry_pair_plan, kry_cb_plan). Plain C++ (no HIP): compiled by
// host_image.cpp, which the library links, and which `make sanitize` builds
// on its own with -fsanitize=address,undefined and -fsanitize=thread
// (tests/test_host_sanitize.py). Templates are instantiated there for
// int32 / int64 indices and float / double values.
#pragma once

#include <stdint.h>

#include <memory>
#include <utility>
#include <vector>

#include "host_common.hpp"

namespace kry {

// ------------------------------------------------- host staging buffers
// Image staging vectors: no zero-initialisation on resize (std::vector's
// value-initialisation writes every page from one thread), filled in
// parallel instead, so the first touch of the pages is spread over threads.
template <class T>
struct NoInit : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInit<U>;
  };
  NoInit() = default;
  template <class U>
  NoInit(const NoInit<U> &) {}
  template <class U, class... A>
  void construct(U *q, A &&...a) {
    if constexpr (sizeof...(A) == 0) ::new ((void *)q) U;
    else ::new ((void *)q) U(std::forward<A>(a)...);
  }
};
template <class T>
using hvec = std::vector<T, NoInit<T>>;


// Releases a staging vector's pages (on a detached thread above 64 MB, once
// its H2D copies have completed).
template <class T>
void release_later(hvec<T> &v);

// Structural check of a square CSR matrix before any image is built from
// it: indptr[0] = 0, indptr non-decreasing, indptr[n] = nnz, and every column
// index in [0, n). Throws Error{KRY_EINVAL} otherwise (the builders index
// host and device arrays with these values; threaded above 2^20 entries).
template <typename I>
void check_csr(int64_t n, int64_t nnz, const I *ip, const I *ix);

// SELL-64 plan: slice s = rows [64 s, 64 s + 64); width = longest row; a
// slice is irregular (CSR walk) when 64 * width > 2 * nnz_slice + 1024.
template <typename I>
void sell_plan(int64_t n, const I *ip, std::vector<int64_t> *sptr, std::vector<int32_t> *width, int64_t *nslices,
               int64_t *nslots, int64_t *nirr);
template <typename I, typename MV>
void sell_fill(int64_t n, const I *ip, const I *ix, const MV *dv, const std::vector<int64_t> &sptr,
               const std::vector<int32_t> &width, hvec<I> &sidx, hvec<MV> &sval);
// uint16 column deltas over per-slot-column bases; false when a slot column
// spans more than 65534 columns
template <typename I>
bool compact_fill(const std::vector<int64_t> &sptr, const std::vector<int32_t> &width, const hvec<I> &sidx,
                  hvec<uint16_t> &sdelta, std::vector<int32_t> &scbase);

template <typename MV>
struct DiaHost {
  std::vector<int64_t> sptr;
  std::vector<int32_t> width;
  std::vector<int32_t> off;
  hvec<uint64_t> mask;
  hvec<MV> val;
  int max_width = 0;
  // per slot column (padded like off): 1 when its present rows all store one
  // bit pattern, and that value (0 otherwise)
  std::vector<int32_t> uflag;
  std::vector<MV> uval;
  int64_t nuniform = 0;
};

template <typename I, typename MV>
bool dia_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, DiaHost<MV> &d,
               bool uniform = true);

// Descriptor classes of a diagonal-offset image (kry_csr::dia_cls_*). A
// slice's descriptor block is its width and, per slot column, the offset, both
// masks, the uniform flag and the bit pattern of the uniform value; slices
// whose blocks are byte-equal form one class, numbered by first occurrence in
// slice order. word[2 s], word[2 s + 1] = the first column of slice s's class
// in the class table, and its width; off / mask / uflag / uval = the distinct
// blocks concatenated in class order, padded by kDiaPad columns like the
// per-slice arrays. dia_classes fills `c` and returns true when the table is
// smaller than the per-slice descriptors and within kDiaClassMaxBytes
// (dia_class_col_bytes per column); otherwise `c` is left empty: no classes.
template <typename MV>
struct DiaClassHost {
  int64_t nclasses = 0, ncols = 0;
  std::vector<int32_t> word;
  std::vector<int32_t> off;
  std::vector<uint64_t> mask;
  std::vector<int32_t> uflag;
  std::vector<MV> uval;
};
template <typename MV>
bool dia_classes(const DiaHost<MV> &d, DiaClassHost<MV> &c);

template <typename MV>
struct CbHost {
  int64_t nb = 0, cols = 0, ng = 0;
  std::vector<int64_t> gptr;
  hvec<uint16_t> roff;
  hvec<int32_t> col;
  hvec<MV> val;
};

template <typename I, typename MV>
bool cb_build(int64_t n, const I *ip, const I *ix, const MV *dv, CbHost<MV> &cb);

template <typename MV>
struct PairHost {
  std::vector<int64_t> sptr;
  std::vector<int32_t> width;
  std::vector<int32_t> cbase;
  hvec<uint16_t> delta;
  hvec<MV> val;
  int max_width = 0;
};

template <typename I, typename MV>
bool pair_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, PairHost<MV> &p);

// ------------------------------------------- bandwidth-reducing renumbering
// Reverse Cuthill-McKee order of the row pattern (round 5), for matrices whose
// columns are scattered but whose graph has small level sets (a mesh or
// stencil numbered badly). Deterministic, level-synchronous, threaded:
//  - root: George-Liu pseudo-peripheral node, starting from the lowest-index
//    node of smallest degree; in each BFS's last level the smallest-degree
//    (then lowest-index) node is the next candidate, while the level count
//    grows (at most 4 BFS sweeps);
//  - Cuthill-McKee numbering level by level: the nodes of level k + 1 are
//    ordered by (the smallest number among their level-k neighbours, degree,
//    index), which is the sequential algorithm's order with children of one
//    parent taken by increasing degree;
//  - a node not reached (another component, or no in-edge of a
//    non-symmetric pattern) starts a new BFS at the lowest unnumbered index;
//  - reversed: perm[r] = cm[n - 1 - r] (new row r is old row perm[r]).
// Returns false (no renumbering) as soon as a level holds more than `wlimit`
// nodes: the graph has no narrow level structure (a random matrix), and the
// column-blocked image serves it instead.
template <typename I>
bool rcm_order(int64_t n, const I *ip, const I *ix, int64_t wlimit, std::vector<int32_t> &perm, int64_t *levels);

// The scatter test of the column-blocked image, without the sortedness
// requirement: x over 8 MB and at least a quarter of the entries farther
// than half a block (max(2^18, n / 16) columns) from the diagonal.
template <typename I>
bool scattered(int64_t n, const I *ip, const I *ix);

// P A P^T with every row's entries kept in their stored order (old row perm[r]
// becomes row r, column c becomes iperm[c]): the same per-row summation
// order as the input, so an SpMV over it is bitwise the input's, permuted.
template <typename I, typename MV>
void renumber_csr(int64_t n, const I *ip, const I *ix, const MV *dv, const std::vector<int32_t> &perm,
                  hvec<I> &ip2, hvec<I> &ix2, hvec<MV> &dv2);

// Rank-sorted SELL-128 image (kry_csr::rs_*, spmv_rs_kernel; round 5): the
// paired-row slice geometry (slices of 128 rows, lane l owns rows 2l, 2l + 1)
// with int32 columns, and within every run of kRsChunk consecutive stored
// entries of a row the entries sorted by column, so that slot column j of
// neighbouring rows gathers neighbouring x entries (renumbered or unsorted
// rows). Each slot word packs the column (low 28 bits) and the entry's
// position within its run of stored entries (high 4 bits); the kernel sums a
// run's products back in that stored order: bitwise csr_matvec. Padding:
// 0xFFFFFFFF. Needs n < 2^28 - 1; refused above 1.25x the SELL-64 slots.
template <typename MV>
struct RsHost {
  std::vector<int64_t> sptr;
  std::vector<int32_t> width;
  hvec<uint32_t> colrank;
  hvec<MV> val;
  int max_width = 0;
};
template <typename I, typename MV>
bool rs_build(int64_t n, const I *ip, const I *ix, const MV *dv, int64_t sell_slots, RsHost<MV> &r);

// Sparse triangular solve x = T^-1 y (kry_tri, tri.hip): the analysis of a
// triangular CSR T (lower or upper, caller's numbering, strictly sorted rows
// with the diagonal stored). level[i] = 1 + max(level[j]) over the
// off-diagonal columns j of row i (1 without any): the rows of one level are
// independent once every lower level is solved. `order` lists the rows by
// (level, row); each level is cut into slices of up to kSlice rows that never
// straddle a level (slice s of level l holds order[lrow[l] + 64 (s -
// lslice[l]) ...)), stored SELL-style: width = the slice's longest
// off-diagonal row, slot (j, r) at sptr[s] + 64 j + r. The launch plan groups
// consecutive levels [launch[q], launch[q + 1]): a run holding at most
// kTriGroupRows rows in total is one launch of one workgroup (a workgroup
// barrier between its levels); a level above kTriGroupRows rows is a launch
// of its own over many workgroups. No launch waits on another workgroup.
// With an elimination order (`rank`, a permutation: rank[i] = row i's position)
// "lower" means rank[j] < rank[i] for every off-diagonal (i, j) and "upper" the
// reverse, `order` lists the rows by (level, rank), and tri_fill stores a row's
// off-diagonal entries in ascending rank[j]: the plan and image of the
// explicitly permuted triangle, in the caller's numbering. rank == null is the
// identity.
struct TriPlan {
  int64_t n = 0, nlevels = 0, nslices = 0, nslots = 0, max_level_rows = 0;
  std::vector<int32_t> level;   // n, from 1
  std::vector<int32_t> order;   // n, rows by (level, row)
  std::vector<int32_t> lrow;    // nlevels + 1, position in order
  std::vector<int32_t> lslice;  // nlevels + 1, first slice
  std::vector<int32_t> swidth;  // nslices
  std::vector<int64_t> sptr;    // nslices + 1, slots
  std::vector<int32_t> launch;  // launches + 1, level boundaries
  std::vector<int32_t> rank;    // n, the elimination order (empty: the identity)
};
template <typename I>
void tri_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, bool lower, TriPlan &p,
              const int32_t *rank = nullptr);
// The image of the plan: rows[64 nslices] (-1 = padding), diag[64 nslices]
// (1 on padding), col / val[nslots] (col -1, val 0 = padding), every row's
// off-diagonal entries in stored order (in ascending rank under an elimination
// order). A zero diagonal is KRY_ESINGULAR.
template <typename I, typename V>
void tri_fill(const TriPlan &p, const I *ip, const I *ix, const V *dv, hvec<int32_t> &rows, hvec<V> &diag,
              hvec<int32_t> &col, hvec<V> &val);

// ILU(0) factorisation in place over A's pattern (precond.hip): the analysis
// of a square CSR A with strictly sorted rows that all store their diagonal.
// Row i is eliminated with the rows k < i of its own pattern, so its level is
// the one tri_plan(lower) gives the pattern of tril(A): `tri` is that plan
// (levels, order, lrow and the launch grouping; its slices are not used by
// the factorisation). diag[i] = the position of (i, i) in the CSR arrays.
// A row without a stored diagonal is KRY_ESINGULAR, an unsorted row KRY_EINVAL.
struct Ilu0Plan {
  TriPlan tri;
  std::vector<int64_t> diag;  // n
};
template <typename I>
void ilu0_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, Ilu0Plan &p);

// Multicolour ordering (kry_color_plan): greedy first-fit colouring, rows
// ascending, of the graph of the stored pattern of A + A^T without the
// diagonal (explicit zeros are edges): color[i] = the smallest integer >= 0
// that no neighbour j < i has. perm lists the rows by (colour, row). O(nnz).
template <typename I>
void color_plan(int64_t n, int64_t nnz, const I *ip, const I *ix, std::vector<int32_t> &color,
                std::vector<int32_t> &perm, int64_t *ncolors, int64_t *max_rows);

// Block-Jacobi (kry_bjacobi, bjacobi.hip): the partition and the task list of
// the factor kernel. starts[nblocks] begins at 0, increases strictly and stays
// below n; block i is rows and columns [starts[i], starts[i + 1]), n closing
// the last one; a block holds 1 to kBjMaxBlock rows. A block of b rows belongs
// to a lane group of g = 4, 8, 16 or 32 lanes (the smallest holding it), 64 / g
// blocks to a wavefront: `blocklist` lists the blocks by (g, block), and task t
// = {first, count, g} is the blocks blocklist[first, first + count) of one
// wavefront (count = 64 / g but for the last task of a class). A malformed
// partition is KRY_EINVAL, a block above kBjMaxBlock rows KRY_EUNSUPPORTED.
constexpr int kBjMaxBlock = 32;
struct BjTask {
  int32_t first, count, g;
};
struct BjPlan {
  int64_t n = 0, nblocks = 0, values = 0;  // values = sum of b_i^2
  int32_t min_block = 0, max_block = 0;
  std::vector<int32_t> blocklist;  // nblocks
  std::vector<BjTask> tasks;
};
void bjacobi_plan(int64_t n, int64_t nblocks, const int32_t *starts, BjPlan &p);

}  // namespace kry
