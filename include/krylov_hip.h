/*
 * krylov_hip.h — C-ABI of libkrylov_hip.so, the MI355X (gfx950) inner loop of
 * the Krylov solvers cg / gmres / minres.
 *
 * The reference (ju-liu/krylov 0.0.3) is pure Python: its hot path ends in
 * SciPy/OpenBLAS/LAPACK calls made from the solver loops. Each entry point
 * below replaces one of those call sites (cited per function) and is bound
 * from Python through ctypes (krylov_amd/_lib.py; INTEGRATION.md shows the
 * stub). Plain pointers and sizes only; no C++ exceptions cross this boundary.
 *
 * Conventions
 *  - Every function returns an int status: KRY_OK (0) or a negative KRY_E*
 *    code; kry_last_error() returns the message of the calling thread's last
 *    failure.
 *  - Handles are opaque and owned by the caller (create/destroy pairs).
 *  - A vector is an n x k block stored row-major (the reference's "blocked"
 *    right-hand sides, b.shape == (n, k)); k = 1 is a plain vector.
 *  - One kry_ctx = one device + one HIP stream; a context is not thread-safe.
 *  - Host buffers are C-contiguous arrays of the stated dtype.
 *  - Device-resident state: per-iteration scalars never leave the GPU; the
 *    solver "run" calls return the residual-norm history of the steps they
 *    executed (the only mandatory device-to-host traffic).
 */
#ifndef KRYLOV_HIP_H
#define KRYLOV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kry_ctx kry_ctx;
typedef struct kry_csr kry_csr;
typedef struct kry_vec kry_vec;
typedef struct kry_cg kry_cg;
typedef struct kry_gmres kry_gmres;
typedef struct kry_minres kry_minres;
typedef struct kry_comm kry_comm;
typedef struct kry_prog kry_prog;
typedef struct kry_tri kry_tri;
typedef struct kry_precond kry_precond;
typedef struct kry_bjacobi kry_bjacobi;

/* value / index types */
enum { KRY_F32 = 1, KRY_F64 = 2 };
enum { KRY_I32 = 1, KRY_I64 = 2 };

/* status codes */
enum {
  KRY_OK = 0,
  KRY_EINVAL = -1,       /* bad argument (shape, dtype, null handle)   -> ValueError      */
  KRY_ENOMEM = -2,       /* device allocation failed                   -> MemoryError     */
  KRY_EDEVICE = -3,      /* HIP runtime / no device                    -> RuntimeError    */
  KRY_EINVARIANT = -4,   /* Krylov space invariant (arnoldi.py:168-171) -> ArgumentError  */
  KRY_EUNSUPPORTED = -5, /* outside the device path's scope            -> NotImplementedError */
  KRY_ESINGULAR = -6,    /* singular triangular factor (gmres.py:36)   -> LinAlgError     */
  KRY_ENONFINITE = -7,   /* NaN/inf handed to solve_triangular         -> ValueError      */
  KRY_ECOMM = -8         /* RCCL failure                               -> RuntimeError    */
};

/* ---- library / context ------------------------------------------------ */
int kry_version(void);
const char *kry_last_error(void);
/* The build stamp of this library (kry_version() >= 106): the first 16 hex
 * digits of the sha256 over its HIP/C++ sources, fixed at build time
 * (csrc/Makefile). Measurements taken on one build (profiles/ PMC passes) are
 * stamped with it, so a benchmark can tell whether they describe the code it
 * runs. No reference counterpart. */
const char *kry_build_id(void);
int kry_device_count(int *count);
int kry_ctx_create(int device, kry_ctx **out);
int kry_ctx_destroy(kry_ctx *ctx);
int kry_ctx_synchronize(kry_ctx *ctx);

/* ---- device memory -------------------------------------------------------
 * The library's device buffers come from a caching allocator: blocks freed by
 * a destroyed solver / operator / vector are reused by the next allocation of
 * the same rounded size (after one device synchronisation), instead of a
 * hipMalloc + hipFree pair per reference-API call (the reference allocates
 * its NumPy work arrays per call, cg.py:116-131, arnoldi.py:129-131).
 * KRYLOV_ALLOC_CACHE=0 disables it; KRYLOV_ALLOC_CACHE_MAX_GB caps it (16).
 * stats: out[0..5] = bytes in use, bytes cached, reuses, hipMallocs, device
 * syncs taken to retire freed blocks, enabled (0/1). release: hipFree every
 * cached block (in use blocks are untouched). */
int kry_mem_stats(int64_t *out);
int kry_mem_release(void);

/* ---- CSR operator ------------------------------------------------------
 * Replaces the scipy.sparse matrix the reference multiplies with `A @ x`
 * (_helpers.py:44-48 Product.__matmul__, cg.py:86, gmres.py:106,
 * minres.py:111,121). Uploads once; the library owns the device copy, which
 * it lays out as SELL-64 (slices of 64 rows = one wavefront, column-major
 * within a slice; slices with very uneven rows stay CSR). Indices may be
 * unsorted and contain duplicates; they are honoured in stored order (SciPy
 * csr_matvec semantics). */
int kry_csr_create(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr,
                   const void *indices, const void *data, int dtype, int itype,
                   kry_csr **out);
int kry_csr_destroy(kry_csr *A);
/* kry_csr_create with another operator's bandwidth-reducing renumbering
 * (kry_version() >= 104): the image holds P M P^T for `like`'s permutation P
 * (rows' entries in their stored order), so M can precondition solves with
 * `like` (kry_*_set_preconditioners refuses operators renumbered differently).
 * Same as kry_csr_create when `like` is not renumbered. Replaces the
 * preconditioner operands M / Ml / Mr of cg.py:70-110, gmres.py:105-139,
 * minres.py:95-151 for a renumbered A. */
int kry_csr_create_like(kry_ctx *ctx, const kry_csr *like, int64_t n, int64_t nnz, const void *indptr,
                        const void *indices, const void *data, int dtype, int itype, kry_csr **out);
/* kry_csr_create with the renumbering under the caller's control
 * (kry_version() >= 110): renumber = 0 keeps the caller's numbering whatever
 * the matrix looks like (KRY_RENUMBER is not consulted), anything else is
 * kry_csr_create. The matrices of a factorised preconditioner's
 * approximate-inverse stages (kry_precond_add_isai) are built this way: the
 * stages work in the caller's numbering. */
int kry_csr_create_ex(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices,
                      const void *data, int dtype, int itype, int renumber, kry_csr **out);
/* Renumbering (kry_version() >= 104). kry_csr_create renumbers a matrix whose
 * columns are scattered (the column-blocked test below) but whose graph has
 * narrow BFS levels (a mesh or stencil stored in a bad order) by reverse
 * Cuthill-McKee; its images then hold P A P^T with every row's entries in
 * stored order, so the SpMV stays bitwise csr_matvec. Every vector still
 * crosses the C-ABI in the caller's numbering: kry_*_start permutes b / x0 /
 * weights in, kry_*_get, kry_gmres_xk_device and kry_spmv permute out. The
 * reference multiplies the caller's matrix as given (_helpers.py:44-48): this
 * is storage order only. kry_csr_permute moves the rows of an n x k block
 * into the operator's numbering (to_operator = 1: dst[r] = src[perm[r]]) or
 * back (0), for callers that keep their own device vectors in the operator's
 * numbering (kry_prog_*). KRY_RENUMBER=0 disables renumbering. */
int kry_csr_permute(kry_ctx *ctx, const kry_csr *A, const kry_vec *src, kry_vec *dst, int to_operator);
/* Byte comparison of two operators' SELL-64 and diagonal-offset images and
 * their sizes (kry_version() >= 104; tests: kry_csr_create builds those images
 * on the device for int32 CSR, KRY_DEVICE_BUILD=0 on the host, and the two
 * must be identical): out[0] = number of differing items, out[1] = bitmask.
 * From kry_version() 107 bits 23, 24 and 25 cover the uniform slot columns of
 * the diagonal-offset image (their count, flags and values); the earlier bits
 * keep their meaning. */
int kry_csr_compare(const kry_csr *A, const kry_csr *B, int64_t *out);
/* kry_spmv with x and y already in the operator's numbering (kry_csr_permute);
 * the same as kry_spmv for an operator that is not renumbered. */
int kry_spmv_op(kry_ctx *ctx, kry_csr *A, kry_vec *x, kry_vec *y);
/* Host-only (no device): the reverse Cuthill-McKee order kry_csr_create
 * would use (int32 indices): info[0..1] = built (0 = a BFS level exceeded
 * wlimit nodes: no narrow level structure), BFS levels of the numbering;
 * when built and perm is non-null: perm[n], new row r = old row perm[r].
 * wlimit <= 0 takes the library's default (max(2^16, n / 32)). */
int kry_rcm_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t wlimit,
                 int64_t *info, int32_t *perm);
/* The same order computed on the device (what kry_csr_create runs; int32
 * CSR from the host, uploaded inside): info[0] = 1 built, 0 refused, -1 gave
 * up (more than 64 components: kry_csr_create then uses the host order),
 * info[1] = levels; perm as kry_rcm_plan's, node for node. */
int kry_rcm_device(kry_ctx *ctx, int64_t n, int64_t nnz, const int32_t *indptr, const int32_t *indices, int64_t wlimit,
                   int64_t *info, int32_t *perm);
/* Host-only: the rank-sorted SELL-128 plan (kry_version() >= 104; the image a
 * matrix takes for single-RHS SpMVs when no DIA, column-blocked or paired
 * image is built): info[0..3] = built, slices, slots, widest slice; when built
 * and the arrays are non-null: widths[slices], colrank[slots] (slot of row r,
 * slot column j of its slice at 128 * (sptr[s] / 128 + j) + r - 128 s: the
 * column in bits 0..27, its position among the run of 16 stored entries it
 * belongs to in bits 28..31, 0xFFFFFFFF = padding). */
int kry_rs_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                int32_t *widths, uint32_t *colrank);
/* Host-only (no GPU needed): the SELL-64 plan kry_csr_create will build —
 * slice count, stored slots (nonzeros + padding of regular slices) and the
 * number of irregular slices (64 * width > 2 * slice_nnz + 1024) that the
 * kernel walks in CSR form instead. */
int kry_csr_layout(int64_t n, const void *indptr, int itype, int64_t *nslices,
                   int64_t *nslots, int64_t *nirregular);
/* Host-only: the diagonal-offset (SELL-128/DIA) plan kry_csr_create would
 * build for these CSR arrays (no device needed). info[0..3] = built (0/1),
 * slices, slots, widest slice; when built and the arrays are non-null:
 * widths[slices], offsets[slots / 128] (each slice's sorted offsets col - row),
 * masks[2 * slots / 128] (word q, bit l: row 128 s + 2 l + q has an entry at
 * that offset). Call once with null arrays to size them. */
int kry_dia_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                 int32_t *widths, int32_t *offsets, uint64_t *masks);
/* Host-only (kry_version() >= 107): the uniform slot columns of that image. A
 * slot column is uniform when the stored values of all its present rows (the
 * mask bits; holes take no part) have one bit pattern (-0.0 differs from
 * +0.0, NaNs compare by payload, a single present row is uniform). The
 * single-RHS SpMV takes such a column's value from its descriptor and does
 * not read its 128 stored values; the result stays bitwise csr_matvec.
 * KRY_DIA_UNIFORM=0 in the environment at kry_csr_create flags no column
 * (this plan ignores the variable). `data` holds nnz values of `dtype`.
 * info[0..2] = built (0/1), slot columns (slots / 128), uniform ones; when
 * built and the arrays are non-null: flags[slots / 128] (0/1) and
 * values[slots / 128] in `dtype` (0 where not flagged). */
int kry_dia_uniform_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data, int dtype,
                         int itype, int64_t *info, int32_t *flags, void *values);
/* Host-only view of the diagonal-offset image's descriptor classes (no device
 * needed, kry_version() >= 112). A slice's descriptor block is its width and,
 * per slot column, the offset, both lane masks, the uniform flag and the bit
 * pattern of the uniform value; slices whose blocks are byte-equal share one
 * class (numbered by first occurrence), and the single-RHS kernel reads the
 * class's descriptors from a table of the distinct blocks. The image takes
 * classes only when that table is smaller than the per-slice descriptors and
 * at most 1 MiB. `uniform` = 0 builds the image without uniform slot columns
 * (KRY_DIA_UNIFORM=0). info[0..3] = built (0/1), slot columns, classes,
 * class-table columns (both 0 when the image takes no classes). */
int kry_dia_class_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data, int dtype,
                       int itype, int uniform, int64_t *info);
/* Host-only view of the paired-row SELL-128 plan (no device needed; the
 * image kry_csr_create builds for a general matrix, kry_version() >= 102):
 * info[0..3] = built (0 = refused: a slot column spans more than 65534
 * columns, n >= 2^31, or more than 1.25x the SELL-64 slots), slices, slots,
 * widest slice; when built and the arrays are non-null: widths[slices],
 * cbase[slots / 128] (each slot column's smallest column), deltas[slots]
 * (column - base at slot 128 * (sptr[s] / 128 + j) + row - 128 s, 0xFFFF =
 * padding). Call once with null arrays to size them. */
int kry_pair_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                  int32_t *widths, int32_t *cbase, uint16_t *deltas);
/* Host-only view of the column-blocked plan (no device needed; the image
 * kry_csr_create builds for single-RHS SpMVs of a matrix with scattered
 * columns when the diagonal-offset image is not built, kry_version() >= 103):
 * info[0..3] = built (0 = refused: int64 indices, x under 8 MB, rows not
 * sorted, fewer than a quarter of the entries more than half a block from the
 * diagonal, or a segment over 65535 entries), column blocks nb, columns per
 * block, 256-row groups ng; when built and gptr is non-null: gptr[nb * ng + 1],
 * the first entry of segment (block b, group g) at gptr[b * ng + g]. */
int kry_cb_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                int64_t *gptr);
/* The device image kry_csr_create built, size-checked: writes the first
 * min(len, KRY_CSR_INFO_LEN) of info[0..8] = slices, slots, irregular slices,
 * compact (1 when the column indices are stored as uint16 deltas over
 * per-slot-column int32 bases: every slot column spans <= 65534 columns,
 * int32 indices and KRY_SELL_COMPACT != 0 in the environment), the number of
 * column blocks of the column-blocked image used by single-RHS SpMVs on
 * scattered sparsity (0 = none; KRY_SPMV_CB=0 disables), dia (1 when the
 * diagonal-offset image serves single-RHS SpMVs: int32 indices, every row
 * strictly sorted, the rows of each 64-row slice sharing a short list of
 * column offsets; KRY_SPMV_DIA=0 disables) and that image's slot count,
 * then (kry_version() >= 102) pair (1 when the paired-row SELL-128 image
 * serves single-RHS SpMVs of a general matrix: no diagonal-offset or
 * column-blocked image, n < 2^31, every 128-row slot column spans <= 65534
 * columns, at most 1.25x the SELL-64 slots; KRY_SPMV_PAIR=0 disables) and
 * that image's slot count. Fields added later go at the end, so a caller
 * built against this header keeps working (kry_version() >= 101). */
/* then (kry_version() >= 104) rs (1 when the rank-sorted SELL-128 image
 * serves single-RHS SpMVs), its slot count, renumbered (1 when the images hold
 * the reverse Cuthill-McKee renumbering P A P^T) and the renumbering's BFS
 * level count. */
/* then (kry_version() >= 107) the number of uniform slot columns of the
 * diagonal-offset image (0 with KRY_DIA_UNIFORM=0) and the bytes of matrix
 * values the single-RHS kernel still streams per SpMV: (slot columns -
 * uniform ones) * 128 * the value size. */
/* then (kry_version() >= 111) dia_lean: 1 when the single-RHS kernel of the
 * diagonal-offset image loads x at 32-bit byte offsets through a buffer
 * descriptor (the default while (n + 2) * 8 bytes fit it), 0 when it forms
 * per-lane 64-bit addresses (KRY_DIA_LEAN=0, or a larger n) or there is no
 * such image. */
/* then (kry_version() >= 112) dia_classes and dia_class_cols: the descriptor
 * classes the single-RHS kernel of the diagonal-offset image reads (see
 * kry_dia_class_plan) and the slot columns of their table; both 0 when the
 * image took none, with KRY_DIA_CLASSES=0, or when the table exceeds
 * KRY_DIA_CLASS_MAX_BYTES (read at the operator's first use; it can only
 * lower the 1 MiB limit). */
#define KRY_CSR_INFO_LEN 18
int kry_csr_info_n(const kry_csr *A, int64_t *info, int32_t len);
/* The version-100 form: info[0..4] only (`info` holds 5 values). */
int kry_csr_info(const kry_csr *A, int64_t *info);

/* ---- vectors (n x k row-major blocks) ---------------------------------- */
int kry_vec_create(kry_ctx *ctx, int64_t n, int32_t k, int dtype, kry_vec **out);
int kry_vec_destroy(kry_vec *v);
int kry_vec_upload(kry_vec *v, const void *host);
int kry_vec_download(kry_vec *v, void *host);

/* ---- primitives --------------------------------------------------------
 * y = A @ x. Replaces SciPy csr_matvec / csr_matvecs (SURVEY §2 kernel
 * table); bitwise equal to them (sequential per-row sum, no FMA). */
int kry_spmv(kry_ctx *ctx, kry_csr *A, kry_vec *x, kry_vec *y);
/* out[c] = sum_i x[i,c] * (w[i] * y[i,c])  (w == NULL: plain). Replaces
 * get_default_inner (_helpers.py:101-110) and the weighted inner of
 * tests/test_solvers.py:157-161. Deterministic two-stage reduction. */
int kry_dot(kry_ctx *ctx, kry_vec *x, kry_vec *y, kry_vec *w, double *out);
/* y = alpha[c] * x + y  (the reference's `y += alpha * x`, e.g. cg.py:196). */
int kry_axpy(kry_ctx *ctx, const double *alpha, kry_vec *x, kry_vec *y);
/* z = one of the reference's vector expressions, per column c (k <= 64),
 * evaluated exactly as its NumPy expression tree; stream-ordered (no sync):
 *   form 0: z = x + a[c] * y             (x += alpha * p, bicgstab.py:120)
 *   form 1: z = x + a[c] * (y + b[c] * w)  (cgs.py:88)
 *   form 2: z = x + a[c] * (y - b[c] * w)  (bicgstab.py:109)
 *   form 3: z = x / a[c]   form 4: z = x - y   form 5: z = x + y
 *   form 6: z = x          form 7: z = a[c] * x
 * z may alias x, y or w. Replaces the AXPY-type lines of the other
 * solvers (bicgstab.py, cgs.py, cgr.py, gcr.py; krylov_amd/extra.py). */
int kry_vec_lincomb(kry_ctx *ctx, int form, kry_vec *z, kry_vec *x, kry_vec *y, kry_vec *w,
                    const double *a, const double *b);
/* ---- device-resident scalar chain of the other solvers --------------------
 * bicgstab.py:24-144, cgs.py:24-117, cgr.py:16-100, gcr.py:18-97 (driven by
 * krylov_amd/extra.py): the per-iteration scalars live in a device register
 * file of nregs rows of k float64 values, so a chunk of iterations is
 * enqueued with no host round trip and read back with one sync.
 * create: nregs registers, k columns (power of two <= 64), history capacity
 *         `cap` steps per chunk.
 * set / get: register r (r = -1 in set: the criterion row, +inf on padded
 *         columns) from / to k host doubles (synchronous).
 * begin: start a chunk (every step runs until a check stops it).
 * scalar: register ops of the reference's scalar lines, float64:
 *         op 0 d = a; 1 d = a / g(b); 2 d = (a * b) / g(c * e); 3 d = sqrt(a);
 *         4 d = g(a); 5 d = value   (g(x) = x != 0 ? x : 1, np.where guard)
 * dot:   register d = inner(x, y) per column (w: weights or NULL).
 * lincomb: kry_vec_lincomb's forms with a = sa * reg[ra], b = sb * reg[rb]
 *         (register -1 = unused; sa, sb = +1 / -1). As there, a form's own
 *         operands are required: KRY_EINVAL for a null y (forms 0, 1, 2, 4,
 *         5) or w (1, 2), and for ra = -1 (0, 1, 2, 3, 7) or rb = -1 (1, 2);
 *         operands a form does not read are ignored and may be NULL / -1.
 * spmv:  y = A x.
 * check: register r against the criterion: mode 0 appends it to the chunk
 *         history and stops the chunk after this step when every column
 *         meets it; mode 1 (bicgstab's mid-step test on the previous iterate,
 *         bicgstab.py:123-127) stops the chunk AT this step on success and
 *         records its row there; mode | 4: compare the norm rounded to
 *         float32 (the history of a float32 solve).
 * end:   one sync: *done steps ran in full, *midstep = 1 if a mode-1 check
 *         stopped step *done; rows receives done (+ midstep) rows of k.
 * Every launch takes the chunk step it belongs to and does nothing once a
 * check has stopped the chunk before it. */
int kry_prog_create(kry_ctx *ctx, int32_t nregs, int32_t k, int32_t cap, kry_prog **out);
int kry_prog_destroy(kry_prog *p);
int kry_prog_set(kry_prog *p, int32_t r, const double *vals);
int kry_prog_get(kry_prog *p, int32_t r, double *vals);
int kry_prog_begin(kry_prog *p);
int kry_prog_end(kry_prog *p, int32_t steps, int32_t *done, int32_t *midstep, double *rows);
int kry_prog_scalar(kry_prog *p, int32_t op, int32_t d, int32_t a, int32_t b, int32_t c, int32_t e, double value,
                    int32_t step);
int kry_prog_dot(kry_prog *p, kry_vec *x, kry_vec *y, kry_vec *w, int32_t d, int32_t step);
int kry_prog_lincomb(kry_prog *p, int32_t form, kry_vec *z, kry_vec *x, kry_vec *y, kry_vec *w, int32_t ra, double sa,
                     int32_t rb, double sb, int32_t step);
int kry_prog_spmv(kry_prog *p, kry_csr *A, kry_vec *x, kry_vec *y, int32_t step);
int kry_prog_check(kry_prog *p, int32_t r, int32_t mode, int32_t step);
/* Chain steps of the stationary solvers (stationary.py:11-157; driven by
 * krylov_amd/stationary.py):
 * rowscale: z = x / d (mul = 0) or z = x * d (mul = 1) with d an (n,) vector
 *         of the vectors' dtype broadcast over the columns (jacobi's
 *         `(r.T / D).T`, stationary.py:21; ssor's `(y.T * d).T`, :78, :90).
 * permute: kry_csr_permute as a chain step (a renumbered A: the residual
 *         leaves the operator's numbering before a triangular solve in the
 *         caller's numbering, and the update re-enters it). src != dst.
 * trisolve: kry_tri_solve as a chain step. */
int kry_prog_rowscale(kry_prog *p, int32_t mul, kry_vec *z, kry_vec *x, kry_vec *d, int32_t step);
int kry_prog_permute(kry_prog *p, const kry_csr *A, const kry_vec *src, kry_vec *dst, int32_t to_operator,
                     int32_t step);
int kry_prog_trisolve(kry_prog *p, const kry_tri *T, const kry_vec *y, kry_vec *x, int32_t step);

/* ---- sparse triangular solve ------------------------------------------------
 * x = T^-1 y for a sparse triangular T (lower != 0: lower, else upper) in CSR
 * with strictly sorted rows and the diagonal stored; values of the vectors'
 * dtype. Replaces scipy spsolve_triangular in gauss_seidel / sor / ssor
 * (stationary.py:26-94). Row i is x_i = (y_i - sum_j T_ij x_j) / T_ii, the sum
 * one term at a time in stored order, a true division, no FMA: bitwise
 * repeatable and independent of the launch plan and of k (<= 64 columns, a
 * power of two). x may alias y.
 * Analysis (host): level[i] = 1 + max(level[j]) over row i's off-diagonal
 * columns; rows ordered by (level, row) and cut into slices of up to 64 rows
 * that never straddle a level (SELL-64 style, slice width = its longest
 * off-diagonal row). Launch plan: consecutive levels holding at most 1024 rows
 * together are one launch of one workgroup (workgroup barriers between the
 * levels); a larger level is a launch of its own over many workgroups. No
 * kernel waits on another workgroup: stream order is the only dependency
 * between launches.
 * kry_tri_plan (host-only, no device): info[0..4] = levels, launches, slices,
 * slots, rows of the largest level; when non-null: level[n] (from 1), order[n]
 * (rows by (level, row)), launch[launches + 1] (launch q runs levels
 * [launch[q], launch[q + 1]), counted from 0), widths[slices]. Call once with
 * null arrays to size them. A row without a diagonal entry is KRY_ESINGULAR,
 * an entry on the wrong side of the diagonal or an unsorted row KRY_EINVAL.
 * kry_tri_create: analysis + upload (a zero diagonal value: KRY_ESINGULAR).
 * kry_tri_info: info[0..5] = the five values above and the image's bytes.
 * kry_tri_plan_ordered / kry_tri_create_ordered (kry_version() >= 109): the
 * same over an elimination order, rank[i] = row i's position in it (a
 * permutation of 0..n-1, else KRY_EINVAL). "Lower" then means rank[j] < rank[i]
 * for every off-diagonal (i, j) and "upper" the reverse (an entry on the wrong
 * side: KRY_EINVAL); the levels come from that dependency graph, the rows are
 * ordered by (level, rank), and a row's terms are summed in ascending rank[j].
 * The solve is bitwise the solve of the explicitly permuted triangle
 * T[perm][:, perm] (rank[perm[r]] = r), but T, y and x stay in the caller's
 * numbering and no permutation pass runs over the vectors. rank = NULL is the
 * identity: exactly kry_tri_plan / kry_tri_create. */
int kry_tri_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int lower, int64_t *info,
                 int32_t *level, int32_t *order, int32_t *launch, int32_t *widths);
int kry_tri_create(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                   int dtype, int itype, int lower, kry_tri **out);
int kry_tri_plan_ordered(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int lower,
                         const int32_t *rank, int64_t *info, int32_t *level, int32_t *order, int32_t *launch,
                         int32_t *widths);
int kry_tri_create_ordered(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices,
                           const void *data, int dtype, int itype, int lower, const int32_t *rank, kry_tri **out);
/* Multicolour ordering (kry_version() >= 109; host-only, no device). In the
 * caller's numbering a stencil's triangles have thousands of thin dependency
 * levels, one launch each; eliminating colour by colour makes every level a
 * whole colour. Graph: the stored pattern of A + A^T without the diagonal
 * (explicit zeros are edges). Greedy first-fit in ascending row order:
 * color[i] = the smallest integer >= 0 that no neighbour j < i has
 * (deterministic, O(nnz)). perm[n] lists the rows by (colour, row): the
 * permuted matrix is A[perm][:, perm], and rank[perm[r]] = r is the
 * elimination order kry_tri_create_ordered takes. info[0] = colours, info[1] =
 * rows of the largest colour. Null arrays size the call. */
int kry_color_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                   int32_t *color, int32_t *perm);
int kry_tri_destroy(kry_tri *T);
int kry_tri_info(const kry_tri *T, int64_t *info);
int kry_tri_solve(kry_ctx *ctx, const kry_tri *T, const kry_vec *y, kry_vec *x);

/* ---- factorised preconditioners: ILU(0) and the stage object (kry_version() >= 108)
 * The reference takes any object with `@` as M / Ml / Mr (_helpers.py:83-90);
 * its users hand it SSOR and incomplete-LU operators built on scipy
 * spsolve_triangular. On the device those are a kry_precond: a short fixed
 * sequence of stages on n x k vectors in the caller's numbering, each a
 * kry_tri solve or a row scale by an (n,) vector (z = z * d). SSOR is lower
 * solve, scale by D (2 - omega) / omega, upper solve; ILU(0) is L solve, U solve.
 * kry_ilu0_plan (host-only, no device): the analysis of the factorisation of a
 * CSR A with strictly sorted rows that all store their diagonal. Row i is
 * eliminated with the rows k < i of its own pattern, so its levels and launch
 * grouping are those of kry_tri_plan(lower = 1) on the pattern of tril(A).
 * info[0..2] = levels, launches, rows of the largest level; when non-null:
 * level[n] (from 1), order[n], launch[launches + 1] as kry_tri_plan's, and
 * diag[n], the position of (i, i) in the CSR arrays. A row without a stored
 * diagonal is KRY_ESINGULAR, an unsorted row KRY_EINVAL.
 * kry_ilu0_factor: the factorisation on the device (int32 indices), in place
 * over a copy of `data` returned in `values` (nnz values of `dtype`; the strict
 * lower part is L, unit diagonal implied, the rest U). For rows i ascending:
 *   for k in cols(i), k < i, ascending:
 *     a_ik = a_ik / a_kk
 *     for j in cols(i), j > k, with (k, j) stored: a_ij = a_ij - (a_ik * a_kj)
 * with a true division and the product rounded before the subtraction (no
 * FMA): bitwise that sequential loop, whatever the launch plan. One wavefront
 * per row, one launch per run of levels as kry_tri_solve's (no kernel waits on
 * another workgroup). info[0..2] as the plan's, info[3] = the smallest row whose
 * pivot came out 0 or non-finite (-1: none); such a pivot is KRY_ESINGULAR.
 * kry_precond_create / add_tri / add_scale / destroy: the stage list. Stages
 * are borrowed: the caller keeps the kry_tri / kry_vec handles alive as long
 * as the preconditioner, which must match them in n and dtype.
 * kry_precond_fuse (kry_version() >= 109; after the last stage, for objects
 * whose solves were built under a multicolour elimination order): apply the
 * stages in fewer launches, bitwise the stage-by-stage apply. A row scale in
 * front of a solve goes into that solve (num = (y * s) - acc, the product
 * rounded first); where the last level of a solve is a launch of its own and
 * the first level of the next solve holds exactly the same rows without
 * off-diagonal entries (two colours), one launch does both, t = (y - acc) / d1,
 * u = t * s, z = u / d2 in that order. KRY_PRECOND_FUSE=0, read by
 * kry_precond_create, makes this call a no-op.
 * kry_precond_info: info[0..4] = launches per apply (an approximate-inverse
 * stage counts its SpMVs, 1 + 2 sweeps), fused (0/1), stages, scales folded
 * into a solve, fused level boundaries.
 * kry_precond_apply: y = P x (k <= 64 columns, a power of two; y may alias x).
 * kry_prog_precond: the same as a chain step.
 * kry_*_set_precond: a factorised preconditioner in slot 0 = M, 1 = Ml, 2 = Mr
 * (CG: 0 or 1) of a solver, after kry_*_set_preconditioners (which clears every
 * slot) and before start. The preconditioner's dtype must be the vectors'; an
 * operator renumbered at upload and a sharded solve are KRY_EUNSUPPORTED. The
 * inner products a matrix preconditioner's SpMV fuses (cg.py:205-209,
 * arnoldi.py:184-185) are taken by one element-wise pass after the stages.
 * Approximate-inverse solves (kry_version() >= 110; the incomplete sparse
 * approximate inverse of Anzt, Huckle, Braeckle and Dongarra). A triangular
 * factor T is replaced by a sparse W on T's own pattern with (W T) = I on that
 * pattern, so a solve is one SpMV; relaxation sweeps x = x + W (y - T x) win
 * back the exact solve's quality.
 * kry_isai_lower: W's values (nnz values of `dtype`, in `values`) for a lower
 * triangular CSR T with int32 indices, strictly sorted rows that each end in
 * their diagonal entry. Row i with pattern J[0..m-1], J[m-1] = i:
 *   w[m-1] = 1 / t(i,i)
 *   for p = m-2 .. 0:
 *     s = 0
 *     for q = p+1 .. m-1 ascending, t(J[q],J[p]) stored: s = s - (t(J[q],J[p]) * w[q])
 *     w[p] = s / t(J[p],J[p])
 * with true divisions and the product rounded before the subtraction (no
 * FMA): bitwise that sequential loop. The rows are independent: one launch,
 * several short rows to a wavefront, the lookups of t(J[q],J[p]) binary
 * searches run in parallel over q. info[0] = the smallest row whose diagonal is
 * 0 or non-finite (-1: none; such a diagonal is KRY_ESINGULAR), info[1] = the
 * longest row, info[2] = the kernel's time in microseconds. A row of more than
 * 1024 entries is KRY_EUNSUPPORTED, a row that does not end in its diagonal or
 * is not strictly sorted KRY_EINVAL. An upper factor U takes the same call on
 * U^T, W_U = W(U^T)^T (the right inverse, (U W_U) = I on U's pattern), so
 * W_U = W_L^T bitwise when U = L^T.
 * kry_precond_add_isai: a stage x = W y, then `sweeps` times
 * x = x + W (y - T x), then x = scale * x when `scale` (an (n,) vector) is
 * non-null, folded into the store of the stage's last SpMV. W and T (NULL
 * exactly when sweeps = 0) are kry_csr operators of the preconditioner's dtype
 * created with kry_csr_create_ex(renumber = 0), borrowed like the other
 * stages; a stage is 1 + 2 sweeps SpMVs. A preconditioner holds either such
 * stages or solves and scales (KRY_EINVAL otherwise); with them it takes up to
 * 256 columns, and it owns the blocks between its SpMVs, allocated at the
 * first apply of a column count. */
int kry_ilu0_plan(int64_t n, int64_t nnz, const void *indptr, const void *indices, int itype, int64_t *info,
                  int32_t *level, int32_t *order, int32_t *launch, int64_t *diag);
int kry_isai_lower(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                   int dtype, int itype, void *values, int64_t *info);
int kry_precond_add_isai(kry_precond *P, const kry_csr *W, const kry_csr *T, int32_t sweeps, const kry_vec *scale);
int kry_ilu0_factor(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                    int dtype, int itype, void *values, int64_t *info);
int kry_precond_create(kry_ctx *ctx, int64_t n, int dtype, kry_precond **out);
int kry_precond_destroy(kry_precond *P);
int kry_precond_add_tri(kry_precond *P, const kry_tri *T);
int kry_precond_add_scale(kry_precond *P, const kry_vec *d);
int kry_precond_fuse(kry_precond *P);
int kry_precond_info(const kry_precond *P, int64_t *info);
int kry_precond_apply(kry_ctx *ctx, const kry_precond *P, const kry_vec *x, kry_vec *y);
int kry_prog_precond(kry_prog *p, const kry_precond *P, const kry_vec *x, kry_vec *y, int32_t step);
int kry_cg_set_precond(kry_cg *s, int32_t slot, const kry_precond *P);
int kry_gmres_set_precond(kry_gmres *s, int32_t slot, const kry_precond *P);
int kry_minres_set_precond(kry_minres *s, int32_t slot, const kry_precond *P);

/* ---- block-Jacobi preconditioner (kry_version() >= 113) ----------------------
 * M = blockdiag(A_11, ..., A_mm)^-1: the diagonal blocks of A inverted once on
 * the device, an apply one batched dense block product in ONE launch, for up
 * to 256 columns (a power of two). Partition: starts[nblocks] (int32) with
 * starts[0] = 0, strictly increasing, every entry < n; block i is rows and
 * columns [starts[i], starts[i + 1]), n closing the last one; 1 to 32 rows per
 * block. Block i is the dense b x b array of A's stored entries inside it
 * (CSR with int32 indices and strictly sorted rows), zeros elsewhere.
 * Inverse: in-place Gauss-Jordan with row pivoting in `dtype` scalars,
 *   for c = 0 .. b-1:
 *     p = c; for r = c+1 .. b-1: if |M[r,c]| > |M[p,c]|: p = r
 *     swap rows c and p; piv[c] = p
 *     d = M[c,c]; d == 0 or not finite: the block is singular
 *     M[c,c] = 1; M[c,j] = M[c,j] / d for every j
 *     for every r != c: f = M[r,c]; M[r,c] = 0; M[r,j] = M[r,j] - (f * M[c,j]) for every j
 *   for c = b-1 .. 0: swap columns c and piv[c]
 * with true divisions and the product rounded before the subtraction (no
 * FMA): bitwise that sequential loop.
 * Apply: y[r,c] = sum_j (X[r-s,j] * x[s+j,c]) for row r of a block with rows
 * [s, s+b) and inverse X, from 0 over j ascending, each product rounded before
 * its addition, all b terms whatever their values (a non-finite x entry
 * poisons its own block and no other); bitwise independent of k, the grid and
 * the launch shape. y may alias x (the apply then works from a copy of x).
 * kry_bjacobi_plan (host-only, no device): checks the partition (malformed:
 * KRY_EINVAL; a block above 32 rows: KRY_EUNSUPPORTED, naming it) and returns
 * the factor kernel's task list. A block of b rows belongs to a group of g =
 * 4, 8, 16 or 32 lanes, the smallest holding it, 64 / g blocks to a wavefront:
 * blocklist[nblocks] lists the blocks by (g, block), and task t is
 * tasks[3 t .. 3 t + 2] = {first, count, g}, the blocks blocklist[first,
 * first + count) of one wavefront (count = 64 / g but for the last task of a
 * class). info[0..3] = tasks, largest block, smallest block, sum of b_i^2. Call
 * once with null arrays to size them.
 * kry_bjacobi_create: plan, upload, extraction and inversion (one launch per
 * group size that occurs; the inverses stay on the device, column-major inside
 * a block, blocks back to back). info[0] = the smallest block with a zero or
 * non-finite pivot (-1: none; such a block is KRY_ESINGULAR and nothing is
 * created), info[1] = the largest block, info[2] = the factor kernels' time in
 * microseconds (HIP events).
 * kry_bjacobi_info: info[0..5] = blocks, smallest block, largest block, bytes
 * of the inverses, bytes of the row-to-block map and block tables, the factor
 * kernels' microseconds.
 * kry_bjacobi_get: the inverses copied to the host (sum of b_i^2 values of
 * `dtype`), row-major inside a block, blocks concatenated.
 * kry_bjacobi_apply: y = M x.
 * kry_precond_add_bjacobi: the object as the single stage of a kry_precond
 * (borrowed like the other stages; any other stage beside it is KRY_EINVAL),
 * which then goes where the other factorised preconditioners go
 * (kry_precond_apply, kry_prog_precond, kry_*_set_precond), counts one launch
 * in kry_precond_info and takes up to 256 columns; kry_precond_fuse leaves it
 * as it is. */
int kry_bjacobi_plan(int64_t n, int64_t nblocks, const int32_t *starts, int64_t *info, int32_t *tasks,
                     int32_t *blocklist);
int kry_bjacobi_create(kry_ctx *ctx, int64_t n, int64_t nnz, const void *indptr, const void *indices, const void *data,
                       int dtype, int itype, int64_t nblocks, const int32_t *starts, int64_t *info,
                       kry_bjacobi **out);
int kry_bjacobi_destroy(kry_bjacobi *B);
int kry_bjacobi_info(const kry_bjacobi *B, int64_t *info);
int kry_bjacobi_get(const kry_bjacobi *B, void *host);
int kry_bjacobi_apply(kry_ctx *ctx, const kry_bjacobi *B, const kry_vec *x, kry_vec *y);
int kry_precond_add_bjacobi(kry_precond *P, const kry_bjacobi *B);

/* Batched LAPACK >= 3.10 ?lartg on device (givens.py:35-40); host arrays of
 * `count` values of `dtype`. Bitwise equal to scipy.linalg.lapack ?lartg. */
int kry_lartg(kry_ctx *ctx, int64_t count, int dtype, const void *f, const void *g,
              void *c, void *s, void *r);

/* ---- CG (cg.py:16-259) ----------------------------------------------------
 * set_preconditioners: M and Ml as device operators (NULL = identity), before
 *        start; the loop then applies Ml (A p) (Product(Ml, A), cg.py:110) and
 *        z = M Ml_r with rho = <Ml_r, z> (cg.py:205-209).
 * start: r0 = Ml (b - A x0), rho0 = <r0, M r0>_w; rho0 (k values) returned.
 * run:   executes up to max_steps iterations of cg.py:175-217 on device; stops
 *        early after the first iteration whose residual norms all satisfy
 *        resnorm <= criterion (the test at cg.py:156). Writes the new residual
 *        norms (steps_done x k) to resnorms.
 * residual: explicit ||M Ml (b - A xk)||_{M^-1} with xk = x0 + yk (cg.py:158-160).
 * get:   download xk (which = 0), the updated residual Ml_r (which = 1) or
 *        M Ml_r (which = 2).
 * scalars: the current [rho, rho_prev, alpha, omega] (4 x k values) of the
 *        recurrence, for the Lanczos relation of return_arnoldi
 *        (cg.py:218-233). */
int kry_cg_create(kry_ctx *ctx, kry_csr *A, int32_t k, int dtype, kry_cg **out);
int kry_cg_destroy(kry_cg *s);
int kry_cg_set_preconditioners(kry_cg *s, kry_csr *M, kry_csr *Ml);
int kry_cg_start(kry_cg *s, kry_vec *b, kry_vec *x0, kry_vec *w, double *rho0);
int kry_cg_set_criterion(kry_cg *s, const double *criterion);
int kry_cg_run(kry_cg *s, int32_t max_steps, int32_t *steps_done, double *resnorms);
/* Iterations per kry_cg_run call this solve is best driven with (after
 * kry_cg_start): 256 when it runs the persistent small-n loop (one launch per
 * call, nothing launched past convergence), 32 otherwise. The driver-side
 * chunking of the reference's loop (cg.py:155-234) is free to use any value. */
int kry_cg_preferred_chunk(kry_cg *s, int32_t *steps);
/* Which path the last kry_cg_run chunk took (host-side bookkeeping, no
 * device work): info[0] = 1 if it ran as the persistent small-n loop (one
 * launch per chunk), 0 if launch per pass; info[1] = chunks that
 * were rerun launch per pass after an in-launch exchange timed out (a block
 * that never became resident). The rerun starts from the chunk-start state,
 * which the persistent loop never overwrites, so the history is that of an
 * uninterrupted solve. Fault injection for tests: KRY_CGP_FAULT=t makes the
 * last block drop out at iteration t of a chunk. */
int kry_cg_path(kry_cg *s, int32_t *info);
/* The same for the one-launch update of the launch-per-pass form (large n,
 * one RHS, no M / Ml, Euclidean inner: alpha, r, rho, omega, y and p of an
 * iteration in one launch after the SpMV): info[0] = 1 if the last
 * kry_cg_run chunk used it; info[1] = chunks whose remaining steps were rerun
 * with separate passes after its exchange timed out (it writes nothing
 * before the exchange completes). KRY_CG_UPD=0 disables it; KRY_CGU_FAULT=t
 * makes the last block drop out at step t of a chunk (tests). */
int kry_cg_update_path(kry_cg *s, int32_t *info);
/* Deferred yk updates (yk += alpha p, cg.py:196, applied D steps at a time;
 * bitwise the per-step updates): *D = the steps per flush this solver uses
 * (0 = one update per step; decided at the first kry_cg_run), *bytes = the
 * device memory its D ring buffers of p and the alpha ring hold until
 * kry_cg_destroy. Default, when an n x k vector exceeds 128 MB: the
 * deepest D of 31, 15, 7, 3 whose ring fits an eighth of the device's total
 * memory, else 0; KRY_CG_YDEFER = D (1..31) overrides; an allocation failure
 * falls back to D = 0. */
int kry_cg_defer_info(kry_cg *s, int32_t *D, int64_t *bytes);
int kry_cg_residual(kry_cg *s, double *resnorm);
int kry_cg_get(kry_cg *s, int which, void *host);
int kry_cg_scalars(kry_cg *s, double *out);

/* ---- GMRES (gmres.py:41-251, ArnoldiMGS arnoldi.py:107-200) --------------
 * set_preconditioners: M, Ml, Mr as device operators (NULL = identity); the
 *         Arnoldi operator is Ml A Mr, M gives the second basis P (V = M P),
 *         and xk = x0 + Mr (sum_i yy_i V_i) (gmres.py:97-99, 139).
 * create: workspace for up to `maxiter` Arnoldi steps with `sweeps` MGS
 *         passes per step ("mgs" = 1, "mgsK" = K), or sweeps = 0 for
 *         Householder Arnoldi (ortho="householder", arnoldi.py:33-104; k = 1,
 *         default inner, no M).
 * start:  r0 = b - A x0, ||r0||, V0 = r0 / ||r0|| (guarded), y[0] = ||r0||.
 * run:    up to max_steps Arnoldi + Givens steps; stops early after a step
 *         whose |y[k+1]| all satisfy the criterion or that found the space
 *         invariant (*invariant = 1). Returns KRY_EINVARIANT if called after
 *         an invariant step (arnoldi.py:168-171).
 * solution: xk = x0 + sum_i yy_i V_i with yy = R^-1 y (gmres.py:89-99),
 *         left on device; residual: explicit ||b - A xk||.
 * get:    which = 0: xk (after solution); 1: the basis V_0..V_m and 2: P_0..P_m
 *         (m = steps, or steps - 1 after an invariant step; n x k each, packed);
 *         3: the Hessenberg matrix H, (maxiter + 1) x maxiter x k (ArnoldiMGS /
 *         ArnoldiHouseholder state, arnoldi.py:33-200). */
int kry_gmres_create(kry_ctx *ctx, kry_csr *A, int32_t k, int dtype, int32_t maxiter,
                     int32_t sweeps, kry_gmres **out);
int kry_gmres_destroy(kry_gmres *s);
int kry_gmres_set_preconditioners(kry_gmres *s, kry_csr *M, kry_csr *Ml, kry_csr *Mr);
int kry_gmres_start(kry_gmres *s, kry_vec *b, kry_vec *x0, kry_vec *w, double *r0norm);
int kry_gmres_set_criterion(kry_gmres *s, const double *criterion);
int kry_gmres_run(kry_gmres *s, int32_t max_steps, int32_t *steps_done,
                  double *resnorms, int32_t *invariant);
int kry_gmres_solution(kry_gmres *s);
int kry_gmres_residual(kry_gmres *s, double *resnorm);
int kry_gmres_get(kry_gmres *s, int which, void *host);
/* xk (after kry_gmres_solution) copied into a device vector of the solver's
 * shape, on the context stream: restarted GMRES(m) chains x0 = xk of the last
 * cycle (gmres.py:41-54 called again with x0) without leaving the device. */
int kry_gmres_xk_device(kry_gmres *s, kry_vec *out);
/* info[0] = 1 while Arnoldi steps run their MGS passes as one persistent
 * launch (gm_mgsp_kernel), 0 launch per pass (not eligible, or switched off
 * after a timeout); info[1] = chunks finished launch per pass after a
 * persistent MGS exchange timed out. The timed-out step is rerun from its
 * SpMV, so the history is that of an uninterrupted solve. Fault injection
 * for tests: KRY_MGS_FAULT=s makes the last block drop out at chunk step s. */
int kry_gmres_path(kry_gmres *s, int32_t *info);
/* multi_solve_triangular (gmres.py:24-38) as a standalone call: per column c
 * of k, out[:, c] = R[:, :, c]^-1 y[:, c] for upper-triangular R (m x m x k,
 * C order) and y (m x k), host float64 arrays; arithmetic in `dtype`
 * (dtrtrs / strtrs). Zero rhs -> 0; KRY_ENONFINITE, KRY_ESINGULAR as LAPACK. */
int kry_trsv_upper(kry_ctx *ctx, int32_t m, int32_t k, int dtype, const double *R, const double *y,
                   double *out);
/* Householder(x) (householder.py:6-53) for one vector (k = 1): v_out = the
 * normalised reflector vector, out3 = [beta, alpha, xnorm] (H x = alpha xnorm
 * e_1); the kernels of Householder Arnoldi, arithmetic in x's dtype. */
int kry_householder(kry_ctx *ctx, kry_vec *x, kry_vec *v_out, double *out3);

/* ---- MINRES (minres.py:28-253, ArnoldiLanczos arnoldi.py:203-281) --------
 * set_preconditioners: M, Ml, Mr as device operators (NULL = identity);
 * Lanczos on Ml A Mr with p / v = M p, xk = x0 + Mr yk (minres.py:95-98).
 * Same run protocol as CG; R, rotations, y, z and W are float64 as in the
 * reference under NumPy-2 promotion (minres.py:195,219). */
int kry_minres_create(kry_ctx *ctx, kry_csr *A, int32_t k, int dtype, kry_minres **out);
int kry_minres_destroy(kry_minres *s);
int kry_minres_set_preconditioners(kry_minres *s, kry_csr *M, kry_csr *Ml, kry_csr *Mr);
int kry_minres_start(kry_minres *s, kry_vec *b, kry_vec *x0, kry_vec *w, double *r0norm);
int kry_minres_set_criterion(kry_minres *s, const double *criterion);
int kry_minres_run(kry_minres *s, int32_t max_steps, int32_t *steps_done,
                   double *resnorms, int32_t *invariant);
/* Whether the last kry_minres_run chunk ran the one-launch step tail (alpha,
 * Lanczos orthogonalisation, QR update and the z / W / yk / p update in one
 * launch after the SpMV: one RHS, no M / Ml / Mr, float64 vectors): info[0];
 * info[1] = chunks whose remaining steps were rerun with the separate kernels
 * after its exchange timed out (it writes nothing before the exchange
 * completes). KRY_MR_UPD=0 disables it; KRY_MRU_FAULT=t drops the last block
 * out at step t of a chunk (tests). */
int kry_minres_update_path(kry_minres *s, int32_t *info);
int kry_minres_residual(kry_minres *s, double *resnorm);
/* get: which = 0: xk; 1: the current Lanczos vector p; 2: v = M p; 3: the last
 * step's [h0, h1, h2] (3 x k; ArnoldiLanczos state, arnoldi.py:203-281). */
int kry_minres_get(kry_minres *s, int which, void *host);

/* ---- multi-GPU: RHS columns sharded one block per GPU ----
 * One RCCL communicator per process/GPU. After attaching, each CG iteration
 * performs exactly one ncclAllReduce(sum, f64, count = total_k + 1) on the
 * zero-padded residual-norm vector so every rank applies the reference's
 * global stop rule np.all(resnorms[-1] <= criterion) (cg.py:156).
 * The last slot of every per-step allreduce (CG, GMRES, MINRES) is a fault
 * count: a rank whose in-launch exchange timed out at a step (a block that
 * never became resident) posts a fault there instead of its norms, so EVERY
 * rank stops the chunk before that step, after the same collectives: the
 * faulting rank's run returns KRY_EDEVICE, every other rank's KRY_ECOMM, and
 * no rank blocks in a later allreduce. KRY_COMM_PEER_FAULT=s makes step s of
 * a run call receive a fault as if a peer had posted it (tests on one GPU). */
int kry_comm_unique_id(void *id128);
int kry_comm_create(kry_ctx *ctx, int32_t nranks, int32_t rank, const void *id128,
                    kry_comm **out);
/* One communicator per context of one process (ncclCommInitAll over the
 * contexts' devices; out[i] is rank i of n), kry_version() >= 104: the
 * single-process multi-GPU path, krylov_amd.cg / gmres / minres(...,
 * devices=[...]), one host thread per device. Replaces the per-process
 * ranks of SURVEY §8(e) when the caller has one process for the node. */
int kry_comm_create_all(kry_ctx **ctxs, int32_t n, kry_comm **out);
int kry_comm_destroy(kry_comm *c);
/* Abort a communicator, from any thread, while a collective on it may be
 * pending (ncclCommAbort; kry_version() >= 105): that and every later
 * collective fail, so a solver waiting on a rank that will not come stops
 * with KRY_ECOMM. kry_comm_destroy still releases the handle. No reference
 * counterpart: the devices=[...] driver aborts every device's communicator
 * when one device's thread fails. */
int kry_comm_abort(kry_comm *c);
/* The communicator as RCCL sees it (kry_version() >= 106): *nranks from
 * ncclCommCount, *rank from ncclCommUserRank; KRY_ECOMM once aborted. */
int kry_comm_info(kry_comm *c, int32_t *nranks, int32_t *rank);
/* in-place sum over ranks of `count` host doubles (setup-time exchanges) */
int kry_comm_allreduce(kry_comm *c, double *host, int32_t count);
int kry_cg_attach_comm(kry_cg *s, kry_comm *c, int32_t col_offset, int32_t total_k);
/* GMRES / MINRES: the same sharding (gmres.py:193 and minres.py:162 stop rules,
 * arnoldi.py:187 / 270-272 invariance over all columns): one
 * ncclAllReduce(sum, f64, count = total_k + 2) per step of the zero-padded
 * residual norms, a count of ranks with a non-invariant column and the fault
 * count. After
 * attaching, set_criterion takes total_k values and each run history row
 * holds total_k values. */
int kry_gmres_attach_comm(kry_gmres *s, kry_comm *c, int32_t col_offset, int32_t total_k);
int kry_minres_attach_comm(kry_minres *s, kry_comm *c, int32_t col_offset, int32_t total_k);

/* ---- timing: HIP events on the context stream --------------------------- */
int kry_timer_start(kry_ctx *ctx);
int kry_timer_stop(kry_ctx *ctx, double *ms);
/* device time of the solvers' launches per kernel id (0 SpMV, 1 update
 * pass, 2 MGS, 3 other), measured with HIP events around the launches when
 * enabled; enable != 0 times every launch of every id, kry_profile_select
 * only the ids whose bit is set in mask and of those one launch in `every`
 * (each timed launch adds two event records to the stream: ~3 us at the
 * metric). Both reset the counts. kry_profile_read: timed launches, total ms. */
int kry_profile_enable(kry_ctx *ctx, int enable);
int kry_profile_select(kry_ctx *ctx, uint32_t mask, int32_t every);
int kry_profile_read(kry_ctx *ctx, int kernel_id, int64_t *count, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* KRYLOV_HIP_H */
