/*
 * mspmv.h -- C ABI of the MI355X-native merge-based CsrMV (libmspmv.so).
 *
 * This is the drop-in boundary for the reference's device API
 *     cub::DeviceSpmv::CsrMV(d_temp_storage, temp_storage_bytes, d_values,
 *         d_row_offsets, d_column_indices, d_vector_x, d_vector_y,
 *         num_rows, num_cols, num_nonzeros, stream, debug_synchronous)
 * (reference cub/device/device_spmv.cuh:129-164, instantiated for float and
 * double with int offsets at gpu_spmv.cu:730,734).  Plain pointers and sizes
 * only; no C++ or torch types.  A header-only C++ shim with the reference's
 * spelling lives in merge_spmv_amd/host/device_spmv.hpp.
 *
 * Conventions kept from the reference:
 *   - two-phase temp storage: d_temp == NULL -> *temp_bytes receives the size
 *     needed, no work is done, returns 0 (dispatch_spmv_orig.cuh:651-655);
 *     otherwise *temp_bytes < needed -> hipErrorInvalidValue
 *     (util_device.cuh:90-93); d_temp (and a plan's storage) must be 16-byte
 *     aligned, as every device allocation is -- it holds 64-bit records that
 *     are updated atomically -- else hipErrorInvalidValue;
 *   - the caller owns every buffer including temp; the callee allocates
 *     nothing and keeps no state between calls (what a call leaves in temp
 *     storage is scratch, except for mspmv_csrmv_prepare); the library reads
 *     nothing from the environment and has no setters -- the forcing and
 *     re-tuning aids of the tests live in libmspmv_dev.so (include/mspmv_dev.h)
 *     only; the one piece of process state is the opt-in event profiler
 *     (mspmv_profile_begin/_end), which never changes what a call launches;
 *   - all array pointers are DEVICE pointers; d_row_offsets has rows+1 entries
 *     ([0]=0, [rows]=nnz, non-decreasing), 0-based int32 column indices,
 *     duplicates allowed (sparse_matrix.h:645-650,666-728); d_x holds cols
 *     readable entries (a tiny x -- cols * sizeof(value) <= 4 KB -- is copied
 *     to LDS whole, whether or not every column is referenced);
 *   - y is fully overwritten: y = A*x (alpha=1, beta=0 as
 *     device_spmv.cuh:155-156 forces); rows without entries get exactly 0;
 *   - asynchronous on `stream` unless debug_sync != 0 (then every kernel is
 *     followed by a stream sync and a launch-config line on stdout, like
 *     dispatch_spmv_orig.cuh:685-739);
 *   - return value: 0 (hipSuccess) or the first hipError_t as int.
 * Deliberate differences (the reference's out-of-bounds habits, SURVEY.md
 * Appendix B, are NOT inherited): nothing outside [0,rows] of d_row_offsets,
 * [0,nnz) of values/columns, [0,cols) of x or [0,rows) of y is touched.
 * Requires rows >= 0, cols >= 0, nnz >= 0 and rows + nnz <= 2^31 - 65537 (int32 path
 * arithmetic with one tile of slack).
 */
#ifndef MSPMV_H_
#define MSPMV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t passed as an opaque pointer so that C/ctypes/cgo callers need
 * no HIP headers (NULL = the default stream). */
typedef void *mspmv_stream_t;

#define MSPMV_VERSION 102 /* (the incomplete LU factorisation mspmv_csrilu0_*, the accessors of the band-major plan's stacked matrix, mspmv_csrmv_plan_row_offsets / _columns / _values, the matrix addition mspmv_csr_add_*, the transpose entry points mspmv_csr_transpose_* / mspmv_csrmv_transpose_* and the COO ones, mspmv_coo_to_csr_* / mspmv_csr_sum_duplicates_* / mspmv_coomv_*, and the mixed-precision ones, mspmv_csrmv_mixed_* / mspmv_csrmv_mixed_prepared_*, came without a bump: find them by symbol); 0.1.2: + mspmv_get_clocked_bands (the clock-scheduled column bands serve the column-band candidates); 0.1.1: mspmv_launch_info_t grew (records_offset, layout_offset), the setters moved to mspmv_dev.h */
int mspmv_version(void);

/* hipGetErrorString for codes returned by this library. */
const char *mspmv_error_string(int status);

/* ---- the drop-in pair: replaces cub::DeviceSpmv::CsrMV<float|double> ---- */
int mspmv_csrmv_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                    const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const float *d_x, float *d_y, int32_t rows, int32_t cols,
                    int32_t nnz, mspmv_stream_t stream, int debug_sync);

int mspmv_csrmv_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                    const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const double *d_x, double *d_y, int32_t rows, int32_t cols,
                    int32_t nnz, mspmv_stream_t stream, int debug_sync);

/* ---- extension: y = alpha*A*x + beta*y.  The reference
 * parses --alpha/--beta (gpu_spmv.cu:721-722) and carries them in SpmvParams
 * (agent_spmv_orig.cuh:109-110) but its CsrMV forces 1/0.  With beta == 0 the
 * old contents of y are ignored (never read), as in BLAS.
 *
 * The definition (every kernel form and dispatch path; tests/test_axpby_exact.py pins it on the bits):
 *   * a row that lies within one tile is written once, as
 *         y[r] = alpha * s + (beta == 0 ? 0 : beta * y[r]),      s = the sum of the row's products, +0.0 for a row without entries;
 *     the multiply and the add may be fused;
 *   * of a row that spans tiles, the tile in which it ENDS writes that formula with s = the sum of the products it holds of the
 *     row, and every other tile's share -- its carry -- arrives as  y[r] = y[r] + alpha * carry  (fix-up kernels), or is added
 *     into s before the formula is applied (the one-launch kernel).  alpha meets every product exactly once and beta * y[r]
 *     enters exactly once; a column-band pass after the first adds its share with beta = 1;
 *   * THE SIGN OF A ZERO.  A row's sum s, and every partial sum that becomes a carry, STARTS FROM +0.0 (the reference's sequential
 *     definition: partial = 0.0; partial += v * x).  A sum of IEEE numbers that starts from +0.0 is never -0.0, so s and every
 *     carry are never -0.0, whatever the products are -- stored zeros and zeros in x of either sign are ordinary inputs.  With
 *     t = (beta == 0 ? +0.0 : beta * y[r]) the row is y[r] = alpha * s_end + t, and every carry c arrives as y[r] + alpha * c or is
 *     added into s first.  Hence, where every intermediate is exactly representable:
 *       - with beta == 0, or whenever t is not -0.0, a zero result is +0.0 -- for mspmv_csrmv_* too, WHATEVER THE SIGN OF alpha,
 *         the path, the tile shape, the band form or the order of the carries: alpha * 0 alone would be -0.0 for alpha < 0, and the
 *         "+ 0" of the formula is what turns it into +0.0;
 *       - where t is -0.0 and every product of the row is zero (or the row has no entries), the result is alpha * (+0.0) + (-0.0):
 *         -0.0 if alpha is negative, +0.0 otherwise;
 *       - where t is -0.0 and the row has non-zero products that cancel to zero, the sign depends on where tiles cut the row
 *         ((+x) + (-x) is +0.0, but alpha * c of a zero carry is -0.0 for alpha < 0): that one corner is UNDEFINED.
 * (alpha, beta) = (1, 0) gives the bits of mspmv_csrmv_*.  Where every intermediate is exactly representable -- subnormal products,
 * sums and carries included: nothing is flushed to zero -- the result does not depend on the path, the tile shape or the order of
 * the carries (the atomic fix-up included).  mspmv_csrmm_*, the mixed calls, the prepared calls, the plans (mspmv_csrmv_plan_*,
 * mspmv_csrmv_hotcols_*), the transposed call and mspmv_coomv_* follow this definition; tests/test_axpby_exact.py,
 * test_spmm_forms.py, test_plan_exact.py and test_mixed_precision.py pin it on the bits. ---- */
int mspmv_csrmv_axpby_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                          const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const float *d_x, float *d_y, int32_t rows, int32_t cols,
                          int32_t nnz, float alpha, float beta,
                          mspmv_stream_t stream, int debug_sync);

int mspmv_csrmv_axpby_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                          const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          const double *d_x, double *d_y, int32_t rows, int32_t cols,
                          int32_t nnz, double alpha, double beta,
                          mspmv_stream_t stream, int debug_sync);

/* ---- extension: SpMM, Y = alpha*A*X + beta*Y for k right-hand sides.
 * X is cols x k and Y is rows x k, both ROW-major with leading dimensions ldx, ldy >= k (elements):
 * the k entries X[col, :] that one column index needs are contiguous, so one gather serves a pack
 * of right-hand sides -- up to 16 bytes of them on the CsrMV-sized tiles, and 32 or 64 bytes (a whole
 * row of X) on smaller tiles when X is larger than 1 MiB, i.e. when its gathers miss the caches;
 * wider blocks run as several groups of the widest pack inside one pass over the matrix.  Matrices of 8 M path items and more
 * (X below 4 GB) take groups of 8 / 16 right-hand sides through the slot form instead (mspmv_spmm.hpp: spmm_lane_kernel -- every
 * nonzero share of a tile walked by four or eight lanes holding 16 bytes of right-hand sides each, rows written from registers);
 * ONE right-hand side stored as a plain vector (k = ldx = ldy = 1) is the CsrMV call.  Same two-phase temp storage, ownership, stream and error
 * conventions as mspmv_csrmv_*; with beta == 0 the old Y is never read.  Results per column are
 * within the same tolerance as CsrMV and bitwise reproducible.  THE SIGN OF A ZERO is that of mspmv_csrmv_axpby_* in every kernel
 * form (row-wise, packs, slot form, fix-up): sums and carries start from +0.0 and Y = alpha * s + (beta == 0 ? +0.0 : beta * Y), so
 * with beta == 0, or wherever beta * Y is not -0.0, a row without entries and a row whose products are zeros or cancel give +0.0,
 * for a negative alpha too; the same corner is undefined (beta * Y = -0.0 over non-zero products that cancel).  No reference counterpart (the
 * reference ships CsrMV only). ---- */
int mspmv_csrmm_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                    const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const float *d_x, int32_t ldx, float *d_y, int32_t ldy,
                    int32_t rows, int32_t cols, int32_t nnz, int32_t k,
                    float alpha, float beta, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmm_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                    const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const double *d_x, int32_t ldx, double *d_y, int32_t ldy,
                    int32_t rows, int32_t cols, int32_t nnz, int32_t k,
                    double alpha, double beta, mspmv_stream_t stream, int debug_sync);

/* ---- extension for iterated SpMV (solvers): the tile coordinates -- the output of the
 * reference's DeviceSpmvSearchKernel, dispatch_spmv_orig.cuh:104-143 -- depend on d_row_offsets
 * alone, yet the reference's stateless CsrMV recomputes them on every call (8-22 us here, 5-15 % of
 * a mid-size SpMV).  mspmv_csrmv_prepare runs that pass once into the caller's temp storage
 * (same two-phase size query; the size equals mspmv_csrmv_*'s for the same rows/nnz/value_bytes).  The default
 * one-launch kernel treats the coordinates it finds in temp storage as hints and verifies them, so a stateless
 * call that follows another on the same temp storage and matrix already runs without a search; preparing makes
 * the FIRST call as fast as the later ones, and it is what the classic pipeline (column-band candidates, arrays that
 * are not 16-byte aligned) skips its coordinate launch on;
 * mspmv_csrmv_prepared_* then compute y = alpha*A*x + beta*y with the coordinates found there.
 * The caller guarantees that d_temp was prepared for this d_row_offsets / rows / nnz / value_bytes
 * and has since been used only by mspmv calls for the same matrix: they leave the prepared coordinates
 * intact (the one family of calls that picks another tile shape by its column count -- mspmv_get_launch_info_cols --
 * keeps that shape's hints in a region of its own behind the default layout, and only in the one-launch form, whose
 * hints are verified).  mspmv_csrmv_prepared_* pick their shape by the same rule as the stateless calls, so results
 * are bitwise those of mspmv_csrmv_* / mspmv_csrmv_axpby_* given the same temp_bytes. ---- */
int mspmv_csrmv_prepare(void *d_temp, size_t *temp_bytes, const int32_t *d_row_offsets,
                        int32_t rows, int32_t nnz, int32_t value_bytes,
                        mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_prepared_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                             const int32_t *d_row_offsets, const int32_t *d_column_indices,
                             const float *d_x, float *d_y, int32_t rows, int32_t cols,
                             int32_t nnz, float alpha, float beta,
                             mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_prepared_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                             const int32_t *d_row_offsets, const int32_t *d_column_indices,
                             const double *d_x, double *d_y, int32_t rows, int32_t cols,
                             int32_t nnz, double alpha, double beta,
                             mspmv_stream_t stream, int debug_sync);

/* ---- extension: MIXED PRECISION -- the matrix values stored narrow, everything else wide (what the generic SpMV of rocSPARSE /
 * cuSPARSE offers; mixed-precision Krylov solvers and iterative refinement keep A narrow and the vectors wide).  Two pairs,
 * written (stored type of d_values -> compute type; x, y, alpha, beta, every product and every sum are in the compute type):
 *     f32  -> f64     const float *d_values,    const double *d_x, double *d_y
 *     bf16 -> f32     const uint16_t *d_values (the upper 16 bits of an IEEE fp32), const float *d_x, float *d_y
 *     y = alpha * A * x + beta * y        (beta == 0: y is never read; alpha = 1, beta = 0 is the plain product)
 * A stream-bound CsrMV costs the bytes of the CSR stream, and two thirds of an fp64 stream are the values: the call reads 8 bytes
 * per nonzero instead of 12 (6 instead of 8 for bf16 -> f32) and needs no widened copy of the matrix.  Every value is widened in
 * registers right before its multiply; widening is exact (every fp32 is an fp64, every bf16 an fp32), so the call computes the
 * product of the WIDENED matrix.  Conventions of mspmv_csrmv_axpby_*: two-phase temp storage (16-byte aligned), caller-owned
 * buffers, no state, rows without entries get exactly 0, nothing outside the arrays is touched, rows + nnz <= 2^31 - 65537,
 * asynchronous on `stream`, debug_sync prints the launch lines.  The 16-byte-per-lane streams need d_row_offsets and
 * d_column_indices 16-byte aligned and d_values aligned to four of its elements (16 bytes for f32, 8 for bf16; any array length,
 * a bf16 array of odd length included); other arrays run the dword-per-lane kernel, as in the wide calls.
 * WHAT IT EQUALS.  Every decision that shapes the association of the sums -- the tile shape, one launch or the classic three,
 * the rule for matrices of long rows -- is taken exactly as mspmv_csrmv_axpby_f64 / _f32 (the wide call of the COMPUTE type)
 * takes it, with value_bytes = sizeof(compute type) (and that precision's mspmv_set_tuning in the development library); only what
 * counts bytes moved sees the stored size (non-temporal loads from a 256 MB stream up).  The mixed call takes none of the
 * special forms: not the compact front end of small problems (bit for bit the same y as the general kernel anyway), not the
 * small-shape layout of large fp64 matrices of short rows over a tiny x (mspmv_get_launch_info_cols), and it is never a
 * column-band CANDIDATE (the rule of the hot-column plan's inner call, below).  Hence:
 *   * the size query (d_temp == NULL) answers mspmv_get_launch_info(rows, nnz, sizeof(compute type)).temp_bytes -- one buffer
 *     serves the mixed and the wide call --, and mspmv_csrmv_prepare(..., value_bytes = sizeof(compute type)) prepares the
 *     coordinates for mspmv_csrmv_mixed_prepared_* (same guarantees as mspmv_csrmv_prepared_*);
 *   * y is BIT FOR BIT what mspmv_csrmv_axpby_f64 / _f32 (prepared: mspmv_csrmv_prepared_*) returns for the widened values on
 *     arrays aligned alike, unless the sizes make the wide call a column-band candidate (mspmv_get_band_passes(rows, cols, nnz,
 *     sizeof(compute type)) > 1) or let it take the small-shape layout (mspmv_get_launch_info_cols reports another
 *     items_per_thread than mspmv_get_launch_info, and the wide call is given room for it);
 *   * for column-band candidates y equals the wide call's ONE-LAUNCH form (dev library: mspmv_set_band_passes(vb, -1)), the
 *     comparison prescribed for the hot-column plan; where the wide call takes the small-shape layout, rows that lie inside
 *     one tile are still bit for bit equal and a longer row is associated as the tiles of the shape that ran cut it.
 * fp16 is not offered (one more widening function and set of kernels if somebody asks).  No reference counterpart. ---- */
int mspmv_csrmv_mixed_f32_f64(void *d_temp, size_t *temp_bytes, const float *d_values,
                              const int32_t *d_row_offsets, const int32_t *d_column_indices,
                              const double *d_x, double *d_y, int32_t rows, int32_t cols,
                              int32_t nnz, double alpha, double beta,
                              mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_mixed_bf16_f32(void *d_temp, size_t *temp_bytes, const uint16_t *d_values,
                               const int32_t *d_row_offsets, const int32_t *d_column_indices,
                               const float *d_x, float *d_y, int32_t rows, int32_t cols,
                               int32_t nnz, float alpha, float beta,
                               mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_mixed_prepared_f32_f64(void *d_temp, size_t *temp_bytes, const float *d_values,
                                       const int32_t *d_row_offsets, const int32_t *d_column_indices,
                                       const double *d_x, double *d_y, int32_t rows, int32_t cols,
                                       int32_t nnz, double alpha, double beta,
                                       mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_mixed_prepared_bf16_f32(void *d_temp, size_t *temp_bytes, const uint16_t *d_values,
                                        const int32_t *d_row_offsets, const int32_t *d_column_indices,
                                        const float *d_x, float *d_y, int32_t rows, int32_t cols,
                                        int32_t nnz, float alpha, float beta,
                                        mspmv_stream_t stream, int debug_sync);

/* ---- extension: PREPARED PLAN for a gather-bound matrix multiplied many times (opt-in; the stateless
 * drop-in calls above never use it).  When x is larger than an XCD's 4 MiB L2, ~70 % of the x gathers miss
 * and every miss moves a 128-byte line: that, not HBM, bounds mspmv_csrmv_* on such a matrix (BASELINE
 * config 2).  mspmv_csrmv_plan_build_* makes, ONCE, a band-major copy of the matrix in the caller's
 * storage: the columns are cut into `bands` equal bands (0 = pick: the fewest of 2, 4, 8, 16, ... with <= 3.25 MiB
 * of x per band; 1 when x fits anyway) and the entries of band b form the b-th block of rows of a stacked CSR
 * matrix; mspmv_csrmv_plan_apply_* then runs the ordinary merge-path CsrMV over the stacked matrix with
 * one contiguous tile range per XCD -- so each XCD's L2 only ever holds one band's slice of x and the CSR
 * stream is read exactly once -- and folds the bands' partial sums in band order:
 *     y = alpha * A * x + beta * y        (beta == 0: y is never read).
 * Conventions: caller-owned storage of mspmv_csrmv_plan_size bytes (device memory; the same rows / cols /
 * nnz / bands must be passed to _size, _build and _apply); nothing is allocated; asynchronous on `stream`;
 * the original arrays are not needed after _build.  Results are within the CsrMV tolerance and bitwise
 * reproducible for a given plan.  Needs bands * rows + nnz <= 2^31 - 65537 (hipErrorInvalidValue otherwise:
 * use the stateless call).  This is the counterpart of what the reference's driver does for its HYB
 * comparison -- conversion timed once as set-up, SpMV timed separately (gpu_spmv.cu:106-257). ---- */
int mspmv_csrmv_plan_size(int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t bands,
                          size_t *plan_bytes, int32_t *bands_used);
int mspmv_csrmv_plan_build_f32(void *d_plan, size_t plan_bytes, const float *d_values,
                               const int32_t *d_row_offsets, const int32_t *d_column_indices,
                               int32_t rows, int32_t cols, int32_t nnz, int32_t bands,
                               mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_plan_build_f64(void *d_plan, size_t plan_bytes, const double *d_values,
                               const int32_t *d_row_offsets, const int32_t *d_column_indices,
                               int32_t rows, int32_t cols, int32_t nnz, int32_t bands,
                               mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_plan_apply_f32(void *d_plan, size_t plan_bytes, const float *d_x, float *d_y,
                               int32_t rows, int32_t cols, int32_t nnz, int32_t bands,
                               float alpha, float beta, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_plan_apply_f64(void *d_plan, size_t plan_bytes, const double *d_x, double *d_y,
                               int32_t rows, int32_t cols, int32_t nnz, int32_t bands,
                               double alpha, double beta, mspmv_stream_t stream, int debug_sync);
/* The plan's pieces, for callers that want the stacked matrix itself and for the tests: A' = [A_0; A_1; ...; A_{bands-1}] as an
 * ordinary CSR matrix of bands * rows rows -- its bands * rows + 1 row offsets, its nnz column indices (absolute, as in A) and its
 * nnz values of value_bytes each.  band_width = max(1, ceil(cols / bands)); entry j of row r of A lies in stacked row
 * (column / band_width) * rows + r; inside a stacked row the entries keep the order they have in A when every row of A has its
 * columns in non-decreasing order (rows in another order: some order, the same entries).  Device pointers into d_plan, valid after
 * _build has completed on its stream; `bands` is the count passed to _build (0 = the automatic one); NULL for a NULL plan or sizes
 * mspmv_csrmv_plan_size refuses.  Nothing is launched, nothing is read from the device. */
const int32_t *mspmv_csrmv_plan_row_offsets(const void *d_plan, int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t bands);
const int32_t *mspmv_csrmv_plan_columns(const void *d_plan, int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t bands);
const void *mspmv_csrmv_plan_values(const void *d_plan, int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t bands);

/* ---- extension: HOT-COLUMN PLAN for a matrix whose x is far larger than the caches and whose columns are referenced
 * very unevenly (scale-free graphs: BASELINE config 5; opt-in, the stateless calls never use it).  Such a CsrMV runs at
 * the DRAM random-line rate -- 57 G gathers/s on MI355X, 0.09 of the HBM roofline -- because the few hot columns that
 * take most of the references are scattered over all of x, each sharing its cache line with cold ones.
 * mspmv_csrmv_hotcols_build renumbers the columns ONCE in order of reference count (by class: floor(log2(count + 1)),
 * hottest first -- a histogram and one ranking pass, no sort) into the caller's storage: the renumbered column indices
 * (4 * nnz bytes; values and row offsets are used from the caller's arrays, not copied), the permutation, x in the new
 * numbering and the inner call's temp storage.  mspmv_csrmv_hotcols_apply_* then permutes x (one pass over cols entries)
 * and runs the ordinary stateless CsrMV on the renumbered indices:
 *     y = alpha * A * x + beta * y        (beta == 0: y is never read).
 * A column permutation only changes where x is read -- every row still sums the same products in the same order -- so y
 * is BIT FOR BIT the result of mspmv_csrmv_* / _axpby_* in its ONE-LAUNCH form.  The plan's inner call is never a CANDIDATE for
 * the column-band passes; a stateless call whose sizes make it one (mspmv_get_band_passes > 1: x of 5.5-40 MiB, >= 8 nonzeros
 * per row, a CSR stream >= 160 MiB) runs the classic three launches -- one carry per tile and a fix-up, another association of
 * the sums of rows that cross tiles -- whether or not the device-side windows then let the passes run, so compare with
 * the one-launch form there (dev library: mspmv_set_band_passes(vb, -1)).  Config 5 on one GPU: 34.2 -> 20.6 ms.  Same conventions as
 * the band-major plan below (caller-owned storage of mspmv_csrmv_hotcols_size bytes, the same rows / cols / nnz /
 * value_bytes to every call, asynchronous on `stream`); d_values / d_row_offsets passed to _apply must be the arrays
 * the plan was built for.  No reference counterpart (its HYB column is the precedent for set-up timed apart,
 * gpu_spmv.cu:106-257). ---- */
/* Would the plan pay?  A cheap look at the column indices (synchronous: a bitmap of one bit per 128-byte line of x, one small kernel,
 * a 12-byte copy): 512 windows of 2048 consecutive nonzeros spread over the matrix (~1 M references); *distinct_permille_of_uniform =
 * 1000 x the number of DISTINCT lines of x the sample touches / what as many uniformly drawn references would touch (-1: fewer than
 * 2048 nonzeros), *wide_windows = how many of the 512 windows span >= 3/4 of the columns.  Uniformly spread columns give ~1000
 * (nothing to concentrate), stencils and bands < 100 (their gathers hit the caches as they are), scale-free matrices 400-700: lines
 * that keep coming back -- the case the plan is for.  mspmv_mg_plan_* builds the plan by itself when x is beyond the Infinity Cache
 * and 150 <= the figure < 800 with >= 256 wide windows (mspmv_mg_plan_hot_columns).  Measured (profiles/r05_skew_probe.txt):
 * uniform columns 1000 / 512 wide, a band 48 / 0, a 5-point grid 206 / 0, R-MAT scale 22-26 289-374 / 370-450 (config 5: 351 / 372),
 * a circuit-shaped matrix 634 / 492, a small R-MAT (scale 18: every line of its 2 MB x referenced) 842 / 456. */
int mspmv_csrmv_hotcols_skew(const int32_t *d_column_indices, int32_t cols, int32_t nnz, int32_t value_bytes, mspmv_stream_t stream,
                             int32_t *distinct_permille_of_uniform, int32_t *wide_windows);
int mspmv_csrmv_hotcols_size(int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, size_t *plan_bytes);
int mspmv_csrmv_hotcols_build(void *d_plan, size_t plan_bytes, const int32_t *d_row_offsets,
                              const int32_t *d_column_indices, int32_t rows, int32_t cols, int32_t nnz,
                              int32_t value_bytes, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_hotcols_apply_f32(void *d_plan, size_t plan_bytes, const float *d_values,
                                  const int32_t *d_row_offsets, const float *d_x, float *d_y,
                                  int32_t rows, int32_t cols, int32_t nnz, float alpha, float beta,
                                  mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_hotcols_apply_f64(void *d_plan, size_t plan_bytes, const double *d_values,
                                  const int32_t *d_row_offsets, const double *d_x, double *d_y,
                                  int32_t rows, int32_t cols, int32_t nnz, double alpha, double beta,
                                  mspmv_stream_t stream, int debug_sync);
/* A caller that keeps x in the plan's numbering -- a fixed right-hand side, or a method whose vector updates are element-wise and can
 * live in that numbering -- pays the permutation once instead of per SpMV (config 5 on one GPU: 0.7 of 21 ms):
 * mspmv_csrmv_hotcols_permute_* writes d_x_permuted[k] = d_x[order[k]] (cols entries; not in place), and
 * mspmv_csrmv_hotcols_apply_permuted_* is mspmv_csrmv_hotcols_apply_* on such a vector, without the pass.  y comes out in the ORIGINAL
 * row order, bit for bit what _apply_* returns for the unpermuted x. */
int mspmv_csrmv_hotcols_permute_f32(const void *d_plan, size_t plan_bytes, const float *d_x, float *d_x_permuted,
                                    int32_t rows, int32_t cols, int32_t nnz, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_hotcols_permute_f64(const void *d_plan, size_t plan_bytes, const double *d_x, double *d_x_permuted,
                                    int32_t rows, int32_t cols, int32_t nnz, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_hotcols_apply_permuted_f32(void *d_plan, size_t plan_bytes, const float *d_values,
                                           const int32_t *d_row_offsets, const float *d_x_permuted, float *d_y,
                                           int32_t rows, int32_t cols, int32_t nnz, float alpha, float beta,
                                           mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_hotcols_apply_permuted_f64(void *d_plan, size_t plan_bytes, const double *d_values,
                                           const int32_t *d_row_offsets, const double *d_x_permuted, double *d_y,
                                           int32_t rows, int32_t cols, int32_t nnz, double alpha, double beta,
                                           mspmv_stream_t stream, int debug_sync);
/* the plan's pieces (device pointers into d_plan): order[k] = the original column that became column k (cols entries),
 * and the renumbered column indices (nnz entries) */
const int32_t *mspmv_csrmv_hotcols_order(const void *d_plan, int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes);
const int32_t *mspmv_csrmv_hotcols_columns(const void *d_plan, int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes);

/* ---- extension: the TRANSPOSE.  A^T as CSR (= A as CSC), built on the device by a stable least-significant-digit radix sort
 * of the nonzeros by column (csrc/mspmv_transpose.hip: 8 bits per pass, max(1, ceil(bits(cols - 1) / 8)) passes of upsweep ->
 * scan -> downsweep, the (row, value, position) payload carried through every pass; no workgroup waits on another).  Outputs:
 * row_offsets_t[cols + 1], column_indices_t[nnz] (the original row of each entry), values_t[nnz], and optionally
 * permutation[nnz] with values_t[j] = values[permutation[j]].  STABLE: the entries of each row of A^T appear in their order in A
 * (ascending original row; entries that share a column inside one row -- duplicates or unsorted rows -- in their original
 * order), so the result is canonical and bit for bit what a stable transpose on the host gives.  d_values == NULL and
 * d_values_t == NULL: structure (+ permutation) only, for either precision.  Same two-phase temp storage, 16-byte alignment,
 * ownership, stream, debug_sync and error conventions as mspmv_csrmv_*; column indices are assumed to lie in [0, cols) as for
 * the forward call; empty rows and empty columns, rows == 0, cols == 0 and nnz == 0 are accepted.  Temp storage: about
 * 2 x nnz x (12 + value bytes) + 4 x nnz bytes when cols > 65536 (fewer for fewer passes; C2 fp32 3.7 GB).  Any forward entry point
 * (prepared coordinates, the plans, SpMM, the multi-GPU operator) then applies to A^T as to any CSR matrix.
 * Measured on MI355X (profiles/transpose_bench.txt): C2 (100 M nonzeros) 6.4 ms fp32 / 7.0 ms fp64 against rocsparse_csr2csc's
 * 6.7 / 6.9 ms; A^T x through the built transpose then runs as the forward call does (C2 fp32 0.68 ms, A x 0.71 ms). ---- */
int mspmv_csr_transpose_f32(void *d_temp, size_t *temp_bytes,
                            const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                            int32_t rows, int32_t cols, int32_t nnz,
                            float *d_values_t, int32_t *d_row_offsets_t, int32_t *d_column_indices_t,
                            int32_t *d_permutation /* may be NULL */, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_transpose_f64(void *d_temp, size_t *temp_bytes,
                            const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                            int32_t rows, int32_t cols, int32_t nnz,
                            double *d_values_t, int32_t *d_row_offsets_t, int32_t *d_column_indices_t,
                            int32_t *d_permutation /* may be NULL */, mspmv_stream_t stream, int debug_sync);
/* New values on the same pattern (Newton steps, training): values_t[j] = values[permutation[j]]. */
int mspmv_csr_transpose_values_f32(const float *d_values, const int32_t *d_permutation, float *d_values_t,
                                   int32_t nnz, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_transpose_values_f64(const double *d_values, const int32_t *d_permutation, double *d_values_t,
                                   int32_t nnz, mspmv_stream_t stream, int debug_sync);
/* Stateless y = alpha*A^T*x + beta*y: x has `rows` entries, y has `cols`; beta == 0 never reads y.  Transposes into temp storage,
 * then runs the ordinary CsrMV on the result: bitwise equal to mspmv_csr_transpose_* followed by mspmv_csrmv_axpby_* on its outputs
 * with that call's queried temp size.  Needs cols + nnz <= 2^31 - 65537 (A^T's rows + nnz; the same int32 path bound as the forward
 * call).  COST: every call pays the whole conversion, which is several times the SpMV itself; a caller that multiplies by A^T more
 * than once builds A^T once (mspmv_csr_transpose_*) and calls the forward entry points on it, which run as fast as on any matrix of
 * that shape.  Reproducibility has that price against a scatter-add transposed SpMV (rocSPARSE's csrmv with the transpose
 * operation), which is faster on large, evenly spread matrices but adds in arrival order.  Measured (DESIGN.md 4 "Transpose"): C2
 * fp32 6.9 ms stateless against 0.68 ms through a built A^T and rocSPARSE's 4.8 ms; grid2d 2000 fp64 1.27 ms against 0.041 / 0.126 ms;
 * on skewed matrices, where the scatter serialises on hot columns, the stateless call is the faster one (C3 stand-in 0.25 against
 * 3.6 ms). */
int mspmv_csrmv_transpose_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                              const int32_t *d_row_offsets, const int32_t *d_column_indices,
                              const float *d_x, float *d_y, int32_t rows, int32_t cols, int32_t nnz,
                              float alpha, float beta, mspmv_stream_t stream, int debug_sync);
int mspmv_csrmv_transpose_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                              const int32_t *d_row_offsets, const int32_t *d_column_indices,
                              const double *d_x, double *d_y, int32_t rows, int32_t cols, int32_t nnz,
                              double alpha, double beta, mspmv_stream_t stream, int debug_sync);

/* ---- extension: CSR FROM UNSORTED COO, built on the device (csrc/mspmv_coo.hip).  The result is the entries sorted STABLY by
 * (row, column) -- the reference's CsrMatrix(coo), sparse_matrix.h:636-643: output entry j is input entry permutation[j],
 * permutation is the unique stable order, duplicates are KEPT, next to each other in input order; row_offsets is right for empty
 * rows anywhere.  The sort is the transpose's radix sort over a two-part key: ceil(bits(cols - 1) / 8) passes over the column
 * digits, then ceil(bits(rows - 1) / 8) over the row digits (a 1-column or 1-row matrix skips that half; C2's 3.1 M x 3.1 M runs
 * 3 + 3), each pass reading and writing (column, row, position, value) as sequential traffic; the first reads the caller's arrays,
 * the last writes them.  No atomics on global memory, no workgroup waits on another, the host launches the same kernels whatever
 * the data and never reads device memory: the result is a function of the input alone and the call can be captured in a graph.
 * d_values == NULL and d_values_csr == NULL: structure (+ permutation) only, for either precision.  Inputs are not modified and
 * must not alias the outputs.  Indices outside [0, rows) x [0, cols) are the caller's error, as for CSR input (not checked).
 * nnz == 0 gives all-zero offsets; rows == 0 or cols == 0 with nnz > 0 is refused; rows + nnz <= 2^31 - 65537 (the forward call's
 * bound, so whatever this builds can be multiplied).  Same two-phase temp storage, 16-byte alignment, ownership, stream,
 * debug_sync and error conventions as mspmv_csr_transpose_*.  Temp storage: about 2 x nnz x (12 + value bytes) + 4 x nnz bytes
 * for three passes and more.  Measured on MI355X (profiles/coo_bench.txt): C2's 100 M shuffled triples 10.5 ms fp32 / 11.6 ms fp64
 * (3 + 3 passes) against 18.1 / 18.4 ms through a stable torch.sort of the 64-bit key and 10.2 / 10.3 ms for rocSPARSE's
 * coosort_by_row + coo2csr + gthr; an R-MAT edge list of 117 M edges 10.6 ms against 26.7 and 14.4 ms. ---- */
int mspmv_coo_to_csr_f32(void *d_temp, size_t *temp_bytes,
                         const float *d_values /* [nnz] or NULL */, const int32_t *d_row_indices, const int32_t *d_column_indices,
                         int32_t rows, int32_t cols, int32_t nnz,
                         int32_t *d_row_offsets /* [rows + 1] */, int32_t *d_column_indices_csr, float *d_values_csr,
                         int32_t *d_permutation /* may be NULL */, mspmv_stream_t stream, int debug_sync);
int mspmv_coo_to_csr_f64(void *d_temp, size_t *temp_bytes,
                         const double *d_values /* [nnz] or NULL */, const int32_t *d_row_indices, const int32_t *d_column_indices,
                         int32_t rows, int32_t cols, int32_t nnz,
                         int32_t *d_row_offsets /* [rows + 1] */, int32_t *d_column_indices_csr, double *d_values_csr,
                         int32_t *d_permutation /* may be NULL */, mspmv_stream_t stream, int debug_sync);
/* New values on the same pattern: values_csr[j] = values[permutation[j]]. */
int mspmv_coo_to_csr_values_f32(const float *d_values, const int32_t *d_permutation, float *d_values_csr,
                                int32_t nnz, mspmv_stream_t stream, int debug_sync);
int mspmv_coo_to_csr_values_f64(const double *d_values, const int32_t *d_permutation, double *d_values_csr,
                                int32_t nnz, mspmv_stream_t stream, int debug_sync);
/* Merges duplicates.  Input: a CSR whose rows are sorted by column (what mspmv_coo_to_csr_* writes).  Output: every run of equal
 * (row, column) replaced by one entry whose value is the run's values added LEFT TO RIGHT in the value type (defined bit for bit;
 * one thread adds one run, so a run of length L costs L serial adds -- meant for the short runs of assembly and edge lists),
 * row_offsets_out[rows + 1], and the new count in *d_nnz_out (one int32 on the device: the host does not learn it inside the
 * call).  The output arrays are sized for nnz; entries past the count are left untouched.  d_values == NULL and
 * d_values_out == NULL: structure only.  Output must not alias input.  Conventions as above. */
int mspmv_csr_sum_duplicates_f32(void *d_temp, size_t *temp_bytes,
                                 const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                                 int32_t rows, int32_t cols, int32_t nnz,
                                 float *d_values_out, int32_t *d_row_offsets_out, int32_t *d_column_indices_out,
                                 int32_t *d_nnz_out, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_sum_duplicates_f64(void *d_temp, size_t *temp_bytes,
                                 const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                                 int32_t rows, int32_t cols, int32_t nnz,
                                 double *d_values_out, int32_t *d_row_offsets_out, int32_t *d_column_indices_out,
                                 int32_t *d_nnz_out, mspmv_stream_t stream, int debug_sync);
/* Stateless y = alpha*A*x + beta*y from unsorted COO: builds the CSR into temp storage (mspmv_coo_to_csr_*), then runs the ordinary
 * CsrMV on it -- bitwise equal to mspmv_coo_to_csr_* followed by mspmv_csrmv_axpby_* on its outputs with that call's queried temp
 * size.  Duplicates add, because they are kept.  COST: every call pays the whole build, many times the SpMV itself; a caller that
 * multiplies more than once builds the CSR once. */
int mspmv_coomv_f32(void *d_temp, size_t *temp_bytes, const float *d_values,
                    const int32_t *d_row_indices, const int32_t *d_column_indices,
                    const float *d_x, float *d_y, int32_t rows, int32_t cols, int32_t nnz,
                    float alpha, float beta, mspmv_stream_t stream, int debug_sync);
int mspmv_coomv_f64(void *d_temp, size_t *temp_bytes, const double *d_values,
                    const int32_t *d_row_indices, const int32_t *d_column_indices,
                    const double *d_x, double *d_y, int32_t rows, int32_t cols, int32_t nnz,
                    double alpha, double beta, mspmv_stream_t stream, int debug_sync);

/* ---- extension: MATRIX ADDITION  C = alpha * A + beta * B  on the device (csrc/mspmv_add.hip; what csrgeam is in rocSPARSE /
 * cuSPARSE): A + A^T of an edge list after mspmv_coo_to_csr_* and mspmv_csr_transpose_*, A - sigma I, M + dt K, L = D - A.
 * INPUTS: two CSR matrices of the same rows x cols, every row sorted by column with no column twice -- what
 * mspmv_csr_sum_duplicates_* writes, what mspmv_coo_to_csr_* writes for triples without duplicates and mspmv_csr_transpose_* for
 * such a matrix.  Not checked: on other rows the result is unspecified, but nothing outside the arrays is read or written and the
 * call terminates (row offsets must be valid, as for every call).  A and B may be the same arrays; outputs must not alias inputs.
 * OUTPUT: C in the same canonical form.  Its pattern is the UNION of the two patterns, a function of the patterns alone: an entry
 * whose value comes out 0 stays, alpha == 0 does not drop A's pattern.  d_row_offsets_c has rows + 1 entries and is right for empty
 * rows anywhere.  d_column_indices_c / d_values_c are sized by the caller for nnz_a + nnz_b entries; the first *d_nnz_c are
 * written, the rest are left untouched.  *d_nnz_c is one int32 on the device (as for mspmv_csr_sum_duplicates_*): the host does
 * not learn it inside the call.
 * VALUES, defined bit for bit in the value type, every operation rounded on its own (no fused multiply-add):
 *     entry only in A: alpha * a      only in B: beta * b      in both: (alpha * a) + (beta * b)
 * so alpha = beta = 1 gives exactly a, b, a + b.  d_values_a == d_values_b == d_values_c == NULL: structure only (either entry
 * point; alpha and beta are ignored); values for some of the matrices and not for others: hipErrorInvalidValue (the pointer of an
 * input without entries has no say).
 * HOW: the union of two sorted sequences of the key (row, column) is a merge.  It is cut into tiles of 1792 merged entries at
 * equally spaced diagonals -- one row holding every entry costs what a million short ones cost --; a count pass, a scan of the tile
 * counts and a fill pass, 5 launches whatever the data.  No atomics on global memory, no workgroup waits on another, the host never
 * reads device memory: every output position and value is a function of the input alone and the call can be captured in a graph.
 * Same two-phase temp storage (d_temp == NULL -> size, no work), 16-byte alignment, ownership, stream, debug_sync (one line per
 * launch) and error conventions as mspmv_csr_transpose_*.  Temp storage: 24 bytes per TILE (a 100 M + 100 M addition: 2.7 MB).
 * LIMITS: rows, cols, nnz_a, nnz_b >= 0; rows + nnz_a + nnz_b <= 2^31 - 65537 (int32 diagonals with the usual tile of slack, and
 * whatever comes out can be multiplied); rows == 0 or cols == 0 with entries is refused; nnz_a == nnz_b == 0 gives all-zero
 * offsets and a count of 0.  Measured on MI355X against rocSPARSE's csrgeam_nnz + csrgeam on the same arrays, patterns equal
 * (profiles/add_bench.txt; DESIGN.md 4 "Addition"): a uniform 100 M-entry matrix plus its transpose 2.72 ms fp32 / 3.18 ms fp64
 * against 48.4 / 51.7 ms; an R-MAT graph of 62 M entries plus its transpose 1.85 / 2.14 against 236 / 251 ms; 2^26 + 2^26 entries over
 * 2^21 rows 2.02 / 2.35 against 2.58 / 2.76 ms; the same entries in ONE row 1.57 / 1.87 ms against 10.9 / 12.0 s. ---- */
int mspmv_csr_add_f32(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t cols,
                      float alpha, const float *d_values_a, const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a,
                      float beta, const float *d_values_b, const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b,
                      float *d_values_c, int32_t *d_row_offsets_c /* [rows + 1] */, int32_t *d_column_indices_c, int32_t *d_nnz_c,
                      mspmv_stream_t stream, int debug_sync);
int mspmv_csr_add_f64(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t cols,
                      double alpha, const double *d_values_a, const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a,
                      double beta, const double *d_values_b, const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b,
                      double *d_values_c, int32_t *d_row_offsets_c /* [rows + 1] */, int32_t *d_column_indices_c, int32_t *d_nnz_c,
                      mspmv_stream_t stream, int debug_sync);

/* ---- extension: MATRIX PRODUCT  C = A * B  of two CSR matrices on the device (csrc/mspmv_gemm.hip; what csrgemm is in rocSPARSE /
 * cuSPARSE): the Galerkin product R A P of a multigrid set-up, A A^T and A^T A, the two-hop neighbourhoods of a graph.
 * INPUTS: A is rows x inner, B is inner x cols, each as three CSR arrays.  ANY valid CSR is accepted: rows need not be sorted and
 * a column may repeat.  Column indices of A lie in [0, inner), those of B in [0, cols) (not checked, as everywhere).  A and B may be
 * the same arrays; outputs must not alias inputs.
 * mspmv_csr_gemm_products writes ONE int64 on the device: the sum over A's entries e of the length of B's row column_indices_a[e],
 * the number of scalar products a * b.  The sum is 64-bit and exact (per-block sums, then one block adds them; no atomics).  The
 * host does not learn it inside the call: the caller reads it (one 8-byte copy) and states it as `products` below.
 * mspmv_csr_gemm_*: `products` is the caller's statement of that count.  The host sizes every launch and the temp storage from it
 * and never reads device memory, so the call launches the same kernels whatever the data and can be captured in a graph.  The
 * device VERIFIES it (the same 64-bit sum): if the true count differs, the call writes *d_nnz_c = -1 and leaves C unspecified, and
 * still reads and writes nothing outside the arrays; it terminates whatever the inputs and whatever `products` says.
 * OUTPUT: C in canonical form (rows sorted by column, no column twice).  Its pattern is the STRUCTURAL product: an entry whose value
 * cancels to 0 stays.  d_row_offsets_c (rows + 1 entries) and *d_nnz_c (one int32 on the device) are always written and right for
 * empty rows anywhere.  d_column_indices_c / d_values_c hold capacity_c entries: they are written only when nnz_c <= capacity_c,
 * and then only their first nnz_c entries; otherwise they are left untouched and *d_nnz_c tells how much room a second call needs.
 * capacity_c = products always suffices; capacity_c = 0 is the "symbolic" phase (count and offsets only).
 * VALUES, defined bit for bit in the value type: each product a * b rounded on its own (no fused multiply-add), the products of one
 * entry (i, j) of C added LEFT TO RIGHT in expansion order -- by the position of A's entry in its row, then by the position of B's
 * entry in its row; the first product starts the sum.  So a lone product of -0.0 stays -0.0 and A * I is the duplicate-merged,
 * sorted A bit for bit.  There is no alpha / beta: alpha A B + beta D is mspmv_csr_add_* on the result.  All three value pointers
 * NULL: structure only (either entry point); values for some of the matrices and not for others: hipErrorInvalidValue (the pointer
 * of a matrix without entries, or of a C without capacity, has no say).
 * HOW: expand - sort - compress.  (1) len[e] per entry of A, its int32 scan start[], and the 64-bit total compared with `products`;
 * (2) the list of products is cut into tiles of 2048 whatever the row lengths -- one entry of A that hits a row of B with a million
 * entries costs what a million short rows cost --, each tile finds its entries of A by a search of start[] and writes its triples
 * (row, column, a * b) with consecutive stores; (3) the triples are sorted stably by (row, column) with the radix passes of
 * mspmv_coo_to_csr_*; (4) runs of equal (row, column) are added as in mspmv_csr_sum_duplicates_*; (5) one thread writes the -1.
 * One thread adds one run, so a run of L products costs L serial adds; L is bounded by the longest row of A.
 * Same two-phase temp storage (d_temp == NULL -> size, no work), 16-byte alignment, ownership, stream, debug_sync (one line per
 * launch) and error conventions as mspmv_csr_add_*.  TEMP STORAGE: 8 bytes per entry of A; per product 8 + v bytes of triples, about
 * 2 x (12 + v) + 4 for the sort, 4 + v for the sorted entries and 8 for the compression -- about 64 bytes per fp32 product, 6.4 GB
 * for 100 M of them.
 * LIMITS: rows, inner, cols, nnz_a, nnz_b, products, capacity_c >= 0; rows + products, rows + nnz_a and inner + nnz_b each
 * <= 2^31 - 65537; entries together with rows == 0, inner == 0 or cols == 0 are refused; products == 0 (nnz_a == 0 included) gives
 * all-zero offsets and a count of 0 (still verified).  Measured on MI355X against rocSPARSE's csrgemm_buffer_size + csrgemm_nnz +
 * csrgemm on the same arrays, patterns equal (profiles/gemm_bench.txt; DESIGN.md 4 "Product"), fp32: A A^T of a 5-point grid of
 * 2000 x 2000 (100 M products) 15.0 ms against 1.5 ms, A A of a uniform matrix of 1 M rows x 8 (64 M) 8.5 against 2.8 ms -- on short
 * regular rows rocSPARSE's LDS hash accumulator is the faster scheme --; A A^T of an R-MAT graph (246 M products, runs up to 5424)
 * 28.6 against 164 ms; 8 entries of A into one row of B of 2^24 entries 12.4 against 804 ms. ---- */
int mspmv_csr_gemm_products(void *d_temp, size_t *temp_bytes,
                            const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t rows, int32_t inner, int32_t nnz_a,
                            const int32_t *d_row_offsets_b, int32_t nnz_b,
                            int64_t *d_products, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_gemm_f32(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t inner, int32_t cols,
                       const float *d_values_a, const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a,
                       const float *d_values_b, const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b,
                       int32_t products, int32_t capacity_c,
                       float *d_values_c, int32_t *d_row_offsets_c /* [rows + 1] */, int32_t *d_column_indices_c, int32_t *d_nnz_c,
                       mspmv_stream_t stream, int debug_sync);
int mspmv_csr_gemm_f64(void *d_temp, size_t *temp_bytes, int32_t rows, int32_t inner, int32_t cols,
                       const double *d_values_a, const int32_t *d_row_offsets_a, const int32_t *d_column_indices_a, int32_t nnz_a,
                       const double *d_values_b, const int32_t *d_row_offsets_b, const int32_t *d_column_indices_b, int32_t nnz_b,
                       int32_t products, int32_t capacity_c,
                       double *d_values_c, int32_t *d_row_offsets_c /* [rows + 1] */, int32_t *d_column_indices_c, int32_t *d_nnz_c,
                       mspmv_stream_t stream, int debug_sync);

/* ---- extension: SDDMM, the sampled dense-dense product  C = alpha * (U V^T sampled at a CSR pattern) + beta * C  on the device
 * (csrc/mspmv_sddmm.hip; what rocsparse_sddmm is in rocSPARSE): the gradient of SpMM with respect to the matrix values,
 * dA = pattern(A) (.) (dY X^T), with U = dY and V = X laid out exactly as mspmv_csrmm_* lays out Y and X -- no copies --; edge scores
 * and attention logits on a graph (U = V = H); the sampled residual of a low-rank factorisation.
 * INPUTS: the pattern (d_row_offsets, d_column_indices; rows x cols, nnz entries) of ANY valid CSR: rows need not be sorted, a
 * repeated column gives the same value twice, empty rows may sit anywhere.  U is rows x k, V is cols x k, both row-major with
 * leading dimensions ldu, ldv >= k in elements.  U and V may be the same array; C must not alias U or V.  The pattern, U and V are
 * not modified.  C is the VALUES array alone (nnz entries).
 * VALUES, defined bit for bit in the compute type, for every stored entry e in row r with c = d_column_indices[e]:
 *     s = +0.0;  for t = 0 .. k-1:  s = s + U[r*ldu + t] * V[c*ldv + t]      (left to right)
 *     C[e] = alpha * s + (beta == 0 ? +0.0 : beta * C[e])
 * every multiply and every add rounded on its own (no fused multiply-add), nothing flushed to zero.  So C[e] is a function of U's
 * row, V's row, k, alpha, beta and the old C[e] alone -- not of where the entry sits in a tile, of nnz, of the alignment or of the
 * code path that ran.  s is never -0.0; with beta == 0 a zero result is +0.0, for negative alpha too, and the old C is never read
 * (it may hold NaN).  k == 0 gives alpha * (+0.0) + the beta term.
 * mspmv_sddmm_bf16_f32: U and V are STORED as bf16 -- the upper 16 bits of an fp32, the convention of mspmv_csrmv_mixed_bf16_f32 --
 * and widened in registers; products, sums, alpha, beta and C are fp32.  Widening is exact: the result is bit for bit that of
 * mspmv_sddmm_f32 on the widened U and V.  The gathers of V are the cost of this operation, and bf16 halves them.
 * HOW: every entry costs the same k, so the entries are cut into tiles of 512 whatever the row lengths -- one row holding every
 * entry costs what a million short ones cost.  A tile finds its rows by searching the row offsets inside the kernel (NO temp
 * storage, as for mspmv_csr_transpose_values_*); one lane owns one entry's sum; V is read in chunks of 128 bytes of k, 8
 * neighbouring lanes loading one entry's slice as consecutive 16-byte words into LDS, from where each lane reads its own entry's
 * slice back (rows of V shorter than 64 bytes are read by their lane directly: measured faster).  That path needs d_u and d_v
 * 16-byte aligned and ldu, ldv multiples of 16 bytes; anything else runs an element-wise kernel with the same bits.  One launch, no atomics, no workgroup waits on another; the host reads no device memory and launches
 * the same kernel whatever the data: the call can be captured in a graph.
 * The caller owns every buffer; asynchronous on `stream`; debug_sync prints one line per launch and waits for it; returns 0 or a
 * hipError_t; nothing outside the arrays is read or written (column indices lie in [0, cols), not checked, as everywhere).
 * LIMITS: rows, cols, nnz, k >= 0; ldu, ldv >= k; rows + nnz <= 2^31 - 65537; entries together with rows == 0 or cols == 0 are
 * refused; nnz == 0 succeeds and launches nothing (every pointer may be NULL); with k == 0, d_u and d_v may be NULL.  r*ldu + t and
 * c*ldv + t are formed in 64 bits: U and V may be larger than 4 GB.
 * Measured on MI355X against rocsparse_sddmm (default algorithm, preprocess outside the timing) on the same arrays
 * (profiles/sddmm_bench.txt; DESIGN.md 4 "SDDMM"): config 2's pattern (3.1 M x 3.1 M, 100 M
 * entries) at k = 16 / 64 / 128: fp32 1.99 / 3.72 / 7.50 ms against 4.61 / 11.6 / 21.4 ms, fp64 2.21 / 7.65 / 16.7 against 6.04 / 18.0 /
 * 32.9 ms, bf16 1.91 / 2.23 / 4.02 ms (this rocSPARSE build's dense descriptors refuse bf16); a 5-point grid of 2000 x 2000, fp32:
 * 0.43 / 0.70 / 1.18 against 0.55 / 1.65 / 3.30 ms; an R-MAT graph of scale 22 (67 M entries), fp32: 1.23 / 2.65 / 6.01 against 149 / 275 /
 * 489 ms; 2^24 entries in ONE row, fp32: 0.27 / 0.72 / 1.45 ms against 13.3 / 28.3 / 48.2 s.  rocSPARSE was faster in no case measured. ---- */
int mspmv_sddmm_f32(const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const float *d_u, int32_t ldu, const float *d_v, int32_t ldv, float *d_values_c,
                    int32_t rows, int32_t cols, int32_t nnz, int32_t k,
                    float alpha, float beta, mspmv_stream_t stream, int debug_sync);
int mspmv_sddmm_f64(const int32_t *d_row_offsets, const int32_t *d_column_indices,
                    const double *d_u, int32_t ldu, const double *d_v, int32_t ldv, double *d_values_c,
                    int32_t rows, int32_t cols, int32_t nnz, int32_t k,
                    double alpha, double beta, mspmv_stream_t stream, int debug_sync);
int mspmv_sddmm_bf16_f32(const int32_t *d_row_offsets, const int32_t *d_column_indices,
                         const uint16_t *d_u, int32_t ldu, const uint16_t *d_v, int32_t ldv, float *d_values_c,
                         int32_t rows, int32_t cols, int32_t nnz, int32_t k,
                         float alpha, float beta, mspmv_stream_t stream, int debug_sync);

/* ---- extension: the sparse triangular solve  op(A) x = alpha * b  for one right-hand side, level-scheduled (csrc/mspmv_csrsv.hip;
 * what rocsparse_csrsv / rocsparse_spsv is in rocSPARSE): L x = b and U x = b for ILU and IC factors, the forward and backward
 * sweeps of Gauss-Seidel and SOR on A itself.
 * INPUTS: A is rows x rows in CSR.  uplo chooses the triangle, diag the diagonal.  Entries of the other triangle are IGNORED: a full
 * matrix may be passed and swept with its lower and its upper part, nothing extracted.  With MSPMV_CSRSV_UNIT stored diagonal
 * entries are ignored too.  Rows need not be sorted; a column repeated inside the strict triangle is simply two products; empty rows
 * may sit anywhere.  L^T x = b is mspmv_csr_transpose_* followed by an UPPER solve.
 * THE PLAN is an opaque handle that OWNS ITS STORAGE (like mspmv_mg_plan_t, the one other place where the library allocates): the
 * host must know a launch schedule that depends on the pattern.  mspmv_csrsv_plan_create ALLOCATES (hipMalloc: scratch for the
 * analysis, freed before it returns; order[] and level_offsets[], kept until mspmv_csrsv_plan_destroy), is SYNCHRONOUS, and reads
 * a few bytes back from the device per step, as mspmv_csrmv_hotcols_skew does.  It depends on the PATTERN ALONE: new values on the
 * same pattern (a refactorisation) need no new plan.  It computes, for the chosen triangle,
 *     level[r] = 0 for a row without strict-triangle entries, else 1 + max(level[c]) over them,
 * order[] = the rows sorted stably by level (ascending row inside a level, for UPPER too) and level_offsets[] (levels + 1 entries):
 * both functions of the pattern alone.  bad_diagonal_row is found here (NON_UNIT: the smallest row with no or with more than one
 * stored diagonal entry; a solve on such a plan is refused).  A numerically zero diagonal is NOT detected: the division yields
 * the IEEE inf or NaN.
 * VALUES, defined bit for bit in the value type, for row r:
 *     s = +0.0;  for every stored entry e of row r in stored order whose column c is in the strict triangle:  s = s + a[e] * x[c]
 *     t = alpha * b[r]
 *     x[r] = (t - s) / d     (NON_UNIT; d = the row's one stored diagonal value)          x[r] = t - s     (UNIT)
 * every multiply, add and the correctly rounded division rounded on its own (no fused multiply-add), nothing flushed to zero.  So
 * x[r] is a function of the row's entries, the x of its dependencies, alpha and b[r] alone -- not of levels, segment cuts,
 * alignment or the kernel that ran.  ONE LANE adds one row's sum: a row of L strict entries costs L serial multiply-adds (as in
 * mspmv_csr_sum_duplicates_*); factors and sweeps have rows of tens of entries.
 * SCHEDULE: a level of at most W = info.narrow_rows rows is narrow.  A maximal run of consecutive narrow levels is one segment: ONE
 * launch of ONE workgroup that walks its levels with a workgroup barrier between them.  Every other level is a segment of its own:
 * one launch of as many workgroups as its rows need.  info.launches is the number of segments, a function of the pattern alone.
 * Nothing else orders two levels: no flags, no spinning, no cooperative launch, no workgroup that depends on another's progress.
 * A solve allocates nothing, reads nothing back, launches the same kernels whatever the values and can be captured in a graph.
 * d_x == d_b (in place) is allowed; any other overlap is not.  The matrix arrays and b are not modified.  The arrays passed to a
 * solve hold the pattern the plan was made from.
 * Asynchronous on `stream` (the solve); debug_sync prints one line per launch and waits for it; returns 0 or a hipError_t; column
 * indices lie in [0, rows), not checked, as everywhere.
 * LIMITS, refused before anything is launched: rows, nnz >= 0; rows + nnz <= 2^31 - 65537; uplo, diag in {0, 1}; NULL arrays with
 * nnz > 0; a NULL plan; a solve on a plan whose bad_diagonal_row >= 0.  rows == 0 gives a valid plan with 0 levels and 0 launches
 * (no device is touched).  nnz == 0 with UNIT gives x = alpha * b in one level (the matrix arrays may be NULL).
 * Measured on MI355X against rocsparse_spsv (analysis outside the solve timing; profiles/csrsv_bench.txt; DESIGN.md 4 "Triangular
 * solve"), fp64 solve / analysis: the lower part of a 5-point grid of 2000 x 2000 16.4 / 38 ms against 91 / 82 ms; the ILU(0)
 * pattern of a 7-point grid of 128^3 2.12 / 12 ms against 44.7 / 24 ms; a bidiagonal chain of 2^16 rows 49 / 70 ms against 84 / 12 ms;
 * the strict lower triangle of an R-MAT graph of scale 20 (rows of tens of thousands of entries, one lane each) 259 / 78 ms against
 * 18.8 / 13 ms: rocSPARSE is 14 times faster there.  W = 256 by the sweep on the two grids. ---- */
#define MSPMV_CSRSV_LOWER 0
#define MSPMV_CSRSV_UPPER 1
#define MSPMV_CSRSV_NON_UNIT 0
#define MSPMV_CSRSV_UNIT 1
typedef struct mspmv_csrsv_plan mspmv_csrsv_plan_t;
typedef struct mspmv_csrsv_info {
    int32_t rows, nnz, uplo, diag;
    int32_t levels;            /* number of levels (0 for rows == 0)                                  */
    int32_t launches;          /* kernels ONE solve launches: a function of the pattern alone         */
    int32_t narrow_rows;       /* W: a level of <= W rows is "narrow" (above)                         */
    int32_t max_level_rows;
    int32_t bad_diagonal_row;  /* NON_UNIT: smallest row with no or more than one stored diagonal; -1 */
    int64_t used_entries;      /* entries of the strict triangle                                      */
    uint64_t device_bytes;     /* what the plan holds on the device                                   */
} mspmv_csrsv_info_t;
int mspmv_csrsv_plan_create(mspmv_csrsv_plan_t **plan, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                            int32_t rows, int32_t nnz, int32_t uplo, int32_t diag, mspmv_stream_t stream, int debug_sync);
int mspmv_csrsv_plan_info(const mspmv_csrsv_plan_t *plan, mspmv_csrsv_info_t *info);
const int32_t *mspmv_csrsv_plan_order(const mspmv_csrsv_plan_t *plan);          /* device, rows entries       */
const int32_t *mspmv_csrsv_plan_level_offsets(const mspmv_csrsv_plan_t *plan);  /* device, levels + 1 entries */
int mspmv_csrsv_solve_f32(mspmv_csrsv_plan_t *plan, const float *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, float alpha, const float *d_b, float *d_x,
                          mspmv_stream_t stream, int debug_sync);
int mspmv_csrsv_solve_f64(mspmv_csrsv_plan_t *plan, const double *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, double alpha, const double *d_b, double *d_x,
                          mspmv_stream_t stream, int debug_sync);
int mspmv_csrsv_plan_destroy(mspmv_csrsv_plan_t *plan);

/* ---- extension: the sparse triangular solve for k right-hand sides  op(A) X = alpha * B, level-scheduled (csrc/mspmv_csrsm.hip; what
 * rocsparse_csrsm / rocsparse_spsm is in rocSPARSE): the two sweeps of a preconditioner inside a block Krylov method, a solver that
 * carries several right-hand sides, a Gauss-Seidel smoother on k vectors.  One chain of launches serves all k columns, where k calls
 * of mspmv_csrsv_solve_* pay the chain k times.
 * THE PLAN is any mspmv_csrsv_plan_t, used as made: the same triangle, the same diagonal rule, the same pattern contract, the same
 * levels, order[] and level_offsets[].  There is no new analysis and no new plan type; one plan serves mspmv_csrsv_solve_* and
 * mspmv_csrsm_solve_* for any k, in any order.
 * INPUTS: A as for mspmv_csrsv_*.  B and X are rows x k, ROW-MAJOR, with leading dimensions ldb, ldx >= k in elements: exactly the
 * layout of Y in mspmv_csrmm_*, so the output of mspmv_csrmm_* feeds the solve and back with no copy.
 * VALUES, defined bit for bit in the value type: column j of X is what mspmv_csrsv_solve_* gives for column j of B.  For row r and
 * right-hand side j:
 *     s = +0.0;  for every stored entry e of row r in stored order whose column c is in the strict triangle:  s = s + a[e] * X[c, j]
 *     t = alpha * B[r, j]
 *     X[r, j] = (t - s) / d     (NON_UNIT; d = the row's one stored diagonal value)          X[r, j] = t - s     (UNIT)
 * every operation rounded on its own (no fused multiply-add), nothing flushed to zero.  The bits depend on none of k, ldb, ldx, P, the
 * schedule, the alignment or the kernel that ran.  X[r, j] for j in [k, ldx) is never written; B's padding is never read.
 * d_x == d_b with ldx == ldb (in place) is allowed; any other overlap is not.  The matrix arrays and B are not modified.
 * MAPPING: P = info.lanes_per_row = the smallest power of two >= min(k, 64) adjacent lanes of one wave work one row.  Lane j of the
 * group takes the right-hand sides j, j + 64, ... (info.passes = ceil(k / 64) of them, each a pass of its own over the row); a lane
 * with j >= k idles.  The group reads cols[e] and vals[e] at one address and gathers X[c, j .. j + P) in one coalesced request.
 * One lane still adds one (row, right-hand side) sum serially: a row of L strict entries costs L multiply-adds per pass.  All index
 * arithmetic on B and X is 64-bit (rows * ld may exceed 2^31).
 * SCHEDULE: a level of n rows is narrow for this k when n * P <= info.narrow_lanes (256: the lanes of csrsv's W = 256, so that k = 1
 * launches what mspmv_csrsv_solve_* launches).  A maximal run of consecutive narrow levels is ONE launch of ONE workgroup of 1024
 * threads that walks its levels with a workgroup barrier between them; every other level is one launch of ceil(n * P / 256)
 * workgroups.  The cut depends on P, so it is made on the host from the plan's copy of level_offsets[] while the solve walks them;
 * mspmv_csrsm_info applies the same rule and states the count: info.launches is a function of the pattern, k and the budget alone.
 * Nothing else orders two levels: no flags, no spinning, no cooperative launch.  A solve allocates nothing on the device or the
 * host, reads nothing back, launches the same kernels whatever the values and can be captured in a graph.
 * mspmv_csrsm_info is host only and touches no device.  The solve is asynchronous on `stream`; debug_sync prints one line per launch
 * (sm_narrow_kernel or sm_level_kernel) and waits for it; returns 0 or a hipError_t.
 * LIMITS, refused before anything is launched: a NULL plan (or, for mspmv_csrsm_info, NULL info); a plan whose bad_diagonal_row >= 0;
 * k < 1; ldb < k or ldx < k; NULL B or X with rows > 0; NULL matrix arrays with nnz > 0.  rows == 0 succeeds and touches no device.
 * nnz == 0 with UNIT gives X = alpha * B (the matrix arrays may be NULL).
 * Measured on MI355X (profiles/csrsm_bench.txt; DESIGN.md 4 "Triangular solve, several right-hand sides"), fp64, one solve against k
 * calls of mspmv_csrsv_solve_* on the columns copied out to vectors / against rocsparse_spsm (analysis outside the timing): the lower
 * part of a 5-point grid of 2000 x 2000 at k = 16 18.5 ms against 302 / 138 ms, at k = 64 19.6 ms against 1220 / 147 ms; the ILU(0)
 * pattern of a 7-point grid of 128^3 at k = 16 2.36 ms against 37.2 / 85.6 ms; at k = 1 the time of mspmv_csrsv_solve_* within the
 * spread.  The strict lower triangle of an R-MAT graph of scale 20 (long rows, one lane per right-hand side each) at k = 16 322 ms
 * against 4096 / 174 ms: rocSPARSE stays 1.9 times faster there.  narrow_lanes = 256 by the sweep on the two grids. ---- */
typedef struct mspmv_csrsm_info {
    int32_t k;
    int32_t lanes_per_row;   /* P: the smallest power of two >= min(k, 64)                        */
    int32_t passes;          /* ceil(k / 64): right-hand sides one lane takes, one after the other */
    int32_t narrow_lanes;    /* the lane budget up to which a level is narrow (above)             */
    int32_t launches;        /* kernels ONE solve with this k launches: pattern, k and budget alone */
} mspmv_csrsm_info_t;
int mspmv_csrsm_info(const mspmv_csrsv_plan_t *plan, int32_t k, mspmv_csrsm_info_t *info);
int mspmv_csrsm_solve_f32(mspmv_csrsv_plan_t *plan, const float *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, float alpha, const float *d_b, int32_t ldb,
                          float *d_x, int32_t ldx, int32_t k, mspmv_stream_t stream, int debug_sync);
int mspmv_csrsm_solve_f64(mspmv_csrsv_plan_t *plan, const double *d_values, const int32_t *d_row_offsets,
                          const int32_t *d_column_indices, double alpha, const double *d_b, int32_t ldb,
                          double *d_x, int32_t ldx, int32_t k, mspmv_stream_t stream, int debug_sync);

/* ---- extension: ILU(0), the incomplete LU factorisation without fill-in, level-scheduled (csrc/mspmv_csrilu0.hip; what
 * rocsparse_csrilu0 is in rocSPARSE): A ~ L U on A's own pattern, the preconditioner whose two sweeps mspmv_csrsv_* solves.  With it
 * the sparse parts of a preconditioned Krylov iteration stay inside this library: mspmv_csrmv_* for A p, mspmv_csrilu0_* once per
 * matrix, two mspmv_csrsv_solve_* per iteration (the loop itself is built for conjugate gradients: mspmv_pcg_* below, and for
 * BiCGStab, the nonsymmetric case this factor is for: mspmv_bicgstab_* of include/mspmv_krylov.h, and GMRES(m): mspmv_gmres_* of include/mspmv_gmres.h).
 * THE PLAN: lower_plan is any plan made by mspmv_csrsv_plan_create with MSPMV_CSRSV_LOWER (either diag) for this pattern: row i of
 * the row-wise elimination needs the finished rows whose column its strict lower part stores, which is the dependency graph of
 * L x = b, so the plan's levels, order and segments are the factorisation's too.  rows and nnz are taken from it; the same plan then
 * serves the L solve (created with MSPMV_CSRSV_UNIT).  An UPPER plan or a NULL plan is refused.
 * INPUT: A is rows x rows in CSR, every row SORTED by column with no column twice: the canonical form mspmv_csr_sum_duplicates_*,
 * mspmv_csr_add_* and mspmv_csr_gemm_* write.  This is NOT checked: on other input the values are unspecified, but nothing outside
 * the arrays is touched and the call ends.  The pattern arrays and d_values are not modified unless d_values_lu == d_values (in
 * place), which is allowed; any other overlap is not.
 * OUTPUT: d_values_lu, nnz entries on A's pattern: the strict lower part holds L (its unit diagonal implied), the diagonal and the
 * upper part hold U -- what mspmv_csrsv_* sweeps with LOWER + UNIT and UPPER + NON_UNIT, nothing extracted.
 * VALUES, defined bit for bit in the value type.  Rows in dependency order; for row i:
 *     for every stored entry e of row i with k = col[e] < i, in stored (= ascending) order:
 *         a[e] = a[e] / piv(k)              piv(k) = the FINAL diagonal value of row k; +0.0 if row k stores no diagonal
 *         for every stored entry f of row k with j = col[f] > k for which row i stores column j, at position g:
 *             a[g] = a[g] - a[e] * a[f]
 * every divide, multiply and subtract rounded on its own (no fused multiply-add; the division correctly rounded), nothing flushed to
 * zero.  So a[g] is a function of A's values and the pattern alone -- not of levels, segments, lanes per row, alignment or the
 * kernel that ran.  Products whose (i, j) is not in the pattern are dropped (the "0").  A missing diagonal acts as a pivot of +0.0
 * and its row has no diagonal to update: the definition is total, and a division by zero gives the IEEE inf or NaN.
 * PIVOT: *d_pivot (one int32 ON THE DEVICE; may be NULL) = the smallest row whose diagonal is not stored or whose final diagonal
 * compares == 0 (so -0.0 counts, NaN does not); -1 if there is none.  The host does not learn it inside the call.
 * TEMP STORAGE, two-phase: d_temp == NULL writes the size to *temp_bytes, does no work and needs no device.  d_temp is 16-byte
 * aligned and holds the diagonal position of every row: 4 * rows bytes rounded up to 16, at least 16.
 * SCHEDULE: one prologue launch (each row's diagonal position by bisection; the copy of d_values to d_values_lu when they differ;
 * rows without a stored diagonal go to *d_pivot), then one launch per segment of the plan: 1 + info.launches in all.  A row is
 * worked by G consecutive lanes of one wave, G = mspmv_csrilu0_group(rows, nnz): the smallest power of two >= the mean row length,
 * within [1, 64]; a function of rows and nnz alone (host only, launches nothing).  Each lane owns every G-th entry of the row; the
 * quotient of a lower entry reaches the group by a shuffle.  No workgroup waits for another.
 * Asynchronous on `stream`; allocates nothing, reads nothing back, launches the same kernels whatever the values and can be
 * captured in a graph; debug_sync prints one line per launch with the lanes per row and waits for it; returns 0 or a hipError_t.
 * LIMITS, refused before anything is launched: a NULL or UPPER plan; a NULL temp_bytes; *temp_bytes too small; a misaligned d_temp;
 * NULL value or pattern arrays with nnz > 0.  rows == 0 succeeds and launches nothing.  nnz == 0 with rows > 0 reports pivot 0.
 * Measured on MI355X against rocsparse_csrilu0 (analysis outside the timing; out of place, the copy included; profiles/
 * csrilu0_bench.txt; DESIGN.md 4 "ILU(0)"), fp32 / fp64: a 5-point grid of 2000 x 2000 22.0 / 26.9 ms against 191 / 192 ms; a
 * 7-point grid of 128^3 2.90 / 3.17 ms against 112 / 112 ms; A + A^T + I of an R-MAT graph of scale 14 (rows of thousands of
 * entries, one group each) 612 / 621 ms against 9.6 / 9.6 ms: rocSPARSE is 64 times faster there, and at scale 16 and 18, where one
 * group would run for seconds to minutes, this call was not run at all (rocSPARSE: 85 ms and 0.82 s).  G by the sweep on the two
 * grids. ---- */
int mspmv_csrilu0_group(int32_t rows, int32_t nnz, int32_t *lanes_per_row);
int mspmv_csrilu0_f32(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const float *d_values,
                      float *d_values_lu, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t *d_pivot,
                      mspmv_stream_t stream, int debug_sync);
int mspmv_csrilu0_f64(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const double *d_values,
                      double *d_values_lu, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t *d_pivot,
                      mspmv_stream_t stream, int debug_sync);

/* ---- extension: IC(0), the incomplete Cholesky factorisation without fill-in, level-scheduled (csrc/mspmv_csric0.hip; what
 * rocsparse_csric0 is in rocSPARSE): A ~ L L^T on the pattern of A's lower triangle, the SYMMETRIC preconditioner that conjugate
 * gradients needs and ILU(0) cannot give, at half of ILU(0)'s work and half of its factor.  With it a preconditioned CG stays
 * inside this library: mspmv_csrmv_* for A p, mspmv_csric0_* once per matrix, two mspmv_csrsv_solve_* per iteration, and the loop
 * itself with its dots and updates: mspmv_pcg_* below (for nonsymmetric matrices: mspmv_bicgstab_* of include/mspmv_krylov.h).
 * THE PLAN: lower_plan is any plan made by mspmv_csrsv_plan_create with MSPMV_CSRSV_LOWER (either diag) for this pattern: row i of
 * the row-wise Cholesky needs the finished rows whose column its strict lower part stores, which is the dependency graph of
 * L x = b, so the plan's levels, order and segments are the factorisation's too, exactly as for mspmv_csrilu0_*.  rows and nnz are
 * taken from it; the same plan then serves the L solve (created with MSPMV_CSRSV_NON_UNIT).  An UPPER or a NULL plan is refused.
 * INPUT: A is rows x rows in CSR, every row SORTED by column with no column twice.  This is NOT checked: on other input the values
 * are unspecified, but nothing outside the arrays is touched and the call ends.  ONLY THE LOWER TRIANGLE AND THE DIAGONAL ARE READ
 * AS NUMBERS: the matrix factorised is the symmetric one they define.  The pattern arrays and d_values are not modified unless
 * d_values_l == d_values (in place), which is allowed; any other overlap is not.
 * OUTPUT: d_values_l, nnz entries on A's pattern: the strict lower part and the diagonal hold L.
 * VALUES, defined bit for bit in the value type.  Rows in dependency order; for row i with stored diagonal position d:
 *     for every stored entry e of row i with j = col[e] < i, in stored (= ascending) order:
 *         a[e] = a[e] / piv(j)              piv(j) = the FINAL (rooted) diagonal of row j; +0.0 if row j stores no diagonal
 *         for every stored entry g of row i behind e with k = col[g], j < k < i,
 *             for which row k stores column j, at position f:       a[g] = a[g] - a[e] * a[f]
 *         if row i stores its diagonal:                              a[d] = a[d] - a[e] * a[e]
 *     a[d] = sqrt(a[d])
 * every divide, multiply, subtract and root rounded on its own (no fused multiply-add; division and square root correctly
 * rounded), nothing flushed to zero.  So a[g] is a function of A's lower triangle and the pattern alone -- not of levels, segments,
 * lanes per row, alignment or the kernel that ran.  A missing diagonal acts as a pivot of +0.0; a negative value under the root
 * gives the IEEE NaN: the definition is total.  Entries with column > i are copied unchanged when mirror == 0.
 * PIVOT: *d_pivot (one int32 ON THE DEVICE; may be NULL) = the smallest row whose diagonal is not stored or whose value under the
 * root compares <= 0 (so -0.0 counts, NaN does not); -1 if there is none.  The host does not learn it inside the call.
 * MIRROR: with mirror == 1 one more launch, after the factorisation, writes L^T into the upper triangle: entry (i, j) with j > i
 * receives the final a[f] of entry (j, i) if row j stores column i, else +0.0.  The array is then L\L^T in A's layout, and
 * mspmv_csrsv_* sweeps it with LOWER + NON_UNIT and UPPER + NON_UNIT, nothing extracted and nothing transposed.  This needs a
 * STRUCTURALLY SYMMETRIC pattern (merge_spmv_amd.csr_symmetrize, mspmv_csr_add_* of A and A^T, makes one): a lower entry without an upper
 * partner is simply absent from the upper sweep, which then solves with another matrix than L^T.  With mirror == 0 the route for
 * other patterns stays mspmv_csr_transpose_* of the factor followed by an UPPER solve.
 * TEMP STORAGE, two-phase: d_temp == NULL writes the size to *temp_bytes, does no work and needs no device.  d_temp is 16-byte
 * aligned and holds the diagonal position of every row: 4 * rows bytes rounded up to 16, at least 16.
 * SCHEDULE: one prologue launch (each row's diagonal position by bisection; the copy of d_values to d_values_l when they differ;
 * rows without a stored diagonal go to *d_pivot), then one launch per segment of the plan, then the mirror: 1 + info.launches +
 * mirror in all.  A row is worked by G consecutive lanes of one wave, G = mspmv_csric0_group(rows, nnz): the smallest power of two
 * >= ceil((nnz + rows) / (2 rows)), the mean length of a row's lower-plus-diagonal part under a symmetric pattern, within [1, 64];
 * a function of rows and nnz alone (host only, launches nothing).  Each lane owns every G-th entry of the row up to the diagonal;
 * the quotient of a lower entry reaches the group by a shuffle; an owned entry of column k looks the quotient's column up in row k
 * by bisection.  No workgroup waits for another.
 * Asynchronous on `stream`; allocates nothing, reads nothing back, launches the same kernels whatever the values and can be
 * captured in a graph; debug_sync prints one line per launch with the lanes per row and waits for it; returns 0 or a hipError_t.
 * LIMITS, refused before anything is launched: a NULL or UPPER plan; a NULL temp_bytes; mirror not in {0, 1}; *temp_bytes too
 * small; a misaligned d_temp; NULL value or pattern arrays with nnz > 0.  rows == 0 succeeds and launches nothing.  nnz == 0 with
 * rows > 0 reports pivot 0.
 * Measured on MI355X against rocsparse_csric0 (analysis outside the timing; out of place, the copy included, mirror == 0; profiles/
 * csric0_bench.txt; DESIGN.md 4 "IC(0)") and against mspmv_csrilu0_* on the same plan and arrays in the same run, fp32 / fp64: a
 * 5-point grid of 2000 x 2000 21.9 / 25.8 ms against 121 / 122 ms (ILU(0): 22.0 / 27.0 ms); a 7-point grid of 128^3 2.89 / 3.02 ms
 * against 75.0 / 75.2 ms (ILU(0): 2.91 / 3.16 ms); the mirror adds 0.03 - 0.08 ms.  IC(0) does half of ILU(0)'s arithmetic and is
 * only 1 - 5 % faster: both are bound by the launches (one per level), not by the rows.  A + A^T + I of an R-MAT graph of scale 14
 * (rows of thousands of entries, one group each) 667 / 677 ms against 6.5 / 6.5 ms: rocSPARSE is 100 times faster there, and ILU(0)
 * (613 / 623 ms, 32 lanes per row against IC(0)'s 16) is 8 % faster than this call; at scale 16, where one group would run for
 * seconds, this call was not run at all (rocSPARSE: 44 / 45 ms).  G by the sweep on the two grids: the rule's 4 is the fastest of
 * 1 ... 64 on both. ---- */
int mspmv_csric0_group(int32_t rows, int32_t nnz, int32_t *lanes_per_row);
int mspmv_csric0_f32(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const float *d_values,
                     float *d_values_l, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t mirror,
                     int32_t *d_pivot, mspmv_stream_t stream, int debug_sync);
int mspmv_csric0_f64(const mspmv_csrsv_plan_t *lower_plan, void *d_temp, size_t *temp_bytes, const double *d_values,
                     double *d_values_l, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t mirror,
                     int32_t *d_pivot, mspmv_stream_t stream, int debug_sync);

/* ---- extension: MULTICOLOUR ORDERING, part 1: a deterministic graph colouring on the device (csrc/mspmv_color.hip; what
 * rocsparse_csrcolor is in rocSPARSE).  The level-scheduled family above (mspmv_csrsv_*, mspmv_csrsm_*, mspmv_csrilu0_*,
 * mspmv_csric0_*) pays one launch per level; after a symmetric permutation by colour a row depends only on rows of smaller colours, so
 * the LOWER plan of P A P^T has at most as many levels as there are colours, and none of that family's code changes.
 * GRAPH: the vertices are the rows of a rows x rows CSR pattern; u and v are neighbours when u != v and A[u,v] OR A[v,u] is stored.  The
 * pattern need not be structurally symmetric (the analysis builds A^T's pattern with mspmv_csr_transpose_*).  Diagonal entries are
 * ignored, repeated columns are harmless, rows need not be sorted, empty rows may sit anywhere.
 * DEFINITION, the pattern and the priorities alone:
 *     key(v)   = (uint64) prio(v) << 32 | v
 *     prio(v)  = d_priority[v] when priorities are given, else fmix32(v), the 32-bit finaliser
 *                h = v;  h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16
 *     color[v] = the smallest non-negative integer that is not the colour of any neighbour u with key(u) > key(v)
 * that is, sequential greedy colouring in descending key order: a total function of its input, not of any schedule, round structure,
 * alignment or kernel.  Equal priorities fall to the vertex index (the larger index first).  Derived from the colours:
 *     order[]   = the vertices sorted stably by colour (ascending vertex inside a colour)
 *     inverse[] : inverse[order[i]] = i
 *     offsets[] : colours + 1 entries; colour c holds order[offsets[c] .. offsets[c + 1])
 * info.edges is the number of stored off-diagonal entries, duplicates counted; info.max_color_rows the largest colour class.
 * SCHEME: Jones-Plassmann in rounds.  A vertex is coloured once every neighbour of larger key holds a colour; its colour goes from -1
 * to its final value in one 32-bit store.  A reader in another workgroup of the same launch sees -1 (and waits one more round) or
 * the final value, so the result is the definition whatever the timing; nothing but the kernel boundary and, inside one workgroup,
 * the barrier orders two rounds: no flags, no spinning, no workgroup that waits on another.  While more than 4096 vertices remain a
 * round is one launch over the compacted list, after which the host reads the remaining count back; at or below 4096 ONE workgroup
 * finishes all remaining rounds.  A vertex of 64 or more neighbour slots is scanned by its whole wave.  info.rounds is the number of
 * those host steps (informational: it may depend on timing, the colours do not).
 * THE HANDLE is opaque and OWNS ITS STORAGE, exactly as mspmv_csrsv_plan_t and for the same reason: the host must learn a
 * pattern-dependent count.  mspmv_csr_color_create ALLOCATES (hipMalloc: scratch, freed before it returns; the four arrays, kept
 * until mspmv_csr_color_destroy), is SYNCHRONOUS and reads a few bytes back per step.  debug_sync prints one line per launch.
 * LIMITS, refused before anything is launched or allocated: rows, nnz >= 0; rows + nnz <= 2^31 - 65537; nnz > 0 with rows == 0; NULL
 * pattern arrays with nnz > 0; a NULL `coloring`.  rows == 0 gives a valid handle with 0 colours (no device is touched; the getters
 * return NULL).  nnz == 0 gives colour 0 everywhere (the pattern arrays may be NULL).  A NULL handle makes the getters return NULL
 * and info and destroy return 1.  Column indices lie in [0, rows), not checked, as everywhere.
 * USE: mspmv_csr_permute_* with row_perm = order and col_map = inverse gives P A P^T; b' = b[order] and x = x'[inverse] are
 * mspmv_coo_to_csr_values_*(b, order, b', rows) and (x', inverse, x, rows).  THE PRICE is a weaker incomplete factor: IC(0)-
 * preconditioned CG on a 5-point grid of 24 x 24 takes 48 iterations in multicolour order against 32 in natural order (88 without).
 * Measured on MI355X (profiles/color_bench.txt; DESIGN.md 4 "Multicolour ordering"), colouring against rocsparse_csrcolor on the same
 * pattern: a 5-point grid of 2000 x 2000 6.2 ms, 5 colours, 11 rounds against 1.3 ms and 16 colours; a 7-point grid of 128^3 5.2 ms, 7
 * colours, 14 rounds against 1.4 ms and 22 colours; A + A^T + I of an R-MAT graph of scale 16 173 ms, 112 colours, 406 rounds against
 * 321 ms and 526 colours: rocSPARSE is 4 - 5 times faster on the grids and uses 3 - 5 times the colours everywhere.  What the order
 * buys, fp64, natural -> multicolour: on the 2000 x 2000 grid the LOWER solve 3999 levels, 29.4 ms -> 5 levels, 0.15 ms, the UPPER
 * solve 25.1 -> 0.34 ms, mspmv_csric0 25.7 -> 0.68 ms, mspmv_csrilu0 26.7 -> 0.75 ms; on the 128^3 grid 382 -> 7 levels, the solves
 * 2.55 / 2.42 -> 0.15 / 0.30 ms, the factorisations 3.15 / 3.17 -> 0.68 / 0.61 ms; on the R-MAT graph 427 -> 112 levels, the solves
 * 91 / 117 -> 60 / 42 ms (one lane per row of thousands of entries either way; not factorised).  IC(0)-preconditioned CG on the
 * 2000 x 2000 grid (the 5-point Laplacian + 0.01 I, to 1e-8 |b|): 74 iterations x 52.3 ms = 3872 ms in natural order, 114
 * iterations x 0.69 ms = 78 ms in multicolour order: 1.5 times the iterations, 50 times sooner. ---- */
typedef struct mspmv_csr_color mspmv_csr_color_t;
typedef struct mspmv_csr_color_info {
    int32_t rows, nnz;
    int32_t colors;            /* number of colours (0 for rows == 0)                                 */
    int32_t max_color_rows;    /* the largest colour class                                            */
    int32_t rounds;            /* host steps of the colouring (informational)                         */
    int64_t edges;             /* stored off-diagonal entries, duplicates counted                     */
    uint64_t device_bytes;     /* what the handle holds on the device                                 */
} mspmv_csr_color_info_t;
int mspmv_csr_color_create(mspmv_csr_color_t **coloring, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                           int32_t rows, int32_t nnz, const uint32_t *d_priority /* rows entries, or NULL */,
                           mspmv_stream_t stream, int debug_sync);
int mspmv_csr_color_info(const mspmv_csr_color_t *coloring, mspmv_csr_color_info_t *info);
const int32_t *mspmv_csr_color_colors(const mspmv_csr_color_t *coloring);   /* device, rows entries       */
const int32_t *mspmv_csr_color_order(const mspmv_csr_color_t *coloring);    /* device, rows entries       */
const int32_t *mspmv_csr_color_inverse(const mspmv_csr_color_t *coloring);  /* device, rows entries       */
const int32_t *mspmv_csr_color_offsets(const mspmv_csr_color_t *coloring);  /* device, colors + 1 entries */
int mspmv_csr_color_destroy(mspmv_csr_color_t *coloring);

/* ---- extension: MULTICOLOUR ORDERING, part 2: B = A[row_perm, :] with the columns renumbered, canonical (csrc/mspmv_permute.hip).
 * DEFINITION: row i of B holds the entries of A's row row_perm[i]; each column c is replaced by col_map[c]; the entries of a row are
 * sorted STABLY by the new column, so entries that map to one column keep their stored order.  B entry j is A entry permutation[j];
 * values are moved, never recomputed.  Equivalently: bit for bit what mspmv_coo_to_csr_* gives on the triples (inverse_row(r),
 * col_map[c], v) listed in A's stored order -- which is how it is computed: one lane per row inverts row_perm, the entries are expanded
 * to (new row, new column) in equal tiles whatever the row lengths (one row of 2^20 entries is no single lane's loop), then the COO
 * build's radix passes sort them.  With row_perm = order and col_map = inverse of a colouring this is P A P^T; a canonical A (sorted
 * rows, no duplicates) stays canonical, which is what mspmv_csrilu0_* and mspmv_csric0_* require.
 * row_perm is a permutation of [0, rows) and col_map maps into [0, cols): neither is checked, as indices are not checked elsewhere.
 * d_row_perm == NULL and d_col_map == NULL mean the identity (both NULL: a stable sort of every row by column).
 * The call allocates nothing, reads nothing back, launches the same kernels whatever the data and can be captured in a graph.  Inputs
 * are not modified and must not alias the outputs.  d_values == NULL and d_values_b == NULL: structure (+ permutation) only.
 * nnz == 0 gives all-zero offsets; rows == 0 or cols == 0 with nnz > 0 is refused; rows + nnz <= 2^31 - 65537.  Same two-phase temp
 * storage, 16-byte alignment, stream, debug_sync and error conventions as mspmv_coo_to_csr_*; temp storage: that call's plus
 * 4 x rows + 8 x nnz bytes.
 * NEW VALUES on the same pattern and the vectors need no entry point of their own: mspmv_coo_to_csr_values_*(values, permutation, out,
 * nnz) is out[j] = values[permutation[j]]; the same call with `order` gives b' = b[order], with `inverse` x = x'[inverse].
 * COST next to mspmv_coo_to_csr_* on the same entries, measured on MI355X (tools/color_bench.py; profiles/color_bench.txt):
 * the two extra launches add 5 - 14 %: P A P^T of a 5-point grid of 2000 x 2000 (20.0 M entries, fp64, 3 + 3 passes) 2.71 ms against
 * 2.44 ms; of a 7-point grid of 128^3 (14.6 M entries) 1.84 against 1.75 ms; of A + A^T + I of an R-MAT graph of scale 16 (1.9 M
 * entries) 0.24 against 0.21 ms. ---- */
int mspmv_csr_permute_f32(void *d_temp, size_t *temp_bytes,
                          const float *d_values /* or NULL */, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          int32_t rows, int32_t cols, int32_t nnz,
                          const int32_t *d_row_perm /* rows entries or NULL = identity */,
                          const int32_t *d_col_map  /* cols entries or NULL = identity */,
                          float *d_values_b, int32_t *d_row_offsets_b, int32_t *d_column_indices_b,
                          int32_t *d_permutation /* nnz entries, may be NULL */, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_permute_f64(void *d_temp, size_t *temp_bytes,
                          const double *d_values /* or NULL */, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                          int32_t rows, int32_t cols, int32_t nnz,
                          const int32_t *d_row_perm /* rows entries or NULL = identity */,
                          const int32_t *d_col_map  /* cols entries or NULL = identity */,
                          double *d_values_b, int32_t *d_row_offsets_b, int32_t *d_column_indices_b,
                          int32_t *d_permutation /* nnz entries, may be NULL */, mspmv_stream_t stream, int debug_sync);

/* ---- extension: THE DETERMINISTIC REDUCTION and the dot product built on it (csrc/mspmv_vec.hpp, mspmv_vec.hip).  The one piece of a
 * Krylov iteration whose bits a BLAS leaves open, defined here like everything else: *d_result = R(a o b), ONE value ON THE DEVICE.
 * Nothing is read back, nothing allocated, no atomics; two launches ordered by the kernel boundary; the call can be captured in a graph.
 * d_a == d_b gives the squared norm.  Inputs are not modified and may have any alignment of their type.
 * DEFINITION, in the value type T.  The summands are the products s[i] = fl(a[i] * b[i]), i in [0, n), each rounded on its own (no
 * fused multiply-add).  R(s) is a fixed tree, a function of n and T alone -- not of the grid, the alignment, the device or the kernel:
 *     chunk(c[0 .. 1024))  =  q[t] = ((c[4t] + c[4t+1]) + c[4t+2]) + c[4t+3]  for t in [0, 256);  then eight times  q <- q[0::2] + q[1::2]
 *                             (neighbours first: q[0] + q[1], q[2] + q[3], ...);  the one value left
 *     level(v)             =  v cut into consecutive chunks of 1024, the last one filled up with +0.0;  [chunk(each)]
 *                             (at least one chunk: an empty v gives one chunk of zeros)
 *     R(s)                 =  p = level(s);   if p has more than 1024 entries:  p = level(p);   R = chunk(p filled up with +0.0 to 1024)
 * The fill is +0.0 and the last step is ALWAYS made, which fixes the sign of a zero: products that are all -0.0 sum to -0.0 inside
 * a chunk, and the result is -0.0 only if no step of the tree met a fill (n = 2^20 or n = 2^30: every level full);
 * n == 0 gives +0.0.  Nothing is flushed to zero; Inf and NaN propagate (a NaN result is a NaN; its sign and payload are not defined).
 * In numpy:  def chunk(c): q = c.reshape(-1, 256, 4); q = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
 *                         while q.shape[1] > 1: q = q[:, 0::2] + q[:, 1::2]
 *                         return q[:, 0]                                          (c: the padded level, a multiple of 1024 long)
 * tests/pcg_model.py is this restatement.
 * TEMP STORAGE, two-phase: d_temp == NULL writes the size to *temp_bytes, does no work and needs no device.  d_temp is 16-byte aligned
 * and holds the level-1 partials: max(1, ceil(n / 1024)) values, rounded up to 16 bytes.  Whatever it held before does not matter.
 * Asynchronous on `stream`; debug_sync prints one line per launch (vec_dot_kernel, vec_fold_kernel) and waits for it; returns 0 or a
 * hipError_t.  LIMITS, refused before anything is launched: a NULL temp_bytes; n < 0; n > 2^30 (the fold has two levels); *temp_bytes
 * too small; a misaligned d_temp; a NULL d_result; NULL d_a or d_b with n > 0.
 * Measured on MI355X against torch.dot (rocBLAS) at n = 4 * 10^6 (tools/pcg_bench.py; profiles/pcg_bench.txt; DESIGN.md 4
 * "Preconditioned conjugate gradients"), fp64 / fp32: 20 calls in a replayed graph, per call, 14.3 / 7.2 us against 16.5 / 9.0 us
 * (4.5 TB/s); one call from Python between events, the host's enqueue of two launches included, 23.6 / 17.4 us against 19.1 /
 * 13.0 us: torch.dot is 1.2 - 1.3 times faster there. ---- */
int mspmv_vec_dot_f32(void *d_temp, size_t *temp_bytes, const float *d_a, const float *d_b, int64_t n, float *d_result,
                      mspmv_stream_t stream, int debug_sync);
int mspmv_vec_dot_f64(void *d_temp, size_t *temp_bytes, const double *d_a, const double *d_b, int64_t n, double *d_result,
                      mspmv_stream_t stream, int debug_sync);

/* ---- extension: PRECONDITIONED CONJUGATE GRADIENTS on the device (csrc/mspmv_pcg.hip): A x = b for a symmetric positive definite A in
 * CSR, the loop that mspmv_csrmv_*, mspmv_csric0_* and mspmv_csrsv_* were built for, as one call.  The scalars of the iteration live
 * on the device, the dots are the reduction R above, and the host reads nothing inside the loop unless asked to.
 * THE HANDLE is opaque and OWNS ITS STORAGE, as mspmv_csrsv_plan_t does.  mspmv_pcg_create ALLOCATES (one hipMalloc: the vectors q, p,
 * r, z, mid, the partials, the state block, the diagonal for JACOBI, and the temp storage of mspmv_csrmv_prepared_* in the size its
 * query states), runs mspmv_csrmv_prepare on d_row_offsets, for JACOBI finds every row's diagonal entry (one lane per row) and reads
 * state.bad_diagonal_row back; it is SYNCHRONOUS.  It depends on the pattern alone: new values need no new handle.
 * PRECONDITIONER M, chosen at creation:
 *     MSPMV_PCG_NONE     z = r
 *     MSPMV_PCG_JACOBI   z[i] = r[i] / d[i], d[i] the stored diagonal entry of row i of d_values, taken once per solve.  A pattern with a
 *                        row of no or of more than one diagonal entry (state.bad_diagonal_row >= 0) is refused by the solve.
 *     MSPMV_PCG_FACTOR   z = second^-1 (first^-1 r): mspmv_csrsv_solve_* with first_plan on r into mid, then with second_plan on mid into
 *                        z, alpha = 1, both on d_factor_values with ITS pattern arrays (mspmv_pcg_set_factor; none of them is copied or
 *                        owned: they live as long as solves use them).  IC(0) with the mirror: first = LOWER + NON_UNIT, second = UPPER +
 *                        NON_UNIT on the factor; ILU(0): LOWER + UNIT, UPPER + NON_UNIT; symmetric Gauss-Seidel: the same on A itself.
 * ARITHMETIC, all in the value type T, every operation rounded on its own (no fused multiply-add), nothing flushed to zero:
 *     x = +0.0, r = b            (use_x_as_guess: q = A x by mspmv_csrmv_prepared_*, r[i] = b[i] - q[i])
 *     bb = R(b o b);  rt = (T) rtol, at = (T) atol;  s = fl(fl(rt * rt) * bb), a2 = fl(at * at);  stop2 = s > a2 ? s : a2
 *     rr = R(r o r);  history[0] = rr;  iterations = 0;      rr <= stop2 and rr < +Inf  ->  CONVERGED
 *     z = M^-1 r;  rz = R(r o z);  p = z
 *     iteration k = 1, 2, ...:
 *         q = A p                                     (mspmv_csrmv_prepared_*, alpha = 1, beta = 0)
 *         pq = R(p o q);                              not (pq > 0)  ->  BREAKDOWN: nothing else of this iteration is written,
 *                                                                       iterations stays k - 1
 *         alpha = rz / pq
 *         x[i] = x[i] + fl(alpha * p[i]);   r[i] = r[i] - fl(alpha * q[i])
 *         rr = R(r o r);  history[k] = rr;  iterations = k;      rr <= stop2 and rr < +Inf  ->  CONVERGED;   rr is NaN  ->  BREAKDOWN
 *         z = M^-1 r;  rz' = R(r o z);                not (rz' > 0)  ->  BREAKDOWN
 *         beta = rz' / rz;  rz = rz';  p[i] = z[i] + fl(beta * p[i])
 * (stop2 with a NaN s is a2.  An infinite rr never converges, whatever stop2 is.  With +-Inf in b, bb and rr are +Inf (and stop2 with
 * rtol > 0): the start stays RUNNING, and the solve ends BREAKDOWN by the rules above, which way depends on the signs.  q = A p holds
 * infinities; if the products p[i] * q[i] hold a -Inf or a NaN beside the +Inf, pq is NaN and the solve ends at 0 iterations with x
 * untouched; if every infinite product is +Inf, pq = +Inf passes, alpha = Inf / Inf is NaN, the update fills x and r with NaN and the
 * solve ends at 1 iteration by the NaN rr.)  x, iterations, the status and the history are functions of the inputs alone -- not of
 * check_every, the grid or the alignment of b and x.
 * LAUNCHES: beside the product and the sweeps, an iteration launches state.launches_per_iteration kernels of the solver's own, a
 * function of the preconditioner alone: 5 for NONE and JACOBI (the chunk sums of p o q; a one-workgroup step that folds them and
 * makes alpha; the x and r updates fused with the chunk sums of r o r and, for JACOBI, with z and those of r o z; the step that folds
 * them, tests and makes beta; the p update), 7 for FACTOR (the chunk sums of r o z and their step are launches of their own behind
 * the sweeps).  No workgroup waits on another; there are no floating-point atomics.
 * THE FREEZE: once the status is not RUNNING, every later kernel of the solver's own reads the status and returns: x, the state and
 * the history entries beyond `iterations` stay as they are (the product and the sweeps still run, on scratch).  Hence
 *     check_every = c > 0   iterations are enqueued c at a time; after each group the state block is read back (one small copy, one
 *                           synchronisation) and the call returns at a status other than RUNNING or at max_iterations;
 *     check_every = 0       max_iterations iterations are enqueued and nothing is read back: the call is asynchronous, allocates
 *                           nothing and can be captured in a graph (one stream, no parallel branches);
 * with the same x, iterations, status and history either way.  A solve that ends at max_iterations leaves the status RUNNING.
 * d_history: max_iterations + 1 values of T on the device, or NULL.  d_x and d_b may have any alignment of T; they must not overlap.
 * The matrix arrays passed to a solve hold the pattern the handle was made from.  mspmv_pcg_state reads the state block back on
 * `stream` and waits for it (rows == 0: host only).  debug_sync prints one line per launch (pcg_*_kernel, and the lines of the
 * product and the sweeps) and waits for each.
 * LIMITS, refused before anything is launched or allocated: create -- a NULL `pcg`; rows, nnz < 0; rows + nnz > 2^31 - 65537; rows >
 * 2^30; nnz > 0 with rows == 0; value_bytes not 4 or 8; an unknown kind; NULL d_row_offsets with rows > 0, NULL d_column_indices with
 * nnz > 0.  set_factor -- a NULL handle or plan; a handle of another kind; a plan whose rows differ from the handle's or whose
 * bad_diagonal_row >= 0; NULL factor arrays with nnz > 0.  solve -- a NULL handle or one of the other value type; rtol or atol
 * negative or NaN; max_iterations < 0; check_every < 0; FACTOR without set_factor; JACOBI on a bad diagonal; NULL d_b, d_x or matrix
 * arrays with rows > 0.  rows == 0 touches no device: create gives a valid handle, a solve returns CONVERGED at 0 iterations.
 * Measured on MI355X (tools/pcg_bench.py; profiles/pcg_bench.txt; DESIGN.md 4 "Preconditioned conjugate gradients"), fp64, multicolour
 * order, IC(0), against the torch loop it replaces (two torch.dot, four elementwise passes, one norm read back per iteration): the
 * 5-point Laplacian + 0.01 I on 2000 x 2000, 114 iterations either way, 70.0 ms with check_every = 0 (72.9 ms with 1, 73.7 ms with 8,
 * 70.0 ms replayed from a graph) against 77.6 ms; a 7-point grid of 128^3, 14 iterations, 7.94 ms (8.28 / 8.98 / 7.97 ms) against
 * 8.58 ms: check_every = 8 enqueues 16 iterations there and LOSES 5 %.  Of 0.614 ms per iteration the product is 0.077, the two sweeps
 * 0.464 and the solver's own launches 0.074 ms (the loop's glue: 0.14 ms), which is 416 MB of vector passes at 5.6 TB/s. ---- */
#define MSPMV_PCG_NONE 0
#define MSPMV_PCG_JACOBI 1
#define MSPMV_PCG_FACTOR 2
#define MSPMV_PCG_RUNNING 0
#define MSPMV_PCG_CONVERGED 1
#define MSPMV_PCG_BREAKDOWN 2
typedef struct mspmv_pcg mspmv_pcg_t;
typedef struct mspmv_pcg_state {
    int32_t status;                  /* MSPMV_PCG_RUNNING (also: ended at max_iterations), _CONVERGED, _BREAKDOWN */
    int32_t iterations;              /* updates of x made                                                         */
    int32_t launches_per_iteration;  /* the solver's own, beside the product and the sweeps: the kind alone       */
    int32_t precond_kind;
    int32_t bad_diagonal_row;        /* JACOBI: smallest row with no or more than one stored diagonal; -1         */
    int32_t reserved;
    double rr, bb, stop2, rz;        /* the values of T, widened                                                  */
    uint64_t device_bytes;           /* what the handle holds on the device                                       */
} mspmv_pcg_state_t;
int mspmv_pcg_create(mspmv_pcg_t **pcg, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows, int32_t nnz,
                     int32_t value_bytes, int32_t precond_kind, mspmv_stream_t stream, int debug_sync);
int mspmv_pcg_set_factor(mspmv_pcg_t *pcg, mspmv_csrsv_plan_t *first_plan, mspmv_csrsv_plan_t *second_plan, const void *d_factor_values,
                         const int32_t *d_row_offsets, const int32_t *d_column_indices);
int mspmv_pcg_solve_f32(mspmv_pcg_t *pcg, const float *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                        const float *d_b, float *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                        int32_t check_every, float *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream,
                        int debug_sync);
int mspmv_pcg_solve_f64(mspmv_pcg_t *pcg, const double *d_values, const int32_t *d_row_offsets, const int32_t *d_column_indices,
                        const double *d_b, double *d_x, int32_t use_x_as_guess, double rtol, double atol, int32_t max_iterations,
                        int32_t check_every, double *d_history /* max_iterations + 1 entries, or NULL */, mspmv_stream_t stream,
                        int debug_sync);
int mspmv_pcg_state(mspmv_pcg_t *pcg, mspmv_pcg_state_t *state, mspmv_stream_t stream);
int mspmv_pcg_destroy(mspmv_pcg_t *pcg);

/* ---- introspection (the counterpart of the reference's debug_synchronous
 * launch log, dispatch_spmv_orig.cuh:685-739, as data) ---- */
typedef struct mspmv_launch_info {
    int32_t block_threads;     /* threads per merge tile                      */
    int32_t items_per_thread;  /* merge items per thread                      */
    int32_t tile_items;        /* block_threads * items_per_thread            */
    int32_t num_tiles;         /* ceil((rows+nnz) / tile_items)               */
    int32_t fixup_chunk;       /* carry pairs per fix-up block                */
    int32_t fixup_levels;      /* fix-up launches (0 when num_tiles <= 1)     */
    int32_t flags;             /* option bits in effect: 0 in this library (mspmv_dev.h: MSPMV_TUNE_*) */
    int32_t snap_head_max;     /* > 0: calls of these sizes run ONE launch of row-snapped tiles (tile_kernel_snap;
                                  16-byte aligned arrays assumed, decided again per call):
                                  a tile boundary that falls <= this many nonzeros into a row is moved to the row's
                                  first nonzero, so the per-tile carry that mspmv_debug_read_tiles returns is 0
                                  there; 0: classic tiles                    */
    uint64_t temp_bytes;       /* what the size query returns                 */
    uint64_t coords_offset;    /* byte offsets of regions inside temp         */
    uint64_t carries_offset;
    uint64_t diag_offset;      /* two int32: [0] = tag of the last one-launch call in which a tile gave up waiting for another
                                  workgroup's record and computed the sum itself (debug_sync reports it), [1] = how many such
                                  episodes this temp storage has seen; neither is ever needed for a result */
    uint64_t records_offset;   /* the tagged records of the one-launch kernel: 16 bytes per tile + per group of 64 tiles; every slot a
                                  launch TOUCHED is (0, 0) again once it has ended (slots it never used keep what the buffer held:
                                  tests/test_forward_progress.py zeroes the buffer first; tests/test_record_protocol_model.py) */
} mspmv_launch_info_t;

/* value_bytes = 4 (float) or 8 (double).  The layout of a call of these sizes under the default choice of tile shape; temp_bytes is
 * large enough for any column count (one family of calls picks its shape by the column count too: see mspmv_get_launch_info_cols). */
int mspmv_get_launch_info(int32_t rows, int32_t nnz, int32_t value_bytes,
                          mspmv_launch_info_t *info);
/* The same with the column count, i.e. exactly what mspmv_csrmv_f32 / _f64 (_axpby_*, _prepared_*) run for these sizes when given at
 * least info->temp_bytes of temp storage and 16-byte aligned arrays: a large fp64 matrix (more than 8 M rows + nonzeros, at most 256 MB
 * of CSR arrays) of at most 8 nonzeros per row on average over an x of at most 4 KB -- the reference's --dense=<cols> inputs,
 * cpu_spmv.cpp:581-587 -- takes the small tile shape behind the compact front end (csrc/mspmv_api.hip: skinny_rule); its layout sits
 * BEHIND the default one in temp storage (the offsets reported here are absolute), so temp_bytes is the sum of the two.  Rows of
 * closed lean tiles -- every row of a --dense input -- are summed left to right whatever the shape, so their y does not change by a
 * bit; a long row among them is associated as that shape's tiles cut it (the stated bound holds either way). */
int mspmv_get_launch_info_cols(int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes,
                               mspmv_launch_info_t *info);

/* Copy the tile coordinates ((num_tiles+1) x {row, nonzero}) and the per-tile
 * carry pairs (num_tiles keys + values of value_bytes each) that the last
 * csrmv call left in d_temp back to HOST arrays (synchronises `stream`).
 * They correspond to d_tile_coordinates / d_tile_carry_pairs of
 * dispatch_spmv_orig.cuh:643-646 and are what the parity tests pin against
 * the oracle.  Any output pointer may be NULL.  (Laid out as mspmv_get_launch_info says: not for the calls that pick their
 * tile shape by the column count, mspmv_get_launch_info_cols.)  After a call that took the skinny layout this describes a region that
 * call did not write: read that call's regions at the offsets of mspmv_get_launch_info_cols instead. */
int mspmv_debug_read_tiles(const void *d_temp, int32_t rows, int32_t nnz,
                           int32_t value_bytes, int32_t *h_coords,
                           int32_t *h_carry_keys, void *h_carry_values,
                           mspmv_stream_t stream);

/* What the automatic column-band policy is derived from on the current device: one XCD's L2 in bytes and the number of XCDs
 * (queried from the runtime once per device), and the
 * CU count.  Without a device: the MI355X figures (4 MiB, 8, 256).  Any pointer may be NULL. */
int mspmv_get_device_caches(int64_t *l2_bytes_per_xcd, int32_t *xcds, int32_t *cus);
/* Measuring aid: ONE launch of a bare read stream over d_buf (16-byte aligned; bytes / 16 sixteen-byte loads, 256 x 11 per block
 * like a tile's nonzero stream; nontemporal != 0: non-temporal loads), asynchronous on `stream`.  Timed over a buffer that stays
 * in the Infinity Cache it gives the rate a cache-resident SpMV's algorithmic bytes are to be read against -- the HBM peak is not
 * the bound of such a call (bench.py: `roofline.bound` = "infinity_cache"). */
int mspmv_probe_read_stream(const void *d_buf, size_t bytes, int32_t nontemporal, mspmv_stream_t stream);
/* Column bands (extension).  A large matrix whose columns are spread uniformly over an x of 1.375-10 x one XCD's L2 (fp32;
 * 1.75-9 x in fp64: 5.5-40 / 7-36 MiB on MI355X) is gather-bound at the Infinity-Cache rate when x is gathered as it comes.  Such a call
 * (a CANDIDATE by its sizes: *passes > 1 below) stays stateless, asynchronous and three launches: 64 blocks added to the coordinate
 * launch sample 64 windows of 2048 consecutive column indices, and the tile kernel reads their verdicts and runs either its ordinary
 * body or, when the columns are spread, the banded form:
 *   CLOCK-SCHEDULED BANDS (round 6; csrc/mspmv_tdm.hpp; what the library runs): one pass.  A block sorts its tile's nonzeros by column
 *     band (1 MiB of x) in LDS and gathers band by band, the band "on air" being read off the chip-wide 100 MHz clock -- blocks never
 *     talk to each other, yet at any moment every XCD gathers from a band or two of x, which its L2 keeps.  y is BIT FOR BIT the
 *     classic three-launch result without bands.  C2: 1.22 -> 0.64 ms (fp32), 1.57 -> 1.00 ms (fp64).
 *   COLUMN-BAND PASSES (rounds 2-5; development library only since: mspmv_set_tdm(vb, -1)): the CSR stream read 2-4 times, each pass
 *     multiplying the nonzeros of one band; a re-association of the sums (0.84 / 1.30 ms on C2).
 * Either way results stay within the strict bound and are bitwise reproducible.
 * *passes = how many passes a call of these sizes would be offered (0: none, not a candidate; the aligned, vectorised path is
 * assumed; csrc/mspmv_api.hip: band_passes_for); the device-side verdicts have the last word. */
int mspmv_get_band_passes(int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t *passes);
/* The bands of the clock-scheduled form for a call of these sizes: *bands = how many (0: not a candidate), *band_cols = columns per
 * band (a power of two: 1 MiB of x, widened until 32 bands cover it). */
int mspmv_get_clocked_bands(int32_t rows, int32_t cols, int32_t nnz, int32_t value_bytes, int32_t *bands, int32_t *band_cols);
/* The 64 window verdicts (1 = columns look uniformly spread) the last automatic call left in d_temp -> HOST
 * array of 64 int32 (synchronises `stream`); at least 56 ones select the band passes.  After a call that took the skinny layout this
 * describes a region that call did not write (use the offsets of mspmv_get_launch_info_cols instead). */
int mspmv_debug_band_windows(const void *d_temp, int32_t rows, int32_t nnz, int32_t value_bytes,
                             int32_t *h_verdicts, mspmv_stream_t stream);

/* Opt-in per-kernel timing with hipEvents recorded on the caller's stream
 * around each of the three passes (the counterpart of the reference's
 * GpuTimer, utils.h:624-658, at kernel granularity).  While active, every
 * csrmv call (up to max_calls) records 4 events; mspmv_profile_end
 * synchronises them, returns the number of profiled calls and the AVERAGE
 * milliseconds per call of the search, tile and fix-up passes, and turns
 * profiling off.  Process-global measuring aid for ONE host thread (a mutex
 * keeps concurrent callers from corrupting it, nothing more); calls that only
 * run the coordinate pass (mspmv_csrmv_prepare) and SpMM calls are not recorded. */
int mspmv_profile_begin(int32_t max_calls);
int mspmv_profile_end(int32_t *calls, float *search_ms, float *tile_ms, float *fixup_ms);

/* ---- multi-GPU merge partitioning (new design, the reference
 * has no multi-device code: its claim is README.md:5).  Host-side, 64-bit. --
 *
 * The global merge path (rows + nnz items) is cut at `parts` equally spaced
 * diagonals; part g owns rows-ending [row_split[g], row_split[g+1]) and
 * nonzeros [nz_split[g], nz_split[g+1]).  Seen locally, part g is an ordinary
 * CSR matrix with  local_rows = row_split[g+1]-row_split[g] + 1  rows: its
 * first row may be the tail of a row begun on an earlier part, and its extra
 * LAST row is the open row cut by the part's right boundary, so the local
 * y[local_rows-1] IS the carry for global row row_split[g+1].
 * h_row_offsets: HOST int64 [rows+1].  row_split/nz_split: HOST int64
 * [parts+1]. */
int mspmv_mg_partition(const int64_t *h_row_offsets, int64_t rows, int64_t nnz,
                       int32_t parts, int64_t *row_split, int64_t *nz_split);

/* Fill the local int32 row_offsets (local_rows+1 entries, rebased by
 * -nz_split[g]) of part g. Returns hipErrorInvalidValue if the part does not
 * fit int32. */
int mspmv_mg_local_offsets(const int64_t *h_row_offsets, int64_t rows,
                           int64_t row_begin, int64_t row_end_,
                           int64_t nz_begin, int64_t nz_end_,
                           int32_t *h_local_offsets);

#define MSPMV_MG_MAX_PARTS 64   /* parts a carry exchange can address (one mask bit each) */

/* After the one exchange (all-gather of every part's carry value into
 * d_carries[parts]): add to d_y_local[0] every carry of parts j < part whose
 * key row_split[j+1] equals row_split[part] ... i.e. the rows this part owns
 * that were begun earlier.  keys are given by the HOST array row_split.
 * Deterministic (rank order).  value_bytes = 4 or 8.  parts <= MSPMV_MG_MAX_PARTS
 * (mspmv_mg_partition itself has no such limit). */
int mspmv_mg_apply_carries(void *d_y_local, const void *d_carries,
                           const int64_t *row_split, int32_t parts,
                           int32_t part, int32_t value_bytes,
                           mspmv_stream_t stream);

/* ---- the multi-GPU operator (mspmv_mg_plan_create / _csrmv / _destroy).  New design; the
 * reference has a single --device (utils.h:465-474).
 *
 * A plan drives the parts ONE PROCESS holds of a matrix cut by mspmv_mg_partition:
 *   - all of them (local_parts == parts: single-process form; device_ids may repeat, so a 1-GPU box can run
 *     G parts on one device), or
 *   - some, typically one (one process per GPU; every process passes the same 128-byte id128 that ONE of
 *     them obtained from mspmv_mg_unique_id and shipped by whatever means the launcher has).
 * The caller owns the part's CSR arrays (values, column indices and the local int32 row offsets of
 * mspmv_mg_local_offsets, all on the part's device) and attaches them with mspmv_mg_plan_set_part, which
 * also finds the part's tile coordinates once.  The plan owns one stream per part, the replicated x (one
 * replica per distinct device, mspmv_mg_plan_x -- the caller fills it before the first SpMV), the row-sharded
 * result (mspmv_mg_plan_y: the part's owned rows, row_split[id+1]-row_split[id] entries, followed by one
 * scratch entry) and the exchange buffers.
 *
 * mspmv_mg_csrmv: y = A*x on every local part + the ONE exchange of the boundary-row carries + the owners'
 * adds, all asynchronous on the parts' streams (mspmv_mg_synchronize waits).  Exchange backends:
 *   MSPMV_MG_EXCHANGE_PEER  (single-process form only) events between the parts' streams and one small kernel
 *                           that reads the carries straight out of the peers' memory over xGMI;
 *   MSPMV_MG_EXCHANGE_RCCL  one ncclAllGather of a scalar per part (needs distinct devices; librccl is loaded
 *                           on first use, the library has no link-time dependency on it);
 *   MSPMV_MG_EXCHANGE_IPC   any split of the parts over processes (typically one process per GPU), no collective library:
 *                           after creating its plan every process calls mspmv_mg_plan_ipc_export, the launcher gathers the
 *                           blobs (MPI / torch.distributed / a file -- anything), and every process passes ALL of them to
 *                           mspmv_mg_plan_ipc_import, which opens the peers' x replicas and mailbox blocks through hipIpc.
 *                           A step is then the SpMV + one tiny kernel that writes the carry, tagged with the step number,
 *                           straight into its owner's mailbox (a peer write) and, on the owner, waits for
 *                           the tags of its sources, adds them in part order and acknowledges; the row all-gather is the
 *                           PEER backend's pushes fenced by step-tagged flags.  Nothing on the host, no rendezvous; a
 *                           producer runs at most two steps ahead of its consumer.  Waits are bounded (seconds):
 *                           mspmv_mg_synchronize returns hipErrorLaunchFailure if one ran out.  (HSA_ENABLE_IPC_MODE_LEGACY=0
 *                           where the host driver only supports dmabuf IPC.)  EXPERIMENTAL: exercised with several processes
 *                           sharing ONE device only (no multi-GPU node has run it); a process's local parts must sit on one
 *                           device; the mailboxes need uncached or fine-grained device memory (hipErrorNotSupported otherwise).
 *   MSPMV_MG_EXCHANGE_AUTO  PEER when the process holds every part, else RCCL.
 * mspmv_mg_allgather_rows (square matrices): x <- y on every replica -- PEER: each part
 * pushes its owned rows into every replica (direct peer writes, unpadded); RCCL: grouped ncclBroadcast.
 * Results are deterministic (carries are added in part order) and within the CsrMV tolerance.
 * ON THE BITS: y of a plan = the prepared single-GPU call per part + the fold in part order.  That is: every part's local y
 * (owned rows, then the open row) is what mspmv_csrmv_prepared_f32 / _f64 (alpha 1, beta 0, default tuning) returns on the
 * part's own arrays -- values, local row offsets, column indices as attached, the replica of x, num_cols = cols -- with their
 * alignment (arrays that are not 16-byte aligned run the dword-per-lane classic launches on the coordinates found when the part
 * was attached); then a part that owns at least one row replaces its first entry by (((y[0] + c_s1) + c_s2) + ...), one add in
 * the value type per source, over the earlier parts s1 < s2 < ... whose open row is that row (row_split[s+1] == row_split[id]),
 * c_s being part s's open-row entry.  Parts that own no row take nothing; their open-row entry is their share of the row and
 * stays in mspmv_mg_plan_y.  The same two exceptions as for the hot-column and mixed calls: a part never takes the small tile
 * shape of a large fp64 matrix of short rows over a tiny x (mspmv_get_launch_info_cols), and with a hot-column plan never the
 * column-band passes (tests/test_mg_exact.py holds every backend that one device can run to this).
 * Returns 0 or a hipError_t; hipErrorNotSupported = librccl could not be loaded, hipErrorUnknown = an
 * RCCL call failed (message on stderr). ---- */
typedef struct mspmv_mg_plan mspmv_mg_plan_t;
#define MSPMV_MG_EXCHANGE_AUTO 0
#define MSPMV_MG_EXCHANGE_RCCL 1
#define MSPMV_MG_EXCHANGE_PEER 2
#define MSPMV_MG_EXCHANGE_IPC  3

typedef struct mspmv_mg_info {
    int32_t parts, local_parts, exchange /* backend in effect */, value_bytes, replicas, hot_parts /* local parts running the hot-column plan */;
    int64_t rows, cols;
    uint64_t carry_bytes_per_step;       /* payload of the carry exchange: parts * value_bytes        */
    uint64_t allgather_bytes_per_step;   /* payload of y -> x: rows * value_bytes to every OTHER GPU  */
    uint64_t steps;                      /* mspmv_mg_csrmv calls so far                               */
} mspmv_mg_info_t;

int mspmv_mg_unique_id(void *id128);
int mspmv_mg_plan_create(mspmv_mg_plan_t **plan, int32_t parts, int32_t local_parts, const int32_t *part_ids,
                         const int32_t *device_ids, const int64_t *row_split, const int64_t *nz_split,
                         int64_t cols, int32_t value_bytes, int32_t exchange, const void *id128);
/* IPC backend: blob == NULL -> *blob_bytes = the size of this process's blob; else the blob is written.  _import takes `count`
 * blobs laid out `blob_stride` bytes apart (every process's, its own included, in any order), once. */
int mspmv_mg_plan_ipc_export(mspmv_mg_plan_t *plan, void *blob, size_t *blob_bytes);
int mspmv_mg_plan_ipc_import(mspmv_mg_plan_t *plan, const void *blobs, int32_t count, size_t blob_stride);
int mspmv_mg_plan_set_part(mspmv_mg_plan_t *plan, int32_t local_index, const void *d_values,
                           const int32_t *d_local_row_offsets, const int32_t *d_column_indices);
void *mspmv_mg_plan_x(mspmv_mg_plan_t *plan, int32_t local_index);
void *mspmv_mg_plan_y(mspmv_mg_plan_t *plan, int32_t local_index);
mspmv_stream_t mspmv_mg_plan_stream(mspmv_mg_plan_t *plan, int32_t local_index);
int mspmv_mg_plan_info(mspmv_mg_plan_t *plan, mspmv_mg_info_t *info);
/* The hot-column plan of the parts (above: columns renumbered by reference count, built once per part in plan-owned storage of
 * 4 * local_nnz + 16 * cols bytes; mspmv_mg_csrmv permutes x into the part's numbering before its SpMV):
 *   enable < 0   AUTOMATIC, the default of every plan: decided per part when its matrix is attached (mspmv_mg_plan_set_part) -- a
 *                part gets the plan when the x replica is beyond the 256 MB Infinity Cache (cols * value_bytes) AND the on-device
 *                sample of its column indices says the columns come back (mspmv_csrmv_hotcols_skew: ~1 M sampled references touch 15-80 % of
 *                the distinct lines of x a uniform draw would, >= 256 of 512 windows spanning most of x): config 5, every part 33 -> 21 ms-equivalent.  Uniformly
 *                spread columns, stencils / bands, an x that fits the cache, or a part that cannot afford the storage: no plan.
 *   enable > 0   always (every local part; hipErrorOutOfMemory if one cannot)
 *   enable == 0  never; releases the storage
 * y is bit for bit the same either way (parts that would take the column-band passes excepted, as above); mspmv_mg_plan_info reports
 * how many local parts run it (hot_parts).  May be called before the parts' matrices are attached: the mode is then applied by
 * mspmv_mg_plan_set_part, which -- in the automatic and "always" modes -- runs a SYNCHRONOUS probe / build on the part's stream and
 * may allocate the storage above; under "always" a part that cannot afford it makes set_part return hipErrorOutOfMemory with the
 * matrix attached and no plan (the part runs the ordinary call). */
int mspmv_mg_plan_hot_columns(mspmv_mg_plan_t *plan, int32_t enable);
/* Milliseconds the EXCHANGE of the last mspmv_mg_csrmv took on local part `local_index` -- hipEvents on the part's stream right after
 * its SpMV and right after its share of the exchange (the all-gather / the peers' events, the owner's add): what a step costs beyond
 * its kernels, measured rather than inferred; includes the time this part waited for slower parts.  Synchronises with the step. */
int mspmv_mg_plan_exchange_ms(mspmv_mg_plan_t *plan, int32_t local_index, float *ms);
int mspmv_mg_csrmv(mspmv_mg_plan_t *plan);
int mspmv_mg_allgather_rows(mspmv_mg_plan_t *plan);
int mspmv_mg_synchronize(mspmv_mg_plan_t *plan);
int mspmv_mg_plan_destroy(mspmv_mg_plan_t *plan);

#ifdef __cplusplus
}
#endif
#endif /* MSPMV_H_ */
