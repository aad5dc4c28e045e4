/* mspmv_fill.h -- level-of-fill patterns on the device: the symbolic phase of ILU(p) / IC(p) (libmspmv_fill.so; plain C99).
 *
 * A library of its own beside libmspmv.so, as mspmv_krylov.h and mspmv_gmres.h are: mspmv.h, what libmspmv.so exports and
 * mspmv_version() stay as they are.  It calls nothing of libmspmv.so; it is built from the same radix and scan pieces
 * (csrc/mspmv_radix.hpp, mspmv_coo.hpp, mspmv_scan.hpp) that the COO build, the sparse product and the permutation use.  The numeric
 * kernels are those of mspmv.h: mspmv_csrilu0_* / mspmv_csric0_* and the sweeps of mspmv_csrsv_* run on the filled pattern unchanged.
 *
 * ---- DEFINITION (a function of the pattern and p alone).  Input: a square pattern in canonical CSR (rows sorted by column, no
 * column twice), rows <= 2^30, and a level p, 0 <= p <= 32.  The diagonal may be missing anywhere; it is not added.
 * Every stored entry (i, j) has lev(i, j) = 0, every other position lev = +inf, and
 *     lev(i, j) = min( lev(i, j), min over m < min(i, j) of lev(i, m) + lev(m, j) + 1 ).
 * The filled pattern F_p holds every (i, j) with lev(i, j) <= p, in canonical CSR.  Beside it, for every entry e of F_p:
 *     levels[e] = lev of the entry;   source[e] = the entry's index in A's arrays, -1 for a fill entry.
 * F_0 is A: the same offsets and columns, levels all 0, source the identity.  This is the pattern of the classical row-by-row
 * symbolic ILU(p) (row i takes its entries k < i in ascending order, fill included, and merges row k's entries j > k at level
 * lev(i, k) + lev(k, j) + 1, keeping the minimum and dropping levels above p): tests/fill_model.py is that algorithm.
 * Every column index must lie in [0, rows) and the offsets must not decrease; a column outside that range is given no pairs, so
 * nothing is read through it, but the result is then undefined.
 * SCHEME (csrc/mspmv_fill.hip): one round per level l = 1 .. p, after which the state is F_l.  A round pairs every entry below the
 * diagonal, (i, m), with every entry of row m right of the diagonal, keeps the pairs whose levels add up to l - 1 (a flag per pair,
 * scanned: the others are written nowhere), sorts the state's entries and the kept pairs stably by (row, column) and compacts runs
 * of equal position to their head, which holds the smallest level.  The pairs are cut into tiles of 2048 whatever the row lengths,
 * and no lane walks a row or a run.  Integer arithmetic only; no atomics on global memory; no workgroup waits on
 * another.  A round with no pair at all ends the analysis.
 * THE HANDLE is opaque and OWNS ITS STORAGE, as mspmv_csr_color_t does.  mspmv_csr_fill_create ALLOCATES (hipMalloc: scratch per
 * round, freed before it returns; the four arrays, kept until mspmv_csr_fill_destroy), is SYNCHRONOUS and reads 16 bytes back per
 * round.  debug_sync prints one line per launch.  The input arrays are only read.
 * REFUSALS (hipErrorInvalidValue, before anything is launched, *fill left NULL): fill == NULL; negative rows or nnz; rows > 2^30;
 * rows + nnz > 2^31 - 65537; level outside [0, 32]; nnz > 0 with rows == 0; a NULL d_row_offsets with rows > 0 or a NULL
 * d_column_indices with nnz > 0.
 * THE COUNT LIMIT.  A round whose rows + entries + pairs (all pairs, before any is dropped for its level) exceed 2^31 - 65537 is
 * refused FROM THE COUNT, read back as 8 bytes before anything proportional to it is allocated: hipErrorInvalidValue, *fill NULL,
 * everything allocated so far freed.  nnz_filled + rows is below every round's count, so a fill that is returned is within the limit.
 * rows == 0 touches no device and gives a valid handle of no entries, whose four arrays are NULL.
 * mspmv_csr_fill_values_*: d_values_filled[e] = source[e] >= 0 ? d_values[source[e]] : +0.0 -- values moved, never recomputed (NaN,
 * Inf and -0.0 arrive as they are).  ONE launch; it allocates nothing, reads nothing back and can be captured in a graph.
 * d_values_filled (nnz_filled entries) may have any alignment of T and must not overlap d_values. ---- */
#ifndef MSPMV_FILL_H
#define MSPMV_FILL_H

#include "mspmv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSPMV_CSR_FILL_MAX_LEVEL 32
typedef struct mspmv_csr_fill mspmv_csr_fill_t;
typedef struct mspmv_csr_fill_info {
    int32_t rows, nnz;         /* the pattern given                                                    */
    int32_t level;             /* p                                                                    */
    int32_t nnz_filled;        /* entries of F_p                                                       */
    int32_t max_level;         /* the largest level present (0 for a pattern of no entries)            */
    int32_t reserved;
    uint64_t device_bytes;     /* what the handle holds on the device                                  */
} mspmv_csr_fill_info_t;
int mspmv_csr_fill_create(mspmv_csr_fill_t **fill, const int32_t *d_row_offsets, const int32_t *d_column_indices, int32_t rows,
                          int32_t nnz, int32_t level, mspmv_stream_t stream, int debug_sync);
int mspmv_csr_fill_info(const mspmv_csr_fill_t *fill, mspmv_csr_fill_info_t *info);
const int32_t *mspmv_csr_fill_row_offsets(const mspmv_csr_fill_t *fill);     /* device, rows + 1 entries   */
const int32_t *mspmv_csr_fill_column_indices(const mspmv_csr_fill_t *fill);  /* device, nnz_filled entries */
const int32_t *mspmv_csr_fill_levels(const mspmv_csr_fill_t *fill);          /* device, nnz_filled entries */
const int32_t *mspmv_csr_fill_source(const mspmv_csr_fill_t *fill);          /* device, nnz_filled entries */
int mspmv_csr_fill_values_f32(const mspmv_csr_fill_t *fill, const float *d_values, float *d_values_filled, mspmv_stream_t stream,
                              int debug_sync);
int mspmv_csr_fill_values_f64(const mspmv_csr_fill_t *fill, const double *d_values, double *d_values_filled, mspmv_stream_t stream,
                              int debug_sync);
int mspmv_csr_fill_destroy(mspmv_csr_fill_t *fill);

#ifdef __cplusplus
}
#endif
#endif /* MSPMV_FILL_H */
