// device_spmv.hpp -- header-only C++ shim with the reference's spelling over the
// C ABI of include/mspmv.h, so that a driver written against
//     cub::DeviceSpmv::CsrMV(d_temp_storage, temp_storage_bytes, d_values,
//         d_row_offsets, d_column_indices, d_vector_x, d_vector_y,
//         num_rows, num_cols, num_nonzeros, stream, debug_synchronous)
// (reference cub/device/device_spmv.cuh:129-145) keeps its source shape:
// replace `cub::` by `mspmv::` and cudaStream_t by hipStream_t.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mspmv.h"

namespace mspmv {

struct DeviceSpmv {
    static hipError_t CsrMV(void *d_temp_storage, size_t &temp_storage_bytes, const float *d_values,
                            const int *d_row_offsets, const int *d_column_indices, const float *d_vector_x,
                            float *d_vector_y, int num_rows, int num_cols, int num_nonzeros, hipStream_t stream = 0,
                            bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                            d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                            num_nonzeros, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    static hipError_t CsrMV(void *d_temp_storage, size_t &temp_storage_bytes, const double *d_values,
                            const int *d_row_offsets, const int *d_column_indices, const double *d_vector_x,
                            double *d_vector_y, int num_rows, int num_cols, int num_nonzeros, hipStream_t stream = 0,
                            bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                            d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                            num_nonzeros, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    // y = alpha*A*x + beta*y (extension; the reference's --alpha/--beta are honoured only by its SpmvGold)
    static hipError_t CsrMV(void *d_temp_storage, size_t &temp_storage_bytes, const float *d_values,
                            const int *d_row_offsets, const int *d_column_indices, const float *d_vector_x,
                            float *d_vector_y, int num_rows, int num_cols, int num_nonzeros, float alpha, float beta,
                            hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_axpby_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                                  d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                                  num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                  debug_synchronous ? 1 : 0);
    }

    static hipError_t CsrMV(void *d_temp_storage, size_t &temp_storage_bytes, const double *d_values,
                            const int *d_row_offsets, const int *d_column_indices, const double *d_vector_x,
                            double *d_vector_y, int num_rows, int num_cols, int num_nonzeros, double alpha, double beta,
                            hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_axpby_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                                  d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                                  num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                  debug_synchronous ? 1 : 0);
    }

    // ---- iterated SpMV on one matrix (extension): find the tile coordinates once ...
    template <typename ValueT>
    static hipError_t CsrMVPrepare(void *d_temp_storage, size_t &temp_storage_bytes, const int *d_row_offsets, int num_rows,
                                   int num_nonzeros, hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_prepare(d_temp_storage, &temp_storage_bytes, d_row_offsets, num_rows, num_nonzeros,
                                                (int) sizeof(ValueT), (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    // ... then y = alpha*A*x + beta*y without the coordinate pass (d_temp_storage as left by CsrMVPrepare)
    static hipError_t CsrMVPrepared(void *d_temp_storage, size_t &temp_storage_bytes, const float *d_values,
                                    const int *d_row_offsets, const int *d_column_indices, const float *d_vector_x,
                                    float *d_vector_y, int num_rows, int num_cols, int num_nonzeros, float alpha = 1.f,
                                    float beta = 0.f, hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_prepared_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                                     d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                                     num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                     debug_synchronous ? 1 : 0);
    }
    static hipError_t CsrMVPrepared(void *d_temp_storage, size_t &temp_storage_bytes, const double *d_values,
                                    const int *d_row_offsets, const int *d_column_indices, const double *d_vector_x,
                                    double *d_vector_y, int num_rows, int num_cols, int num_nonzeros, double alpha = 1.0,
                                    double beta = 0.0, hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_prepared_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets,
                                                     d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
                                                     num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                     debug_synchronous ? 1 : 0);
    }

    // ---- mixed precision (extension): the matrix values stored narrow -- float with double x / y, bf16 (uint16_t: the upper half of
    //      a float) with float x / y --, y = alpha*A*x + beta*y in the vectors' type; bit for bit the wide call on the widened values
    //      (mspmv.h says when).  prepared: d_temp_storage as left by CsrMVPrepare<type of x>.
    static hipError_t CsrMVMixed(void *d_temp_storage, size_t &temp_storage_bytes, const float *d_values,
                                 const int *d_row_offsets, const int *d_column_indices, const double *d_vector_x,
                                 double *d_vector_y, int num_rows, int num_cols, int num_nonzeros, double alpha = 1.0,
                                 double beta = 0.0, hipStream_t stream = 0, bool debug_synchronous = false, bool prepared = false)
    {
        return (hipError_t) (prepared ? mspmv_csrmv_mixed_prepared_f32_f64 : mspmv_csrmv_mixed_f32_f64)(
            d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
            num_nonzeros, alpha, beta, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    static hipError_t CsrMVMixed(void *d_temp_storage, size_t &temp_storage_bytes, const uint16_t *d_values,
                                 const int *d_row_offsets, const int *d_column_indices, const float *d_vector_x,
                                 float *d_vector_y, int num_rows, int num_cols, int num_nonzeros, float alpha = 1.f,
                                 float beta = 0.f, hipStream_t stream = 0, bool debug_synchronous = false, bool prepared = false)
    {
        return (hipError_t) (prepared ? mspmv_csrmv_mixed_prepared_bf16_f32 : mspmv_csrmv_mixed_bf16_f32)(
            d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices, d_vector_x, d_vector_y, num_rows, num_cols,
            num_nonzeros, alpha, beta, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    // ---- addition (extension): C = alpha*A + beta*B for two CSR matrices whose rows are sorted by column without repeated columns;
    //      C's arrays are sized for nnz_a + nnz_b, *d_num_nonzeros_c (device) receives the count of the union; all three value
    //      pointers nullptr: structure only (mspmv.h: mspmv_csr_add_*)
    static hipError_t CsrAdd(void *d_temp_storage, size_t &temp_storage_bytes, int num_rows, int num_cols, float alpha, const float *d_values_a,
                             const int *d_row_offsets_a, const int *d_column_indices_a, int num_nonzeros_a, float beta,
                             const float *d_values_b, const int *d_row_offsets_b, const int *d_column_indices_b, int num_nonzeros_b,
                             float *d_values_c, int *d_row_offsets_c, int *d_column_indices_c, int *d_num_nonzeros_c,
                             hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csr_add_f32(d_temp_storage, &temp_storage_bytes, num_rows, num_cols, alpha, d_values_a, d_row_offsets_a,
                                              d_column_indices_a, num_nonzeros_a, beta, d_values_b, d_row_offsets_b, d_column_indices_b,
                                              num_nonzeros_b, d_values_c, d_row_offsets_c, d_column_indices_c, d_num_nonzeros_c,
                                              (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    static hipError_t CsrAdd(void *d_temp_storage, size_t &temp_storage_bytes, int num_rows, int num_cols, double alpha, const double *d_values_a,
                             const int *d_row_offsets_a, const int *d_column_indices_a, int num_nonzeros_a, double beta,
                             const double *d_values_b, const int *d_row_offsets_b, const int *d_column_indices_b, int num_nonzeros_b,
                             double *d_values_c, int *d_row_offsets_c, int *d_column_indices_c, int *d_num_nonzeros_c,
                             hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csr_add_f64(d_temp_storage, &temp_storage_bytes, num_rows, num_cols, alpha, d_values_a, d_row_offsets_a,
                                              d_column_indices_a, num_nonzeros_a, beta, d_values_b, d_row_offsets_b, d_column_indices_b,
                                              num_nonzeros_b, d_values_c, d_row_offsets_c, d_column_indices_c, d_num_nonzeros_c,
                                              (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    // ---- prepared band-major plan (extension, opt-in): build once, multiply many times
    template <typename ValueT>
    static hipError_t PlanSize(int num_rows, int num_cols, int num_nonzeros, int bands, size_t &plan_bytes, int &bands_used)
    {
        int32_t used = 0;
        const hipError_t e = (hipError_t) mspmv_csrmv_plan_size(num_rows, num_cols, num_nonzeros, (int) sizeof(ValueT), bands, &plan_bytes, &used);
        bands_used = used;
        return e;
    }
    static hipError_t PlanBuild(void *d_plan, size_t plan_bytes, const float *d_values, const int *d_row_offsets,
                                const int *d_column_indices, int num_rows, int num_cols, int num_nonzeros, int bands,
                                hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_plan_build_f32(d_plan, plan_bytes, d_values, d_row_offsets, d_column_indices, num_rows, num_cols,
                                                       num_nonzeros, bands, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    static hipError_t PlanBuild(void *d_plan, size_t plan_bytes, const double *d_values, const int *d_row_offsets,
                                const int *d_column_indices, int num_rows, int num_cols, int num_nonzeros, int bands,
                                hipStream_t stream = 0, bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_plan_build_f64(d_plan, plan_bytes, d_values, d_row_offsets, d_column_indices, num_rows, num_cols,
                                                       num_nonzeros, bands, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    static hipError_t PlanApply(void *d_plan, size_t plan_bytes, const float *d_vector_x, float *d_vector_y, int num_rows, int num_cols,
                                int num_nonzeros, int bands, float alpha = 1.f, float beta = 0.f, hipStream_t stream = 0,
                                bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_plan_apply_f32(d_plan, plan_bytes, d_vector_x, d_vector_y, num_rows, num_cols, num_nonzeros, bands,
                                                       alpha, beta, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    static hipError_t PlanApply(void *d_plan, size_t plan_bytes, const double *d_vector_x, double *d_vector_y, int num_rows, int num_cols,
                                int num_nonzeros, int bands, double alpha = 1.0, double beta = 0.0, hipStream_t stream = 0,
                                bool debug_synchronous = false)
    {
        return (hipError_t) mspmv_csrmv_plan_apply_f64(d_plan, plan_bytes, d_vector_x, d_vector_y, num_rows, num_cols, num_nonzeros, bands,
                                                       alpha, beta, (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    // ---- transpose (extension): A^T as CSR on the device, stable (d_values == d_values_t == nullptr: structure only) ...
    template <typename ValueT>
    static hipError_t CsrTranspose(void *d_temp_storage, size_t &temp_storage_bytes, const ValueT *d_values, const int *d_row_offsets,
                                   const int *d_column_indices, int num_rows, int num_cols, int num_nonzeros, ValueT *d_values_t,
                                   int *d_row_offsets_t, int *d_column_indices_t, int *d_permutation = nullptr, hipStream_t stream = 0,
                                   bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_csr_transpose_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices, num_rows,
                                                        num_cols, num_nonzeros, d_values_t, d_row_offsets_t, d_column_indices_t, d_permutation,
                                                        (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_csr_transpose_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices, num_rows,
                                                        num_cols, num_nonzeros, d_values_t, d_row_offsets_t, d_column_indices_t, d_permutation,
                                                        (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    // ... new values on the same pattern: values_t[j] = values[permutation[j]]
    template <typename ValueT>
    static hipError_t CsrTransposeValues(const ValueT *d_values, const int *d_permutation, ValueT *d_values_t, int num_nonzeros,
                                         hipStream_t stream = 0, bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_csr_transpose_values_f32(d_values, d_permutation, d_values_t, num_nonzeros, (mspmv_stream_t) stream,
                                                               debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_csr_transpose_values_f64(d_values, d_permutation, d_values_t, num_nonzeros, (mspmv_stream_t) stream,
                                                               debug_synchronous ? 1 : 0);
    }
    // ... stateless y = alpha*A^T*x + beta*y (x: num_rows entries, y: num_cols): transposes into temp storage every call
    template <typename ValueT>
    static hipError_t CsrMVTranspose(void *d_temp_storage, size_t &temp_storage_bytes, const ValueT *d_values, const int *d_row_offsets,
                                     const int *d_column_indices, const ValueT *d_vector_x, ValueT *d_vector_y, int num_rows, int num_cols,
                                     int num_nonzeros, ValueT alpha = 1, ValueT beta = 0, hipStream_t stream = 0,
                                     bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_csrmv_transpose_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices,
                                                          d_vector_x, d_vector_y, num_rows, num_cols, num_nonzeros, alpha, beta,
                                                          (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_csrmv_transpose_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices,
                                                          d_vector_x, d_vector_y, num_rows, num_cols, num_nonzeros, alpha, beta,
                                                          (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }

    // ---- COO (extension): CSR built on the device from unsorted triples -- the entries sorted stably by (row, column), duplicates kept
    // (d_values == d_values_csr == nullptr: structure only) ...
    template <typename ValueT>
    static hipError_t CooToCsr(void *d_temp_storage, size_t &temp_storage_bytes, const ValueT *d_values, const int *d_row_indices,
                               const int *d_column_indices, int num_rows, int num_cols, int num_nonzeros, int *d_row_offsets,
                               int *d_column_indices_csr, ValueT *d_values_csr, int *d_permutation = nullptr, hipStream_t stream = 0,
                               bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_coo_to_csr_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_indices, d_column_indices, num_rows,
                                                     num_cols, num_nonzeros, d_row_offsets, d_column_indices_csr, d_values_csr, d_permutation,
                                                     (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_coo_to_csr_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_indices, d_column_indices, num_rows,
                                                     num_cols, num_nonzeros, d_row_offsets, d_column_indices_csr, d_values_csr, d_permutation,
                                                     (mspmv_stream_t) stream, debug_synchronous ? 1 : 0);
    }
    // ... new values on the same pattern: values_csr[j] = values[permutation[j]]
    template <typename ValueT>
    static hipError_t CooToCsrValues(const ValueT *d_values, const int *d_permutation, ValueT *d_values_csr, int num_nonzeros,
                                     hipStream_t stream = 0, bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_coo_to_csr_values_f32(d_values, d_permutation, d_values_csr, num_nonzeros, (mspmv_stream_t) stream,
                                                            debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_coo_to_csr_values_f64(d_values, d_permutation, d_values_csr, num_nonzeros, (mspmv_stream_t) stream,
                                                            debug_synchronous ? 1 : 0);
    }
    // ... duplicates of a CSR with sorted rows merged, each run added left to right; the new count goes to *d_num_nonzeros_out (device)
    template <typename ValueT>
    static hipError_t CsrSumDuplicates(void *d_temp_storage, size_t &temp_storage_bytes, const ValueT *d_values, const int *d_row_offsets,
                                       const int *d_column_indices, int num_rows, int num_cols, int num_nonzeros, ValueT *d_values_out,
                                       int *d_row_offsets_out, int *d_column_indices_out, int *d_num_nonzeros_out, hipStream_t stream = 0,
                                       bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_csr_sum_duplicates_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices,
                                                             num_rows, num_cols, num_nonzeros, d_values_out, d_row_offsets_out,
                                                             d_column_indices_out, d_num_nonzeros_out, (mspmv_stream_t) stream,
                                                             debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_csr_sum_duplicates_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_offsets, d_column_indices,
                                                             num_rows, num_cols, num_nonzeros, d_values_out, d_row_offsets_out,
                                                             d_column_indices_out, d_num_nonzeros_out, (mspmv_stream_t) stream,
                                                             debug_synchronous ? 1 : 0);
    }
    // ... stateless y = alpha*A*x + beta*y from unsorted triples: builds the CSR into temp storage every call
    template <typename ValueT>
    static hipError_t CooMV(void *d_temp_storage, size_t &temp_storage_bytes, const ValueT *d_values, const int *d_row_indices,
                            const int *d_column_indices, const ValueT *d_vector_x, ValueT *d_vector_y, int num_rows, int num_cols,
                            int num_nonzeros, ValueT alpha = 1, ValueT beta = 0, hipStream_t stream = 0, bool debug_synchronous = false)
    {
        static_assert(std::is_same<ValueT, float>::value || std::is_same<ValueT, double>::value, "float or double");
        if constexpr (std::is_same<ValueT, float>::value)
            return (hipError_t) mspmv_coomv_f32(d_temp_storage, &temp_storage_bytes, d_values, d_row_indices, d_column_indices, d_vector_x,
                                                d_vector_y, num_rows, num_cols, num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                debug_synchronous ? 1 : 0);
        else
            return (hipError_t) mspmv_coomv_f64(d_temp_storage, &temp_storage_bytes, d_values, d_row_indices, d_column_indices, d_vector_x,
                                                d_vector_y, num_rows, num_cols, num_nonzeros, alpha, beta, (mspmv_stream_t) stream,
                                                debug_synchronous ? 1 : 0);
    }
};

}  // namespace mspmv
