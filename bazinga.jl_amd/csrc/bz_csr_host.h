// bz_csr_host.h — host-side CSR helpers of the sparse kinds (no HIP, no device types: a stand-alone program can include it,
// tests/test_csr_host.py does).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bz {

using std::size_t;

// The transpose of a validated CSR matrix (rows x cols; rp[0] = 0, rp non-decreasing, every column index in [0, cols)) by a
// stable counting sort: the entries of a column come out in ascending row order, and those of one row in their stored
// order.  A' of the sparse constraint and A_f' of the sparse least squares are built with it, once, at creation.
template <class T>
void csr_transpose(int64_t rows, int64_t cols, const std::vector<int64_t>& rp, const std::vector<int32_t>& col,
                   const std::vector<T>& val, std::vector<int64_t>& tp, std::vector<int32_t>& tcol, std::vector<T>& tval) {
    const int64_t nnz = rp[(size_t)rows];
    tp.assign((size_t)cols + 1, 0);
    for (int64_t k = 0; k < nnz; ++k) ++tp[(size_t)col[(size_t)k] + 1];
    for (int64_t j = 0; j < cols; ++j) tp[(size_t)j + 1] += tp[(size_t)j];
    tcol.resize((size_t)nnz); tval.resize((size_t)nnz);
    std::vector<int64_t> next(tp.begin(), tp.end() - 1);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t k = rp[(size_t)r]; k < rp[(size_t)r + 1]; ++k) {
            const int64_t at = next[(size_t)col[(size_t)k]]++;
            tcol[(size_t)at] = (int32_t)r; tval[(size_t)at] = val[(size_t)k];
        }
}

}  // namespace bz
