// sparse_kernels.hpp — launch interface of the sparse product (sparse.hip; internal to librlnc_hip).
//
// The sending side's operator for sparse coding vectors (include/rlnc_hip.h, "Sparse coding vectors"): a coefficient
// matrix given as w (index, value) entries per output row instead of n_in dense bytes,
//   out[o][i][0:width) = XOR_t val[o][i][t] · in[o][idx[o][i][t]][0:width)      (t < w)
// and, with hdr, the expanded dense row hdr[o][i][0:n_in) (hdr[j] = XOR of val[t] over the t with idx[t] == j).  An
// entry with val == 0 or an index outside [0, n_in) contributes nothing and no source row is read for it.
// The kernel needs no workspace and no LDS; one launch, and a second one for a row's last partial 16-byte slot.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rlnc {

// Byte strides everywhere; idx 4-byte aligned with strides that are multiples of 4 (the C ABI checks it).  w == 0:
// idx / val are not read (may be null) and every output row, header included, is zero.
struct SparseMatmulParams {
    const uint8_t *in;
    int64_t in_obj, in_row;
    const int32_t *idx;
    int64_t idx_obj, idx_row;
    const uint8_t *val;
    int64_t val_obj, val_row;
    uint8_t *out;
    int64_t out_obj, out_row;
    uint8_t *hdr;  // optional
    int64_t hdr_obj, hdr_row;
    int n_out, n_in, w, n_obj;
    int64_t width;
};

constexpr int kSparseRows = 4;  // output rows per workgroup

// workgroups of the launch: n_obj x ceil(n_out / kSparseRows) x ceil(width / 4 KiB); launch_sparse_matmul fails with
// hipErrorInvalidValue above 2^31 - 1
int64_t sparse_matmul_workgroups(const SparseMatmulParams &p);
hipError_t launch_sparse_matmul(const SparseMatmulParams &p, hipStream_t s);

}  // namespace rlnc
