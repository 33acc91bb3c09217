// rank_large_kernels.hpp — launch interface of the true-rank elimination for generations beyond LDS (rank_large.hip;
// internal to librlnc_hip).
//
// A third producer of {T, status, rank} from RrefParams, with rank.hip's semantics (RLNC_RANK_MODE_TRUE;
// include/rlnc_hip.h, "Rank mode") and rank.hip's fields of RrefParams (the batch form only: objs must be null).  The
// per-object state lives in a device workspace instead of LDS, and the pieces are taken B at a time, three launches
// per block plus one at the end (rank_large.hip), so one object is spread over many workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace rlnc {

constexpr int kLargeMaxK = 4096;   // the final launch keeps two k-entry int arrays in LDS
constexpr int kLargeMaxM = 8192;
constexpr int kLargeMaxB = 32;     // pieces per block
constexpr size_t kLargeStepFixedBytes = 8192 + 1024;  // the block step's LDS beside X: multiplier table, small arrays

// dwords of one stored row [c | e]: D = ceil(k/4) + ceil(m/4)
__host__ __device__ inline int large_row_dwords(int k, int m) { return ((k + 3) >> 2) + ((m + 3) >> 2); }

// pieces per block: the largest multiple of 4, at most 32, with 8192 + 1024 + B·4·D <= 160 KiB (the block step keeps
// the block's B rows in LDS beside the 8 KiB multiplier table and 1 KiB of pivot / quotient arrays); 0 = the shape is
// outside the limits (k <= 4096, m <= 8192, B >= 4)
__host__ __device__ inline int large_block(int64_t k, int64_t m) {
    if (k <= 0 || m <= 0 || k > kLargeMaxK || m > kLargeMaxM) return 0;
    const size_t row = size_t(large_row_dwords(int(k), int(m))) * 4;
    const size_t fit = (kRrefMaxLds - kLargeStepFixedBytes) / row;
    const int B = int(fit > size_t(kLargeMaxB) ? size_t(kLargeMaxB) : fit) & ~3;
    return B >= 4 ? B : 0;
}

// one object's workspace, in dwords (every array starts on a multiple of 4 dwords):
//   state[4] {rank, rank before the last block, pieces answered, -}, piv[k], St[m], Q[k][32 bytes], X[B][D], R[k][D]
__host__ __device__ inline size_t up4(size_t v) { return (v + 3) & ~size_t(3); }
struct LargeLayout {
    size_t piv, st, q, x, r, total;
    int D, B;
};
__host__ __device__ inline LargeLayout large_layout(int k, int m) {
    LargeLayout l{};
    l.D = large_row_dwords(k, m);
    l.B = large_block(k, m);
    l.piv = 4;
    l.st = up4(l.piv + size_t(k));
    l.q = up4(l.st + size_t(m));
    l.x = l.q + size_t(k) * (kLargeMaxB / 4);
    l.r = up4(l.x + size_t(l.B) * size_t(l.D));
    l.total = up4(l.r + size_t(k) * size_t(l.D));
    return l;
}

// bytes of the workspace of nobj objects; 0 = outside the limits
inline size_t rank_large_workspace_bytes(size_t k, size_t m, size_t nobj) {
    if (nobj == 0 || nobj > 0x7FFFFFFF || large_block(int64_t(k > 0x7FFFFFFF ? 0 : k), int64_t(m > 0x7FFFFFFF ? 0 : m)) == 0)
        return 0;
    return nobj * large_layout(int(k), int(m)).total * 4;
}

// 3·ceil(m / B) + 1 launches on s (reduce, block step, update per block; the T / status / rank writer), no host
// synchronisation.  ws: rank_large_workspace_bytes(k, m, n_obj) bytes, 16-byte aligned, used until the launches ran.
// hipErrorInvalidValue for a shape outside the limits, a ragged table or a short workspace.
hipError_t launch_rank_large(const RrefParams &p, void *ws, size_t ws_bytes, hipStream_t s);

}  // namespace rlnc
