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

#include "rref.hpp"

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

// ---- Decode streams (include/rlnc_hip.h, rlnc_decode_stream_*): the same state kept by the caller between calls ----
// The state buffer has the workspace's layout; its fourth state word, spare in the one-shot form, holds the target of
// the push in flight (pieces answered after it).  A push is one latch launch (target = min(max(avail, done), m, done +
// max_new) per object), ceil(min(max_new, m) / B) blocks of the same three launches in their stream form -- each
// object's block is pieces done .. min(done + B, target) - 1, read from its state; an object with nothing left returns
// at once -- and, when asked for, one launch that copies out every object's rank and done.  The state after a push is
// the one-piece-at-a-time model's after the same pieces (rank_large.hip: the proof is per block and does not care
// where a block starts), so it does not depend on how the pieces were split over pushes.  Generations that fit LDS have
// a one-launch form of the push besides (rank_stream_kernels.hpp) on the same state buffer.
inline size_t rank_stream_state_bytes(size_t k, size_t m, size_t nobj) { return rank_large_workspace_bytes(k, m, nobj); }
// rank, answered and target of every object to 0 (one launch); hipErrorInvalidValue as launch_rank_large
hipError_t launch_rank_stream_init(int k, int m, int n_obj, void *state, size_t state_bytes, hipStream_t s);
// p: pieces, obj_stride, piece_stride, k, m, n_obj.  avail int32 [n_obj] is read by the latch launch only; rank /
// answered int32 [n_obj], each optional.  No synchronisation, no workspace beside the state.
hipError_t launch_rank_stream_push(const RrefParams &p, void *state, size_t state_bytes, const int32_t *avail,
                                   int max_new, int32_t *rank, int32_t *answered, hipStream_t s);
// p: k, m, n_obj, T, T_obj, status, rank (each output optional): launch_rank_large's last launch on the stream's
// state, RLNC_STATUS_PENDING for the slots not yet answered.  The state is only read.
hipError_t launch_rank_stream_snapshot(const RrefParams &p, const void *state, size_t state_bytes, hipStream_t s);

}  // namespace rlnc
