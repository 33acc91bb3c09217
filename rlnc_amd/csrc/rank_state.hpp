// rank_state.hpp — the per-object state buffer of the true-rank elimination beyond LDS and of decode streams (internal
// to librlnc_hip): limits, layout, the four state words and their protocol, the check of a caller's buffer.  The
// launches on it: rank_large_kernels.hpp, rank_stream_kernels.hpp (the LDS push), rank_compact_kernels.hpp,
// stream_deliver_kernels.hpp, stream_recode_kernels.hpp and stream_accept_kernels.hpp (read only).
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

// one object's state, in dwords (every array starts on a multiple of 4 dwords):
//   the four state words (StateWord), piv[k], St[m], Q[k][32 bytes], X[B][D], R[k][D]
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

// bytes of the state of nobj objects, 0 = outside the limits; a decode stream's state buffer is that workspace
inline size_t rank_large_workspace_bytes(size_t k, size_t m, size_t nobj) {
    if (nobj == 0 || nobj > 0x7FFFFFFF || large_block(int64_t(k > 0x7FFFFFFF ? 0 : k), int64_t(m > 0x7FFFFFFF ? 0 : m)) == 0)
        return 0;
    return nobj * large_layout(int(k), int(m)).total * 4;
}
inline size_t rank_stream_state_bytes(size_t k, size_t m, size_t nobj) { return rank_large_workspace_bytes(k, m, nobj); }

// ---- The state words: an object's first four dwords, and the one account of their protocol --------------------------
enum StateWord : int {
    kStRank = 0,        // stored rows: piv[0 .. rank) and R[0 .. rank)[D] are live
    kStRankBefore = 1,  // the rank before the last block, whose update applies the rank - rank before new rows
    kStDone = 2,        // slots answered: St[0 .. done) are live
    kStTarget = 3,      // done after the push in flight; spare in the one-shot form
};
// Who reads (r) and writes (w) which word.  Launches are ordered by the stream only; inside one, a workgroup reads its
// object's words (readfirstlane) before its first barrier, and one thread writes those it read behind its last.
//                            Rank  RankBefore  Done  Target
//   one-shot reduce           r                              a block at t0 = 0 reads no word (its rank is 0), so the
//   one-shot step             rw       w        w            workspace needs no initialisation
//   update (both forms)       r        r                     both as the step of the same block left them
//   final, stream snapshot,   r                 r
//   progress, compact plan, rows and move
//   deliver offsets, product, r                 r            no word written (stream_deliver.hip; its first launch is the
//   tail and scan                                            stream snapshot)
//   recode expand, offsets,   r                 r            no word written (stream_recode.hip); the expand launch reads
//   product and tail                                         St[0 .. done) too and keeps its numbering in LDS
//   accept base               r                              no word written (stream_accept.hip): rank == k is the
//                                                            finished filter; the rank and move launches read no word
//   stream init               w        w        w      w     all 0
//   stream latch                                r      w     the target rule; no later launch of the push reads avail
//   stream reduce             r                 r      r     its block: slots done .. min(done + B, target) - 1
//   stream step               rw       w        rw     r     RankBefore on every path, for an idle object too (or the
//                                                            update would apply the previous block's Q and rows again)
//   LDS push (one launch)     rw       w        rw     w     store_state(rank', target); no word for an idle object
//   compact commit            rw       w        rw     w     store_state(r, r), retired (0, 0); no word when idle
//
// The push target rule: target = min(max(avail, done), m, done + max_new), and an object whose done lies outside
// [0, m) is idle (target = done).  The workspace push latches it in kStTarget, the LDS push keeps it in registers.
//
// Why the two push forms and compaction may alternate on one buffer.  The live state -- kStRank, kStDone,
// piv[0 .. rank), St[0 .. done), R[0 .. rank)[D] -- is after any call the one-piece-at-a-time model's after the same
// slots, and its rows are the unique reduced rows of the span in arrival order (rank_large.hip's proof), so it is the
// same bytes whichever form ran.  The rest -- kStRankBefore, kStTarget, Q, X -- is scratch: by the table, no launch
// reads it as an earlier call left it (each reduce rewrites X and each step Q before the launch that reads them).

// the one 16-byte store of {rank, rank, done, done}
__device__ __forceinline__ void store_state(uint32_t *ws, int rank, int done) {
    *reinterpret_cast<uint4 *>(ws) = make_uint4(uint32_t(rank), uint32_t(rank), uint32_t(done), uint32_t(done));
}

// a caller's buffer for n_obj objects of k x m: the shape within the limits, non-null, 16-byte aligned, long enough
inline hipError_t rank_state_check(int k, int m, int n_obj, const void *state, size_t bytes) {
    const size_t need = k > 0 && m > 0 && n_obj > 0 ? rank_stream_state_bytes(size_t(k), size_t(m), size_t(n_obj)) : 0;
    const bool ok = need != 0 && state != nullptr && (reinterpret_cast<uintptr_t>(state) & 15) == 0 && bytes >= need;
    return ok ? hipSuccess : hipErrorInvalidValue;
}

}  // namespace rlnc
