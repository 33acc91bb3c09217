// rank_compact_kernels.hpp — launch interface of a decode stream's compaction (rank_compact.hip; internal to
// librlnc_hip).
//
// rlnc_decode_stream_compact (include/rlnc_hip.h, "Decode streams"): per object the slots below done whose status is Ok
// -- u_0 < u_1 < ... < u_{r-1}, r = rank -- become the slots 0 .. r - 1, or the object is retired (its four state words
// become 0).  Nothing is eliminated again: a useless piece was discarded by the elimination, so its column of e is zero
// in every stored row, and the stored rows are the unique reduced rows of the span (rank_large.hip's proof); the state
// after the slots 0 .. done - 1 is therefore a fresh stream's state after the useful slots alone, up to the renumbering
// of the e columns that this call performs.  The state buffer and its words: rank_state.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rank_state.hpp"
#include "rref.hpp"

namespace rlnc {

// bytes of a piece per workgroup of the move grid, 256 lanes x 16 bytes; a piece's last chunk takes its tail too
constexpr int kCompactColChunk = 4096;

// p: obj_stride, piece_stride, k, m, n_obj (its pieces field is not used: the pieces are written).  pieces: null = the
// state alone is compacted.  retire int32 [n_obj], kept int32 [n_obj][k], answered int32 [n_obj], each optional.  Four
// launches on s -- plan, row gather, piece move (none without pieces), commit -- no synchronisation, no workspace
// beside the state (the list u lives in the object's Q region, which no launch reads as an earlier call left it).
// vec16: the move takes 16-byte accesses at any byte address (unaligned_vector_ok()); otherwise single bytes.
// hipErrorInvalidValue for a shape outside the limits, a ragged table, a short state or a grid beyond 2^31 - 1
// workgroups.
hipError_t launch_rank_stream_compact(const RrefParams &p, uint8_t *pieces, void *state, size_t state_bytes,
                                      const int32_t *retire, int32_t *kept, int32_t *answered, bool vec16,
                                      hipStream_t s);

}  // namespace rlnc
