// rank_large_kernels.hpp — launch interface of the true-rank elimination for generations beyond LDS (rank_large.hip;
// internal to librlnc_hip).
//
// A third producer of {T, status, rank} from RrefParams, with rank.hip's semantics (RLNC_RANK_MODE_TRUE;
// include/rlnc_hip.h, "Rank mode") and rank.hip's fields of RrefParams (the batch form only: objs must be null).  The
// per-object state lives in a device workspace instead of LDS (rank_state.hpp: limits, layout, state words), and the
// pieces are taken B at a time, three launches per block plus one at the end (rank_large.hip), so one object is spread
// over many workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include "rank_state.hpp"
#include "rref.hpp"

namespace rlnc {

// 3·ceil(m / B) + 1 launches on s (reduce, block step, update per block; the T / status / rank writer), no host
// synchronisation.  ws: rank_large_workspace_bytes(k, m, n_obj) bytes, 16-byte aligned, used until the launches ran.
// hipErrorInvalidValue for a shape outside the limits, a ragged table or a short workspace.
hipError_t launch_rank_large(const RrefParams &p, void *ws, size_t ws_bytes, hipStream_t s);

// ---- Decode streams (include/rlnc_hip.h, rlnc_decode_stream_*): the same state kept by the caller between calls ----
// A push is one latch launch, ceil(min(max_new, m) / B) blocks of the same three launches in their stream form -- each
// object's own block, read from its state; an object with nothing left returns at once -- and, when asked for, one
// launch that copies out every object's rank and done (the words and the target rule: rank_state.hpp).  The state
// after a push does not depend on how the pieces were split over pushes (rank_large.hip: the proof is per block).
// Generations that fit LDS have a one-launch form of the push besides (rank_stream_kernels.hpp) on the same buffer.
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
