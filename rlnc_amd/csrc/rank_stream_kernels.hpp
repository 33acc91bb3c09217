// rank_stream_kernels.hpp — launch interface of the LDS form of a decode stream's push (rank_stream.hip; internal to
// librlnc_hip).
//
// A second producer of a decode stream's state (include/rlnc_hip.h, "Decode streams"; the state buffer, its words and
// why the two forms may be mixed from push to push on one buffer: rank_state.hpp; the workspace form of the push:
// rank_large_kernels.hpp).  One launch per push: each object's stored rows and pivots come from the state into LDS,
// rank.hip's per-piece loop runs over the object's new slots only, and the rows, pivots, statuses and state words go
// back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rank_kernels.hpp"
#include "rank_state.hpp"
#include "rref.hpp"

namespace rlnc {

// the shapes of this form: exactly those of the one-shot LDS kernel, rank_lds_bytes(k, m) <= kRrefMaxLds (its region
// for m staged headers covers any number of new slots); false for k = 0 or m = 0
bool rank_stream_lds_fits(size_t k, size_t m);

// p: pieces, obj_stride, piece_stride, k, m, n_obj; state, avail, max_new, rank, answered as launch_rank_stream_push.
// One launch: a workgroup of 4 waves per object, or -- k <= 16, rows of <= 16 dwords and >= 1024 objects, the rule of
// launch_rank_batch -- one wave per object, 4 objects per workgroup over one table copy.  avail[o] is read once, by
// object o's workgroup (wave).  An object with nothing new has no word of its state written; rank / answered are
// written for every object.  hipErrorInvalidValue for a shape that does not fit, a ragged table or a short state.
hipError_t launch_rank_stream_push_lds(const RrefParams &p, void *state, size_t state_bytes, const int32_t *avail,
                                       int max_new, int32_t *rank, int32_t *answered, hipStream_t s);

}  // namespace rlnc
