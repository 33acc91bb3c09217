// stream_deliver_kernels.hpp — launch interface of a decode stream's delivery (stream_deliver.hip; internal to
// librlnc_hip).
//
// The way out of a decode stream that the device decides (include/rlnc_hip.h, rlnc_decode_stream_deliver): the objects
// whose rank is k -- and only those -- get decoded = T x the data rows of their answered slots, every launch finding an
// object's rank, done and select on the device.  The state is only read (rank_state.hpp: kStRank and kStDone).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rank_state.hpp"

namespace rlnc {

struct DeliverParams {
    const uint8_t *pieces;   // [obj][m][k + L]; the data rows start at byte k of a piece
    int64_t obj_stride;      // bytes between objects of pieces, >= m * (k + L)
    int k, m, n_obj;
    int64_t L;
    const int32_t *select;   // [obj], or nullptr: every object
    uint8_t *decoded;        // [obj][k][L]
    int32_t *status;         // [obj]
    int64_t *len;            // [obj]
    void *plan;              // stream_deliver_plan_bytes(k, m, n_obj) bytes, 16-byte aligned: the T extract [obj][k][m],
                             // then the block-address stream, object o at o x (the entries of m columns)
};

// bytes of the plan buffer: a multiple of 16; 0 exactly where rank_stream_state_bytes is 0
size_t stream_deliver_plan_bytes(size_t k, size_t m, size_t n_obj);
// every launch of the delivery fits a grid (2^31 - 1 workgroups)
bool stream_deliver_fits(const DeliverParams &p);
// At most five launches on s, no synchronisation (but the shared programs' one block-table probe per device,
// bsj_shared_base; inside a capture that has not seen it the tail kernel takes every column): the snapshot's T extract
// into the plan, the block-address streams of the delivering objects, the bit-sliced product over the whole 4 KiB column
// blocks, the perm product over the rest, the marker scan of the selected objects.  unaligned_ok: unaligned_vector_ok().
hipError_t launch_stream_deliver(const DeliverParams &p, const void *state, size_t state_bytes, bool unaligned_ok,
                                 hipStream_t s);

}  // namespace rlnc
