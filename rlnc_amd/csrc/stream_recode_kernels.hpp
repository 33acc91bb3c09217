// stream_recode_kernels.hpp — launch interface of a decode stream's recode (stream_recode.hip; internal to
// librlnc_hip).
//
// The relay's call on a decode stream (include/rlnc_hip.h, rlnc_decode_stream_recode): every selected object of rank
// r >= 1 gets count recoded pieces, each a combination of the r useful pieces it holds -- the slots below done_o whose
// status is Ok, u_0 < ... < u_{r-1}, the list rlnc_decode_stream_compact keeps -- found on the device.  The state is
// only read (rank_state.hpp: kStRank, kStDone and St).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rank_state.hpp"

namespace rlnc {

constexpr int kRecodeMaxCount = 4096;  // recoded pieces per object and call

struct RecodeParams {
    const uint8_t *pieces;   // [obj][m][k + L]; a full piece, header included, is a source row
    int64_t obj_stride;      // bytes between objects of pieces, >= m * (k + L)
    int k, m, n_obj, count;
    int64_t L;
    const int32_t *select;   // [obj], or nullptr: every object
    const uint8_t *r;        // [obj][count][k]: row i's first rank bytes are the recoding vector
    uint8_t *out;            // [obj][count][k + L]
    int32_t *status;         // [obj]
    int32_t *used;           // [obj], or nullptr
    void *plan;              // stream_recode_plan_bytes(k, m, count, n_obj) bytes, 16-byte aligned: the expanded
                             // coefficients C [obj][count][m], then the block-address stream, object o at o x (the
                             // entries of m columns)
};

// bytes of the plan buffer: a multiple of 16; 0 exactly where rank_stream_state_bytes is 0 or count is outside
// [1, kRecodeMaxCount]
size_t stream_recode_plan_bytes(size_t k, size_t m, size_t count, size_t n_obj);
// every launch of the recode fits a grid (2^31 - 1 workgroups)
bool stream_recode_fits(const RecodeParams &p);
// At most four launches on s, no synchronisation (but the shared programs' one block-table probe per device,
// bsj_shared_base; inside a capture that has not seen it the tail kernel takes every column): the expansion of r into
// C with status and used, the block-address streams of the recoding objects, the bit-sliced product over the whole
// 4 KiB column blocks of k + L, the perm product over the rest.  unaligned_ok: unaligned_vector_ok().
hipError_t launch_stream_recode(const RecodeParams &p, const void *state, size_t state_bytes, bool unaligned_ok,
                                hipStream_t s);

}  // namespace rlnc
