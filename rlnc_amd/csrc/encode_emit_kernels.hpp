// encode_emit_kernels.hpp — launch interface of the sender's emit (encode_emit.hip; internal to librlnc_hip).
//
// The sender's call (include/rlnc_hip.h, rlnc_encode_emit; encode_emit_call.cpp): want[o] coded pieces per object, read on the device, are
// written as one packed run of packets with an object id per packet and a device-side count -- what
// rlnc_decode_stream_accept takes as (arrivals, object, count).  src, want and r are only read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rlnc {

constexpr int kEmitMaxK = 4096;          // pieces coded together
constexpr int kEmitMaxPerObject = 4096;  // packets per object and call
constexpr int kEmitMaxPackets = 1 << 20;
constexpr int kEmitMaxObjects = 1 << 20;
constexpr int kEmitChunk = 1024;         // objects per workgroup of the scan launch
constexpr int kEmitLabelPackets = 16;    // packets per workgroup of the label launch

struct EmitParams {
    const uint8_t *src;      // [obj][k][L]
    int64_t src_obj;         // bytes between objects of src, >= k * L
    int k, n_obj, max_per, n;
    int64_t L;
    const int32_t *want;     // [obj]
    const uint8_t *r;        // [n][k]: packet i's random bytes
    uint8_t *out;            // n packets of k + L bytes
    int64_t out_stride;      // bytes between packets, >= k + L
    int32_t *object;         // [n]
    int32_t *count;          // one int32
    int32_t *granted;        // [obj], or nullptr
    void *plan;              // encode_emit_plan_bytes(k, max_per, n_obj, n) bytes, 16-byte aligned: base [obj],
                             // grant [obj], the chunk sums, the total, then (max_per >= 4) the block-address streams,
                             // object o at o x (row tiles of max_per x k x tile rows) entries
};

// bytes of the plan buffer: a multiple of 16, non-decreasing in each argument inside the limits; 0 for a zero argument
// and beyond kEmitMaxK, kEmitMaxPerObject, kEmitMaxObjects, kEmitMaxPackets
size_t encode_emit_plan_bytes(size_t k, size_t max_per, size_t n_obj, size_t n);
// every launch of the emit fits a grid (2^31 - 1 workgroups)
bool encode_emit_fits(const EmitParams &p);
// At most six launches on s, no synchronisation (but the shared programs' one block-table probe per device,
// bsj_shared_base; inside a capture that has not seen it the tail kernel takes every column): the scan over chunks of
// 1,024 objects, the base launch (one workgroup: base, grant, granted, count), the labels and headers, the
// block-address streams of the objects granted >= 4, the bit-sliced product over the whole 4 KiB column blocks of L,
// the perm product over the rest.  unaligned_ok: unaligned_vector_ok().
hipError_t launch_encode_emit(const EmitParams &p, bool unaligned_ok, hipStream_t s);

}  // namespace rlnc
