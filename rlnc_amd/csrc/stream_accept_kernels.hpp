// stream_accept_kernels.hpp — launch interface of a decode stream's accept (stream_accept.hip; internal to
// librlnc_hip).
//
// The receiver's call before the push (include/rlnc_hip.h, rlnc_decode_stream_accept): n arrivals for many objects,
// interleaved in one staging buffer, go into their objects' next free slots in arrival order.  The slot of an arrival
// depends on what lives on the device -- avail, and with a state the rank -- so it is decided there.  The state is only
// read (rank_state.hpp: kStRank).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rank_state.hpp"

namespace rlnc {

constexpr int kAcceptMaxArrivals = 1 << 20;  // arrivals per call
constexpr int kAcceptChunk = 1024;           // arrivals per workgroup of the rank launch and per step of the base launch
constexpr int kAcceptColChunk = 4096;        // bytes of a piece per workgroup of the move grid, 256 lanes x 16 bytes
constexpr int kAcceptLdsObjects = 8192;      // objects up to which the base launch keeps next[] in LDS (32 KiB)

struct AcceptParams {
    const uint8_t *arrivals;  // [n] full pieces of k + L bytes, arrival i at i x arrival_stride: any byte address
    int64_t arrival_stride;   // bytes, >= k + L
    const int32_t *object;    // [n]
    const int32_t *count;     // one int32, or nullptr: all n arrivals
    int n;
    uint8_t *pieces;          // [obj][m][k + L]
    int64_t obj_stride;       // bytes between objects of pieces, >= m * (k + L)
    int64_t piece;            // k + L
    int k, m, n_obj;
    int32_t *avail;           // [obj], read and rewritten
    int32_t *slot;            // [n], or nullptr
    int32_t *refused;         // [obj], or nullptr
    void *plan;               // stream_accept_plan_bytes(n, n_obj) bytes, 16-byte aligned
};

// bytes of the plan buffer: int32 local, lead, cnt and base [n] and next [obj], each array rounded up to 16 bytes.
// A multiple of 16, non-decreasing in both arguments; 0 for n == 0, n > kAcceptMaxArrivals, n_obj == 0 and n_obj >= 2^31
size_t stream_accept_plan_bytes(size_t n, size_t n_obj);
// the move grid, n x column chunks, fits 2^31 - 1 workgroups (the other two launches always do)
bool stream_accept_fits(const AcceptParams &p);
// Three launches on s, no synchronisation: rank, base, move (stream_accept.hip).  state: nullptr = no finished filter.
// vec16: the move takes 16-byte accesses at any byte address (unaligned_vector_ok()); otherwise single bytes.
// hipErrorInvalidValue for arguments outside the limits above, a short state or a move grid that does not fit.
hipError_t launch_stream_accept(const AcceptParams &p, const void *state, size_t state_bytes, bool vec16, hipStream_t s);

}  // namespace rlnc
