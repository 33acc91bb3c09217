// stream_accept.hip — a decode stream's accept (rlnc_decode_stream_accept, decode_stream.cpp; interface:
// stream_accept_kernels.hpp): n arrivals for many objects, interleaved in one staging buffer, are copied into their
// objects' next free slots in arrival order, with the slot decided on the device.
//
// Arrival i of object o (object[i]) takes slot a_o + j when it is the j-th arrival of o in the call, a_o = avail[o]
// clamped to [0, m]; from slot m on it is refused (NoRoom).  The assignment is a stable ranking per object, so no slot
// is claimed with an atomic: it is computed in three launches, ordered by the stream only.
//   rank   (one workgroup of 1,024 threads per chunk of 1,024 arrivals, a thread per arrival) the chunk's ids go into
//          LDS, an invalid id and an index at or beyond the device count n' as a sentinel.  Every thread walks the ids
//          before its own, last first (16-byte broadcast LDS reads; a wave stops at its own last position): local = the
//          equal ids before its own, lead = the first of them (itself: a leader).  Every ranked arrival then adds one to
//          its leader's counter in LDS -- a sum, so the order of the additions does not show -- which gives a leader the
//          chunk's count of its id.  Written for every i < n: local[i], lead[i] (the leader's index in the call; NoObject
//          or Absent for an arrival that is not ranked), cnt[i] (0 but for a leader).
//   base   (one workgroup of 1,024 threads) next[o] = a_o, or Finished when the state is given and rank_o == k, for
//          every object; then the chunks in order, a thread per arrival: a leader (lead[i] == i) takes base[i] = next[o]
//          and adds cnt[i] to next[o] unless that is Finished.  A chunk has one leader per id, so no two threads of a
//          step touch one next[o]; a barrier separates the steps.  The next step's lead, id and cnt are loaded before
//          the step's barrier, so that a step waits for next[] alone, which lives in LDS for up to 8,192 objects and in
//          the plan beyond.  At the end avail and refused are written from next.  This is the call's only serial part:
//          ceil(n' / 1,024) dependent steps.
//   move   (arrival x 4,096-byte column chunk of a piece; a piece's last chunk takes its tail too, in a second pass)
//          slot = base[lead[i]] + local[i]; the chunk-0 workgroup writes slot[i]; a workgroup whose arrival is not
//          placed returns before any other work.  VEC: 16 bytes per lane at any byte address (k + L and the strides are
//          arbitrary, so source and destination differ in alignment; unaligned_vector_access), the last lane of a piece
//          byte by byte; otherwise every lane owns 16 single bytes, 256 apart.  Ownership is by bytes in both: no
//          access is wider than what the thread owns.  Exactly rank_compact.hip's move, one copy a lane.
//
// Rules kept by every kernel (rank_large.hip): no workgroup waits for another; every branch around a barrier is
// workgroup-uniform, on values passed through readfirstlane; early returns come before any barrier; shared global
// state is ordered by barriers and kernel boundaries only.  The state, the arrivals, the ids and the count are only
// read.
#include "../../include/rlnc_hip.h"
#include "stream_accept_kernels.hpp"

namespace rlnc {

namespace {

struct AcceptArgs {
    const uint8_t *arrivals;
    int64_t arrival_stride;
    const int32_t *object, *count;
    uint8_t *pieces;
    int64_t obj_stride, piece;
    const uint32_t *ws;  // the state, or nullptr
    int64_t ws_obj;      // dwords
    int32_t *avail, *slot, *refused;
    int32_t *local, *lead, *cnt, *base, *next;  // the plan
    int n, k, m, n_obj;
    uint32_t col_chunks;
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kNoId = -1;  // in LDS: an arrival that is not ranked

// n' = min(max(*count, 0), n): the arrivals the call takes; workgroup-uniform
__device__ __forceinline__ int taken(const AcceptArgs &a) {
    return a.count != nullptr ? min(max(__builtin_amdgcn_readfirstlane(*a.count), 0), a.n) : a.n;
}

// one 16-byte group of the chunk's ids against the thread's own, last id first, so that `first` ends at the smallest
// matching position; OWN: the group may reach the thread's own position, so only the ids before it count
template <bool OWN>
__device__ __forceinline__ void rank_group(const int4 &v, int j, int my, int pos, int &loc, int &first) {
    const int vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 3; c >= 0; --c) {
        const bool hit = vs[c] == my && (!OWN || j + c < pos);
        loc += hit ? 1 : 0;
        first = hit ? j + c : first;
    }
}

__global__ __launch_bounds__(kAcceptChunk) void gf_stream_accept_rank(AcceptArgs a) {
    __shared__ int4 ids4[kAcceptChunk / 4];
    __shared__ int32_t cnts[kAcceptChunk];
    int32_t *ids = reinterpret_cast<int32_t *>(ids4);
    const int pos = int(threadIdx.x), c0 = int(blockIdx.x) * kAcceptChunk, i = c0 + pos;
    const int np = taken(a);
    const int id = i < np ? a.object[i] : kNoId;
    const int my = uint32_t(id) < uint32_t(a.n_obj) ? id : kNoId;
    ids[pos] = my;
    cnts[pos] = 0;
    __syncthreads();
    // a wave walks the ids before its last position, and none when the chunk ends before its first
    const int w0 = __builtin_amdgcn_readfirstlane(pos & ~63), len = min(kAcceptChunk, max(np - c0, 0));
    const int g0 = w0 >> 2, g1 = w0 < len ? (min(len, w0 + 64) + 3) >> 2 : 0;
    int loc = 0, first = pos;
    for (int g = g1 - 1; g >= g0; --g) rank_group<true>(ids4[g], 4 * g, my, pos, loc, first);
    if (g1 > 0) {
#pragma unroll 4
        for (int g = g0 - 1; g >= 0; --g) rank_group<false>(ids4[g], 4 * g, my, pos, loc, first);
    }
    const bool ranked = my != kNoId;
    if (ranked) atomicAdd(&cnts[first], 1);  // a sum: the same whatever the order
    __syncthreads();
    if (i >= a.n) return;
    a.local[i] = ranked ? loc : 0;
    a.lead[i] = ranked ? c0 + first : i < np ? RLNC_ACCEPT_NO_OBJECT : RLNC_ACCEPT_ABSENT;
    a.cnt[i] = ranked ? cnts[pos] : 0;
}

// LDS: next[] lives in LDS (n_obj <= kAcceptLdsObjects), so that a step waits for LDS and not for a round trip to L2
template <bool LDS>
__global__ __launch_bounds__(kAcceptChunk) void gf_stream_accept_base(AcceptArgs a) {
    __shared__ int32_t next_lds[LDS ? kAcceptLdsObjects : 1];
    int32_t *next;
    if constexpr (LDS)
        next = next_lds;
    else
        next = a.next;
    const int tid = int(threadIdx.x), m = a.m;
    const int np = taken(a);
    for (int64_t o = tid; o < a.n_obj; o += kAcceptChunk) {
        const bool fin = a.ws != nullptr && int(a.ws[o * a.ws_obj + kStRank]) == a.k;
        next[o] = fin ? RLNC_ACCEPT_FINISHED : min(max(a.avail[o], 0), m);
    }
    __syncthreads();
    const int chunks = (np + kAcceptChunk - 1) / kAcceptChunk;
    int i = tid;
    int l = i < np ? a.lead[i] : kNoId, o = i < np ? a.object[i] : 0, c = i < np ? a.cnt[i] : 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int in = i + kAcceptChunk;  // the next step's, in flight over this step's round trip to next[]
        const int nl = in < np ? a.lead[in] : kNoId, no = in < np ? a.object[in] : 0, nc = in < np ? a.cnt[in] : 0;
        // (a leader's id is in range, rank ranked it: the second test only keeps a caller who rewrites object_dev
        // under the call inside next[])
        if (l == i && uint32_t(o) < uint32_t(a.n_obj)) {
            const int b = next[o];
            a.base[i] = b;  // Finished for every leader of a finished object
            if (b >= 0) next[o] = b + c;
        }
        __syncthreads();
        i = in, l = nl, o = no, c = nc;
    }
    for (int64_t ob = tid; ob < a.n_obj; ob += kAcceptChunk) {
        const int nx = next[ob];
        if (nx >= 0) a.avail[ob] = min(nx, m);  // a finished object's avail keeps its value, unclamped
        if (a.refused != nullptr) a.refused[ob] = max(nx - m, 0);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gf_stream_accept_move(AcceptArgs a) {
    const uint32_t i = blockIdx.x / a.col_chunks, chunk = blockIdx.x % a.col_chunks;
    const int l = __builtin_amdgcn_readfirstlane(a.lead[i]);
    int slot = l, o = 0;
    if (l >= 0) {
        o = __builtin_amdgcn_readfirstlane(a.object[i]);
        const int b = __builtin_amdgcn_readfirstlane(a.base[min(l, a.n - 1)]);
        slot = b < 0 ? b : b + __builtin_amdgcn_readfirstlane(a.local[i]);
        if (slot >= a.m) slot = RLNC_ACCEPT_NO_ROOM;
    }
    const int tid = int(threadIdx.x);
    if (chunk == 0 && tid == 0 && a.slot != nullptr) a.slot[i] = slot;
    // not placed: no byte of the pieces (the id test and the clamp of l above cannot fire on what rank and base wrote:
    // they keep every address inside the caller's buffers whatever the plan held)
    if (slot < 0 || uint32_t(o) >= uint32_t(a.n_obj)) return;
    const int64_t S = a.piece, cbase = int64_t(chunk) * kAcceptColChunk;
    const uint8_t *src = a.arrivals + int64_t(i) * a.arrival_stride + cbase;
    uint8_t *dst = a.pieces + int64_t(o) * a.obj_stride + int64_t(slot) * S + cbase;
    // a piece's last chunk takes its tail too (up to two chunks less a byte, in a second pass)
    const int64_t width = chunk + 1 == a.col_chunks ? S - cbase : int64_t(kAcceptColChunk);
    for (int64_t c0 = 0; c0 < width; c0 += kAcceptColChunk) {
        const int64_t left = width - c0;  // > 0: bytes of the piece from this pass's first column on
        if constexpr (VEC) {
            const int64_t at = c0 + 16 * tid, n = left - 16 * tid;
            if (n >= 16) {
                *reinterpret_cast<u32x4_t *>(dst + at) = *reinterpret_cast<const u32x4_t *>(src + at);
            } else if (n > 0) {
                // the last lane of a piece: its columns byte by byte
                for (int b = 0; b < int(n); ++b) dst[at + b] = src[at + b];
            }
        } else {
            // single bytes: every lane owns the 16 columns tid + 256 b of the pass
            uint8_t x[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) x[b] = tid + 256 * b < left ? src[c0 + tid + 256 * b] : uint8_t(0);
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (tid + 256 * b < left) dst[c0 + tid + 256 * b] = x[b];
        }
    }
}

size_t up4_dwords(size_t v) { return (v + 3) & ~size_t(3); }

int64_t col_chunks_of(int64_t piece) { return piece < kAcceptColChunk ? 1 : piece / kAcceptColChunk; }  // floor, >= 1

}  // namespace

size_t stream_accept_plan_bytes(size_t n, size_t n_obj) {
    if (n == 0 || n > size_t(kAcceptMaxArrivals) || n_obj == 0 || n_obj > 0x7FFFFFFF) return 0;
    return 4 * (4 * up4_dwords(n) + up4_dwords(n_obj));
}

bool stream_accept_fits(const AcceptParams &p) {
    const int64_t chunks = col_chunks_of(p.piece);
    return chunks <= 0x7FFFFFFF && int64_t(p.n) * chunks <= 0x7FFFFFFF;
}

hipError_t launch_stream_accept(const AcceptParams &p, const void *state, size_t state_bytes, bool vec16,
                                hipStream_t s) {
    if (p.n == 0 || p.n_obj == 0) return hipSuccess;
    if (p.n < 0 || p.n > kAcceptMaxArrivals || p.n_obj < 0 || p.k <= 0 || p.k > kLargeMaxK || p.m <= 0 ||
        p.m > kLargeMaxM || p.piece <= p.k || p.arrival_stride < p.piece || p.obj_stride < int64_t(p.m) * p.piece ||
        p.arrivals == nullptr || p.object == nullptr || p.pieces == nullptr || p.avail == nullptr || p.plan == nullptr ||
        (reinterpret_cast<uintptr_t>(p.plan) & 15) != 0 || !stream_accept_fits(p))
        return hipErrorInvalidValue;
    if (state != nullptr && rank_state_check(p.k, p.m, p.n_obj, state, state_bytes) != hipSuccess)
        return hipErrorInvalidValue;
    AcceptArgs a{};
    a.arrivals = p.arrivals;
    a.arrival_stride = p.arrival_stride;
    a.object = p.object;
    a.count = p.count;
    a.pieces = p.pieces;
    a.obj_stride = p.obj_stride;
    a.piece = p.piece;
    a.ws = static_cast<const uint32_t *>(state);
    a.ws_obj = state != nullptr ? int64_t(large_layout(p.k, p.m).total) : 0;
    a.avail = p.avail;
    a.slot = p.slot;
    a.refused = p.refused;
    const size_t n4 = up4_dwords(size_t(p.n));
    a.local = static_cast<int32_t *>(p.plan);
    a.lead = a.local + n4;
    a.cnt = a.lead + n4;
    a.base = a.cnt + n4;
    a.next = a.base + n4;
    a.n = p.n, a.k = p.k, a.m = p.m, a.n_obj = p.n_obj;
    a.col_chunks = uint32_t(col_chunks_of(p.piece));
    const unsigned g_rank = unsigned((p.n + kAcceptChunk - 1) / kAcceptChunk);
    const unsigned g_move = unsigned(int64_t(p.n) * a.col_chunks);
    hipLaunchKernelGGL(gf_stream_accept_rank, dim3(g_rank), dim3(kAcceptChunk), 0, s, a);
    if (p.n_obj <= kAcceptLdsObjects)
        hipLaunchKernelGGL(gf_stream_accept_base<true>, dim3(1), dim3(kAcceptChunk), 0, s, a);
    else
        hipLaunchKernelGGL(gf_stream_accept_base<false>, dim3(1), dim3(kAcceptChunk), 0, s, a);
    if (vec16)
        hipLaunchKernelGGL(gf_stream_accept_move<true>, dim3(g_move), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(gf_stream_accept_move<false>, dim3(g_move), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rlnc
