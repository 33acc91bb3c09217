// stream_deliver.hip — a decode stream's delivery (rlnc_decode_stream_deliver, decode_stream.cpp): decoded = T x data
// rows for the objects whose rank is k, chosen on the device.  The product -- its arguments, the predicate every
// workgroup returns on, the offset, tile and tail bodies, the geometry and the launch sequence -- is stream_product.hpp's,
// shared with the relay's recode (stream_recode.hip); here are the delivery's kernels by name, its marker scan and its
// launcher.
//
// A delivering object's product takes n_in = done_o source rows (the snapshot's T has zero columns from done_o on):
// the data rows of its answered slots, from byte k of a piece.
//
// Rules (rank_large.hip's): the early return depends on workgroup-uniform values only (blockIdx, the state words and
// select through readfirstlane) and comes before any LDS use or barrier; no launch reads what a workgroup of the same
// launch writes; the state, the pieces and select are only read.
#include <hip/hip_runtime.h>

#include "../../include/rlnc_hip.h"
#include "rank_large_kernels.hpp"
#include "stream_deliver_kernels.hpp"
#include "stream_product.hpp"

namespace rlnc {

namespace {

// the delivery's arguments: in = the data rows, coef = the T extract [obj][k][m], out = decoded, n_out = min_rank = k,
// width = L
using DeliverArgs = StreamProdArgs;

__global__ __launch_bounds__(256) void deliver_offset_kernel(DeliverArgs a, uint64_t *stream, uint64_t base) {
    stream_offset_body(a, stream, base);
}

template <int W>
__global__ __launch_bounds__(64 * W) void gf_stream_deliver(DeliverArgs a, const uint64_t *stream) {
    stream_product_body<W>(a, stream);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gf_stream_deliver_tail(DeliverArgs a) {
    __shared__ uint32_t tab[kMulTabDw];
    stream_tail_body<VEC>(a, tab);
}

struct DeliverKernels {
    static constexpr auto offset = &deliver_offset_kernel;
    template <int W>
    static constexpr auto product = &gf_stream_deliver<W>;
    template <bool VEC>
    static constexpr auto tail = &gf_stream_deliver_tail<VEC>;
};

// The marker scan of the selected objects (decoder.rs:136-177), one wave each, four to a workgroup and no barrier: below
// rank k NotAllPiecesReceivedYet and length 0; else the last nonzero byte of decoded[o] must be the 0x81 marker, not at
// index 0 -- found from the end, 4 KiB a step (64 B a lane), by a wave maximum of (offset + 1) << 8 | byte.  It writes
// what launch_final_data_len_ranked writes for the object, and nothing for an unselected one.
template <bool VEC>
__global__ __launch_bounds__(256) void deliver_scan_kernel(DeliverArgs a, int32_t *status, int64_t *final_len) {
    const int o = int(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    if (o >= a.n_obj) return;
    const int lane = int(threadIdx.x & 63u);
    if (a.select != nullptr && __builtin_amdgcn_readfirstlane(a.select[o]) == 0) return;
    const int rank = __builtin_amdgcn_readfirstlane(int(a.ws[int64_t(o) * a.ws_obj + kStRank]));
    if (rank < a.n_out) {
        if (lane == 0) {
            status[o] = RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET;
            final_len[o] = 0;
        }
        return;
    }
    const int64_t len = int64_t(a.n_out) * a.width;
    const uint8_t *d = a.out + int64_t(o) * len;
    int64_t hit = -1;
    uint32_t byte = 0;
    for (int64_t c = (len + 4095) / 4096 - 1; c >= 0; --c) {
        uint32_t mine = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t off = c * 4096 + lane * 64 + u * kBytesPerThread;
            if (off < len) {
                const uint4 x = load16<VEC>(d + off, int(min<int64_t>(kBytesPerThread, len - off)));
                const uint32_t wd[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (wd[q]) {
                        const int b = (31 - __builtin_clz(wd[q])) / 8;
                        mine = (uint32_t(lane * 64 + u * kBytesPerThread + 4 * q + b + 1) << 8) |
                               ((wd[q] >> (8 * b)) & 0xFFu);
                    }
            }
        }
        const uint32_t best = __builtin_amdgcn_readfirstlane(tile_wave_max(mine));
        if (best) {
            hit = c * 4096 + int64_t(best >> 8) - 1;
            byte = best & 0xFFu;
            break;
        }
    }
    if (lane == 0) {
        const bool ok = hit > 0 && byte == kBoundaryMarker;
        status[o] = ok ? RLNC_OK : RLNC_ERR_INVALID_DECODED_DATA_FORMAT;
        final_len[o] = ok ? hit : 0;
    }
}

}  // namespace

size_t stream_deliver_plan_bytes(size_t k, size_t m, size_t n_obj) {
    if (rank_stream_state_bytes(k, m, n_obj) == 0) return 0;
    // the T extract, then the block-address streams
    return ((n_obj * k * m + 15) & ~size_t(15)) + stream_geom_bytes(stream_geom(int(k), int(m), int(n_obj), 0));
}

bool stream_deliver_fits(const DeliverParams &p) { return stream_geom(p.k, p.m, p.n_obj, p.L).fits(); }

hipError_t launch_stream_deliver(const DeliverParams &p, const void *state, size_t state_bytes, bool unaligned_ok,
                                 hipStream_t s) {
    if (p.n_obj <= 0) return hipSuccess;
    hipError_t e = rank_state_check(p.k, p.m, p.n_obj, state, state_bytes);
    if (e != hipSuccess) return e;
    if (p.L <= 0 || p.plan == nullptr || !al16(p.plan) || !stream_deliver_fits(p)) return hipErrorInvalidValue;
    const StreamGeom g = stream_geom(p.k, p.m, p.n_obj, p.L);
    const size_t t_bytes = (size_t(p.n_obj) * p.k * p.m + 15) & ~size_t(15);
    uint8_t *T = static_cast<uint8_t *>(p.plan);
    uint64_t *stream = reinterpret_cast<uint64_t *>(T + t_bytes);

    // 1. the T extract: the snapshot's launch
    RrefParams rp{};
    rp.k = p.k, rp.m = p.m, rp.n_obj = p.n_obj;
    rp.T = T;
    rp.T_obj = int64_t(p.k) * p.m;
    if ((e = launch_rank_stream_snapshot(rp, state, state_bytes, s)) != hipSuccess) return e;

    DeliverArgs a{};
    a.ws = static_cast<const uint32_t *>(state);
    a.ws_obj = int64_t(large_layout(p.k, p.m).total);
    a.in = p.pieces + p.k;
    a.in_obj = p.obj_stride;
    a.in_row = int64_t(p.k) + p.L;
    a.select = p.select;
    a.coef = T;
    a.out = p.decoded;
    a.width = p.L;
    a.n_out = a.min_rank = p.k;
    a.m = p.m, a.n_obj = p.n_obj;
    stream_args_geom(a, g);

    // every object's operands at once: 16-byte vector accesses at any address, or all of them aligned
    const bool vec = unaligned_ok || (al16(p.pieces) && al16(p.decoded) && al16(int64_t(p.k)) && al16(p.L) &&
                                      al16(p.obj_stride));
    const bool bsj = ragged_bsj_eligible(a.in, p.decoded, a.in_row, p.L, p.L, p.k, vec);
    // 2. - 4. the block-address streams of the delivering objects, the bit-sliced product over the whole column blocks,
    // the perm product over the rest
    if ((e = launch_stream_product<DeliverKernels>(a, g, vec, bsj, stream, s)) != hipSuccess) return e;
    // 5. status and length of the selected objects
    hipLaunchKernelGGL(vec ? &deliver_scan_kernel<true> : &deliver_scan_kernel<false>, dim3(unsigned((p.n_obj + 3) / 4)),
                       dim3(256), 0, s, a, p.status, p.len);
    return hipGetLastError();
}

}  // namespace rlnc
