// stream_deliver.hip — a decode stream's delivery (rlnc_decode_stream_deliver, decode_stream.cpp): decoded = T x data
// rows for the objects whose rank is k, chosen on the device.  The host launches over every object; each workgroup
// reads its object's rank, done and select and returns at once unless the object delivers, so an unfinished object
// costs a workgroup's start and nothing else.
//
// A delivering object's product takes n_in = done_o source rows (the snapshot's T has zero columns from done_o on) and
// runs the bit-sliced engine's tile (bsj_tile.hpp) over its whole 4 KiB column blocks, as the ragged kernels of
// ragged.hip run it per object; the rest -- L mod 4096, generations of k < 4, operands the program does not take --
// goes to a perm-multiply kernel (gf_perm.hpp) over 8 rows x 4 KiB tiles.
//
// Rules (rank_large.hip's): the early return depends on workgroup-uniform values only (blockIdx, the state words and
// select through readfirstlane) and comes before any LDS use or barrier; no launch reads what a workgroup of the same
// launch writes; the state, the pieces and select are only read.
#include <hip/hip_runtime.h>

#include "../../include/rlnc_hip.h"
#include "bsj_tile.hpp"
#include "gf256.hpp"
#include "gf_perm.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"
#include "rank_large_kernels.hpp"
#include "rank_state.hpp"
#include "stream_deliver_kernels.hpp"

namespace rlnc {

namespace {

constexpr int kTailRows = 8;  // output rows per workgroup of the tail kernel

// what every launch takes (by value)
struct DeliverArgs {
    const uint32_t *ws;     // the stream's state
    int64_t ws_obj;         // dwords per object
    const uint8_t *pieces;
    int64_t obj_stride, piece_stride;
    const int32_t *select;
    const uint8_t *T;       // the T extract [obj][k][m]
    uint8_t *decoded;
    int64_t L;
    int k, m, n_obj;
    int tile_rows, row_tiles;  // the bit-sliced product's
    int64_t per_obj;        // stream entries of one object: row_tiles x m x tile_rows
    int blocks_per_obj;     // ... in blocks of 256 (the offset launch)
    int col_blocks;         // column blocks of the launch (product: whole ones; tail: those of the rest)
    int64_t col0;           // first column of the launch
    int64_t total;          // workgroups of the launch
};

// whether object o delivers, and its done (workgroup-uniform when o is)
__device__ __forceinline__ bool delivers(const DeliverArgs &a, int o, int &done) {
    const uint32_t *ws = a.ws + int64_t(o) * a.ws_obj;
    const int rank = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    done = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
    const int sel = a.select != nullptr ? __builtin_amdgcn_readfirstlane(a.select[o]) : 1;
    return sel != 0 && rank >= a.k && done <= a.m;  // (done <= m always: no entry beyond an object's part of the plan)
}

// the product of object o (no header): the data rows of its answered slots in, decoded[o] out, columns from col0
__device__ __forceinline__ MatmulParams deliver_params(const DeliverArgs &a, int o, int done, int64_t width) {
    MatmulParams q{};
    q.in = a.pieces + int64_t(o) * a.obj_stride + a.k + a.col0;
    q.in_row = a.piece_stride;
    q.coef = a.T + int64_t(o) * a.k * a.m;
    q.coef_row = a.m;
    q.out = a.decoded + int64_t(o) * a.k * a.L + a.col0;
    q.out_row = a.L;
    q.n_out = a.k;
    q.n_in = done;
    q.width = width;
    q.n_obj = 1;
    return q;
}

// The block-address streams of the delivering objects, as ragged_offset_kernel writes an object's: entry l of object
// o = the code block of coefficient T[o][row][j], laid out [rt][j][row in tile] for j < done_o from o x per_obj (8-byte
// units) -- its absolute address for the 4- and 8-wave programs, its 4-byte offset for the 1- and 2-wave ones.  One
// thread per entry of m columns; those past done_o, and every thread of an object that does not deliver, return.
__global__ __launch_bounds__(256) void deliver_offset_kernel(DeliverArgs a, uint64_t *stream, uint64_t base) {
    // blocks_per_obj blocks of 256 entries an object; 32-bit arithmetic throughout (per_obj <= 2^25)
    const uint32_t o = blockIdx.x / uint32_t(a.blocks_per_obj);
    const uint32_t l = (blockIdx.x % uint32_t(a.blocks_per_obj)) * 256u + threadIdx.x;
    const uint32_t *ws = a.ws + int64_t(o) * a.ws_obj;
    const int rank = int(ws[kStRank]), done = int(ws[kStDone]);
    if (rank < a.k || done > a.m || (a.select != nullptr && a.select[o] == 0)) return;
    const uint32_t tr = uint32_t(a.tile_rows);  // 8, 16, 32 or 64
    if (l >= uint32_t(a.row_tiles) * uint32_t(done) * tr) return;
    const uint32_t i = l % tr, lj = l / tr;
    const uint32_t j = lj % uint32_t(done), rt = lj / uint32_t(done);
    const uint32_t row = rt * tr + i;
    const uint32_t c = row < uint32_t(a.k) ? a.T[(int64_t(o) * a.k + row) * a.m + j] : 0u;
    if (tr > 16)
        stream[int64_t(o) * a.per_obj + l] = base + kBsjSharedOff[c];
    else
        reinterpret_cast<uint32_t *>(stream + int64_t(o) * a.per_obj)[l] = c * uint32_t(RLNC_BSJ_BLOCK_BYTES);
}

// objects x row tiles x whole column blocks, row tile fastest (the row tiles of a column block re-read its source rows
// from one XCD's L2: ragged's order, xcd_work_index for W >= 4)
template <int W>
__global__ __launch_bounds__(64 * W) void gf_stream_deliver(DeliverArgs a, const uint64_t *stream) {
    const int64_t w = W <= 2 ? int64_t(blockIdx.x) : xcd_work_index(a.total);
    const int64_t per = int64_t(a.row_tiles) * a.col_blocks;
    const int o = int(w / per);
    int done;
    if (!delivers(a, o, done)) return;
    const int l = int(w % per);
    const int rt = l % a.row_tiles, cb = l / a.row_tiles;
    const MatmulParams q = deliver_params(a, o, done, int64_t(a.col_blocks) * kBsjColBlock);
    bsj_tile<W, (W >= 4), false>(q, stream + int64_t(o) * a.per_obj, a.row_tiles, rt, cb, 0, 1u, nullptr);
}

// The columns the program above does not take: kTailRows output rows x 4 KiB of columns per workgroup, one 16-byte slot
// a lane, the multipliers 0..255 of the elimination's table in LDS (gf_perm.hpp).  The coefficients are
// workgroup-uniform (scalar loads), the table reads broadcasts.  VEC: 16-byte accesses for full slots, else single bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void gf_stream_deliver_tail(DeliverArgs a) {
    __shared__ uint32_t tab[kMulTabDw];
    const int64_t w = xcd_work_index(a.total);
    const int row_tiles = (a.k + kTailRows - 1) / kTailRows;
    const int64_t per = int64_t(row_tiles) * a.col_blocks;
    const int o = int(w / per);
    int done;
    if (!delivers(a, o, done)) return;
    const int l = int(w % per);
    const int rt = l % row_tiles, cb = l / row_tiles;
    const MatmulParams q = deliver_params(a, o, done, a.L - a.col0);
    const Tile t = make_tile_at<kTailRows>(q, rt, cb);
    copy_table(tab);
    __syncthreads();
    if (t.nbytes <= 0) return;  // behind the only barrier
    const uint8_t *in = q.in + t.col;
    const uint8_t *coef = q.coef + int64_t(t.row0) * q.coef_row;
    uint32_t acc[kTailRows][4];
#pragma unroll
    for (int i = 0; i < kTailRows; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j = 0; j < done; ++j) {
        const uint4 x = load16<VEC>(in + int64_t(j) * q.in_row, t.nbytes);
#pragma unroll
        for (int i = 0; i < kTailRows; ++i) {
            if (i >= t.rows_here) break;
            const uint32_t c = coef[int64_t(i) * q.coef_row + j];
            const uint4 tt = *reinterpret_cast<const uint4 *>(tab + c * kTabDw);
            const uint32_t t2 = tab[c * kTabDw + 4];
            acc[i][0] ^= mul4t(tt, t2, x.x);
            acc[i][1] ^= mul4t(tt, t2, x.y);
            acc[i][2] ^= mul4t(tt, t2, x.z);
            acc[i][3] ^= mul4t(tt, t2, x.w);
        }
    }
    uint8_t *out = q.out + int64_t(t.row0) * q.out_row + t.col;
#pragma unroll
    for (int i = 0; i < kTailRows; ++i)
        if (i < t.rows_here)
            store16<VEC>(out + int64_t(i) * q.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), t.nbytes);
}

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
    if (rank < a.k) {
        if (lane == 0) {
            status[o] = RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET;
            final_len[o] = 0;
        }
        return;
    }
    const int64_t len = int64_t(a.k) * a.L;
    const uint8_t *d = a.decoded + int64_t(o) * len;
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

// the launch geometry of a delivery
struct DeliverGeom {
    int W, tile_rows, row_tiles;
    int64_t per_obj;     // stream entries of one object
    int64_t entries;     // ... of all
    int64_t off_wgs;     // workgroups of the offset launch: 256 entries each, whole blocks per object
    int64_t full;        // columns the bit-sliced program takes, were every operand eligible
    int64_t prod_wgs;    // ... and its workgroups
    int64_t tail_wgs_all, tail_wgs_rest;  // the tail launch over all of L / over L - full
};
DeliverGeom deliver_geom(int k, int m, int n_obj, int64_t L) {
    DeliverGeom g{};
    g.W = bsj_waves(k, true);
    g.tile_rows = kBsjWaveRows * g.W;
    g.row_tiles = (k + g.tile_rows - 1) / g.tile_rows;
    g.per_obj = int64_t(g.row_tiles) * m * g.tile_rows;
    g.entries = g.per_obj * n_obj;
    g.off_wgs = ((g.per_obj + 255) / 256) * n_obj;
    g.full = k >= 4 ? (L / kBsjColBlock) * kBsjColBlock : 0;
    g.prod_wgs = int64_t(n_obj) * g.row_tiles * (g.full / kBsjColBlock);
    const int64_t tail_tiles = int64_t(n_obj) * ((k + kTailRows - 1) / kTailRows);
    g.tail_wgs_all = tail_tiles * ((L + kColBlock - 1) / kColBlock);
    g.tail_wgs_rest = tail_tiles * ((L - g.full + kColBlock - 1) / kColBlock);
    return g;
}

}  // namespace

size_t stream_deliver_plan_bytes(size_t k, size_t m, size_t n_obj) {
    if (rank_stream_state_bytes(k, m, n_obj) == 0) return 0;
    const DeliverGeom g = deliver_geom(int(k), int(m), int(n_obj), 0);
    // the T extract; 8 bytes a stream entry (the 1- and 2-wave programs use half) + one source: the program loads the
    // entries of the source after the last one (bsj_scratch_bytes)
    return ((n_obj * k * m + 15) & ~size_t(15)) + size_t(g.entries) * 8 + 512;
}

bool stream_deliver_fits(const DeliverParams &p) {
    const DeliverGeom g = deliver_geom(p.k, p.m, p.n_obj, p.L);
    return g.off_wgs <= 0x7FFFFFFFLL && g.prod_wgs <= 0x7FFFFFFFLL && g.tail_wgs_all <= 0x7FFFFFFFLL;
}

hipError_t launch_stream_deliver(const DeliverParams &p, const void *state, size_t state_bytes, bool unaligned_ok,
                                 hipStream_t s) {
    if (p.n_obj <= 0) return hipSuccess;
    hipError_t e = rank_state_check(p.k, p.m, p.n_obj, state, state_bytes);
    if (e != hipSuccess) return e;
    if (p.L <= 0 || p.plan == nullptr || !al16(p.plan) || !stream_deliver_fits(p)) return hipErrorInvalidValue;
    const DeliverGeom g = deliver_geom(p.k, p.m, p.n_obj, p.L);
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
    a.pieces = p.pieces;
    a.obj_stride = p.obj_stride;
    a.piece_stride = int64_t(p.k) + p.L;
    a.select = p.select;
    a.T = T;
    a.decoded = p.decoded;
    a.L = p.L;
    a.k = p.k, a.m = p.m, a.n_obj = p.n_obj;
    a.tile_rows = g.tile_rows;
    a.row_tiles = g.row_tiles;
    a.per_obj = g.per_obj;
    a.blocks_per_obj = int((g.per_obj + 255) / 256);

    // every object's operands at once: 16-byte vector accesses at any address, or all of them aligned
    const bool vec = unaligned_ok || (al16(p.pieces) && al16(p.decoded) && al16(int64_t(p.k)) && al16(p.L) &&
                                      al16(p.obj_stride));
    bool bsj = g.full > 0 && ragged_bsj_eligible(p.pieces + p.k, p.decoded, a.piece_stride, p.L, p.L, p.k, vec);
    uint64_t base = 0;
    if (bsj && g.W >= 4) {
        // the shared programs' block table (one probe per device; the stream region serves as its 8 bytes); a first
        // probe inside a capture cannot run: the tail kernel, bit-identical, takes every column this time
        if ((e = bsj_shared_base(s, stream, base)) != hipSuccess) return e;
        bsj = base != 0;
    }
    const int64_t full = bsj ? g.full : 0;
    if (bsj) {
        // 2. the block-address streams of the delivering objects
        hipLaunchKernelGGL(deliver_offset_kernel, dim3(unsigned(g.off_wgs)), dim3(256), 0, s, a, stream, base);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // 3. the bit-sliced product over the whole column blocks
        a.col_blocks = int(full / kBsjColBlock);
        a.col0 = 0;
        a.total = g.prod_wgs;
        const dim3 grid{unsigned(g.prod_wgs)};
        if (g.W == 8)
            hipLaunchKernelGGL(gf_stream_deliver<8>, grid, dim3(512), 0, s, a, stream);
        else if (g.W == 4)
            hipLaunchKernelGGL(gf_stream_deliver<4>, grid, dim3(256), 0, s, a, stream);
        else if (g.W == 2)
            hipLaunchKernelGGL(gf_stream_deliver<2>, grid, dim3(128), 0, s, a, stream);
        else
            hipLaunchKernelGGL(gf_stream_deliver<1>, grid, dim3(64), 0, s, a, stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (full < p.L) {
        // 4. the perm product over the rest
        a.col0 = full;
        a.col_blocks = int((p.L - full + kColBlock - 1) / kColBlock);
        a.total = full ? g.tail_wgs_rest : g.tail_wgs_all;
        hipLaunchKernelGGL(vec ? &gf_stream_deliver_tail<true> : &gf_stream_deliver_tail<false>, dim3(unsigned(a.total)),
                           dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // 5. status and length of the selected objects
    hipLaunchKernelGGL(vec ? &deliver_scan_kernel<true> : &deliver_scan_kernel<false>, dim3(unsigned((p.n_obj + 3) / 4)),
                       dim3(256), 0, s, a, p.status, p.len);
    return hipGetLastError();
}

}  // namespace rlnc
