// stream_product.hpp — the product of the decode-stream calls that choose their objects on the device (internal to
// librlnc_hip): the delivery (stream_deliver.hip: decoded = T x data rows, for the objects of rank k) and the relay's
// recode (stream_recode.hip: recoded = C x full pieces, for the objects of rank >= 1).  The host launches over every
// object; each workgroup reads its object's rank, done and select and returns at once unless the object takes part, so
// an object that does not costs a workgroup's start and nothing else.
//
// An object's product takes n_in = done_o source rows (the coefficient columns from done_o on are never read) and runs
// the bit-sliced engine's tile (bsj_tile.hpp) over its whole 4 KiB column blocks, as the ragged kernels of ragged.hip
// run it per object; the rest -- width mod 4096, fewer than 4 output rows, operands the program does not take -- goes to
// a perm-multiply kernel (gf_perm.hpp) over 8 rows x 4 KiB tiles.
//
// Here: the arguments of every launch, the one predicate, the device bodies of the three kernels, the geometry and the
// launch sequence.  The __global__ kernels themselves are defined by each call's file (they carry its name in a
// profile) and handed to launch_stream_product as a traits class.
//
// Rules (rank_large.hip's): the early return depends on workgroup-uniform values only (blockIdx, the state words and
// select through readfirstlane) and comes before any LDS use or barrier; no launch reads what a workgroup of the same
// launch writes; the state, the source rows and select are only read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bsj_tile.hpp"
#include "gf256.hpp"
#include "gf_perm.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"
#include "rank_state.hpp"

namespace rlnc {
namespace {

constexpr int kStreamTailRows = 8;  // output rows per workgroup of the tail kernel

// what every launch takes (by value)
struct StreamProdArgs {
    const uint32_t *ws;     // the stream's state
    int64_t ws_obj;         // dwords per object
    const uint8_t *in;      // object 0's source row 0, from the product's first column
    int64_t in_obj, in_row;
    const int32_t *select;
    const uint8_t *coef;    // [obj][n_out][m]
    uint8_t *out;           // [obj][n_out][width]
    int64_t width;          // columns of the whole product
    int n_out, m, n_obj;
    int min_rank;           // an object takes part from this rank on (the delivery: k; the recode: 1)
    int tile_rows, row_tiles;  // the bit-sliced product's
    int64_t per_obj;        // stream entries of one object: row_tiles x m x tile_rows
    int blocks_per_obj;     // ... in blocks of 256 (the offset launch)
    int col_blocks;         // column blocks of the launch (product: whole ones; tail: those of the rest)
    int64_t col0;           // first column of the launch
    int64_t total;          // workgroups of the launch
};

// whether object o takes part, and its done (workgroup-uniform when o is)
__device__ __forceinline__ bool stream_takes(const StreamProdArgs &a, int o, int &done) {
    const uint32_t *ws = a.ws + int64_t(o) * a.ws_obj;
    const int rank = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    done = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
    const int sel = a.select != nullptr ? __builtin_amdgcn_readfirstlane(a.select[o]) : 1;
    // (min_rank <= done <= m always: no source row of another object, no entry beyond an object's part of the plan)
    return sel != 0 && rank >= a.min_rank && done >= a.min_rank && done <= a.m;
}

// the product of object o (no header): its answered slots' rows in, out[o] out, columns from col0
__device__ __forceinline__ MatmulParams stream_params(const StreamProdArgs &a, int o, int done, int64_t width) {
    MatmulParams q{};
    q.in = a.in + int64_t(o) * a.in_obj + a.col0;
    q.in_row = a.in_row;
    q.coef = a.coef + int64_t(o) * a.n_out * a.m;
    q.coef_row = a.m;
    q.out = a.out + int64_t(o) * a.n_out * a.width + a.col0;
    q.out_row = a.width;
    q.n_out = a.n_out;
    q.n_in = done;
    q.width = width;
    q.n_obj = 1;
    return q;
}

// The block-address streams of the objects that take part, as ragged_offset_kernel writes an object's: entry l of
// object o = the code block of coefficient coef[o][row][j], laid out [rt][j][row in tile] for j < done_o from
// o x per_obj (8-byte units) -- its absolute address for the 4- and 8-wave programs, its 4-byte offset for the 1- and
// 2-wave ones.  One thread per entry of m columns; those past done_o, and every thread of an object that does not take
// part, return.
__device__ __forceinline__ void stream_offset_body(const StreamProdArgs &a, uint64_t *stream, uint64_t base) {
    // blocks_per_obj blocks of 256 entries an object; 32-bit arithmetic throughout (per_obj <= 2^25)
    const uint32_t o = blockIdx.x / uint32_t(a.blocks_per_obj);
    const uint32_t l = (blockIdx.x % uint32_t(a.blocks_per_obj)) * 256u + threadIdx.x;
    const uint32_t *ws = a.ws + int64_t(o) * a.ws_obj;
    const int rank = int(ws[kStRank]), done = int(ws[kStDone]);
    if (rank < a.min_rank || done < a.min_rank || done > a.m || (a.select != nullptr && a.select[o] == 0)) return;
    const uint32_t tr = uint32_t(a.tile_rows);  // 8, 16, 32 or 64
    if (l >= uint32_t(a.row_tiles) * uint32_t(done) * tr) return;
    const uint32_t i = l % tr, lj = l / tr;
    const uint32_t j = lj % uint32_t(done), rt = lj / uint32_t(done);
    const uint32_t row = rt * tr + i;
    const uint32_t c = row < uint32_t(a.n_out) ? a.coef[(int64_t(o) * a.n_out + row) * a.m + j] : 0u;
    if (tr > 16)
        stream[int64_t(o) * a.per_obj + l] = base + kBsjSharedOff[c];
    else
        reinterpret_cast<uint32_t *>(stream + int64_t(o) * a.per_obj)[l] = c * uint32_t(RLNC_BSJ_BLOCK_BYTES);
}

// objects x row tiles x whole column blocks, row tile fastest (the row tiles of a column block re-read its source rows
// from one XCD's L2: ragged's order, xcd_work_index for W >= 4)
template <int W>
__device__ __forceinline__ void stream_product_body(const StreamProdArgs &a, const uint64_t *stream) {
    const int64_t w = W <= 2 ? int64_t(blockIdx.x) : xcd_work_index(a.total);
    const int64_t per = int64_t(a.row_tiles) * a.col_blocks;
    const int o = int(w / per);
    int done;
    if (!stream_takes(a, o, done)) return;
    const int l = int(w % per);
    const int rt = l % a.row_tiles, cb = l / a.row_tiles;
    const MatmulParams q = stream_params(a, o, done, int64_t(a.col_blocks) * kBsjColBlock);
    bsj_tile<W, (W >= 4), false>(q, stream + int64_t(o) * a.per_obj, a.row_tiles, rt, cb, 0, 1u, nullptr);
}

// The columns the program above does not take: kStreamTailRows output rows x 4 KiB of columns per workgroup, one
// 16-byte slot a lane, the multipliers 0..255 of the elimination's table in LDS (tab: kMulTabDw dwords; gf_perm.hpp).
// The coefficients are workgroup-uniform (scalar loads), the table reads broadcasts.  VEC: 16-byte accesses for full
// slots, else single bytes.
template <bool VEC>
__device__ __forceinline__ void stream_tail_body(const StreamProdArgs &a, uint32_t *tab) {
    const int64_t w = xcd_work_index(a.total);
    const int row_tiles = (a.n_out + kStreamTailRows - 1) / kStreamTailRows;
    const int64_t per = int64_t(row_tiles) * a.col_blocks;
    const int o = int(w / per);
    int done;
    if (!stream_takes(a, o, done)) return;
    const int l = int(w % per);
    const int rt = l % row_tiles, cb = l / row_tiles;
    const MatmulParams q = stream_params(a, o, done, a.width - a.col0);
    const Tile t = make_tile_at<kStreamTailRows>(q, rt, cb);
    copy_table(tab);
    __syncthreads();
    if (t.nbytes <= 0) return;  // behind the only barrier
    const uint8_t *in = q.in + t.col;
    const uint8_t *coef = q.coef + int64_t(t.row0) * q.coef_row;
    uint32_t acc[kStreamTailRows][4];
#pragma unroll
    for (int i = 0; i < kStreamTailRows; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j = 0; j < done; ++j) {
        const uint4 x = load16<VEC>(in + int64_t(j) * q.in_row, t.nbytes);
#pragma unroll
        for (int i = 0; i < kStreamTailRows; ++i) {
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
    for (int i = 0; i < kStreamTailRows; ++i)
        if (i < t.rows_here)
            store16<VEC>(out + int64_t(i) * q.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), t.nbytes);
}

// the launch geometry of a product of n_out rows per object, m coefficient columns, `width` columns
struct StreamGeom {
    int W, tile_rows, row_tiles;
    int64_t per_obj;     // stream entries of one object
    int64_t entries;     // ... of all
    int64_t off_wgs;     // workgroups of the offset launch: 256 entries each, whole blocks per object
    int64_t full;        // columns the bit-sliced program takes, were every operand eligible
    int64_t prod_wgs;    // ... and its workgroups
    int64_t tail_wgs_all, tail_wgs_rest;  // the tail launch over all of width / over width - full
    bool fits() const {  // every launch within a grid (2^31 - 1 workgroups)
        return off_wgs <= 0x7FFFFFFFLL && prod_wgs <= 0x7FFFFFFFLL && tail_wgs_all <= 0x7FFFFFFFLL;
    }
};
inline StreamGeom stream_geom(int n_out, int m, int n_obj, int64_t width) {
    StreamGeom g{};
    g.W = bsj_waves(n_out, true);
    g.tile_rows = kBsjWaveRows * g.W;
    g.row_tiles = (n_out + g.tile_rows - 1) / g.tile_rows;
    g.per_obj = int64_t(g.row_tiles) * m * g.tile_rows;
    g.entries = g.per_obj * n_obj;
    g.off_wgs = ((g.per_obj + 255) / 256) * n_obj;
    g.full = n_out >= 4 ? (width / kBsjColBlock) * kBsjColBlock : 0;
    g.prod_wgs = int64_t(n_obj) * g.row_tiles * (g.full / kBsjColBlock);
    const int64_t tail_tiles = int64_t(n_obj) * ((n_out + kStreamTailRows - 1) / kStreamTailRows);
    g.tail_wgs_all = tail_tiles * ((width + kColBlock - 1) / kColBlock);
    g.tail_wgs_rest = tail_tiles * ((width - g.full + kColBlock - 1) / kColBlock);
    return g;
}
// bytes of the block-address streams in a plan buffer: 8 bytes a stream entry (the 1- and 2-wave programs use half) +
// one source: the program loads the entries of the source after the last one (bsj_scratch_bytes)
inline size_t stream_geom_bytes(const StreamGeom &g) { return size_t(g.entries) * 8 + 512; }

// the geometry's part of the arguments
inline void stream_args_geom(StreamProdArgs &a, const StreamGeom &g) {
    a.tile_rows = g.tile_rows;
    a.row_tiles = g.row_tiles;
    a.per_obj = g.per_obj;
    a.blocks_per_obj = int((g.per_obj + 255) / 256);
}

// The launches of a product on s, at most three: the block-address streams of the objects that take part, the
// bit-sliced product over the whole column blocks, the perm product over the rest.  K: the call's kernels --
// K::offset, K::product<W>, K::tail<VEC>.  vec: every object's operands take 16-byte vector accesses (at any address,
// or all of them aligned).  bsj: the operands are the program's (ragged_bsj_eligible on object 0's, which stand for
// all under vec).  stream: the plan buffer's block-address region, stream_geom_bytes(g) long.
template <class K>
hipError_t launch_stream_product(StreamProdArgs a, const StreamGeom &g, bool vec, bool bsj, uint64_t *stream,
                                 hipStream_t s) {
    hipError_t e;
    bsj = bsj && g.full > 0;
    uint64_t base = 0;
    if (bsj && g.W >= 4) {
        // the shared programs' block table (one probe per device; the stream region serves as its 8 bytes); a first
        // probe inside a capture cannot run: the tail kernel, bit-identical, takes every column this time
        if ((e = bsj_shared_base(s, stream, base)) != hipSuccess) return e;
        bsj = base != 0;
    }
    const int64_t full = bsj ? g.full : 0;
    if (bsj) {
        // the block-address streams of the objects that take part
        hipLaunchKernelGGL(K::offset, dim3(unsigned(g.off_wgs)), dim3(256), 0, s, a, stream, base);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // the bit-sliced product over the whole column blocks
        a.col_blocks = int(full / kBsjColBlock);
        a.col0 = 0;
        a.total = g.prod_wgs;
        const dim3 grid{unsigned(g.prod_wgs)};
        if (g.W == 8)
            hipLaunchKernelGGL(K::template product<8>, grid, dim3(512), 0, s, a, stream);
        else if (g.W == 4)
            hipLaunchKernelGGL(K::template product<4>, grid, dim3(256), 0, s, a, stream);
        else if (g.W == 2)
            hipLaunchKernelGGL(K::template product<2>, grid, dim3(128), 0, s, a, stream);
        else
            hipLaunchKernelGGL(K::template product<1>, grid, dim3(64), 0, s, a, stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (full < a.width) {
        // the perm product over the rest
        a.col0 = full;
        a.col_blocks = int((a.width - full + kColBlock - 1) / kColBlock);
        a.total = full ? g.tail_wgs_rest : g.tail_wgs_all;
        hipLaunchKernelGGL(vec ? K::template tail<true> : K::template tail<false>, dim3(unsigned(a.total)), dim3(256), 0,
                           s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace
}  // namespace rlnc
