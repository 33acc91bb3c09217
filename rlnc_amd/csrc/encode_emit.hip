// encode_emit.hip — the sender's emit (rlnc_encode_emit, encode_emit_call.cpp; interface: encode_emit_kernels.hpp): want[o]
// coded pieces per object, read on the device, written as one packed run of packets with an object id per packet and
// a device-side count -- what rlnc_decode_stream_accept takes.
//
// With w_o = min(max(want[o], 0), max_per), base_o = min(sum of the w before o, n) and g_o = min(w_o, n - base_o),
// packets [base_o, base_o + g_o) are object o's: out[i] = r[i] || XOR_j r[i][j] . src[o][j].  The order is object-major
// and every running sum saturates at n (n <= 2^20, w <= 4,096: int32 throughout), so the split is a prefix sum and no
// packet is claimed with an atomic.  At most six launches, ordered by the stream only:
//   scan     (a workgroup of 1,024 threads per chunk of 1,024 objects) w_o, its exclusive prefix inside the chunk and
//            the chunk's sum, into the plan.
//   base     (one workgroup of 1,024 threads) the saturating prefix over the chunk sums (<= 1,024 of them), then every
//            object's base_o and g_o into the plan, granted[o], the total into the plan and *count.
//   label    (a workgroup per 16 packets, over all n) object[i] by binary search over the bases (the last object
//            whose base is <= i), RLNC_EMIT_NONE from the total on; the k header bytes of the packets below the
//            total, byte by byte (out sits at any byte address).
//   offset   the block-address streams of the objects with g_o >= 4, as stream_offset_body writes them: [rt][j][row in
//            tile] for j < k, the coefficient 0 for rows at or beyond g_o; the row tiles at or beyond g_o are not
//            written (no workgroup reads them).
//   product  objects x row tiles x whole 4 KiB column blocks of L: bsj_tile on MatmulParams built on the device
//            (in = src[o], coef = r + base_o k, out = out + base_o out_stride + k, n_out = g_o).
//   tail     the perm multiply over 8 rows x 4 KiB tiles: L mod 4,096 for the objects the program took, all of L for
//            the objects with 1 <= g_o < 4 and for every object when the operands are not the program's.
//
// Why g_o < 4 goes to the tail: ragged_bsj_eligible refuses products of fewer than four output rows, so a whole
// product of 1-3 rows is outside what the tile programs are established for (a last tile of 1-3 live rows of a larger
// product is routine).  The grant is known on the device only, so the tail launch covers all of L for every object's
// first row tile and each workgroup decides.
//
// Rules (rank_large.hip's): the early return depends on workgroup-uniform values only (blockIdx and the plan's words
// through readfirstlane) and comes before any LDS use or barrier; no launch reads what another workgroup of the same
// launch writes; src, want and r are only read.
#include <hip/hip_runtime.h>

#include "../../include/rlnc_hip.h"
#include "bsj_tile.hpp"
#include "encode_emit_kernels.hpp"
#include "gf256.hpp"
#include "gf_perm.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"

namespace rlnc {

namespace {

constexpr int kEmitTailRows = 8;  // output rows per workgroup of the tail kernel

// what every launch takes (by value)
struct EmitArgs {
    const uint8_t *src;
    int64_t src_obj, L;
    const int32_t *want;
    const uint8_t *r;
    uint8_t *out;
    int64_t out_stride;
    int32_t *object, *count, *granted;
    int32_t *base, *grant, *csum, *total;  // the plan: [obj], [obj], [chunks], one
    int k, n_obj, max_per, n, chunks;
    int tile_rows, row_tiles;  // the bit-sliced product's, of max_per rows
    int64_t per_obj;           // stream entries of one object: row_tiles x k x tile_rows
    int blocks_per_obj;        // ... in blocks of 256 (the offset launch)
    int col_blocks;            // product: whole column blocks of L; tail: all of them, ceil(L / 4096)
    int full_blocks;           // tail: the leading column blocks the program took from the objects with g_o >= 4
    int64_t tail_per_obj;      // tail: workgroups of one object
    int64_t total_wgs;         // workgroups of the launch
};

// The inclusive prefix sum of v over the 1,024 threads of the workgroup, every partial sum saturating at cap (the
// addends are non-negative, so saturation keeps the sum associative); buf: 2 x 1,024 ints of LDS
__device__ __forceinline__ int block_scan(int v, int *buf, int cap) {
    const int tid = int(threadIdx.x);
    int cur = 0;
    buf[tid] = v;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < kEmitChunk; d <<= 1) {
        int x = buf[cur * kEmitChunk + tid];
        if (tid >= d) x = min(x + buf[cur * kEmitChunk + tid - d], cap);
        cur ^= 1;
        buf[cur * kEmitChunk + tid] = x;
        __syncthreads();
    }
    return buf[cur * kEmitChunk + tid];
}

__global__ __launch_bounds__(kEmitChunk) void gf_encode_emit_scan(EmitArgs a) {
    __shared__ int buf[2 * kEmitChunk];
    const int tid = int(threadIdx.x), o = int(blockIdx.x) * kEmitChunk + tid;
    const int w = o < a.n_obj ? min(max(a.want[o], 0), a.max_per) : 0;
    const int incl = block_scan(w, buf, 0x7FFFFFFF);  // <= 1,024 x 4,096
    if (o < a.n_obj) {
        a.base[o] = incl - w;
        a.grant[o] = w;
    }
    if (tid == kEmitChunk - 1) a.csum[blockIdx.x] = min(incl, a.n);
}

__global__ __launch_bounds__(kEmitChunk) void gf_encode_emit_base(EmitArgs a) {
    __shared__ int buf[2 * kEmitChunk];
    __shared__ int cbase[kEmitChunk + 1];  // the packets before chunk c; [chunks .. ]: the total
    const int tid = int(threadIdx.x), n = a.n;
    const int v = tid < a.chunks ? a.csum[tid] : 0;
    const int incl = block_scan(v, buf, n);
    cbase[tid + 1] = incl;
    if (tid == 0) cbase[0] = 0;
    __syncthreads();
    if (tid == 0) {
        const int total = cbase[kEmitChunk];
        *a.total = total;
        *a.count = total;
    }
    for (int c = 0; c < a.chunks; ++c) {
        const int o = c * kEmitChunk + tid;
        if (o >= a.n_obj) break;
        const int b = min(cbase[c] + a.base[o], n);  // <= 2^20 + 2^22
        const int g = min(a.grant[o], n - b);
        a.base[o] = b;
        a.grant[o] = g;
        if (a.granted != nullptr) a.granted[o] = g;
    }
}

__global__ __launch_bounds__(256) void gf_encode_emit_label(EmitArgs a) {
    const int tid = int(threadIdx.x), i0 = int(blockIdx.x) * kEmitLabelPackets;
    const int total = __builtin_amdgcn_readfirstlane(*a.total);
    if (tid < kEmitLabelPackets && i0 + tid < a.n) {
        const int i = i0 + tid;
        int id = RLNC_EMIT_NONE;
        if (i < total) {
            // the last object whose base is <= i: base_{o+1} = base_o + g_o > i, so i is one of its g_o packets
            int lo = 0, hi = a.n_obj - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (a.base[mid] <= i)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            id = lo;
        }
        a.object[i] = id;
    }
    // the headers of the workgroup's packets below the total: one run of r, k bytes a packet
    const int live = min(kEmitLabelPackets, total - i0);
    if (live <= 0) return;
    const uint32_t k = uint32_t(a.k), cells = uint32_t(live) * k;  // <= 2^16
    const uint8_t *rp = a.r + int64_t(i0) * a.k;
    uint8_t *op = a.out + int64_t(i0) * a.out_stride;
    for (uint32_t e = uint32_t(tid); e < cells; e += 256u) {
        const uint32_t p = e / k, b = e % k;
        op[int64_t(p) * a.out_stride + b] = rp[e];
    }
}

// object o's base and grant (workgroup-uniform when o is)
__device__ __forceinline__ void emit_range(const EmitArgs &a, int o, int &base, int &g) {
    base = __builtin_amdgcn_readfirstlane(a.base[o]);
    g = __builtin_amdgcn_readfirstlane(a.grant[o]);
    // (0 <= base, 0 <= g <= max_per and base + g <= n always: no row of r, no packet of out beyond the caller's)
    if (base < 0 || g < 0 || g > a.max_per || base > a.n - g) g = 0;
}

// the product of object o (no header): k source rows in, its g packets' data out
__device__ __forceinline__ MatmulParams emit_params(const EmitArgs &a, int o, int base, int g) {
    MatmulParams q{};
    q.in = a.src + int64_t(o) * a.src_obj;
    q.in_row = a.L;
    q.coef = a.r + int64_t(base) * a.k;
    q.coef_row = a.k;
    q.out = a.out + int64_t(base) * a.out_stride + a.k;
    q.out_row = a.out_stride;
    q.n_out = g;
    q.n_in = a.k;
    q.width = a.L;
    q.n_obj = 1;
    return q;
}

// blocks_per_obj blocks of 256 entries an object; 32-bit arithmetic inside an object (per_obj <= 2^24)
__global__ __launch_bounds__(256) void gf_encode_emit_offset(EmitArgs a, uint64_t *stream, uint64_t base) {
    const uint32_t o = blockIdx.x / uint32_t(a.blocks_per_obj);
    const uint32_t l = (blockIdx.x % uint32_t(a.blocks_per_obj)) * 256u + threadIdx.x;
    int b0, g;
    emit_range(a, int(o), b0, g);
    if (g < 4) return;
    const uint32_t tr = uint32_t(a.tile_rows), k = uint32_t(a.k);  // tr: 8, 16, 32 or 64
    const uint32_t live_tiles = (uint32_t(g) + tr - 1) / tr;
    if (l >= live_tiles * k * tr) return;
    const uint32_t i = l % tr, lj = l / tr;
    const uint32_t j = lj % k, rt = lj / k;
    const uint32_t row = rt * tr + i;
    const uint32_t c = row < uint32_t(g) ? a.r[(int64_t(b0) + row) * a.k + j] : 0u;
    if (tr > 16)
        stream[int64_t(o) * a.per_obj + l] = base + kBsjSharedOff[c];
    else
        reinterpret_cast<uint32_t *>(stream + int64_t(o) * a.per_obj)[l] = c * uint32_t(RLNC_BSJ_BLOCK_BYTES);
}

// objects x row tiles x whole column blocks, row tile fastest (stream_product.hpp's order)
template <int W>
__global__ __launch_bounds__(64 * W) void gf_encode_emit_product(EmitArgs a, const uint64_t *stream) {
    const int64_t w = W <= 2 ? int64_t(blockIdx.x) : xcd_work_index(a.total_wgs);
    const int64_t per = int64_t(a.row_tiles) * a.col_blocks;
    const int o = int(w / per);
    const int l = int(w % per);
    const int rt = l % a.row_tiles, cb = l / a.row_tiles;
    int base, g;
    emit_range(a, o, base, g);
    if (g < 4 || rt * a.tile_rows >= g) return;
    const MatmulParams q = emit_params(a, o, base, g);
    bsj_tile<W, (W >= 4), false>(q, stream + int64_t(o) * a.per_obj, a.row_tiles, rt, cb, 0, 1u, nullptr);
}

// An object's workgroups: its first row tile over every column block of L, then (max_per > 8) the later row tiles over
// the blocks from full_blocks on -- rows from 8 on belong to a grant >= 8, whose leading full_blocks the program took.
// A workgroup returns unless its rows are granted and its block is not the program's.
template <bool VEC>
__global__ __launch_bounds__(256) void gf_encode_emit_tail(EmitArgs a) {
    __shared__ uint32_t tab[kMulTabDw];
    const int64_t w = int64_t(blockIdx.x);
    const int o = int(w / a.tail_per_obj);
    const int64_t l = w % a.tail_per_obj;
    const int rest = a.col_blocks - a.full_blocks;
    int rt = 0, cb = int(l);
    if (l >= a.col_blocks && rest > 0) {
        rt = 1 + int((l - a.col_blocks) / rest);
        cb = a.full_blocks + int((l - a.col_blocks) % rest);
    }
    int base, g;
    emit_range(a, o, base, g);
    if (rt * kEmitTailRows >= g || (g >= 4 && cb < a.full_blocks)) return;
    const MatmulParams q = emit_params(a, o, base, g);
    const Tile t = make_tile_at<kEmitTailRows>(q, rt, cb);
    copy_table(tab);
    __syncthreads();
    if (t.nbytes <= 0) return;  // behind the only barrier
    const uint8_t *in = q.in + t.col;
    const uint8_t *coef = q.coef + int64_t(t.row0) * q.coef_row;
    uint32_t acc[kEmitTailRows][4];
#pragma unroll
    for (int i = 0; i < kEmitTailRows; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j = 0; j < q.n_in; ++j) {
        const uint4 x = load16<VEC>(in + int64_t(j) * q.in_row, t.nbytes);
#pragma unroll
        for (int i = 0; i < kEmitTailRows; ++i) {
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
    for (int i = 0; i < kEmitTailRows; ++i)
        if (i < t.rows_here)
            store16<VEC>(out + int64_t(i) * q.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), t.nbytes);
}

size_t up4_dwords(size_t v) { return (v + 3) & ~size_t(3); }

// the launch geometry of an emit
struct EmitGeom {
    int chunks;
    int W, tile_rows, row_tiles;
    int64_t per_obj;      // stream entries of one object
    int64_t label_wgs, off_wgs;
    int64_t full_blocks;  // whole column blocks of L, were every operand the program's
    int64_t all_blocks;   // ceil(L / 4096)
    int64_t prod_wgs;
    int tail_tiles;       // row tiles of the tail kernel
    // the tail launch's workgroups per object with the program taking `fb` leading blocks
    int64_t tail_per_obj(int64_t fb) const { return all_blocks + int64_t(tail_tiles - 1) * (all_blocks - fb); }
    bool fits(int n_obj) const {
        return label_wgs <= 0x7FFFFFFFLL && off_wgs <= 0x7FFFFFFFLL && prod_wgs <= 0x7FFFFFFFLL &&
               all_blocks <= 0x7FFFFFFFLL && tail_per_obj(0) <= 0x7FFFFFFFLL &&
               tail_per_obj(0) * n_obj <= 0x7FFFFFFFLL;
    }
};
EmitGeom emit_geom(int k, int max_per, int n_obj, int n, int64_t L) {
    EmitGeom g{};
    g.chunks = (n_obj + kEmitChunk - 1) / kEmitChunk;
    g.W = bsj_waves(max_per, true);
    g.tile_rows = kBsjWaveRows * g.W;
    g.row_tiles = (max_per + g.tile_rows - 1) / g.tile_rows;
    g.per_obj = int64_t(g.row_tiles) * k * g.tile_rows;
    g.label_wgs = (int64_t(n) + kEmitLabelPackets - 1) / kEmitLabelPackets;
    g.off_wgs = ((g.per_obj + 255) / 256) * n_obj;
    g.full_blocks = max_per >= 4 ? L / kBsjColBlock : 0;
    g.all_blocks = (L + kColBlock - 1) / kColBlock;
    g.prod_wgs = int64_t(n_obj) * g.row_tiles * g.full_blocks;
    g.tail_tiles = (max_per + kEmitTailRows - 1) / kEmitTailRows;
    return g;
}
// bytes of the plan's words before the block-address streams
size_t emit_words_bytes(size_t n_obj) {
    const size_t chunks = (n_obj + kEmitChunk - 1) / kEmitChunk;
    return 4 * (2 * up4_dwords(n_obj) + up4_dwords(chunks) + 4);
}

}  // namespace

size_t encode_emit_plan_bytes(size_t k, size_t max_per, size_t n_obj, size_t n) {
    if (k == 0 || k > size_t(kEmitMaxK) || max_per == 0 || max_per > size_t(kEmitMaxPerObject) || n_obj == 0 ||
        n_obj > size_t(kEmitMaxObjects) || n == 0 || n > size_t(kEmitMaxPackets))
        return 0;
    size_t bytes = emit_words_bytes(n_obj);
    if (max_per >= 4) {
        // 8 bytes a stream entry (the 1- and 2-wave programs use half) + one source: the program loads the entries of
        // the source after the last one (bsj_scratch_bytes)
        const EmitGeom g = emit_geom(int(k), int(max_per), int(n_obj), int(n), 0);
        bytes += size_t(g.per_obj) * n_obj * 8 + 512;
    }
    return bytes;
}

bool encode_emit_fits(const EmitParams &p) { return emit_geom(p.k, p.max_per, p.n_obj, p.n, p.L).fits(p.n_obj); }

hipError_t launch_encode_emit(const EmitParams &p, bool unaligned_ok, hipStream_t s) {
    if (p.n == 0 || p.n_obj == 0 || p.max_per == 0) return hipSuccess;
    if (p.k <= 0 || p.k > kEmitMaxK || p.max_per < 0 || p.max_per > kEmitMaxPerObject || p.n < 0 ||
        p.n > kEmitMaxPackets || p.n_obj < 0 || p.n_obj > kEmitMaxObjects || p.L <= 0 ||
        p.src_obj < int64_t(p.k) * p.L || p.out_stride < int64_t(p.k) + p.L || p.src == nullptr || p.want == nullptr ||
        p.r == nullptr || p.out == nullptr || p.object == nullptr || p.count == nullptr || p.plan == nullptr ||
        !al16(p.plan) || !encode_emit_fits(p))
        return hipErrorInvalidValue;
    const EmitGeom g = emit_geom(p.k, p.max_per, p.n_obj, p.n, p.L);
    hipError_t e;

    EmitArgs a{};
    a.src = p.src, a.src_obj = p.src_obj, a.L = p.L;
    a.want = p.want, a.r = p.r;
    a.out = p.out, a.out_stride = p.out_stride;
    a.object = p.object, a.count = p.count, a.granted = p.granted;
    const size_t o4 = up4_dwords(size_t(p.n_obj));
    a.base = static_cast<int32_t *>(p.plan);
    a.grant = a.base + o4;
    a.csum = a.grant + o4;
    a.total = a.csum + up4_dwords(size_t(g.chunks));
    uint64_t *stream = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(p.plan) + emit_words_bytes(size_t(p.n_obj)));
    a.k = p.k, a.n_obj = p.n_obj, a.max_per = p.max_per, a.n = p.n, a.chunks = g.chunks;
    a.tile_rows = g.tile_rows, a.row_tiles = g.row_tiles;
    a.per_obj = g.per_obj;
    a.blocks_per_obj = int((g.per_obj + 255) / 256);

    // 1. - 3. w and its prefix per chunk; base, grant, granted and the count; the labels and the headers
    hipLaunchKernelGGL(gf_encode_emit_scan, dim3(unsigned(g.chunks)), dim3(kEmitChunk), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(gf_encode_emit_base, dim3(1), dim3(kEmitChunk), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(gf_encode_emit_label, dim3(unsigned(g.label_wgs)), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    // every object's operands at once: 16-byte vector accesses at any address, or all of them aligned
    const uint8_t *data0 = p.out + p.k;
    const bool vec = unaligned_ok || (al16(p.src) && al16(p.src_obj) && al16(p.L) && al16(data0) && al16(p.out_stride));
    bool bsj = g.full_blocks > 0 && ragged_bsj_eligible(p.src, data0, p.L, p.out_stride, p.L, p.max_per, vec);
    uint64_t base = 0;
    if (bsj && g.W >= 4) {
        // the shared programs' block table (one probe per device; the stream region serves as its 8 bytes); a first
        // probe inside a capture cannot run: the tail kernel, bit-identical, takes every column this time
        if ((e = bsj_shared_base(s, stream, base)) != hipSuccess) return e;
        bsj = base != 0;
    }
    if (bsj) {
        // 4. the block-address streams of the objects granted >= 4
        hipLaunchKernelGGL(gf_encode_emit_offset, dim3(unsigned(g.off_wgs)), dim3(256), 0, s, a, stream, base);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // 5. the bit-sliced product over the whole column blocks
        a.col_blocks = int(g.full_blocks);
        a.total_wgs = g.prod_wgs;
        const dim3 grid{unsigned(g.prod_wgs)};
        if (g.W == 8)
            hipLaunchKernelGGL(gf_encode_emit_product<8>, grid, dim3(512), 0, s, a, stream);
        else if (g.W == 4)
            hipLaunchKernelGGL(gf_encode_emit_product<4>, grid, dim3(256), 0, s, a, stream);
        else if (g.W == 2)
            hipLaunchKernelGGL(gf_encode_emit_product<2>, grid, dim3(128), 0, s, a, stream);
        else
            hipLaunchKernelGGL(gf_encode_emit_product<1>, grid, dim3(64), 0, s, a, stream);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // 6. the perm product over the rest
    a.col_blocks = int(g.all_blocks);
    a.full_blocks = bsj ? int(g.full_blocks) : 0;
    a.tail_per_obj = g.tail_per_obj(a.full_blocks);
    a.total_wgs = a.tail_per_obj * p.n_obj;
    hipLaunchKernelGGL(vec ? gf_encode_emit_tail<true> : gf_encode_emit_tail<false>, dim3(unsigned(a.total_wgs)),
                       dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rlnc
