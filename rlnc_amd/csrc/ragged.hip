// ragged.hip — ragged batches (wire.hip: rlnc_encode_ragged / rlnc_recode_ragged / rlnc_decode_ragged): objects of
// different shapes and buffers in ONE launch per kernel stage, driven by a device-side descriptor table (RaggedObj,
// kernels.hpp).  A workgroup finds its object by binary search over the objects' first workgroups (wg0), then runs
// exactly the tile the uniform kernels of kernels.hip run for that object.
#include <hip/hip_runtime.h>

#include "../../include/rlnc_hip.h"
#include "bsj_tile.hpp"
#include "gf256.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"

namespace rlnc {

namespace {

// the object of workgroup w (workgroup-uniform): the last one whose first workgroup is <= w (wg0 ascends)
__device__ __forceinline__ int ragged_find(const RaggedObj *objs, int n, int64_t w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (objs[mid].wg0 <= w)
            lo = mid;
        else
            hi = mid - 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ MatmulParams ragged_params(const RaggedObj &d) {
    MatmulParams q{};
    q.in = d.in + d.col0;
    q.coef = d.coef;
    q.out = d.out + d.col0;
    q.hdr = d.hdr;
    q.in_row = d.in_row;
    q.coef_row = d.coef_row;
    q.out_row = d.out_row;
    q.hdr_row = d.hdr_row;
    q.n_out = d.n_out;
    q.n_in = d.n_in;
    q.width = d.width;
    q.n_obj = 1;
    return q;
}

// the block-address stream of every object of the table (all wave classes at once): entry e of object o is the
// code block of coefficient c = coef[row][j] (0 past n_out), laid out [rt][j][row in tile] from objs[o].idx0 (in
// 8-byte units), as bsj_offset_kernel lays out one object -- its absolute address for the 4- and 8-wave classes, its
// 4-byte offset for the 1- and 2-wave ones (whose half-used space the table still reserves at 8 bytes an entry)
__global__ __launch_bounds__(256) void ragged_offset_kernel(const RaggedObj *objs, int n, int64_t entries,
                                                            uint64_t *stream, uint64_t base) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= entries) return;
    // ragged_find's search over idx0, per lane; written out: through a shared helper the compiler commutes the operands
    // of the loop's v_add3_u32, and this kernel keeps the parent's instructions to the letter
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (objs[mid].idx0 <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    const RaggedObj &d = objs[lo];
    const int64_t l = e - d.idx0;
    const int tr = d.tile_rows;
    const int i = int(l % tr);
    const int j = int((l / tr) % d.n_in);
    const int rt = int(l / (int64_t(tr) * d.n_in));
    const int row = rt * tr + i;
    const uint32_t c = row < d.n_out ? d.coef[int64_t(row) * d.coef_row + j] : 0u;
    if (tr > 16)  // the shared-set programs (4 and 8 waves): absolute block addresses
        stream[e] = base + kBsjSharedOff[c];
    else  // 1 and 2 waves: block offsets, 4 bytes each, packed from the object's first entry
        reinterpret_cast<uint32_t *>(stream + d.idx0)[l] = c * uint32_t(RLNC_BSJ_BLOCK_BYTES);
}

template <int W>
__global__ __launch_bounds__(64 * W) void gf_matmul_bsj_ragged_kernel(const RaggedObj *objs, int n, int64_t total,
                                                                      const uint64_t *stream) {
    // 1 and 2 waves: objects of <= 16 rows have one row tile, so no two workgroups share source rows (nothing for an
    // XCD's L2 to keep); the table lists them by source count, most first, and the launch order spreads them over the
    // XCDs and CUs as they come -- the long tiles start first and side by side, not wherever an XCD's contiguous range
    // of the launch happens to hold them (8-row recodes of 16-130 sources: profiles/r04_ragged_ab.txt)
    const int64_t w = W <= 2 ? int64_t(blockIdx.x) : xcd_work_index(total);
    const int o = ragged_find(objs, n, w);
    const RaggedObj &d = objs[o];
    const int64_t l = w - d.wg0;
    const int rt = int(l % d.row_tiles), cb = int(l / d.row_tiles);
    const MatmulParams q = ragged_params(d);
    bsj_tile<W, (W >= 4), false>(q, stream + d.idx0, d.row_tiles, rt, cb, 0, 1u, nullptr);
}

// tails and shapes the bit-sliced program does not take: the perm kernel's tile on one object (byte-granular
// loads, vector ones for full slots of an aligned object).  Like the kernels of perm_kernels.hpp, the two tiles keep
// the table build, the multiply and the accumulator zeroing written out (see there).
template <bool AL>
__device__ __forceinline__ void perm_ragged_tile(const MatmulParams &q, int rt, int cb) {
    constexpr int NT = kRaggedPermRows;
    __shared__ uint4 s_t01[kKC][NT];
    __shared__ uint32_t s_t2[kKC][NT];
    const Tile t = make_tile_at<NT>(q, rt, cb);
    const uint8_t *in_base = q.in + t.col;
    const uint8_t *coef_base = q.coef + int64_t(t.row0) * q.coef_row;
    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j0 = 0; j0 < q.n_in; j0 += kKC) {
        const int kc = min(kKC, q.n_in - j0);
        if (j0) __syncthreads();
        for (int e = threadIdx.x; e < kKC * NT; e += kThreads) {
            const int i = e % NT, j = e / NT;
            const uint8_t c = (i < t.rows_here && j < kc) ? coef_base[int64_t(i) * q.coef_row + j0 + j] : uint8_t(0);
            const PermTable pt = make_perm_table(c);
            s_t01[j][i] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
            s_t2[j][i] = pt.t2;
        }
        __syncthreads();
        if (t.nbytes > 0) {
            const uint8_t *rowp = in_base + int64_t(j0) * q.in_row;
            for (int j = 0; j < kc; ++j) {
                const uint4 x = load16<AL>(rowp + int64_t(j) * q.in_row, t.nbytes);
                const Sel a = selectors(x);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const uint4 ta = s_t01[j][i];
                    const uint32_t ta2 = s_t2[j][i];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
                        acc[i][qq] = xor3(xor3(acc[i][qq], vperm(ta.y, ta.x, a.s0[qq]), vperm(ta.w, ta.z, a.s1[qq])),
                                          vperm(ta2, ta2, a.s2[qq]), 0u);
                }
            }
        }
    }
    if (t.nbytes > 0) {
        uint8_t *out_base = q.out + int64_t(t.row0) * q.out_row + t.col;
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < t.rows_here)
                store16<AL>(out_base + int64_t(i) * q.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]),
                            t.nbytes);
    }
    copy_header(q, t);
}

// A partial column block (the < 4 KiB tail of an object -- a recode's k coefficient bytes after its bit-sliced
// blocks, a narrow piece): S = ceil(bytes / 16) slots, so a one-lane-per-slot tile leaves most of the workgroup idle
// and walks all n_in sources one dependent load after another (~1 us each: 124 us for the 130-source recode tails of
// scripts/ragged_rate.py).  Here the sources are split over G = min(256 / S2, 32) lane groups (S2 = S rounded up to a
// power of two): group g takes sources g, g + G, ... with PF rows in flight, each lane builds the perm tables of its
// (row, source) coefficients in registers (no LDS table chunks, no barriers in the loop), and the G partial products
// are XOR-reduced through LDS.
template <bool AL>
__device__ __forceinline__ void perm_ragged_split_tile(const MatmulParams &q, int rt, int cb, uint4 *red) {
    constexpr int NT = kRaggedPermRows, PF = 4;
    const int tid = threadIdx.x;
    const int64_t c0 = int64_t(cb) * kColBlock;
    const int S = int((min<int64_t>(kColBlock, q.width - c0) + 15) / 16);
    int lg = 0;
    while ((1 << lg) < S) ++lg;
    const int S2 = 1 << lg, G = min(kThreads >> lg, 32);
    const int slot = tid & (S2 - 1), g = tid >> lg;
    const int row0 = rt * NT, rows_here = min(NT, q.n_out - row0);
    const int64_t col = c0 + int64_t(slot) * kBytesPerThread;
    const int nbytes = (g < G && slot < S) ? int(min<int64_t>(kBytesPerThread, q.width - col)) : 0;
    const uint8_t *coef_base = q.coef + int64_t(row0) * q.coef_row;
    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    if (nbytes > 0) {
        const uint8_t *in = q.in + col;
        for (int j0 = g; j0 < q.n_in; j0 += G * PF) {
            uint4 x[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u)  // clamped: past n_in re-read the last source (its product is skipped)
                x[u] = load16<AL>(in + int64_t(min(j0 + u * G, q.n_in - 1)) * q.in_row, nbytes);
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int j = j0 + u * G;
                if (j >= q.n_in) break;
                const Sel a = selectors(x[u]);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    if (i >= rows_here) break;
                    uint32_t t0lo, t0hi, t1lo, t1hi, t2;
                    perm_table_regs(coef_base[int64_t(i) * q.coef_row + j], t0lo, t0hi, t1lo, t1hi, t2);
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
                        acc[i][qq] = xor3(xor3(acc[i][qq], vperm(t0hi, t0lo, a.s0[qq]), vperm(t1hi, t1lo, a.s1[qq])),
                                          vperm(t2, t2, a.s2[qq]), 0u);
                }
            }
        }
    }
    if (G > 1) {  // red[i][g][slot]: the G partials of row i, slot
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (g < G) red[(i * G + g) * S2 + slot] = make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        __syncthreads();
    }
    // output (row i, slot): one lane each, XOR of its G partials
    for (int e = tid; e < NT * S2; e += kThreads) {
        const int i = e >> lg, sl = e & (S2 - 1);
        if (i >= rows_here || sl >= S) continue;
        const int64_t oc = c0 + int64_t(sl) * kBytesPerThread;
        const int nb = int(min<int64_t>(kBytesPerThread, q.width - oc));
        uint4 v;
        if (G > 1) {
            v = red[(i * G) * S2 + sl];
            for (int gg = 1; gg < G; ++gg) {
                const uint4 r = red[(i * G + gg) * S2 + sl];
                v.x ^= r.x;
                v.y ^= r.y;
                v.z ^= r.z;
                v.w ^= r.w;
            }
        } else {  // G = 1 (S2 = 256): lane e = slot e holds row i's product itself
            v = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int ii = 0; ii < NT; ++ii)
                if (ii == i) v = make_uint4(acc[ii][0], acc[ii][1], acc[ii][2], acc[ii][3]);
        }
        store16<AL>(q.out + int64_t(row0 + i) * q.out_row + oc, v, nb);
    }
    copy_header(q, make_tile_at<NT>(q, rt, cb));
}

__global__ __launch_bounds__(kThreads) void gf_matmul_perm_ragged_kernel(const RaggedObj *objs, int n, int64_t total) {
    // the split tile's partials: NT rows x 256 lanes x 16 bytes at most (G x S2 <= 256)
    __shared__ uint4 red[kRaggedPermRows * kThreads];
    const int64_t w = xcd_work_index(total);
    const int o = ragged_find(objs, n, w);
    const RaggedObj &d = objs[o];
    const int64_t l = w - d.wg0;
    const int rt = int(l % d.row_tiles), cb = int(l / d.row_tiles);
    const MatmulParams q = ragged_params(d);
    const bool partial = q.width - int64_t(cb) * kColBlock < kColBlock;  // workgroup-uniform
    if (partial) {
        if (d.aligned)
            perm_ragged_split_tile<true>(q, rt, cb, red);
        else
            perm_ragged_split_tile<false>(q, rt, cb, red);
    } else if (d.aligned) {
        perm_ragged_tile<true>(q, rt, cb);
    } else {
        perm_ragged_tile<false>(q, rt, cb);
    }
}

}  // namespace

bool ragged_bsj_eligible(const uint8_t *in, const uint8_t *out, int64_t in_row, int64_t out_row, int64_t width,
                         int n_out, bool unaligned_ok) {
    return (unaligned_ok || (al16(in) && al16(out) && al16(in_row) && al16(out_row))) && width >= kBsjColBlock &&
           n_out >= 4 && in_row >= 0 && in_row < (int64_t(1) << 32) && out_row >= 0 &&
           out_row < (int64_t(1) << 32);  // the tile assembly's unsigned 32-bit row strides (bsj_tile.hpp)
}

hipError_t launch_ragged_offsets(const RaggedObj *objs, int n, int64_t entries, void *stream, uint64_t base,
                                 hipStream_t s) {
    if (entries <= 0) return hipSuccess;
    if ((entries + 255) / 256 > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_offset_kernel, dim3(unsigned((entries + 255) / 256)), dim3(256), 0, s, objs, n, entries,
                       static_cast<uint64_t *>(stream), base);
    return hipGetLastError();
}

hipError_t launch_ragged_bsj(int W, const RaggedObj *objs, int n, int64_t wgs, const void *stream, hipStream_t s) {
    if (wgs <= 0) return hipSuccess;
    if (wgs > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const uint64_t *st = static_cast<const uint64_t *>(stream);
    if (W == 8)
        hipLaunchKernelGGL(gf_matmul_bsj_ragged_kernel<8>, dim3(unsigned(wgs)), dim3(512), 0, s, objs, n, wgs, st);
    else if (W == 4)
        hipLaunchKernelGGL(gf_matmul_bsj_ragged_kernel<4>, dim3(unsigned(wgs)), dim3(256), 0, s, objs, n, wgs, st);
    else if (W == 2)
        hipLaunchKernelGGL(gf_matmul_bsj_ragged_kernel<2>, dim3(unsigned(wgs)), dim3(128), 0, s, objs, n, wgs, st);
    else if (W == 1)
        hipLaunchKernelGGL(gf_matmul_bsj_ragged_kernel<1>, dim3(unsigned(wgs)), dim3(64), 0, s, objs, n, wgs, st);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_ragged_perm(const RaggedObj *objs, int n, int64_t wgs, hipStream_t s) {
    if (wgs <= 0) return hipSuccess;
    if (wgs > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gf_matmul_perm_ragged_kernel, dim3(unsigned(wgs)), dim3(kThreads), 0, s, objs, n, wgs);
    return hipGetLastError();
}

}  // namespace rlnc
