// perm_kernels.hpp — the perm-family product kernels (see kernels.hip for the dispatch; internal to librlnc_hip).
//
// GF multiply on CDNA4 without MFMA (byte-field arithmetic, not a dense FP contraction):
//   c·x = T0[x & 7] ^ T1[(x >> 3) & 7] ^ T2[x >> 6]      (3-bit split; T0/T1 8 entries, T2 4 entries)
// Each table fits in two VGPR dwords, and v_perm_b32 looks up FOUR bytes per instruction (one per byte
// lane of the selector), so one multiply-accumulate of a 32-bit word costs 3 v_perm_b32 + 1.5 v_bitop3_b32
// (3-way XOR).  The per-coefficient tables are built once per workgroup into LDS and read back as
// broadcast ds_read_b128/b32 (every lane reads the same address).  The selectors depend only on the
// source word, so they are computed once per source row and reused by all NT output rows of the tile.
//
// The LDS table build, the single-source multiply-accumulate and the accumulator zeroing are written out in each kernel
// on purpose: as __forceinline__ helpers they changed the loop bodies of every kernel here and the VGPR count of some
// (gf_matmul_stream_kernel<1, 2>: 40 -> 42, gf_matmul_perm_kernel<1, true>: 59 -> 61).  The tile decode and the
// header copy are shared; with them every kernel keeps its instructions (profiles/r14_product_isa_identity.txt).
//
// A second variant (NibbleLds) keeps the reference's 4-bit split tables (simd_mul_table.rs:36-80,
// LOW[c][x&15] ^ HIGH[c][x>>4]) in LDS and looks them up one byte per lane per ds_read_u8, i.e. the
// north-star's literal design; it is kept as the ablation baseline.
#pragma once
#include <hip/hip_runtime.h>

#include "gf256.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"

namespace rlnc {
namespace {

// main loop of the 2-source perm kernel over one coefficient chunk (tables already in LDS)
template <int NT, bool VEC>
__device__ __forceinline__ void perm_chunk(const MatmulParams &p, const uint8_t *rowp, int kc, int nbytes,
                                           const uint4 (*s_t01)[NT], const uint32_t (*s_t2)[NT], uint32_t (&acc)[NT][4]) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4 na = ld16<VEC>(rowp, nbytes);
    uint4 nb = kc > 1 ? ld16<VEC>(rowp + p.in_row, nbytes) : zero;
    for (int j = 0; j < kc; j += 2) {
        const uint4 xa = na, xb = nb;
        // software prefetch of the next row pair while this pair is multiplied
        if (j + 2 < kc) na = ld16<VEC>(rowp + int64_t(j + 2) * p.in_row, nbytes);
        nb = (j + 3 < kc) ? ld16<VEC>(rowp + int64_t(j + 3) * p.in_row, nbytes) : zero;
        const Sel a = selectors(xa);
        const Sel b = selectors(xb);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const uint4 ta = s_t01[j][i];
            const uint32_t ta2 = s_t2[j][i];
            const uint4 tb = s_t01[j + 1][i];  // zero table when j+1 == kc
            const uint32_t tb2 = s_t2[j + 1][i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t r = xor3(acc[i][q], vperm(ta.y, ta.x, a.s0[q]), vperm(ta.w, ta.z, a.s1[q]));
                r = xor3(r, vperm(ta2, ta2, a.s2[q]), vperm(tb.y, tb.x, b.s0[q]));
                acc[i][q] = xor3(r, vperm(tb.w, tb.z, b.s1[q]), vperm(tb2, tb2, b.s2[q]));
            }
        }
    }
}

// VEC: every lane owns a full, aligned 16-byte slot (all blocks but a ragged/unaligned tail)
template <int NT, bool VEC>
__global__ __launch_bounds__(kThreads) void gf_matmul_perm_kernel(MatmulParams p, int row_tiles, int col_blocks) {
    __shared__ uint4 s_t01[kKC][NT];
    __shared__ uint32_t s_t2[kKC][NT];

    const Tile t = make_tile<NT>(p, row_tiles, col_blocks);
    const uint8_t *in_base = p.in + int64_t(t.obj) * p.in_obj + t.col;
    const uint8_t *coef_base = p.coef + int64_t(t.obj) * p.coef_obj + int64_t(t.row0) * p.coef_row;

    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;

    for (int j0 = 0; j0 < p.n_in; j0 += kKC) {
        const int kc = min(kKC, p.n_in - j0);
        if (j0) __syncthreads();  // the previous chunk's tables are consumed
        for (int e = threadIdx.x; e < kKC * NT; e += kThreads) {
            const int i = e % NT, j = e / NT;
            const uint8_t c = (i < t.rows_here && j < kc) ? coef_base[int64_t(i) * p.coef_row + j0 + j] : uint8_t(0);
            const PermTable pt = make_perm_table(c);
            s_t01[j][i] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
            s_t2[j][i] = pt.t2;
        }
        __syncthreads();
        if (VEC || t.nbytes > 0)
            perm_chunk<NT, VEC>(p, in_base + int64_t(j0) * p.in_row, kc, t.nbytes, s_t01, s_t2, acc);
    }
    store_tile<NT, VEC>(p, t, acc);
    copy_header(p, t);
}

// Narrow operands (< one 4 KiB column block: the ragged k + L tail of a recode, small pieces).  The work is a
// chain over the sources, so it is latency-bound: one workgroup per (object, NT-row tile) builds the tables of ALL
// its (source, row) coefficients at once (one barrier, no per-chunk rebuild), then each lane walks the sources
// with PF source rows in flight; full 16-byte slots load and store as vectors (AL), the last partial one bytewise.
// (The perm kernel it replaces here -- two rows in flight, tables per 32-source chunk -- took 91 us for configs[3]'s
// 64-byte tail: profiles/r02_narrow_ab.txt.)
template <int NT, bool AL>
__global__ __launch_bounds__(kThreads) void gf_matmul_narrow_kernel(MatmulParams p, int row_tiles) {
    extern __shared__ uint4 narrow_lds[];  // [n_in][NT] of (t0lo, t0hi, t1lo, t1hi), then [n_in][NT] of t2
    constexpr int PF = 8;
    const int rt = int(blockIdx.x) % row_tiles, obj = int(blockIdx.x) / row_tiles;
    const int row0 = rt * NT, rows_here = min(NT, p.n_out - row0);
    uint4 *t01 = narrow_lds;
    uint32_t *t2 = reinterpret_cast<uint32_t *>(narrow_lds + p.n_in * NT);
    const uint8_t *coef_base = p.coef + int64_t(obj) * p.coef_obj + int64_t(row0) * p.coef_row;
    for (int e = threadIdx.x; e < p.n_in * NT; e += kThreads) {
        const int i = e % NT, j = e / NT;
        const PermTable pt = make_perm_table(i < rows_here ? coef_base[int64_t(i) * p.coef_row + j] : uint8_t(0));
        t01[e] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
        t2[e] = pt.t2;
    }
    if (p.hdr != nullptr) copy_header_rows(p, obj, row0, rows_here, kThreads);  // when the whole product is narrow
    __syncthreads();
    for (int64_t col = int64_t(threadIdx.x) * kBytesPerThread; col < p.width; col += int64_t(kColBlock)) {
        const int nbytes = int(min<int64_t>(kBytesPerThread, p.width - col));
        const uint8_t *in = p.in + int64_t(obj) * p.in_obj + col;
        uint32_t acc[NT][4];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
        for (int j0 = 0; j0 < p.n_in; j0 += PF) {
            uint4 x[PF];
#pragma unroll
            for (int u = 0; u < PF; ++u) x[u] = load16<AL>(in + int64_t(min(j0 + u, p.n_in - 1)) * p.in_row, nbytes);
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int j = j0 + u;
                if (j >= p.n_in) break;
                const Sel a = selectors(x[u]);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const uint4 ta = t01[j * NT + i];
                    const uint32_t ta2 = t2[j * NT + i];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[i][q] = xor3(xor3(acc[i][q], vperm(ta.y, ta.x, a.s0[q]), vperm(ta.w, ta.z, a.s1[q])),
                                         vperm(ta2, ta2, a.s2[q]), 0u);
                }
            }
        }
        uint8_t *out = p.out + int64_t(obj) * p.out_obj + int64_t(row0) * p.out_row + col;
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < rows_here)
                store16<AL>(out + int64_t(i) * p.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]),
                            nbytes);
    }
}

// Streaming variant for few output rows (n_out <= 3: one coded piece per pass is HBM-bound, ~1 multiply-add
// per source byte read): the perm kernel's arithmetic with PF source rows in flight per lane (it keeps one
// row pair), loaded non-temporally (each source byte is read once).  Whole aligned 4 KiB blocks only.

template <int NT, int PF>
__global__ __launch_bounds__(kThreads) void gf_matmul_stream_kernel(MatmulParams p, int row_tiles, int col_blocks) {
    __shared__ uint4 s_t01[kKC][NT];
    __shared__ uint32_t s_t2[kKC][NT];
    const Tile t = make_tile<NT>(p, row_tiles, col_blocks);
    const uint8_t *in_base = p.in + int64_t(t.obj) * p.in_obj + t.col;
    const uint8_t *coef_base = p.coef + int64_t(t.obj) * p.coef_obj + int64_t(t.row0) * p.coef_row;
    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j0 = 0; j0 < p.n_in; j0 += kKC) {
        const int kc = min(kKC, p.n_in - j0);
        if (j0) __syncthreads();
        for (int e = threadIdx.x; e < kKC * NT; e += kThreads) {
            const int i = e % NT, j = e / NT;
            const uint8_t c = (i < t.rows_here && j < kc) ? coef_base[int64_t(i) * p.coef_row + j0 + j] : uint8_t(0);
            const PermTable pt = make_perm_table(c);
            s_t01[j][i] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
            s_t2[j][i] = pt.t2;
        }
        __syncthreads();
        const uint8_t *rowp = in_base + int64_t(j0) * p.in_row;
        // rows past the chunk re-read its last row (in bounds, unconditional: the loads stay countable, so
        // the compiler waits for the oldest one only instead of draining all PF)
        uint4 buf[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) buf[u] = ld16_nt(rowp + int64_t(min(u, kc - 1)) * p.in_row);
        for (int jb = 0; jb < kc; jb += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int j = jb + u;
                if (j >= kc) break;
                const uint4 x = buf[u];
                buf[u] = ld16_nt(rowp + int64_t(min(j + PF, kc - 1)) * p.in_row);
                const Sel a = selectors(x);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const uint4 ta = s_t01[j][i];
                    const uint32_t ta2 = s_t2[j][i];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[i][q] = xor3(xor3(acc[i][q], vperm(ta.y, ta.x, a.s0[q]), vperm(ta.w, ta.z, a.s1[q])),
                                         vperm(ta2, ta2, a.s2[q]), 0u);
                }
            }
        }
    }
    store_tile<NT, true>(p, t, acc);
    copy_header(p, t);
}


// One-block streaming form with VW 16-byte slots per lane (slot v at column v * 4 KiB of a VW * 4 KiB block:
// every table read feeds VW x the bytes, VW x PF loads in flight per lane) and optionally 64-bit-shift selectors.
// tail > 0: the grid carries one more workgroup per (object, row tile) after the blocks, for the ragged tail of
// `tail` (< 4 KiB) bytes at column p.width -- saves the tail's own launch (≈ 13 us of a one-piece encode call)
template <int NT>
__device__ __forceinline__ void stream_tail(const MatmulParams &p, int row_tiles, int64_t tail, int64_t u,
                                            const uint4 (*s_t01)[NT], const uint32_t (*s_t2)[NT]) {
    const int obj = int(u / row_tiles), rt = int(u % row_tiles);
    const int row0 = rt * NT, rows_here = min(NT, p.n_out - row0), kc = p.n_in;
    const int64_t col = p.width + int64_t(threadIdx.x) * kBytesPerThread;
    const int nbytes = int(max<int64_t>(0, min<int64_t>(kBytesPerThread, p.width + tail - col)));
    if (nbytes == 0) return;
    const uint8_t *rowp = p.in + int64_t(obj) * p.in_obj + col;
    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;
    for (int j0 = 0; j0 < kc; j0 += 4) {  // four source rows in flight
        uint4 x[4];
#pragma unroll
        for (int u2 = 0; u2 < 4; ++u2) x[u2] = load16<true>(rowp + int64_t(min(j0 + u2, kc - 1)) * p.in_row, nbytes);
#pragma unroll
        for (int u2 = 0; u2 < 4; ++u2) {
            const int j = j0 + u2;
            if (j >= kc) break;
            const Sel a = selectors(x[u2]);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const uint4 ta = s_t01[j][i];
                const uint32_t ta2 = s_t2[j][i];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[i][q] = xor3(xor3(acc[i][q], vperm(ta.y, ta.x, a.s0[q]), vperm(ta.w, ta.z, a.s1[q])),
                                     vperm(ta2, ta2, a.s2[q]), 0u);
            }
        }
    }
    uint8_t *outp = p.out + int64_t(obj) * p.out_obj + int64_t(row0) * p.out_row + col;
#pragma unroll
    for (int i = 0; i < NT; ++i)
        if (i < rows_here)
            store16<true>(outp + int64_t(i) * p.out_row, make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), nbytes);
}

template <int NT, int PF, int VW, bool SH64>
__global__ __launch_bounds__(kThreads) void gf_matmul_stream3_kernel(MatmulParams p, int row_tiles, int col_blocks,
                                                                     int64_t tail) {
    __shared__ uint4 s_t01[kKC][NT];
    __shared__ uint32_t s_t2[kKC][NT];
    const int64_t blocks = int64_t(p.n_obj) * row_tiles * col_blocks;
    if (int64_t(blockIdx.x) >= blocks) {  // a ragged-tail workgroup: its tables, then the tail
        const int64_t u = int64_t(blockIdx.x) - blocks;
        const int rt = int(u % row_tiles), obj = int(u / row_tiles), row0 = rt * NT;
        const int rows_here = min(NT, p.n_out - row0);
        const uint8_t *coef_base = p.coef + int64_t(obj) * p.coef_obj + int64_t(row0) * p.coef_row;
        for (int e = threadIdx.x; e < kKC * NT; e += kThreads) {
            const int i = e % NT, j = e / NT;
            const uint8_t c = (i < rows_here && j < p.n_in) ? coef_base[int64_t(i) * p.coef_row + j] : uint8_t(0);
            const PermTable pt = make_perm_table(c);
            s_t01[j][i] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
            s_t2[j][i] = pt.t2;
        }
        __syncthreads();
        stream_tail<NT>(p, row_tiles, tail, u, s_t01, s_t2);
        return;
    }
    int rt, cb, obj;
    decode_block(int(blocks), row_tiles, col_blocks, rt, cb, obj);
    const int row0 = rt * NT;
    const int rows_here = min(NT, p.n_out - row0);
    const int kc = p.n_in;
    const uint8_t *rowp = p.in + int64_t(obj) * p.in_obj + int64_t(cb) * kColBlock * VW + threadIdx.x * kBytesPerThread;
    uint4 buf[PF][VW];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int v = 0; v < VW; ++v) buf[u][v] = ld16_nt(rowp + int64_t(min(u, kc - 1)) * p.in_row + v * kColBlock);
    const uint8_t *coef_base = p.coef + int64_t(obj) * p.coef_obj + int64_t(row0) * p.coef_row;
    for (int e = threadIdx.x; e < kKC * NT; e += kThreads) {
        const int i = e % NT, j = e / NT;
        const uint8_t c = (i < rows_here && j < kc) ? coef_base[int64_t(i) * p.coef_row + j] : uint8_t(0);
        const PermTable pt = make_perm_table(c);
        s_t01[j][i] = make_uint4(pt.t0lo, pt.t0hi, pt.t1lo, pt.t1hi);
        s_t2[j][i] = pt.t2;
    }
    __syncthreads();
    uint32_t acc[NT][VW][4];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int v = 0; v < VW; ++v) acc[i][v][0] = acc[i][v][1] = acc[i][v][2] = acc[i][v][3] = 0u;
    for (int jb = 0; jb < kc; jb += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int j = jb + u;
            if (j >= kc) break;
            Sel a[VW];
#pragma unroll
            for (int v = 0; v < VW; ++v) {
                a[v] = SH64 ? selectors64(buf[u][v]) : selectors(buf[u][v]);
                buf[u][v] = ld16_nt(rowp + int64_t(min(j + PF, kc - 1)) * p.in_row + v * kColBlock);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const uint4 ta = s_t01[j][i];
                const uint32_t ta2 = s_t2[j][i];
#pragma unroll
                for (int v = 0; v < VW; ++v)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[i][v][q] = xor3(xor3(acc[i][v][q], vperm(ta.y, ta.x, a[v].s0[q]), vperm(ta.w, ta.z, a[v].s1[q])),
                                            vperm(ta2, ta2, a[v].s2[q]), 0u);
            }
        }
    }
    uint8_t *outp = p.out + int64_t(obj) * p.out_obj + int64_t(row0) * p.out_row + int64_t(cb) * kColBlock * VW +
                    threadIdx.x * kBytesPerThread;
#pragma unroll
    for (int i = 0; i < NT; ++i)
        if (i < rows_here)
#pragma unroll
            for (int v = 0; v < VW; ++v)
                *reinterpret_cast<uint4 *>(outp + int64_t(i) * p.out_row + v * kColBlock) =
                    make_uint4(acc[i][v][0], acc[i][v][1], acc[i][v][2], acc[i][v][3]);
    if (p.hdr != nullptr && cb == 0) copy_header_rows(p, obj, row0, rows_here, kThreads);
}

// Ablation baseline: the reference's 4-bit split (LOW/HIGH nibble tables, simd_mul_table.rs:36-80) in
// LDS, one ds_read_u8 per nibble per byte per lane.
template <int NT, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void gf_matmul_nibble_kernel(MatmulParams p, int row_tiles, int col_blocks) {
    __shared__ uint8_t s_tab[kKC][NT][32];  // [0:16) LOW[c][i]=c·i, [16:32) HIGH[c][i]=c·(i<<4)

    int rt, cb, obj;
    decode_block(p.n_obj * row_tiles * col_blocks, row_tiles, col_blocks, rt, cb, obj);
    const int row0 = rt * NT;
    const int rows_here = min(NT, p.n_out - row0);
    const int64_t col = int64_t(cb) * kColBlock + int64_t(threadIdx.x) * kBytesPerThread;
    const int nbytes = col < p.width ? int(min<int64_t>(kBytesPerThread, p.width - col)) : 0;
    const uint8_t *in_base = p.in + int64_t(obj) * p.in_obj + col;
    const uint8_t *coef_base = p.coef + int64_t(obj) * p.coef_obj + int64_t(row0) * p.coef_row;

    uint32_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0u;

    for (int j0 = 0; j0 < p.n_in; j0 += kKC) {
        const int kc = min(kKC, p.n_in - j0);
        if (j0) __syncthreads();
        for (int e = threadIdx.x; e < kKC * NT * 16; e += kThreads) {
            const int v = e & 15, i = (e >> 4) % NT, j = (e >> 4) / NT;
            const uint8_t c = (i < rows_here && j < kc) ? coef_base[int64_t(i) * p.coef_row + j0 + j] : uint8_t(0);
            s_tab[j][i][v] = gf_mul_slow(c, uint8_t(v));
            s_tab[j][i][16 + v] = gf_mul_slow(c, uint8_t(v << 4));
        }
        __syncthreads();
        if (nbytes > 0) {
            for (int j = 0; j < kc; ++j) {
                const uint4 x = load16<ALIGNED>(in_base + int64_t(j0 + j) * p.in_row, nbytes);
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const uint8_t *t = s_tab[j][i];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t r = 0;
#pragma unroll
                        for (int bb = 0; bb < 4; ++bb) {
                            const uint32_t byte = (w[q] >> (8 * bb)) & 0xFFu;
                            r |= uint32_t(t[byte & 15] ^ t[16 + (byte >> 4)]) << (8 * bb);
                        }
                        acc[i][q] ^= r;
                    }
                }
            }
        }
    }
    if (nbytes > 0) {
        uint8_t *out_base = p.out + int64_t(obj) * p.out_obj + int64_t(row0) * p.out_row + col;
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < rows_here)
                store16<ALIGNED>(out_base + int64_t(i) * p.out_row,
                                 make_uint4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]), nbytes);
    }
    if (p.hdr != nullptr && cb == 0) copy_header_rows(p, obj, row0, rows_here, kThreads);
}

}  // namespace
}  // namespace rlnc
