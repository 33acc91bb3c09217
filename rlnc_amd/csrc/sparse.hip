// sparse.hip — the sparse product on the device (see sparse_kernels.hpp and the "Sparse coding vectors" block of
// include/rlnc_hip.h for the format and its rules).
//
// The work is w source rows gathered, multiplied and XORed per output row: a memory-bound gather, where the dense
// programs of kernels.hip stage all n_in source rows per row tile.  One workgroup of 256 threads takes (object, 4 KiB
// column block, tile of kSparseRows output rows), each lane one 16-byte column slot; nothing is shared between the
// waves (no LDS, no barrier), so a wave past the operand's width simply leaves.  Whole 16-byte slots go to the vector
// instantiation; a row's last partial slot -- or every slot, for misaligned rows on a device without unaligned vector
// access -- goes to the byte-granular one in a second launch.
//   entries  a row's (index, value) pairs are loaded 64 at a time, one per lane (one coalesced load each), and a
//            ballot keeps the ones that count (value nonzero, index unsigned-below n_in): padding and out-of-range
//            entries cost nothing and never form an address.  The kept ones are walked with readlane, so index and
//            coefficient are scalar.
//   product  the coefficient's 3-bit-split perm tables come from a constant table through scalar loads (five scalar
//            registers), the source slot's selectors are built once, 12 v_perm + 8 XOR3/XOR per 16 bytes; coefficient
//            1 is a plain XOR.
//   gather   kSparsePF (4) source loads are issued per group and the next group's before the current one is
//            multiplied: up to 8 16-byte loads in flight per lane (the loop is a dependent chain otherwise).
//   header   hdr[i][j] = XOR of the row's values at index j: wave v of the tile's first column block takes row v;
//            lane l owns columns l, l + 64, ... and folds the row's entries, in entry order, into its byte.  Every
//            header byte has one owner: no atomics, duplicates exact.
// Workgroups are ordered by decode_block: the row tiles of one column block run on one XCD and share its L2.
#include "sparse_kernels.hpp"

#include "kernels_common.hpp"

namespace rlnc {

namespace {

// source loads per group: 4 slots on the vector path, 2 on the byte-granular one (16 byte loads per slot there)
template <bool VEC>
constexpr int kSparsePF = VEC ? 4 : 2;

__device__ __forceinline__ uint64_t wave_ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

// The 3-bit-split perm tables of every multiplier (make_perm_table's five dwords, at a stride of 8), built at compile
// time.  An entry's coefficient is scalar, so its table comes through two scalar loads issued beside the entry's
// gather; building it in scalar registers instead (perm_table_regs, ~60 scalar instructions per entry and wave on the
// CU's one scalar unit) held the kernel at 7-8 TB/s of gathered bytes (profiles/r08_sparse_product_salu.jsonl).
struct SparseTab {
    uint32_t v[256 * 8];
};
constexpr SparseTab build_sparse_tab() {
    SparseTab t{};
    for (int c = 0; c < 256; ++c) {
        uint32_t m[8] = {};
        m[0] = uint32_t(c);
        for (int b = 1; b < 8; ++b) m[b] = gf_xtime(uint8_t(m[b - 1]));
        uint32_t *e = t.v + c * 8;
        e[0] = (m[0] << 8) | (m[1] << 16) | ((m[0] ^ m[1]) << 24);
        e[1] = e[0] ^ (m[2] * 0x01010101u);
        e[2] = (m[3] << 8) | (m[4] << 16) | ((m[3] ^ m[4]) << 24);
        e[3] = e[2] ^ (m[5] * 0x01010101u);
        e[4] = (m[6] << 8) | (m[7] << 16) | ((m[6] ^ m[7]) << 24);
    }
    return t;
}
__constant__ SparseTab kSparseTab = build_sparse_tab();
static_assert(build_sparse_tab().v[1 * 8 + 0] == 0x03020100u && build_sparse_tab().v[1 * 8 + 1] == 0x07060504u &&
                  build_sparse_tab().v[1 * 8 + 2] == 0x18100800u && build_sparse_tab().v[1 * 8 + 4] == 0xC0804000u,
              "multiplier 1 is the identity");
static_assert(build_sparse_tab().v[2 * 8 + 4] == 0x9B1B8000u, "2 * 0x40 = 0x80, 2 * 0x80 = 0x1B");

struct SparseCoef {
    uint32_t c;  // 0 = no entry
    uint32_t t0lo, t0hi, t1lo, t1hi, t2;
};

// acc ^= c · x for a scalar coefficient c != 0
__device__ __forceinline__ void sparse_mac(uint32_t (&acc)[4], uint4 x, const SparseCoef &k) {
    if (k.c == 1u) {
        acc[0] ^= x.x;
        acc[1] ^= x.y;
        acc[2] ^= x.z;
        acc[3] ^= x.w;
        return;
    }
    const Sel s = selectors(x);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        acc[q] = xor3(acc[q], vperm(k.t0hi, k.t0lo, s.s0[q]), vperm(k.t1hi, k.t1lo, s.s1[q])) ^
                 vperm(k.t2, k.t2, s.s2[q]);
}

// This lane's slot of a source row.  The byte-granular form (a partial last slot, or rows the device cannot read as
// misaligned vectors) reads inside [p, p + nbytes) only, all 16 byte loads in flight at once: the address of a byte past
// nbytes is clamped to the last valid one and its value dropped, where per-byte branches would wait for each load.
template <bool VEC>
__device__ __forceinline__ uint4 sparse_ld16(const uint8_t *p, int nbytes) {
    if (VEC) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (nbytes > 0) {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint32_t v = p[min(b, nbytes - 1)];
            w[b >> 2] |= (b < nbytes ? v : 0u) << (8 * (b & 3));
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the next up to kSparsePF<VEC> kept entries of the chunk (mk: their lanes): coefficients into c (0 = no entry) and their
// source slots requested into x
template <bool VEC>
__device__ __forceinline__ void sparse_fetch(const uint8_t *in_base, int64_t in_row, int nbytes, int32_t ej, uint32_t ev,
                                             uint64_t &mk, uint4 (&x)[kSparsePF<VEC>], SparseCoef (&c)[kSparsePF<VEC>]) {
#pragma unroll
    for (int u = 0; u < kSparsePF<VEC>; ++u) {
        c[u] = SparseCoef{0u, 0u, 0u, 0u, 0u, 0u};
        x[u] = make_uint4(0, 0, 0, 0);
        if (mk != 0) {
            const int l = __builtin_ctzll(mk);
            mk &= mk - 1;
            const int64_t j = int64_t(uint32_t(__builtin_amdgcn_readlane(ej, l)));
            const uint32_t cv = uint32_t(__builtin_amdgcn_readlane(int(ev), l));
            const uint32_t *e = kSparseTab.v + cv * 8;
            c[u] = SparseCoef{cv, e[0], e[1], e[2], e[3], e[4]};
            x[u] = sparse_ld16<VEC>(in_base + j * in_row, nbytes);
        }
    }
}

template <int PF>
__device__ __forceinline__ void sparse_group(uint32_t (&acc)[4], const uint4 (&x)[PF], const SparseCoef (&c)[PF]) {
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (c[u].c != 0u) sparse_mac(acc, x[u], c[u]);
}

template <bool VEC>
__device__ __forceinline__ void sparse_rows(const SparseMatmulParams &p, int obj, int row0, int rows_here, int64_t col,
                                            int nbytes) {
    const int lane = int(threadIdx.x) & 63;
    const uint8_t *in_base = p.in + int64_t(obj) * p.in_obj + col;
    uint8_t *out_base = p.out + int64_t(obj) * p.out_obj + col;
    for (int i = 0; i < rows_here; ++i) {
        const int64_t row = row0 + i;
        const uint8_t *ib = reinterpret_cast<const uint8_t *>(p.idx) + int64_t(obj) * p.idx_obj + row * p.idx_row;
        const uint8_t *vb = p.val + int64_t(obj) * p.val_obj + row * p.val_row;
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        // (loading a row's entries a chunk ahead, under the previous row's gathers, measured no faster at any w:
        // profiles/r08_sparse_product_entry_prefetch.jsonl)
        for (int t0 = 0; t0 < p.w; t0 += 64) {
            const int t = t0 + lane;
            int32_t ej = -1;
            uint32_t ev = 0u;
            if (t < p.w) {
                ej = *reinterpret_cast<const int32_t *>(ib + int64_t(t) * 4);
                ev = vb[t];
            }
            // the guard: one unsigned compare, before any address is formed
            uint64_t mk = wave_ballot(ev != 0u && uint32_t(ej) < uint32_t(p.n_in));
            // two groups alternate (no register copies: a copy would wait for the load it copies)
            uint4 xa[kSparsePF<VEC>], xb[kSparsePF<VEC>];
            SparseCoef ca[kSparsePF<VEC>], cb[kSparsePF<VEC>];
            sparse_fetch<VEC>(in_base, p.in_row, nbytes, ej, ev, mk, xa, ca);
            while (ca[0].c != 0u) {
                sparse_fetch<VEC>(in_base, p.in_row, nbytes, ej, ev, mk, xb, cb);
                sparse_group(acc, xa, ca);
                if (cb[0].c == 0u) break;
                sparse_fetch<VEC>(in_base, p.in_row, nbytes, ej, ev, mk, xa, ca);
                sparse_group(acc, xb, cb);
            }
        }
        if (!VEC || nbytes > 0)
            st16<VEC>(out_base + row * p.out_row, make_uint4(acc[0], acc[1], acc[2], acc[3]), nbytes);
    }
}

// the expanded dense rows of the tile (wave v: rows v, v + 4, ...)
__device__ __forceinline__ void sparse_header(const SparseMatmulParams &p, int obj, int row0, int rows_here) {
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    for (int i = wave; i < rows_here; i += kThreads / 64) {
        const int64_t row = row0 + i;
        const uint8_t *ib = reinterpret_cast<const uint8_t *>(p.idx) + int64_t(obj) * p.idx_obj + row * p.idx_row;
        const uint8_t *vb = p.val + int64_t(obj) * p.val_obj + row * p.val_row;
        uint8_t *h = p.hdr + int64_t(obj) * p.hdr_obj + row * p.hdr_row;
        for (int64_t s0 = 0; s0 < p.n_in; s0 += 64) {
            const int64_t colj = s0 + lane;
            uint32_t a = 0u;
            for (int t0 = 0; t0 < p.w; t0 += 64) {
                const int t = t0 + lane;
                int32_t ej = -1;
                uint32_t ev = 0u;
                if (t < p.w) {
                    ej = *reinterpret_cast<const int32_t *>(ib + int64_t(t) * 4);
                    ev = vb[t];
                }
                // only the entries of this column chunk (an index outside [0, n_in) is in none)
                uint64_t mk = wave_ballot(ev != 0u && int64_t(ej) >= s0 && int64_t(ej) < s0 + 64);
                while (mk != 0) {
                    const int l = __builtin_ctzll(mk);
                    mk &= mk - 1;
                    const int32_t j = __builtin_amdgcn_readlane(ej, l);
                    const uint32_t c = uint32_t(__builtin_amdgcn_readlane(int(ev), l));
                    a ^= int64_t(j) == colj ? c : 0u;
                }
            }
            if (colj < p.n_in) h[colj] = uint8_t(a);
        }
    }
}

// Columns [col0, wend) of the operands.  VEC: whole 16-byte slots on vector access (wend - col0 a multiple of 16); a
// lane past wend gathers the last slot again instead of branching in the loop, and stores nothing.  Otherwise
// byte-granular, bounded by each lane's bytes inside [col0, wend): the operand's partial last slot, or everything on
// misaligned rows where the device has no unaligned vector access.  A wave with no column leaves.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void gf_sparse_matmul_kernel(SparseMatmulParams p, int row_tiles, int col_blocks,
                                                                    int64_t col0, int64_t wend, int with_hdr) {
    int rt, cb, obj;
    decode_block(p.n_obj * row_tiles * col_blocks, row_tiles, col_blocks, rt, cb, obj);
    const int row0 = rt * kSparseRows;
    const int rows_here = min(kSparseRows, p.n_out - row0);
    const int64_t col = col0 + int64_t(cb) * kColBlock + int64_t(threadIdx.x) * kBytesPerThread;
    const int nbytes = col < wend ? int(min<int64_t>(kBytesPerThread, wend - col)) : 0;
    if (wave_ballot(nbytes > 0) != 0)
        sparse_rows<VEC>(p, obj, row0, rows_here, VEC ? min(col, wend - kBytesPerThread) : col, nbytes);
    if (with_hdr && cb == 0) sparse_header(p, obj, row0, rows_here);
}

}  // namespace

int64_t sparse_matmul_workgroups(const SparseMatmulParams &p) {
    if (p.n_out <= 0 || p.n_obj <= 0 || p.width <= 0) return 0;
    const int64_t row_tiles = (int64_t(p.n_out) + kSparseRows - 1) / kSparseRows;
    const int64_t col_blocks = (p.width + kColBlock - 1) / kColBlock;
    // no overflow: each factor is below 2^31 and the first product is checked before the second
    const int64_t a = int64_t(p.n_obj) * row_tiles;
    if (a > 0x7FFFFFFF || col_blocks > 0x7FFFFFFF) return INT64_MAX;
    return a * col_blocks;
}

hipError_t launch_sparse_matmul(const SparseMatmulParams &p, hipStream_t s) {
    const int64_t total = sparse_matmul_workgroups(p);
    if (total == 0) return hipSuccess;
    if (total > 0x7FFFFFFF || p.n_in <= 0 || p.w < 0) return hipErrorInvalidValue;
    const int row_tiles = (p.n_out + kSparseRows - 1) / kSparseRows;
    const bool vec_ok = unaligned_vector_ok() ||
                        (al16(p.in) && (p.n_in == 1 || al16(p.in_row)) && (p.n_obj == 1 || al16(p.in_obj)) &&
                         al16(p.out) && (p.n_out == 1 || al16(p.out_row)) && (p.n_obj == 1 || al16(p.out_obj)));
    // whole slots to the vector kernel, the rest (< 16 bytes of every row, or all of it) to the byte-granular one;
    // the first launch also writes the header
    const int64_t vend = vec_ok ? p.width & ~int64_t(kBytesPerThread - 1) : 0;
    const int with_hdr = p.hdr != nullptr ? 1 : 0;
    if (vend > 0) {
        const int col_blocks = int((vend + kColBlock - 1) / kColBlock);
        hipLaunchKernelGGL(gf_sparse_matmul_kernel<true>, dim3(unsigned(p.n_obj) * row_tiles * col_blocks),
                           dim3(kThreads), 0, s, p, row_tiles, col_blocks, int64_t(0), vend, with_hdr);
    }
    if (vend < p.width) {
        const int col_blocks = int((p.width - vend + kColBlock - 1) / kColBlock);
        hipLaunchKernelGGL(gf_sparse_matmul_kernel<false>, dim3(unsigned(p.n_obj) * row_tiles * col_blocks),
                           dim3(kThreads), 0, s, p, row_tiles, col_blocks, vend, p.width, vend > 0 ? 0 : with_hdr);
    }
    return hipGetLastError();
}

}  // namespace rlnc
