// kernels.hip — hand-written gfx950 (CDNA4) kernels for the RLNC GF(2^8) hot path.
//
// The reference's one hot primitive is dst ^= c·src over GF(2^8) (src/common/simd/mod.rs:89-119), called
// k times per coded piece by the encoder (encoder.rs:138-141), n times per recoded piece
// (recoder.rs:146-150) and ≈k² times per object by the decoder's RREF (decoder_matrix.rs:143-211).
// On MI355X that call is far too small to launch (1 MiB ≈ 0.13 µs of HBM time), so the device operator
// is the matrix form Out = Coef ⊗ In (kernels.hpp) with one workgroup per 4 KiB column block × row tile.
//
// This file is the uniform product: launch_matmul's dispatch, the realigned form of misaligned operands, the
// bit-sliced jump program's planning and kernels, and the launchers of the perm family (kernels: perm_kernels.hpp).
// The ragged batches are ragged.hip, the element-wise primitives and the marker scan elementwise.hip.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "../../include/rlnc_hip.h"
#include "gf256.hpp"
#include "bsj_tile.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"
#include "perm_kernels.hpp"

namespace rlnc {

namespace {

constexpr int kNarrowRows = 4;
inline size_t narrow_lds_bytes(int n_in) { return size_t(n_in) * kNarrowRows * 20; }
constexpr size_t kNarrowMaxLds = 64 * 1024;

hipError_t launch_narrow(const MatmulParams &p, bool aligned, hipStream_t s) {
    const int row_tiles = (p.n_out + kNarrowRows - 1) / kNarrowRows;
    const int64_t total = int64_t(p.n_obj) * row_tiles;
    if (total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const size_t lds = narrow_lds_bytes(p.n_in);
    const auto kern = aligned ? &gf_matmul_narrow_kernel<kNarrowRows, true> : &gf_matmul_narrow_kernel<kNarrowRows, false>;
    hipLaunchKernelGGL(kern, dim3(unsigned(total)), dim3(kThreads), lds, s, p, row_tiles);
    return hipGetLastError();
}

// The streaming kernels for few output rows (n_out <= 3), whole aligned 4 KiB blocks
constexpr int kStreamPF = 2;  // rows in flight of gf_matmul_stream_kernel (2..16 A/B: r01_stream_pf_ab.txt)

template <int NT, int PF, int VW, bool SH64>
hipError_t launch_stream3(const MatmulParams &q, int row_tiles, int col_blocks, hipStream_t s, int64_t tail) {
    if (col_blocks % VW) return launch_stream3<NT, PF, 1, SH64>(q, row_tiles, col_blocks, s, tail);
    const int64_t total = int64_t(q.n_obj) * row_tiles * (col_blocks / VW) + (tail > 0 ? int64_t(q.n_obj) * row_tiles : 0);
    if (total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((gf_matmul_stream3_kernel<NT, PF, VW, SH64>), dim3(unsigned(total)), dim3(kThreads), 0, s, q,
                       row_tiles, col_blocks / VW, tail);
    return hipGetLastError();
}

// Up to kKC sources: the one-block stream3 forms (64-bit-shift selectors; the forms measured against them:
// profiles/r02_stream_ab.txt), which also take the ragged tail (p.width - full bytes) in the same launch (tail_done)
template <int NT>
hipError_t launch_stream(const MatmulParams &p, int64_t full, hipStream_t s, bool &tail_done) {
    MatmulParams q = p;
    q.width = full;
    const int row_tiles = (p.n_out + NT - 1) / NT;
    const int col_blocks = int(full / kColBlock);
    const int64_t tail = p.width - full;
    const int64_t total = int64_t(p.n_obj) * row_tiles * col_blocks;
    tail_done = p.n_in <= kKC;
    if (tail_done) {
        // a launch too small to fill the device (one coded piece of a small object: latency-bound) keeps four rows
        // in flight per lane over one 4 KiB slot instead of one row pair over two
        if (total < 1024) return launch_stream3<NT, 4, 1, true>(q, row_tiles, col_blocks, s, tail);
        return launch_stream3<NT, 1, 2, true>(q, row_tiles, col_blocks, s, tail);
    }
    if (total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((gf_matmul_stream_kernel<NT, kStreamPF>), dim3(unsigned(total)), dim3(kThreads), 0, s, q,
                       row_tiles, col_blocks);
    return hipGetLastError();
}

template <int NT, bool VEC>
hipError_t launch_one(const MatmulParams &p, int64_t width, hipStream_t s, MatmulVariant v) {
    const int row_tiles = (p.n_out + NT - 1) / NT;
    const int col_blocks = int((width + kColBlock - 1) / kColBlock);
    const int64_t total = int64_t(p.n_obj) * row_tiles * col_blocks;
    if (total <= 0) return hipSuccess;
    if (total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    MatmulParams q = p;
    q.width = width;
    const dim3 grid{unsigned(total)}, block{unsigned(kThreads)};
    const auto kern = v == MatmulVariant::NibbleLds ? &gf_matmul_nibble_kernel<NT, VEC> : &gf_matmul_perm_kernel<NT, VEC>;
    hipLaunchKernelGGL(kern, grid, block, 0, s, q, row_tiles, col_blocks);
    return hipGetLastError();
}

// Aligned operands: whole 4 KiB column blocks go to the branch-free vector kernel, a ragged tail block
// (width % 4096) to a second launch of the byte-granular kernel.  Unaligned operands: byte kernel only.
template <int NT>
hipError_t launch_nt(const MatmulParams &p, hipStream_t s, MatmulVariant v, bool aligned) {
    if (!aligned) return launch_one<NT, false>(p, p.width, s, v);
    const int64_t full = (p.width / kColBlock) * kColBlock;
    if (full > 0) {
        hipError_t e = launch_one<NT, true>(p, full, s, v);
        if (e != hipSuccess) return e;
    }
    if (full == p.width) return hipSuccess;
    return launch_one<NT, false>(tail_params(p, full), p.width - full, s, v);
}

// ---------------------------------------------------------------------------------------------------
// Bit-sliced variant with one code block per coefficient (gen_bsjump.py has the derivation): the (row,
// source) work is a call into block c -- 16 v_bitop3_b32 XOR3s with the combination registers baked in and
// only the accumulator relative to the row slot -- instead of 32 GPR-index-relative XORs + 16 M0 writes.
// ---------------------------------------------------------------------------------------------------
// The program, its constants and the tile body: bsj_tile.hpp.

// stream[obj][row tile][j][row in tile] = c · RLNC_BSJ_BLOCK_BYTES (c = 0 for rows past n_out); ABS: the
// block's absolute address (64-bit, the shared-set programs call it directly): base + kBsjSharedOff[c]
template <bool ABS>
__global__ __launch_bounds__(256) void bsj_offset_kernel(const uint8_t *coef, int64_t coef_obj, int64_t coef_row,
                                                         int n_out, int n_in, int row_tiles, int tile_rows,
                                                         void *stream, uint64_t base) {
    const int64_t per_obj = int64_t(row_tiles) * n_in * tile_rows;
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int obj = blockIdx.y;
    if (e >= per_obj) return;
    const int i = int(e % tile_rows);
    const int j = int((e / tile_rows) % n_in);
    const int rt = int(e / (int64_t(tile_rows) * n_in));
    const int row = rt * tile_rows + i;
    const uint32_t c = row < n_out ? coef[int64_t(obj) * coef_obj + int64_t(row) * coef_row + j] : 0u;
    if constexpr (ABS)
        static_cast<uint64_t *>(stream)[int64_t(obj) * per_obj + e] = base + kBsjSharedOff[c];
    else
        static_cast<uint32_t *>(stream)[int64_t(obj) * per_obj + e] = c * uint32_t(RLNC_BSJ_BLOCK_BYTES);
}

template <int W, bool SHARE = false>
__global__ __launch_bounds__(64 * W) void gf_matmul_bsj_kernel(MatmulParams p, const void *stream, int row_tiles,
                                                               int col_blocks) {
    static_assert(!SHARE || W == 4 || W == 8, "the shared-set programs are generated for 4 and 8 waves");
    int rt, cb, obj;
    decode_block(p.n_obj * row_tiles * col_blocks, row_tiles, col_blocks, rt, cb, obj);
    bsj_tile<W, SHARE, false>(p, stream, row_tiles, rt, cb, obj, 1u, nullptr);
}

// Persistent tiles (the 8-wave program over one row tile, RLNC_BSJ_ASM_W8P): min(tiles, CUs) workgroups, one per CU,
// stay for the whole launch.  Workgroup b serves counter x = b & 7 (the XCD it is dispatched to, as in decode_block):
// counter x owns a contiguous eighth of the tiles (column block fastest, then object: an XCD's L2 sees a source column
// block once and successive claims are neighbours), its workgroups start on its first tiles and claim the rest in
// order, one tile ahead of their work.  counters[0..7] are the claims, counters[8] counts finished workgroups: the last
// one to finish -- every claim of the launch is then made -- zeroes all nine, so the next launch needs no memset.
// (A launch that does not run to its end -- a device fault or abort -- leaves them as they were; the context is lost
// with the device then, like every other buffer of it, and nothing re-zeroes them.)
__global__ __launch_bounds__(512) void gf_matmul_bsj_persist_kernel(MatmulParams p, const void *stream, int col_blocks,
                                                                   uint32_t *counters) {
    const uint32_t total = uint32_t(p.n_obj) * uint32_t(col_blocks), wgs = gridDim.x;
    const uint32_t x = blockIdx.x & 7u, i = blockIdx.x >> 3;
    const uint32_t q = total >> 3, r = total & 7u;
    BsjClaim c;
    c.counter = counters + x;
    c.limit = q + (x < r ? 1u : 0u);                           // tiles of counter x
    c.claim_base = (wgs >> 3) + (x < (wgs & 7u) ? 1u : 0u);    // ... of which its workgroups start on these
    c.first = i;
    c.col_blocks = uint32_t(col_blocks);
    const uint32_t t = x * q + min(x, r) + i;
    const int cb = int(t % uint32_t(col_blocks)), obj = int(t / uint32_t(col_blocks));
    if (p.hdr != nullptr)
        for (int o = blockIdx.x; o < p.n_obj; o += int(wgs)) copy_header_rows(p, o, 0, p.n_out, 512);
    bsj_tile<8, true, true, true>(p, stream, 1, 0, cb, obj, 0u, nullptr, c);
    if (threadIdx.x == 0) {  // wave 0 made the claims, the last of them long returned
        const uint32_t done = __hip_atomic_fetch_add(counters + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == wgs - 1)
            for (int k = 0; k < kBsjPersistCounters; ++k)
                __hip_atomic_store(counters + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// compute units of the current device (looked up once per device)
static int device_cus() {
    static std::mutex mu;
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lock(mu);
    if (cus[dev] == 0 &&
        (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus[dev] <= 0))
        cus[dev] = 256;
    return cus[dev];
}

// the shared program's probe launch: stores its block table's address and returns (bsj_shared_base)
__global__ __launch_bounds__(256) void gf_matmul_bsj_probe_kernel(MatmulParams p, const void *stream, uint64_t *probe) {
    bsj_tile<4, true, false>(p, stream, 1, 0, 0, 0, 1u, probe);
}

// waves per workgroup: 8 output rows each, at most 4 (a 32-row tile), no more than the rows need
inline int bsj_waves(int n_out) { return n_out <= 8 ? 1 : n_out <= 16 ? 2 : 4; }

}  // namespace

int bsj_waves(int n_out, bool wide) { return wide && n_out > 32 ? 8 : bsj_waves(n_out); }

// Whole 4 KiB column blocks of 16-byte-aligned operands; the ragged tail goes to the perm kernel.  The tile assembly
// adds the row strides to its row pointers as unsigned 32-bit numbers (bsj_tile.hpp), so they are in [0, 2^32) here.
bool bsj_eligible(const MatmulParams &p, bool aligned) {
    return aligned && p.width >= kBsjColBlock && p.n_out >= 4 && p.in_row >= 0 && p.in_row < (int64_t(1) << 32) &&
           p.out_row >= 0 && p.out_row < (int64_t(1) << 32);
}

size_t bsj_scratch_bytes(const MatmulParams &p, bool wide) {
    const int tile_rows = kBsjWaveRows * bsj_waves(p.n_out, wide);
    const int64_t tiles = (p.n_out + tile_rows - 1) / tile_rows;
    // 8 bytes per entry (absolute addresses of the shared program, 4 otherwise) + one source: the main loop
    // loads the entries of the source after the last one
    return size_t(int64_t(p.n_obj) * tiles * p.n_in * tile_rows * 8 + 512);
}

// Address of the shared-set program's block table on the current device: one probe launch per device (the
// code object does not move while the process runs).  Synchronous on `s` the first time only; base = 0 when
// that first time is inside a stream capture (the caller then takes the relative-offset program).
hipError_t bsj_shared_base(hipStream_t s, void *scratch, uint64_t &base) {
    static std::mutex mu;
    static uint64_t bases[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    base = 0;
    if (bases[dev] == 0) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if ((e = hipStreamIsCapturing(s, &cs)) != hipSuccess) return e;
        if (cs != hipStreamCaptureStatusNone) return hipSuccess;
        MatmulParams q{};
        q.n_obj = 1;
        q.n_out = 1;
        q.n_in = 1;
        uint64_t *slot = static_cast<uint64_t *>(scratch);
        hipLaunchKernelGGL(gf_matmul_bsj_probe_kernel, dim3(1), dim3(256), 0, s, q, scratch, slot);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        uint64_t h = 0;
        if ((e = hipMemcpyAsync(&h, slot, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (h == 0) return hipErrorLaunchFailure;
        bases[dev] = h;
    }
    base = bases[dev];
    return hipSuccess;
}

constexpr int kBsjOffsetObjects = 65535;  // objects per bsj_offset_kernel launch (blockIdx.y)

// The block-address stream of a bit-sliced jump product (one bsj_offset_kernel launch per 65,535 objects) and the
// launch geometry of its whole 4 KiB column blocks (kernels.hpp BsjPlan)
hipError_t bsj_prepare(const MatmulParams &p, hipStream_t s, void *scratch, size_t scratch_bytes, bool share,
                       bool wide, BsjPlan &b) {
    b.full = (p.width / kBsjColBlock) * kBsjColBlock;
    if (scratch == nullptr || scratch_bytes < bsj_scratch_bytes(p, share && wide)) return hipErrorInvalidValue;
    int W = bsj_waves(p.n_out, share && wide);
    bool abs = share && W >= 4;  // the shared-set programs call absolute block addresses
    uint64_t base = 0;
    if (abs) {
        hipError_t e = bsj_shared_base(s, scratch, base);
        if (e != hipSuccess) return e;
        abs = base != 0;  // first use inside a stream capture: the (bit-identical) variant-6 program this time
        share = abs;
        if (!abs) W = bsj_waves(p.n_out);
    }
    const int tile_rows = kBsjWaveRows * W;
    b.waves = W;
    b.share = share;
    b.row_tiles = (p.n_out + tile_rows - 1) / tile_rows;
    b.col_blocks = int(b.full / kBsjColBlock);
    b.total = int64_t(p.n_obj) * b.row_tiles * b.col_blocks;
    if (b.total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    if (p.bsj_stream != nullptr && p.bsj_stream_rows == tile_rows && (p.bsj_stream_abs != 0) == abs) {
        // written already: by the small-object elimination (4-byte offsets) or by launch_bsj_stream ahead
        b.stream = const_cast<void *>(p.bsj_stream);
        return hipSuccess;
    }
    b.stream = scratch;
    const int64_t per_obj = int64_t(b.row_tiles) * p.n_in * tile_rows;
    if ((per_obj + 255) / 256 > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    // the object is the grid's y, which holds 65,535: more objects take one launch per range of that many, each on its
    // own coefficients and its own part of the stream (the layout is the same as one launch's)
    const int64_t entry = abs ? 8 : 4;
    for (int o0 = 0; o0 < p.n_obj; o0 += kBsjOffsetObjects) {
        const int c = std::min(kBsjOffsetObjects, p.n_obj - o0);
        const dim3 og(unsigned((per_obj + 255) / 256), unsigned(c));
        hipLaunchKernelGGL(abs ? &bsj_offset_kernel<true> : &bsj_offset_kernel<false>, og, dim3(256), 0, s,
                           p.coef + int64_t(o0) * p.coef_obj, p.coef_obj, p.coef_row, p.n_out, p.n_in, b.row_tiles,
                           tile_rows, static_cast<uint8_t *>(b.stream) + int64_t(o0) * per_obj * entry,
                           base);  // !abs: base 0
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

static hipError_t launch_bsj(const MatmulParams &p, hipStream_t s, void *scratch, size_t scratch_bytes, int64_t &full,
                      bool share, bool wide, const BsjPersist &pt) {
    BsjPlan b;
    hipError_t e = bsj_prepare(p, s, scratch, scratch_bytes, share, wide, b);
    full = b.full;
    if (e != hipSuccess) return e;
    MatmulParams q = p;
    q.width = b.full;
    // the marker scan of undecided objects in the tiles (MatmulParams::scan_need) when each object is one workgroup's
    // whole tile (the 1- and 2-wave programs are never the shared ones, whatever b.share says)
    const bool scan = p.scan_status != nullptr && p.scan_need != nullptr && b.waves <= 2 && b.row_tiles == 1 &&
                      b.col_blocks == 1 && b.full == p.width && p.width == kBsjColBlock && p.n_out == p.scan_k &&
                      p.out_row == p.width && p.out_obj == int64_t(p.scan_k) * p.width;
    if (!scan) q.scan_status = nullptr;
    const dim3 grid(unsigned(b.total));
    // persistent tiles: the 64-row program over one row tile whose DMA stream stays within one tile of the work, from 2
    // tiles per workgroup on (fewer: nothing to claim, the present grid is as good)
    if (b.waves == 8 && b.share && pt.counters != nullptr && pt.mode != kBsjPersistOff && b.row_tiles == 1 &&
        p.n_in >= RLNC_BSJ_PERSIST_MIN_SOURCES && p.n_in < (1 << 22)) {
        const int64_t wgs = std::min<int64_t>(b.total, pt.max_wgs >= 8 ? pt.max_wgs : device_cus());
        if (pt.mode == kBsjPersistAlways || b.total >= 2 * wgs) {
            hipLaunchKernelGGL(gf_matmul_bsj_persist_kernel, dim3(unsigned(wgs)), dim3(512), 0, s, q, b.stream,
                               b.col_blocks, pt.counters);
            return hipGetLastError();
        }
    }
    if (b.waves == 1)
        hipLaunchKernelGGL(gf_matmul_bsj_kernel<1>, grid, dim3(64), 0, s, q, b.stream, b.row_tiles, b.col_blocks);
    else if (b.waves == 2)
        hipLaunchKernelGGL(gf_matmul_bsj_kernel<2>, grid, dim3(128), 0, s, q, b.stream, b.row_tiles, b.col_blocks);
    else if (b.waves == 8)
        hipLaunchKernelGGL((gf_matmul_bsj_kernel<8, true>), grid, dim3(512), 0, s, q, b.stream, b.row_tiles,
                           b.col_blocks);
    else if (b.share)
        hipLaunchKernelGGL((gf_matmul_bsj_kernel<4, true>), grid, dim3(256), 0, s, q, b.stream, b.row_tiles,
                           b.col_blocks);
    else
        hipLaunchKernelGGL(gf_matmul_bsj_kernel<4>, grid, dim3(256), 0, s, q, b.stream, b.row_tiles, b.col_blocks);
    const hipError_t e2 = hipGetLastError();
    if (e2 == hipSuccess && scan && p.scan_done != nullptr) *p.scan_done = true;
    return e2;
}

// 16-byte alignment of an operand: its base, and the strides of the dimensions that have more than one element (a
// single row's stride is never used).  On a device that executes 16-byte vector memory instructions at any byte
// address (unaligned_vector_ok) every operand counts as aligned.
static bool in_aligned(const MatmulParams &p) {
    return unaligned_vector_ok() ||
           (al16(p.in) && (p.n_in == 1 || al16(p.in_row)) && (p.n_obj == 1 || al16(p.in_obj)));
}
static bool out_aligned(const MatmulParams &p) {
    return unaligned_vector_ok() ||
           (al16(p.out) && (p.n_out == 1 || al16(p.out_row)) && (p.n_obj == 1 || al16(p.out_obj)));
}
static bool matmul_aligned(const MatmulParams &p) { return in_aligned(p) && out_aligned(p); }

// ---------------------------------------------------------------------------------------------------
// Byte-misaligned vector memory access.  gfx9 executes global_load/store_dwordx4 and global_load_lds_dwordx4 at any
// byte address when the queue's SH_MEM_CONFIG alignment mode is "unaligned" (the ROCm driver's default for compute
// queues; in "dword" mode the low address bits are dropped).  Measured on the MI355X boxes
// (scripts/ubench_unaligned.hip, profiles/r03_ubench_unaligned.jsonl): exact bytes at every offset, and a 1 GiB copy
// at 4.3-5.2 TB/s misaligned against 4.8 aligned.  A probe kernel checks it once per device; where it holds, rows at
// any alignment take the vector kernels directly, else the realigned path (realign_plan) copies them through
// 16-byte scratch rows.  RLNC_ASSUME_ALIGNED_ONLY=1 forces the realigned path (its tests).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void unaligned_probe_kernel(const uint8_t *src, uint8_t *dst, uint8_t *dst_lds) {
    __shared__ __attribute__((aligned(16))) uint32_t buf[64 * 4];
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const int l = threadIdx.x;
    const int off = 1 + l % 15;  // every misalignment 1..15
    const uint8_t *s = src + 32 * l + off;
    uint8_t *d = dst + 32 * l + (16 - off);
    u4 x;
    asm volatile("global_load_dwordx4 %0, %1, off\n s_waitcnt vmcnt(0)" : "=v"(x) : "v"(s) : "memory");
    asm volatile("global_store_dwordx4 %0, %1, off\n s_waitcnt vmcnt(0)" ::"v"(d), "v"(x) : "memory");
    __builtin_amdgcn_global_load_lds(s, (__attribute__((address_space(3))) void *)buf, 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    reinterpret_cast<u4 *>(dst_lds)[l] = reinterpret_cast<const u4 *>(buf)[l];
}

static std::atomic<int> g_unaligned[64];  // per device: 0 not probed, 1 any byte address works, 2 not (or forced)

static bool run_unaligned_probe() {
    constexpr int kB = 4096;
    uint8_t *src = nullptr, *dst = nullptr, *dl = nullptr;
    hipStream_t st = nullptr;
    bool ok = hipMalloc(&src, kB) == hipSuccess && hipMalloc(&dst, kB) == hipSuccess && hipMalloc(&dl, kB) == hipSuccess &&
              hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    std::vector<uint8_t> h(kB), g(kB), gl(kB);
    for (int i = 0; i < kB; ++i) h[i] = uint8_t(i * 73 + (i >> 8) + 1);
    if (ok) {
        ok = hipMemcpyAsync(src, h.data(), kB, hipMemcpyHostToDevice, st) == hipSuccess &&
             hipMemsetAsync(dst, 0, kB, st) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(unaligned_probe_kernel, dim3(1), dim3(64), 0, st, src, dst, dl);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(g.data(), dst, kB, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipMemcpyAsync(gl.data(), dl, kB, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess;
        }
    }
    for (int l = 0; ok && l < 64; ++l) {
        const int off = 1 + l % 15;
        for (int b = 0; b < 16; ++b)
            ok = ok && g[32 * l + 16 - off + b] == h[32 * l + off + b] && gl[16 * l + b] == h[32 * l + off + b];
    }
    if (st) (void)hipStreamDestroy(st);
    for (uint8_t *x : {src, dst, dl})
        if (x) (void)hipFree(x);
    (void)hipGetLastError();  // a failed probe leaves no sticky error behind
    return ok;
}

int probe_unaligned_vector_access(int device) {
    if (device < 0 || device >= 64) return 0;
    int v = g_unaligned[device].load();
    if (v != 0) return v == 1;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if ((v = g_unaligned[device].load()) != 0) return v == 1;
    const char *e = getenv("RLNC_ASSUME_ALIGNED_ONLY");
    // relaxed capture mode on this thread while probing, so a context created while another stream of the process
    // is being captured neither fails nor invalidates that capture (the probe's allocations are not stream work)
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    const bool swapped = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    const bool ok = !(e != nullptr && atoi(e) != 0) && run_unaligned_probe();
    if (swapped) (void)hipThreadExchangeStreamCaptureMode(&mode);
    g_unaligned[device].store(ok ? 1 : 2);
    return ok;
}

int unaligned_vector_access(int device) {
    if (device < 0 || device >= 64) return -1;
    const int v = g_unaligned[device].load();
    return v == 0 ? -1 : v == 1;
}

bool unaligned_vector_ok() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    return g_unaligned[dev].load(std::memory_order_relaxed) == 1;
}

// ---------------------------------------------------------------------------------------------------
// Realigned products.  A piece row is rarely 16-byte aligned: Encoder::new pads to L = ceil((len + 1) / k)
// (encoder.rs:93-95), so the reference's own bench shapes (2^20..2^25 bytes over k = 16..256) give odd L, and a
// coded piece's data starts at byte k of a (k + L)-byte row.  The vector kernels need 16-byte rows; the byte-granular
// kernels run 5-7x slower.  So a misaligned operand of a product the bit-sliced or stream kernels take is copied
// into 16-byte-aligned scratch rows (input) or out of them (output) around the aligned product, in chunks of objects
// and column blocks of at most kRealignBudget bytes of scratch.
// ---------------------------------------------------------------------------------------------------
constexpr size_t kRealignBudget = size_t(512) << 20;
constexpr int kRealignDwords = 4;  // destination dwords per thread

// dst[o][r][0:w) = src[o][r][0:w) at any byte alignment of either side: thread t writes dwords of the destination's
// 4-byte grid (a dword the row covers only in part is written byte by byte, so the neighbouring bytes -- e.g. the
// coded piece's coefficient header -- are never touched), reading the source as aligned dwords joined by v_alignbyte;
// every dword read holds at least one byte of the row, so no read leaves the row's pages
__global__ __launch_bounds__(256) void realign_rows_kernel(uint8_t *dst, int64_t dst_row, int64_t dst_obj,
                                                           const uint8_t *src, int64_t src_row, int64_t src_obj,
                                                           int rows, int64_t width, int chunks) {
    const int64_t wg = blockIdx.x;
    const int64_t rr = wg / chunks;
    const int64_t ch = wg % chunks;
    const int64_t o = rr / rows, r = rr % rows;
    uint8_t *d = dst + o * dst_obj + r * dst_row;
    const uint8_t *sp = src + o * src_obj + r * src_row;
    const int dmis = int(reinterpret_cast<uintptr_t>(d) & 3);
    uint32_t *dw = reinterpret_cast<uint32_t *>(d - dmis);
    const int64_t ndw = (dmis + width + 3) >> 2;  // dword t covers row bytes [4t - dmis, 4t - dmis + 4)
#pragma unroll
    for (int u = 0; u < kRealignDwords; ++u) {
        const int64_t t = ch * (256 * kRealignDwords) + u * 256 + threadIdx.x;
        if (t >= ndw) break;
        const int64_t x0 = 4 * t - dmis;
        if (x0 >= 0 && x0 + 4 <= width) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(sp + x0);
            const uint32_t *A = reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3));
            const uint32_t sh = uint32_t(a & 3);
            const uint32_t lo = A[0];
            const uint32_t hi = sh ? A[1] : 0u;
            dw[t] = __builtin_amdgcn_alignbyte(hi, lo, sh);  // ({hi, lo} >> 8 sh)[31:0]
        } else {
            for (int b = 0; b < 4; ++b) {
                const int64_t x = x0 + b;
                if (x >= 0 && x < width) d[x] = sp[x];
            }
        }
    }
}

static hipError_t launch_realign(uint8_t *dst, int64_t dst_row, int64_t dst_obj, const uint8_t *src, int64_t src_row,
                                 int64_t src_obj, int rows, int64_t width, int n_obj, hipStream_t s) {
    const int64_t per_wg = 256 * kRealignDwords * 4;
    const int64_t chunks = (width + 3 + per_wg) / per_wg;  // dwords of the destination grid, + 1 for its offset
    const int64_t total = int64_t(n_obj) * rows * chunks;
    if (total <= 0) return hipSuccess;
    if (total > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(realign_rows_kernel, dim3(unsigned(total)), dim3(256), 0, s, dst, dst_row, dst_obj, src, src_row,
                       src_obj, rows, width, int(chunks));
    return hipGetLastError();
}

static bool jump_variant(MatmulVariant v) {
    return v == MatmulVariant::BitSlicedJump || v == MatmulVariant::BitSlicedJumpShared ||
           v == MatmulVariant::BitSlicedJumpShared8;
}
// the shared-set programs (variants 7 and 8), and variant 8's 64-row tiles of 8 waves above 32 output rows
static bool share_variant(MatmulVariant v) {
    return v == MatmulVariant::BitSlicedJumpShared || v == MatmulVariant::BitSlicedJumpShared8;
}
static bool wide_variant(MatmulVariant v) { return v == MatmulVariant::BitSlicedJumpShared8; }

// the shipped variants; the others (2-5, 9) are the A/B history of kernels_ab.hip (make ab)
static bool shipped_variant(MatmulVariant v) {
    return v == MatmulVariant::Perm || v == MatmulVariant::NibbleLds || jump_variant(v);
}

struct RealignPlan {
    bool in_mis = false, out_mis = false;
    int objs = 0;                           // objects per chunk
    int64_t cw = 0;                         // columns per chunk (a multiple of 4 KiB, or the whole width)
    int64_t lr = 0;                         // scratch row stride (cw rounded up to 16)
    size_t prod_bytes = 0, in_bytes = 0, out_bytes = 0;
};

size_t matmul_scratch_bytes_aligned(const MatmulParams &p, MatmulVariant v);

// The realigned form of a misaligned product that the bit-sliced or stream kernels would take if it were aligned
static bool realign_plan(const MatmulParams &p, MatmulVariant v, RealignPlan &r) {
    if (!jump_variant(v) || p.width < kColBlock || p.n_out <= 0 || p.n_in <= 0 || p.n_obj <= 0 || matmul_aligned(p))
        return false;
    r.in_mis = !in_aligned(p);
    r.out_mis = !out_aligned(p);
    const int64_t rows = (r.in_mis ? p.n_in : 0) + (r.out_mis ? p.n_out : 0);
    const int64_t whole = (p.width + 15) & ~int64_t(15);
    int64_t objs = p.n_obj, cw = whole;
    if (objs * rows * cw > int64_t(kRealignBudget)) {
        cw = std::max<int64_t>(kColBlock, int64_t(kRealignBudget) / (objs * rows) / kColBlock * kColBlock);
        if (cw >= whole) cw = whole;
        if (objs * rows * cw > int64_t(kRealignBudget)) objs = std::max<int64_t>(1, int64_t(kRealignBudget) / (rows * cw));
    }
    r.objs = int(objs);
    r.cw = cw;
    r.lr = (cw + 15) & ~int64_t(15);
    MatmulParams q = p;  // one chunk, aligned
    q.n_obj = r.objs;
    q.width = std::min<int64_t>(cw, p.width);
    q.in = q.out = nullptr;
    q.in_row = q.out_row = r.lr;
    q.in_obj = int64_t(p.n_in) * r.lr;
    q.out_obj = int64_t(p.n_out) * r.lr;
    r.prod_bytes = (matmul_scratch_bytes_aligned(q, v) + 255) & ~size_t(255);
    r.in_bytes = r.in_mis ? size_t(objs) * p.n_in * r.lr : 0;
    r.out_bytes = r.out_mis ? size_t(objs) * p.n_out * r.lr : 0;
    return true;
}

size_t bsj_stream_bytes_bound(int n_obj, int n_out, int n_in) {
    // tiles x tile_rows < n_out + 64 rows, 8 bytes an entry, + the main loop's one-source overrun
    return size_t(n_obj) * size_t(n_out + 64) * size_t(n_in) * 8 + 512;
}

hipError_t launch_bsj_stream(const MatmulParams &p, MatmulVariant v, hipStream_t s, void *buf, size_t bytes,
                             BsjStreamPlan &plan) {
    plan = BsjStreamPlan{};
    if (p.n_out <= 0 || p.width <= 0 || p.n_obj <= 0 || p.n_in <= 0 || !shipped_variant(v) || !jump_variant(v))
        return hipSuccess;
    RealignPlan r;
    if (realign_plan(p, v, r)) return hipSuccess;  // the realigned chunks write their own streams
    const bool aligned = matmul_aligned(p);
    if (aligned && p.n_out <= 3 && p.width >= kColBlock) return hipSuccess;  // the single-pass stream kernel
    if (!bsj_eligible(p, aligned)) return hipSuccess;
    MatmulParams q = p;
    q.bsj_stream = nullptr;
    BsjPlan b;
    if (hipError_t e = bsj_prepare(q, s, buf, bytes, share_variant(v), wide_variant(v), b); e != hipSuccess) return e;
    plan.tile_rows = kBsjWaveRows * b.waves;
    plan.abs = (b.share && b.waves >= 4) ? 1 : 0;  // the shared programs (4 and 8 waves) call absolute addresses
    return hipSuccess;
}

size_t matmul_scratch_bytes(const MatmulParams &p, MatmulVariant v) {
    if (!shipped_variant(v)) return matmul_scratch_bytes_ab(p, v);
    RealignPlan r;
    if (realign_plan(p, v, r)) return r.prod_bytes + r.in_bytes + r.out_bytes;
    return matmul_scratch_bytes_aligned(p, v);
}

size_t matmul_scratch_bytes_aligned(const MatmulParams &p, MatmulVariant v) {
    if (!jump_variant(v) || p.n_out <= 0 || p.n_in <= 0 || p.n_obj <= 0) return 0;
    return bsj_eligible(p, matmul_aligned(p)) ? bsj_scratch_bytes(p, wide_variant(v)) : 0;
}

hipError_t launch_matmul(const MatmulParams &p, hipStream_t s, MatmulVariant v, void *scratch, size_t scratch_bytes,
                         const BsjPersist &pt) {
    if (p.n_out <= 0 || p.width <= 0 || p.n_obj <= 0) return hipSuccess;
    const bool aligned = matmul_aligned(p);
    if (p.n_in <= 0) return hipErrorInvalidValue;
    if (!shipped_variant(v)) {  // the A/B variants never take the in-tile marker scan
        MatmulParams q = p;
        q.scan_status = nullptr;
        return launch_matmul_ab(q, s, v, scratch, scratch_bytes);
    }
    RealignPlan r;
    if (realign_plan(p, v, r)) {  // misaligned rows: realign copies around the aligned product
        if (scratch == nullptr || scratch_bytes < r.prod_bytes + r.in_bytes + r.out_bytes) return hipErrorInvalidValue;
        uint8_t *ib = static_cast<uint8_t *>(scratch) + r.prod_bytes;
        uint8_t *ob = ib + r.in_bytes;
        for (int o0 = 0; o0 < p.n_obj; o0 += r.objs) {
            const int c = std::min(r.objs, p.n_obj - o0);
            for (int64_t c0 = 0; c0 < p.width; c0 += r.cw) {
                const int64_t w = std::min(r.cw, p.width - c0);
                MatmulParams q = p;
                q.bsj_stream = nullptr;   // laid out for the whole batch
                q.scan_status = nullptr;  // chunks of columns: no workgroup holds a whole object
                q.n_obj = c;
                q.width = w;
                q.in = p.in + int64_t(o0) * p.in_obj + c0;
                q.coef = p.coef + int64_t(o0) * p.coef_obj;
                q.out = p.out + int64_t(o0) * p.out_obj + c0;
                q.hdr = (p.hdr != nullptr && c0 == 0) ? p.hdr + int64_t(o0) * p.hdr_obj : nullptr;
                hipError_t e;
                if (r.in_mis) {
                    if ((e = launch_realign(ib, r.lr, int64_t(p.n_in) * r.lr, q.in, p.in_row, p.in_obj, p.n_in, w, c, s)) !=
                        hipSuccess)
                        return e;
                    q.in = ib;
                    q.in_row = r.lr;
                    q.in_obj = int64_t(p.n_in) * r.lr;
                }
                if (r.out_mis) {
                    q.out = ob;
                    q.out_row = r.lr;
                    q.out_obj = int64_t(p.n_out) * r.lr;
                }
                if ((e = launch_matmul(q, s, v, scratch, r.prod_bytes, pt)) != hipSuccess) return e;
                if (r.out_mis &&
                    (e = launch_realign(p.out + int64_t(o0) * p.out_obj + c0, p.out_row, p.out_obj, ob, r.lr,
                                        int64_t(p.n_out) * r.lr, p.n_out, w, c, s)) != hipSuccess)
                    return e;
            }
        }
        return hipSuccess;
    }
    const bool jump = jump_variant(v);
    if (jump && aligned && p.n_out <= 3 && p.width >= kColBlock) {
        // one to three coded pieces per source pass: HBM-bound, streamed with deep prefetch
        const int64_t full = (p.width / kColBlock) * kColBlock;
        bool tail_done = false;
        hipError_t e = p.n_out == 1   ? launch_stream<1>(p, full, s, tail_done)
                       : p.n_out == 2 ? launch_stream<2>(p, full, s, tail_done)
                                      : launch_stream<3>(p, full, s, tail_done);
        if (e != hipSuccess || full == p.width || tail_done) return e;
        return launch_matmul(tail_params(p, full), s, MatmulVariant::Perm);
    }
    if (jump) {
        if (bsj_eligible(p, aligned)) {
            int64_t full = 0;
            hipError_t e = launch_bsj(p, s, scratch, scratch_bytes, full, share_variant(v), wide_variant(v), pt);
            if (e != hipSuccess || full == p.width) return e;
            return launch_matmul(tail_params(p, full), s, MatmulVariant::Perm);
        }
        v = MatmulVariant::Perm;  // whatever the bit-sliced kernels do not cover
    }
    // narrow (< one 4 KiB column block, e.g. the ragged tail of a recode over k + L bytes): the work is the
    // sources x rows chain of one block, so split the rows over many workgroups (2 rows each)
    // (1-2 rows too while the sources are few, e.g. the short tail of one recoded piece: 107 -> 80 us per
    // Recoder::recode_with_buf call at 16 MiB / k = 64 over 32 pieces with the small-launch stream form below; over 128+
    // sources the perm kernel's chunked tables were faster: profiles/r03_object_api_rates.jsonl)
    if (p.width < kColBlock && (p.n_out > 2 || p.n_in <= kKC)) {
        if (v == MatmulVariant::Perm && narrow_lds_bytes(p.n_in) <= kNarrowMaxLds)
            return launch_narrow(p, aligned, s);
        if (p.n_out > 2) return launch_nt<2>(p, s, v, aligned);
    }
    if (p.n_out <= 1) return launch_nt<1>(p, s, v, aligned);
    if (p.n_out <= 2) return launch_nt<2>(p, s, v, aligned);
    if (p.n_out <= 4) return launch_nt<4>(p, s, v, aligned);
    if (p.n_out <= 8) return launch_nt<8>(p, s, v, aligned);
    if (p.n_out <= 16) return launch_nt<16>(p, s, v, aligned);
    return launch_nt<32>(p, s, v, aligned);
}

uint32_t bsj_block_bytes() { return uint32_t(RLNC_BSJ_BLOCK_BYTES); }
int bsj_unshared_tile_rows(int n_out) { return bsj_waves(n_out) <= 2 ? kBsjWaveRows * bsj_waves(n_out) : 0; }

// The A/B build (make ab) links kernels_ab.hip, whose definitions replace these
__attribute__((weak)) bool ab_build() { return false; }
__attribute__((weak)) hipError_t launch_matmul_ab(const MatmulParams &, hipStream_t, MatmulVariant, void *, size_t) {
    return hipErrorInvalidValue;  // the A/B variants exist in the diagnostic build only
}
__attribute__((weak)) size_t matmul_scratch_bytes_ab(const MatmulParams &, MatmulVariant) { return 0; }

}  // namespace rlnc
