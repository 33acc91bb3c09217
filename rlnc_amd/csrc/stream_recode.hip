// stream_recode.hip — a decode stream's recode (rlnc_decode_stream_recode, decode_stream.cpp): count recoded pieces
// for every selected object of rank r >= 1, each a combination of the r useful pieces the object holds, found on the
// device.  The product is stream_product.hpp's, shared with the delivery (stream_deliver.hip): the same predicate, tile
// and tail, with n_out = count, the full piece from byte 0 as a source row and min_rank = 1.
//
// The useful pieces of object o are the slots below done_o whose status is Ok, u_0 < ... < u_{r-1} (the list
// rlnc_decode_stream_compact keeps: rank_compact.hip's plan launch).  The expand launch numbers them and writes the
// coefficient matrix the product reads, C[o][i][u_j] = r[o][i][j] and 0 in every other column below done_o, so that
//   out[o][i] = XOR_{t < done_o} C[o][i][t] . pieces[o][t] = XOR_{j < r} r[o][i][j] . pieces[o][u_j]
// over all k + L bytes: header and data are one linear map (recoder.rs:122-153).  A useless slot is a zero column: it
// costs its source row's read and a multiplication by zero, and nothing after a compaction (u_j = j, done_o = r).
//
// Rules (rank_large.hip's): the early return depends on workgroup-uniform values only (blockIdx, the state words and
// select through readfirstlane) and comes before any LDS use or barrier; no launch reads what a workgroup of the same
// launch writes; the state, the pieces, r and select are only read.
#include <hip/hip_runtime.h>

#include "../../include/rlnc_hip.h"
#include "stream_product.hpp"
#include "stream_recode_kernels.hpp"

namespace rlnc {

namespace {

// the recode's arguments: in = the full pieces, coef = C [obj][count][m], out = the recoded pieces, n_out = count,
// min_rank = 1, width = k + L
using RecodeArgs = StreamProdArgs;

constexpr uint16_t kNoPos = 0xFFFF;  // a slot below done that is not among the useful ones

constexpr int kExpandRows = 16;  // rows of C per workgroup of the expand launch

// Object x chunk of kExpandRows rows of C (`chunks` of them an object), chunk fastest.  Unselected: nothing.  Nothing to
// recode from (rank 0; a state the library did not write): status NotEnoughPiecesToRecode and used 0 by the object's
// first chunk, before any LDS use.  Else the Ok statuses below done are numbered as the compaction's plan launch
// numbers them -- a count per thread segment, the exclusive prefix sum over the 256 threads -- into pos[t] = j for
// t = u_j (kNoPos for the others) in LDS, by every chunk for itself (done <= 8,192 statuses: cheaper than a launch
// of its own that hands the numbering on), and the chunk's rows of C are written from it, a byte a thread: every byte of C[o][i][0 .. done) exactly
// once.  Nothing of the state is written.
__global__ __launch_bounds__(256) void recode_expand_kernel(RecodeArgs a, int chunks, int off_st, int k, const uint8_t *r,
                                                            uint8_t *C, int32_t *status, int32_t *used) {
    __shared__ int32_t cnt[256];
    __shared__ uint16_t pos[kLargeMaxM];
    const int o = int(blockIdx.x / uint32_t(chunks)), chunk = int(blockIdx.x % uint32_t(chunks)), tid = int(threadIdx.x);
    if (a.select != nullptr && __builtin_amdgcn_readfirstlane(a.select[o]) == 0) return;
    int done;
    if (!stream_takes(a, o, done)) {
        if (chunk == 0 && tid == 0) {
            status[o] = RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE;
            if (used != nullptr) used[o] = 0;
        }
        return;
    }
    const int32_t *St = reinterpret_cast<const int32_t *>(a.ws + int64_t(o) * a.ws_obj + off_st);
    const int seg = (done + 255) >> 8, t0 = min(tid * seg, done), t1 = min(t0 + seg, done);
    int n = 0;
    for (int t = t0; t < t1; ++t) n += St[t] == RLNC_OK ? 1 : 0;
    cnt[tid] = n;
    __syncthreads();
    int p = 0, total = 0;
    for (int j = 0; j < 256; ++j) {
        const int c = cnt[j];
        p += j < tid ? c : 0;
        total += c;
    }
    for (int t = t0; t < t1; ++t) {
        const bool ok = St[t] == RLNC_OK;
        pos[t] = ok && p < k ? uint16_t(p) : kNoPos;  // (p < k always: no byte beyond a row of r)
        p += ok ? 1 : 0;
    }
    __syncthreads();
    const int count = a.n_out, i0 = chunk * kExpandRows, rows = min(kExpandRows, count - i0);
    const uint8_t *ro = r + (int64_t(o) * count + i0) * k;
    uint8_t *Co = C + (int64_t(o) * count + i0) * a.m;
    const uint32_t cells = uint32_t(rows) * uint32_t(done);  // <= 2^17
    for (uint32_t e = uint32_t(tid); e < cells; e += 256u) {
        const uint32_t i = e / uint32_t(done), t = e % uint32_t(done);
        const uint16_t j = pos[t];
        Co[int64_t(i) * a.m + t] = j != kNoPos ? ro[int64_t(i) * k + j] : uint8_t(0);
    }
    if (chunk == 0 && tid == 0) {
        status[o] = RLNC_OK;
        if (used != nullptr) used[o] = min(total, k);
    }
}

__global__ __launch_bounds__(256) void recode_offset_kernel(RecodeArgs a, uint64_t *stream, uint64_t base) {
    stream_offset_body(a, stream, base);
}

template <int W>
__global__ __launch_bounds__(64 * W) void gf_stream_recode(RecodeArgs a, const uint64_t *stream) {
    stream_product_body<W>(a, stream);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gf_stream_recode_tail(RecodeArgs a) {
    __shared__ uint32_t tab[kMulTabDw];
    stream_tail_body<VEC>(a, tab);
}

struct RecodeKernels {
    static constexpr auto offset = &recode_offset_kernel;
    template <int W>
    static constexpr auto product = &gf_stream_recode<W>;
    template <bool VEC>
    static constexpr auto tail = &gf_stream_recode_tail<VEC>;
};

bool count_ok(size_t count) { return count >= 1 && count <= size_t(kRecodeMaxCount); }

}  // namespace

size_t stream_recode_plan_bytes(size_t k, size_t m, size_t count, size_t n_obj) {
    if (rank_stream_state_bytes(k, m, n_obj) == 0 || !count_ok(count)) return 0;
    // the expanded coefficients, then the block-address streams
    return ((n_obj * count * m + 15) & ~size_t(15)) + stream_geom_bytes(stream_geom(int(count), int(m), int(n_obj), 0));
}

bool stream_recode_fits(const RecodeParams &p) {
    const int64_t expand_wgs = int64_t(p.n_obj) * ((p.count + kExpandRows - 1) / kExpandRows);
    return expand_wgs <= 0x7FFFFFFFLL && stream_geom(p.count, p.m, p.n_obj, int64_t(p.k) + p.L).fits();
}

hipError_t launch_stream_recode(const RecodeParams &p, const void *state, size_t state_bytes, bool unaligned_ok,
                                hipStream_t s) {
    if (p.n_obj <= 0 || p.count == 0) return hipSuccess;
    hipError_t e = rank_state_check(p.k, p.m, p.n_obj, state, state_bytes);
    if (e != hipSuccess) return e;
    if (p.L <= 0 || p.count < 0 || !count_ok(size_t(p.count)) || p.pieces == nullptr || p.r == nullptr ||
        p.out == nullptr || p.status == nullptr || p.plan == nullptr || !al16(p.plan) ||
        p.obj_stride < int64_t(p.m) * (int64_t(p.k) + p.L) || !stream_recode_fits(p))
        return hipErrorInvalidValue;
    const int64_t piece = int64_t(p.k) + p.L;
    const StreamGeom g = stream_geom(p.count, p.m, p.n_obj, piece);
    const size_t c_bytes = (size_t(p.n_obj) * p.count * p.m + 15) & ~size_t(15);
    uint8_t *C = static_cast<uint8_t *>(p.plan);
    uint64_t *stream = reinterpret_cast<uint64_t *>(C + c_bytes);
    const LargeLayout lay = large_layout(p.k, p.m);

    RecodeArgs a{};
    a.ws = static_cast<const uint32_t *>(state);
    a.ws_obj = int64_t(lay.total);
    a.in = p.pieces;
    a.in_obj = p.obj_stride;
    a.in_row = piece;
    a.select = p.select;
    a.coef = C;
    a.out = p.out;
    a.width = piece;
    a.n_out = p.count;
    a.min_rank = 1;
    a.m = p.m, a.n_obj = p.n_obj;
    stream_args_geom(a, g);

    // 1. the useful slots of every selected object, r expanded over them into C; status and used
    const int chunks = (p.count + kExpandRows - 1) / kExpandRows;
    hipLaunchKernelGGL(recode_expand_kernel, dim3(unsigned(int64_t(p.n_obj) * chunks)), dim3(256), 0, s, a, chunks,
                       int(lay.st), p.k, p.r, C, p.status, p.used);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    // every object's operands at once: 16-byte vector accesses at any address, or all of them aligned
    const bool vec = unaligned_ok || (al16(p.pieces) && al16(p.out) && al16(piece) && al16(p.obj_stride));
    const bool bsj = ragged_bsj_eligible(p.pieces, p.out, piece, piece, piece, p.count, vec);
    // 2. - 4. the block-address streams of the recoding objects, the bit-sliced product over the whole column blocks,
    // the perm product over the rest
    return launch_stream_product<RecodeKernels>(a, g, vec, bsj, stream, s);
}

}  // namespace rlnc
