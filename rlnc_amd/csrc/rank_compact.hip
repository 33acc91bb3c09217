// rank_compact.hip — a decode stream's compaction (include/rlnc_hip.h, rlnc_decode_stream_compact; interface and the
// equivalence argument: rank_compact_kernels.hpp; the state buffer, its words and their protocol: rank_state.hpp).
//
// Per object the call reads rank and done (kStRank, kStDone) as the last push left them, and the retire flag:
//   retired    retire[o] != 0: the four state words become 0; nothing else of the object is written;
//   idle       done == rank (every slot below done is Ok, or done = 0): nothing of the object is written;
//   active     done > rank: u_0 < ... < u_{r-1}, r = rank, are the slots below done with status Ok.  Byte j of every
//              stored row's e part becomes the old byte u_j (zero from r on), piece slot u_j moves to slot j,
//              St[0 .. r) = Ok and the state words become {r, r, r, r}.
// A state whose words the library did not write (rank outside [0, k], done outside [rank, m]) is left as it is.
//
// Four launches, ordered by the stream only:
//   plan    (one workgroup per object) counts the Ok statuses below done per thread segment, takes the exclusive prefix
//           sum over the 256 threads, and writes the list u into the object's Q region (active objects only; Q is dead
//           between pushes, k x 8 dwords of which the list takes r <= k) and kept.
//   rows    (object x 16 stored rows; a wave per row, four rows at a time) reads a row's e part whole into LDS, and
//           after the barrier writes it back gathered through u, zero from byte r on: all reads of a row come before
//           any write of it.  The coefficient part is not touched.
//   move    (object x 4,096-byte column chunk of a piece; a piece's last chunk takes its tail too, in a second pass)
//           each thread owns a fixed byte-column range of the object's pieces and copies slot u_j to slot j for j = j0
//           .. r - 1 in increasing order, j0 the first j with u_j != j (u is strictly increasing with u_j >= j, so
//           u_j == j exactly below j0).  In place needs no order between threads: a step writes slot j <= u_j within
//           the thread's own columns, and every later step of that thread reads a slot u_j' > u_j >= j, so no source
//           is overwritten before it is read; for the same reason the loads of several consecutive steps may be issued
//           before their stores, which keeps kMoveDepth x 16 bytes per lane in flight.  VEC: 16 bytes per lane at any
//           byte address (k + L is arbitrary, so source and destination differ in alignment;
//           unaligned_vector_access), the last lane of a piece byte by byte; otherwise every lane owns 16 single
//           bytes, 256 apart.  Ownership is by bytes in both: no access is wider than what the thread owns.
//   commit  (one workgroup per object) St[0 .. r) = Ok, the state words, answered.
// Only commit writes St and the state words, each object's own workgroup behind its barrier (rank_state.hpp).  rows and
// move both read the list that plan wrote and write disjoint memory (rows of R; pieces): they are independent.
//
// Rules kept by every kernel (rank_large.hip): no workgroup waits for another; every branch around a barrier is
// workgroup-uniform, on values passed through readfirstlane; early returns come before any barrier; shared global
// state is ordered by barriers and kernel boundaries only.
#include "../../include/rlnc_hip.h"
#include "rank_compact_kernels.hpp"

namespace rlnc {

namespace {

constexpr int kCompactRows = 16;  // stored rows per workgroup of the rows grid: four passes of a row per wave
constexpr int kMoveDepth = 8;     // steps of the move whose loads are issued before their stores

struct CompactParams {
    uint8_t *pieces;
    int64_t obj_stride, piece_stride;
    uint32_t *ws;
    int64_t ws_obj;  // dwords
    const int32_t *retire;
    int32_t *kept, *answered;  // each optional
    int k, m, n_obj;
    int off_st, off_q, off_r;  // large_layout(k, m), dwords from the object's state words
    int D, kd, me;             // dwords of a row, of its coefficient part, of its e part
    int row_chunks, col_chunks;  // flat grids: chunks fastest, then objects
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

enum class Obj { Retired, Bad, Idle, Active };

// what the call does with object o, from its state words and the retire flag; workgroup-uniform.  No launch but commit
// writes either, and commit calls this before its barrier.
__device__ __forceinline__ Obj classify(const CompactParams &p, const uint32_t *ws, int o, int &rank, int &done) {
    rank = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    done = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
    const int ret = p.retire != nullptr ? __builtin_amdgcn_readfirstlane(p.retire[o]) : 0;
    if (ret != 0) return Obj::Retired;
    if (rank < 0 || rank > p.k || done < rank || done > p.m) return Obj::Bad;
    return done == rank ? Obj::Idle : Obj::Active;
}

// the list u of an active object into LDS, each entry clamped to a slot of the object (a list that plan wrote is
// within [0, done) already: the clamp keeps every later address inside the object whatever the state held)
__device__ __forceinline__ void stage_list(uint16_t *us, const uint32_t *list, int r, int m) {
    for (int j = int(threadIdx.x); j < r; j += 256) us[j] = uint16_t(min(list[j], uint32_t(m - 1)));
}

__global__ __launch_bounds__(256) void gf_stream_compact_plan(CompactParams p) {
    __shared__ int32_t cnt[256];
    const int o = int(blockIdx.x), tid = int(threadIdx.x), k = p.k;
    uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    int32_t *kept = p.kept != nullptr ? p.kept + int64_t(o) * k : nullptr;
    int rank, done;
    const Obj what = classify(p, ws, o, rank, done);
    if (what == Obj::Retired || what == Obj::Bad) {  // before any barrier
        if (kept != nullptr)
            for (int j = tid; j < k; j += 256) kept[j] = -1;
        return;
    }
    const int32_t *St = reinterpret_cast<const int32_t *>(ws + p.off_st);
    uint32_t *list = what == Obj::Active ? ws + p.off_q : nullptr;
    const int seg = (done + 255) >> 8, t0 = min(tid * seg, done), t1 = min(t0 + seg, done);
    int n = 0;
    for (int t = t0; t < t1; ++t) n += St[t] == RLNC_OK ? 1 : 0;
    cnt[tid] = n;
    __syncthreads();
    int pos = 0, total = 0;
    for (int j = 0; j < 256; ++j) {
        const int c = cnt[j];
        pos += j < tid ? c : 0;
        total += c;
    }
    for (int t = t0; t < t1; ++t)
        if (St[t] == RLNC_OK) {
            if (pos < k) {
                if (list != nullptr) list[pos] = uint32_t(t);
                if (kept != nullptr) kept[pos] = t;
            }
            ++pos;
        }
    if (kept != nullptr)
        for (int j = min(total, k) + tid; j < k; j += 256) kept[j] = -1;
}

__global__ __launch_bounds__(256) void gf_stream_compact_rows(CompactParams p) {
    __shared__ uint16_t us[kLargeMaxK];
    __shared__ uint32_t eb[4][kLargeMaxM / 4];
    const int o = int(blockIdx.x) / p.row_chunks, rc = int(blockIdx.x) % p.row_chunks;
    uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    int r, done;
    if (classify(p, ws, o, r, done) != Obj::Active) return;
    const int row0 = rc * kCompactRows;
    if (row0 >= r) return;
    stage_list(us, ws + p.off_q, r, p.m);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6), lane = int(threadIdx.x) & 63;
    const int me = p.me;
    uint32_t *ew = eb[wave];
    const uint8_t *eB = reinterpret_cast<const uint8_t *>(ew);
    for (int it = 0; it < kCompactRows / 4; ++it) {
        const int row = row0 + 4 * it + wave;
        const bool live = row < r;
        uint32_t *e = ws + p.off_r + int64_t(row) * p.D + p.kd;
        if (live)
            for (int d = lane; d < me; d += 64) ew[d] = e[d];
        __syncthreads();
        if (live)
            for (int d = lane; d < me; d += 64) {
                uint32_t w = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (4 * d + c < r) w |= uint32_t(eB[us[4 * d + c]]) << (8 * c);
                e[d] = w;
            }
        __syncthreads();
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gf_stream_compact_move(CompactParams p) {
    __shared__ uint16_t us[kLargeMaxK];
    const int o = int(blockIdx.x) / p.col_chunks, chunk = int(blockIdx.x) % p.col_chunks;
    const uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    int r, done;
    if (classify(p, ws, o, r, done) != Obj::Active) return;
    stage_list(us, ws + p.off_q, r, p.m);
    __syncthreads();
    int j0 = 0;  // the first j with u_j != j
    for (int hi = r; j0 < hi;) {
        const int mid = (j0 + hi) >> 1;
        if (int(us[mid]) == mid)
            j0 = mid + 1;
        else
            hi = mid;
    }
    const int tid = int(threadIdx.x);
    const int64_t S = p.piece_stride, cbase = int64_t(chunk) * kCompactColChunk;
    uint8_t *base = p.pieces + int64_t(o) * p.obj_stride + cbase;
    // a piece's last chunk takes its tail too (up to two chunks less a byte, in a second pass), so that a piece a few
    // bytes beyond a multiple of the chunk does not cost a workgroup of its own
    const int64_t width = chunk + 1 == p.col_chunks ? S - cbase : int64_t(kCompactColChunk);
    for (int64_t c0 = 0; c0 < width; c0 += kCompactColChunk) {
        const int64_t left = width - c0;  // > 0: bytes of a piece from this pass's first column on
        if constexpr (VEC) {
            uint8_t *col = base + c0 + 16 * tid;
            const int64_t n = left - 16 * tid;
            if (n >= 16) {
                int j = j0;
                for (; j + kMoveDepth <= r; j += kMoveDepth) {
                    u32x4_t x[kMoveDepth];
#pragma unroll
                    for (int q = 0; q < kMoveDepth; ++q)
                        x[q] = *reinterpret_cast<const u32x4_t *>(col + int64_t(us[j + q]) * S);
#pragma unroll
                    for (int q = 0; q < kMoveDepth; ++q) *reinterpret_cast<u32x4_t *>(col + int64_t(j + q) * S) = x[q];
                }
                for (; j < r; ++j)
                    *reinterpret_cast<u32x4_t *>(col + int64_t(j) * S) =
                        *reinterpret_cast<const u32x4_t *>(col + int64_t(us[j]) * S);
            } else if (n > 0) {
                // the last lane of a piece: its columns byte by byte (source and destination slots differ)
                for (int j = j0; j < r; ++j) {
                    const uint8_t *src = col + int64_t(us[j]) * S;
                    uint8_t *dst = col + int64_t(j) * S;
                    for (int i = 0; i < int(n); ++i) dst[i] = src[i];
                }
            }
        } else {
            // single bytes: every lane owns the 16 columns tid + 256 i of the pass
            for (int j = j0; j < r; ++j) {
                const uint8_t *src = base + c0 + tid + int64_t(us[j]) * S;
                uint8_t *dst = base + c0 + tid + int64_t(j) * S;
                uint8_t x[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) x[i] = tid + 256 * i < left ? src[256 * i] : uint8_t(0);
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (tid + 256 * i < left) dst[256 * i] = x[i];
            }
        }
    }
}

__global__ __launch_bounds__(256) void gf_stream_compact_commit(CompactParams p) {
    const int o = int(blockIdx.x), tid = int(threadIdx.x);
    uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    int r, done;
    const Obj what = classify(p, ws, o, r, done);
    if (what == Obj::Bad || what == Obj::Idle) {  // before any barrier: nothing of the state is written
        if (tid == 0 && p.answered != nullptr) p.answered[o] = what == Obj::Idle ? r : 0;
        return;
    }
    __syncthreads();  // every wave has read the words that thread 0 rewrites
    if (what == Obj::Retired) r = 0;
    int32_t *St = reinterpret_cast<int32_t *>(ws + p.off_st);
    for (int t = tid; t < r; t += 256) St[t] = RLNC_OK;
    if (tid == 0) {
        store_state(ws, r, r);
        if (p.answered != nullptr) p.answered[o] = r;
    }
}

}  // namespace

hipError_t launch_rank_stream_compact(const RrefParams &rp, uint8_t *pieces, void *state, size_t state_bytes,
                                      const int32_t *retire, int32_t *kept, int32_t *answered, bool vec16,
                                      hipStream_t s) {
    if (rp.n_obj <= 0) return hipSuccess;
    if (rp.objs != nullptr || rank_state_check(rp.k, rp.m, rp.n_obj, state, state_bytes) != hipSuccess)
        return hipErrorInvalidValue;
    const LargeLayout L = large_layout(rp.k, rp.m);
    CompactParams p{};
    p.pieces = pieces;
    p.obj_stride = rp.obj_stride;
    p.piece_stride = rp.piece_stride;
    p.ws = static_cast<uint32_t *>(state);
    p.ws_obj = int64_t(L.total);
    p.retire = retire;
    p.kept = kept;
    p.answered = answered;
    p.k = rp.k;
    p.m = rp.m;
    p.n_obj = rp.n_obj;
    p.off_st = int(L.st);
    p.off_q = int(L.q);
    p.off_r = int(L.r);
    p.D = L.D;
    p.kd = (rp.k + 3) >> 2;
    p.me = (rp.m + 3) >> 2;
    p.row_chunks = (rp.k + kCompactRows - 1) / kCompactRows;
    const int64_t nobj = rp.n_obj;
    int64_t g_move = 0;
    if (pieces != nullptr) {
        if (rp.piece_stride <= 0 || rp.obj_stride < int64_t(rp.m) * rp.piece_stride) return hipErrorInvalidValue;
        // a piece's last chunk takes its tail too: floor, at least one
        const int64_t chunks = rp.piece_stride < kCompactColChunk ? 1 : rp.piece_stride / kCompactColChunk;
        g_move = nobj * chunks;
        if (chunks > 0x7FFFFFFF || g_move > 0x7FFFFFFF) return hipErrorInvalidValue;
        p.col_chunks = int(chunks);
    }
    const int64_t g_rows = nobj * p.row_chunks;
    if (g_rows > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gf_stream_compact_plan, dim3(unsigned(nobj)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(gf_stream_compact_rows, dim3(unsigned(g_rows)), dim3(256), 0, s, p);
    if (pieces != nullptr) {
        if (vec16)
            hipLaunchKernelGGL(gf_stream_compact_move<true>, dim3(unsigned(g_move)), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL(gf_stream_compact_move<false>, dim3(unsigned(g_move)), dim3(256), 0, s, p);
    }
    hipLaunchKernelGGL(gf_stream_compact_commit, dim3(unsigned(nobj)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace rlnc
