// rank_large.hip — the true-rank elimination for generations whose [coeffs | E] matrix does not fit one workgroup's LDS
// (decode paths 7 and 8; semantics: include/rlnc_hip.h, "Rank mode"; interface: rank_large_kernels.hpp; the limits, the
// layout and the state words with their protocol: rank_state.hpp).
//
// Per object the state lives in a device workspace: the stored rows R[rank][D] in arrival order (D = ceil(k/4) +
// ceil(m/4) dwords, [c | e] as in rank.hip), their pivot columns piv[], the statuses St[], and the four state words.
// The pieces are taken B at a time (large_block); every row operation is independent per column, only the decisions
// read particular columns, so a block is three launches with no waiting between workgroups -- the order between them
// is the stream's:
//   reduce  (object x 64-dword column chunk; 4 waves = 4 groups of the block's pieces, piece t = 4j + wave)
//           X_t = [h_t | unit(t)] ^ XOR_{i < rank} h_t[piv_i] · R_i.  The quotients are bytes of the headers themselves:
//           R is a reduced row-echelon form, so row i is the only stored row with a nonzero byte in column piv_i.
//           They are staged 256 rows at a time in LDS; a ballot over 64 rows keeps those with a nonzero quotient for the
//           wave's pieces, and only those are loaded and multiplied -- sparse coding vectors keep this short.
//   step    (one workgroup per object, X in LDS) rank.hip's per-piece loop over the block only: reduce X_t against the
//           block's earlier new rows (quotients: X_t's bytes in their pivot columns, snapshotted first), first nonzero
//           coefficient byte = pivot (none: PieceNotUseful), normalise, clear the pivot column from the earlier new
//           rows.  rank = k: ReceivedAllPieces for the rest.  The c new rows go to R[rank .. rank + c), and
//           Q[i][s] = R_i[pc_s] is snapshotted for every older row i, so that the update reads no column another
//           workgroup is rewriting.
//   update  (object x 64-dword column chunk x 64-row chunk) R_i ^= XOR_s Q[i][s] · Y_s for the older rows i.
// A last launch writes T through the pivot-order permutation (all k rows, zero past rank), the statuses and the rank.
//
// Why this equals the one-piece-at-a-time model: write P for the pivot set after a block.  X_t lies in [h_t | unit(t)] +
// span(stored rows) and is zero in every old pivot column (row i has 1 there, the other old rows 0).  The new rows are
// built from such vectors only, so they are zero in the old pivot columns too, and the step keeps them reduced among
// themselves; piece t's vector after the step's reduction is therefore the element of [h_t | unit(t)] + span(rows
// so far) that is zero in all pivot columns so far.  That element is unique (two of them differ by a combination of
// the rows that is zero in every pivot column, i.e. the zero combination), and it is what the model computes -- so the
// pivot, the status and the normalised row are the model's.  After the update every row has 1 in its own pivot column
// and 0 in the rest of P, which determines it within the span: the state is the model's state after the same pieces.
//
// The stream form (template parameter STREAM; decode streams, rank_large_kernels.hpp): the state outlives the call, and
// a block is each object's own, read from its state words (rank_state.hpp).  The proof above is per block and does not
// say where a block starts, so it holds for these blocks as it stands.  What differs from the one-shot form: an object
// with b = 0 is idle (every workgroup of it returns before any barrier), and an object at rank k still has its slots
// answered by the step (ReceivedAllPieces, done += b), because the snapshot tells answered slots from pending ones.
// The one-shot instantiations keep the instructions they had before the parameter existed.
//
// Rules kept by every kernel: no workgroup waits for another; every branch around a barrier is workgroup-uniform, on
// values read after the previous barrier and passed through readfirstlane; the early return (nothing left to do) comes
// before any barrier; shared global state is ordered by barriers and kernel boundaries only.
#include <type_traits>

#include "../../include/rlnc_hip.h"
#include "gf_perm.hpp"
#include "rref.hpp"
#include "rank_large_kernels.hpp"

namespace rlnc {

namespace {

constexpr int kColChunk = 64;             // dwords of a row per workgroup of the reduce and update grids
constexpr int kQTile = 256;               // stored rows whose quotients the reduce stages at a time (a multiple of 64)
constexpr int kUpdRows = 64;              // stored rows per workgroup of the update grid
constexpr int kFinRows = 16;              // T rows per workgroup of the final grid

struct LargeParams {
    const uint8_t *pieces;
    int64_t obj_stride, piece_stride;
    uint8_t *T;
    int64_t T_obj;
    int32_t *status;
    int32_t *rank;
    uint32_t *ws;
    int64_t ws_obj;  // dwords
    int k, m;
    int t0, b;  // this block: pieces t0 .. t0 + b - 1 (t0 = 0: the state is not read, the rank is 0)
    // the grids are flat (blockIdx.x only, so the object count is not bound by a grid dimension): column chunks
    // fastest, then the update's row chunks / the final launch's row chunks, then objects
    int chunks, row_chunks, fin_chunks;
};

// The stream form of a block (STREAM kernels): the object's own block, from its state instead of the launch's t0 and
// b -- pieces done .. min(done + B, target) - 1.  b <= 0: the object is idle in this block.  Both values are
// workgroup-uniform: no launch that calls this writes kStDone or kStTarget before a barrier that follows the call.
__device__ __forceinline__ void stream_block(const uint32_t *ws, int B, int &t0, int &b) {
    t0 = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
    b = min(B, __builtin_amdgcn_readfirstlane(int(ws[kStTarget])) - t0);
}

template <bool STREAM>
__global__ __launch_bounds__(256) void gf_rank_large_reduce(LargeParams p) {
    __shared__ uint32_t tab[kMulTabDw];
    __shared__ uint2 qh[4][kQTile];
    const int k = p.k, m = p.m;
    const LargeLayout L = large_layout(k, m);
    const int kd = (k + 3) >> 2, D = L.D;
    const int o = int(blockIdx.x) / p.chunks, chunk = int(blockIdx.x) % p.chunks;
    uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    int t0 = p.t0, b = p.b;
    if constexpr (STREAM) {
        stream_block(ws, L.B, t0, b);
        if (b <= 0) return;  // an idle object: nothing new in this block
    }
    const int rank = (!STREAM && t0 == 0) ? 0 : __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    if (rank >= k) return;  // ReceivedAllPieces for the whole block: the step only answers
    const int32_t *piv = reinterpret_cast<const int32_t *>(ws + L.piv);
    const uint32_t *R = ws + L.r;
    uint32_t *X = ws + L.x;
    const int tid = int(threadIdx.x), lane = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);  // this wave's pieces: t = 4j + g
    const int d = chunk * kColChunk + lane;
    const bool act = d < D;
    const uint8_t *base = p.pieces + int64_t(o) * p.obj_stride;

    copy_table(tab);
    uint32_t acc[kLargeMaxB / 4];
#pragma unroll
    for (int j = 0; j < kLargeMaxB / 4; ++j) {
        acc[j] = 0;
        const int t = 4 * j + g;
        if (t < b && act) {
            const int pi = t0 + t;
            if (d < kd) {
                const uint8_t *h = base + int64_t(pi) * p.piece_stride;
                uint32_t w = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (4 * d + c < k) w |= uint32_t(h[4 * d + c]) << (8 * c);
                acc[j] = w;
            } else {
                acc[j] = (d - kd) == (pi >> 2) ? 1u << (8 * (pi & 3)) : 0u;
            }
        }
    }
    for (int i0 = 0; i0 < rank; i0 += kQTile) {
        __syncthreads();  // the previous tile's quotients are consumed (first pass: the table is in LDS)
        {  // a thread takes kQTile / 64 (row, piece group) pairs: their pivot columns first, then 8 header bytes each,
           // all in flight at once
            constexpr int NP = kQTile / 64;
            const int gg = tid & 3;
            int pc[NP];
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                const int i = i0 + (tid >> 2) + 64 * r;
                pc[r] = i < rank ? piv[i] : -1;
            }
            uint8_t hb[NP][kLargeMaxB / 4];
#pragma unroll
            for (int r = 0; r < NP; ++r)
#pragma unroll
                for (int j = 0; j < kLargeMaxB / 4; ++j) {
                    const int t = 4 * j + gg;
                    hb[r][j] = (pc[r] >= 0 && t < b) ? base[int64_t(t0 + t) * p.piece_stride + pc[r]] : uint8_t(0);
                }
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                uint32_t q[2] = {0u, 0u};
#pragma unroll
                for (int j = 0; j < kLargeMaxB / 4; ++j) q[j >> 2] |= uint32_t(hb[r][j]) << (8 * (j & 3));
                qh[gg][(tid >> 2) + 64 * r] = make_uint2(q[0], q[1]);
            }
        }
        __syncthreads();
        const int n = min(kQTile, rank - i0);
        // 64 rows at a time, a lane each: a ballot keeps the rows with a nonzero quotient for this wave's pieces, so the
        // others cost nothing.  The kept rows go four at a time, quotients scalar (readlane), the next four's row dwords
        // fetched while these are multiplied; a group is empty exactly when its first entry is (bits are taken in order).
        for (int s0 = 0; s0 < n; s0 += 64) {
            const uint2 ql = s0 + lane < n ? qh[g][s0 + lane] : make_uint2(0u, 0u);
            uint64_t mk = ballot((ql.x | ql.y) != 0u);
            uint32_t qa[4], qb[4], x[4];
            auto fetch = [&]() {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    qa[u] = qb[u] = x[u] = 0u;
                    if (mk) {
                        const int r = __builtin_ctzll(mk);
                        mk &= mk - 1;
                        qa[u] = uint32_t(__builtin_amdgcn_readlane(int(ql.x), r));
                        qb[u] = uint32_t(__builtin_amdgcn_readlane(int(ql.y), r));
                        if (act) x[u] = R[int64_t(i0 + s0 + r) * D + d];
                    }
                }
            };
            fetch();
            for (;;) {
                uint32_t ca[4], cb[4], cx[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) ca[u] = qa[u], cb[u] = qb[u], cx[u] = x[u];
                if ((ca[0] | cb[0]) == 0u) break;
                fetch();
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if ((ca[u] | cb[u]) == 0u) continue;
#pragma unroll
                    for (int j = 0; j < kLargeMaxB / 4; ++j) {  // no test per product: the table reads issue together
                        const uint32_t q = ((j < 4 ? ca[u] : cb[u]) >> (8 * (j & 3))) & 0xFFu;
                        acc[j] ^= mul4(tab, q, cx[u]);  // pieces past the block have zero quotients
                    }
                }
            }
        }
    }
    if (act) {
#pragma unroll
        for (int j = 0; j < kLargeMaxB / 4; ++j) {
            const int t = 4 * j + g;
            if (t < b) X[int64_t(t) * D + d] = acc[j];
        }
    }
}

template <bool STREAM>
__global__ __launch_bounds__(256) void gf_rank_large_step(LargeParams p) {
    extern __shared__ uint32_t lds[];
    const int k = p.k, m = p.m;
    const LargeLayout L = large_layout(k, m);
    const int kd = (k + 3) >> 2, D = L.D;
    uint32_t *ws = p.ws + int64_t(blockIdx.x) * p.ws_obj;
    const int tid = int(threadIdx.x), lane = tid & 63;
    int t0 = p.t0, b = p.b;
    if constexpr (STREAM) stream_block(ws, L.B, t0, b);
    const int rank0 = (!STREAM && t0 == 0) ? 0 : __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    int32_t *St = reinterpret_cast<int32_t *>(ws + L.st);
    if constexpr (STREAM) {
        if (b <= 0) {  // an idle object: kStRankBefore still moves up to the rank (rank_state.hpp)
            if (tid == 0) ws[kStRankBefore] = uint32_t(rank0);
            return;
        }
        if (rank0 >= k) {  // the block's slots are consumed all the same: the snapshot tells them from pending ones
            __syncthreads();  // every wave has read the state that thread 0 rewrites
            for (int tt = tid; tt < b; tt += 256) St[t0 + tt] = RLNC_ERR_RECEIVED_ALL_PIECES;
            if (tid == 0) {
                ws[kStRankBefore] = uint32_t(rank0);
                ws[kStDone] = uint32_t(t0 + b);
            }
            return;
        }
    } else if (rank0 >= k) {  // nothing to do: the update sees no new rows, the final launch answers ReceivedAllPieces
        if (tid == 0) ws[kStRankBefore] = uint32_t(rank0);
        return;
    }
    int32_t *piv = reinterpret_cast<int32_t *>(ws + L.piv);
    uint32_t *Q = ws + L.q;
    const uint32_t *X = ws + L.x;
    uint32_t *R = ws + L.r;
    uint32_t *tab = lds;
    uint32_t *Xs = lds + kMulTabDw;  // the block's rows, then the small arrays
    const uint8_t *XsB = reinterpret_cast<const uint8_t *>(Xs);
    int32_t *npiv = reinterpret_cast<int32_t *>(Xs + size_t(L.B) * D);  // pivot column of new row s
    int32_t *nrow = npiv + kLargeMaxB;                                  // its row of Xs
    int32_t *rpiv = nrow + kLargeMaxB;                                  // pivot column of block row t, -1: not a new row
    uint32_t *qx = reinterpret_cast<uint32_t *>(rpiv + kLargeMaxB);     // 32 quotient bytes, one per block row
    uint8_t *qxB = reinterpret_cast<uint8_t *>(qx);

    copy_table(tab);
    {  // the block's rows, 16 bytes a lane and four loads in flight
        const int n4 = (b * D) >> 2;
        const uint4 *src = reinterpret_cast<const uint4 *>(X);
        uint4 *dst = reinterpret_cast<uint4 *>(Xs);
        for (int i0 = tid; i0 < n4; i0 += 4 * 256) {
            uint4 x4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x4[u] = i0 + 256 * u < n4 ? src[i0 + 256 * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + 256 * u < n4) dst[i0 + 256 * u] = x4[u];
        }
        for (int idx = 4 * n4 + tid; idx < b * D; idx += 256) Xs[idx] = X[idx];
    }
    if (tid < kLargeMaxB) rpiv[tid] = -1;
    __syncthreads();

    // row_t ^= XOR_{t' < t} q[t'] · row_t' (read) or row_t' ^= q[t'] · row_t (!read), q = the 32 bytes of qx (zero for a
    // row that takes no part).  Wave w owns the 64-dword slots w, w + 4, ... of every row, two slots at a time.  Rows go
    // four at a time, skipped when their four quotients are zero; inside a group nothing is tested, so its LDS reads
    // issue together: lanes past the row's end work on a dummy dword of their own instead of being masked.  A group
    // never reaches past row B - 1 (B is a multiple of 4, and rows >= t have zero quotients).
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslots = (D + 63) >> 6;
    const int dummy = L.B * D + 3 * kLargeMaxB + kLargeMaxB / 4 + lane;  // index from Xs, after the small arrays
    auto rows_muladd = [&](int t, auto read_c, uint32_t scale) {
        constexpr bool read = decltype(read_c)::value;
        uint32_t qw[kLargeMaxB / 4];
#pragma unroll
        for (int j = 0; j < kLargeMaxB / 4; ++j) qw[j] = uni(qx[j]);
        for (int s0 = wv; s0 < nslots; s0 += 8) {
            int dd[2];  // this lane's dword of the two slots, or -1
            uint32_t a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int d = 64 * (s0 + 4 * i) + lane;
                dd[i] = d < D ? d : -1;
                a[i] = Xs[dd[i] >= 0 ? t * D + dd[i] : dummy];
                if (!read) a[i] = mul4(tab, scale, a[i]);  // the normalised new row
            }
#pragma unroll
            for (int j = 0; j < kLargeMaxB / 4; ++j) {
                if (qw[j] == 0u) continue;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t q = (qw[j] >> (8 * u)) & 0xFFu;
                    const uint4 t4 = *reinterpret_cast<const uint4 *>(tab + q * kTabDw);
                    const uint32_t t2 = tab[q * kTabDw + 4];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int at = dd[i] >= 0 ? (4 * j + u) * D + dd[i] : dummy;
                        if (read) a[i] ^= mul4t(t4, t2, Xs[at]);
                        else Xs[at] ^= mul4t(t4, t2, a[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) Xs[dd[i] >= 0 ? t * D + dd[i] : dummy] = a[i];
        }
    };

    int c = 0, t = 0;
    for (; t < b; ++t) {
        if (rank0 + c == k) break;
        uint32_t *v = Xs + t * D;
        // reduce against the block's earlier new rows: the quotients are the piece's bytes in their pivot columns
        if (tid < kLargeMaxB) {
            const int pv = tid < t ? rpiv[tid] : -1;
            qxB[tid] = pv >= 0 ? XsB[size_t(t) * 4 * D + pv] : uint8_t(0);
        }
        __syncthreads();
        rows_muladd(t, std::true_type{}, 0u);
        __syncthreads();
        // pivot: every wave scans the coefficient dwords
        int pc = -1;
        uint32_t val = 0;
        for (int b0 = 0; b0 < kd; b0 += 64) {
            const int d = b0 + lane;
            const uint32_t w = d < kd ? v[d] : 0u;
            const uint64_t mk = ballot(w != 0);
            if (mk) {
                const int j = __builtin_ctzll(mk);
                const uint32_t word = uint32_t(__builtin_amdgcn_readlane(int(w), j));
                const int by = __builtin_ctz(word) >> 3;
                pc = (b0 + j) * 4 + by;
                val = (word >> (8 * by)) & 0xFFu;
                break;
            }
        }
        pc = __builtin_amdgcn_readfirstlane(pc);
        val = uni(val);
        if (pc < 0) {
            if (tid == 0) St[t0 + t] = RLNC_ERR_PIECE_NOT_USEFUL;
            continue;
        }
        // insert: snapshot the earlier new rows' bytes in the pivot column, normalise, clear (a thread owns its columns)
        if (tid < kLargeMaxB) {
            const int pv = tid < t ? rpiv[tid] : -1;
            qxB[tid] = pv >= 0 ? XsB[size_t(tid) * 4 * D + pc] : uint8_t(0);
        }
        __syncthreads();  // every wave has scanned row t, the quotients are in place
        if (tid == 0) {
            npiv[c] = pc;
            nrow[c] = t;
            rpiv[t] = pc;
            St[t0 + t] = RLNC_OK;
        }
        rows_muladd(t, std::false_type{}, gfinv(tab, val));
        ++c;
        __syncthreads();
    }
    for (int tt = t + tid; tt < b; tt += 256) St[t0 + tt] = RLNC_ERR_RECEIVED_ALL_PIECES;
    // the new rows, their pivots and the older rows' quotients
    for (int s = 0; s < c; ++s) {
        const uint32_t *y = Xs + nrow[s] * D;
        uint32_t *dst = R + int64_t(rank0 + s) * D;
        for (int d = tid; d < D; d += 256) dst[d] = y[d];
    }
    if (tid < c) piv[rank0 + tid] = npiv[tid];
    const uint8_t *RB = reinterpret_cast<const uint8_t *>(R);
    {  // thread = (row, dword of four quotients): the new pivot columns once, then four rows' bytes in flight
        const int w = tid & 7;
        int pcs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pcs[u] = 4 * w + u < c ? npiv[4 * w + u] : -1;
        for (int i0 = tid >> 3; i0 < rank0; i0 += 4 * 32) {
            uint8_t qb[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 32 * r;
                    qb[r][u] = (i < rank0 && pcs[u] >= 0) ? RB[int64_t(i) * 4 * D + pcs[u]] : uint8_t(0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 32 * r;
                if (i < rank0)
                    Q[i * (kLargeMaxB / 4) + w] = uint32_t(qb[r][0]) | uint32_t(qb[r][1]) << 8 | uint32_t(qb[r][2]) << 16 |
                                                  uint32_t(qb[r][3]) << 24;
            }
        }
    }
    if (tid == 0) {
        ws[kStRankBefore] = uint32_t(rank0);
        ws[kStRank] = uint32_t(rank0 + c);
        ws[kStDone] = uint32_t(t0 + b);
    }
}

__global__ __launch_bounds__(256) void gf_rank_large_update(LargeParams p) {
    __shared__ uint32_t tab[kMulTabDw];
    const LargeLayout L = large_layout(p.k, p.m);
    const int D = L.D;
    const int chunk = int(blockIdx.x) % p.chunks, rest = int(blockIdx.x) / p.chunks;
    uint32_t *ws = p.ws + int64_t(rest / p.row_chunks) * p.ws_obj;
    const int rank = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    const int rprev = __builtin_amdgcn_readfirstlane(int(ws[kStRankBefore]));
    const int c = rank - rprev;
    const int row0 = (rest % p.row_chunks) * kUpdRows;
    if (c <= 0 || row0 >= rprev) return;  // no new rows in this block, or no older rows in this chunk
    const uint4 *Q = reinterpret_cast<const uint4 *>(ws + L.q);
    uint32_t *R = ws + L.r;
    const int tid = int(threadIdx.x), lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int d = chunk * kColChunk + lane;
    const bool act = d < D;
    copy_table(tab);
    uint32_t y[kLargeMaxB];
#pragma unroll
    for (int s = 0; s < kLargeMaxB; ++s) y[s] = (s < c && act) ? R[int64_t(rprev + s) * D + d] : 0u;
    __syncthreads();
    const int row1 = min(row0 + kUpdRows, rprev);
    for (int i = row0 + w; i < row1; i += 8) {  // two rows of this wave in flight
        uint32_t q[2][8], r[2];
        bool any[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int iu = i + 4 * u;
            const bool in = iu < row1;
            const uint4 a = in ? Q[2 * iu] : make_uint4(0, 0, 0, 0), bq = in ? Q[2 * iu + 1] : make_uint4(0, 0, 0, 0);
            q[u][0] = uni(a.x), q[u][1] = uni(a.y), q[u][2] = uni(a.z), q[u][3] = uni(a.w);
            q[u][4] = uni(bq.x), q[u][5] = uni(bq.y), q[u][6] = uni(bq.z), q[u][7] = uni(bq.w);
            any[u] = (q[u][0] | q[u][1] | q[u][2] | q[u][3] | q[u][4] | q[u][5] | q[u][6] | q[u][7]) != 0u;
            r[u] = 0;
            if (any[u] && act) r[u] = R[int64_t(iu) * D + d];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!any[u]) continue;
            uint32_t a = r[u];
#pragma unroll
            for (int s4 = 0; s4 < kLargeMaxB / 4; ++s4) {  // four products per test: their table reads issue together
                if (q[u][s4] == 0u) continue;
#pragma unroll
                for (int s = 4 * s4; s < 4 * s4 + 4; ++s) a ^= mul4(tab, (q[u][s4] >> (8 * (s & 3))) & 0xFFu, y[s]);
            }
            if (act) R[int64_t(i + 4 * u) * D + d] = a;
        }
    }
}

// STREAM: the snapshot of a decode stream -- every output optional, RLNC_STATUS_PENDING for the slots not yet answered
template <bool STREAM>
__global__ __launch_bounds__(256) void gf_rank_large_final(LargeParams p) {
    __shared__ int32_t colrow[kLargeMaxK];  // stored row of pivot column c, or -1
    __shared__ int32_t ord[kLargeMaxK];     // stored row of T row r
    __shared__ int32_t cnt[256];
    const int k = p.k, m = p.m;
    const LargeLayout L = large_layout(k, m);
    const int kd = (k + 3) >> 2, D = L.D;
    const int o = int(blockIdx.x) / p.fin_chunks, fc = int(blockIdx.x) % p.fin_chunks;
    const uint32_t *ws = p.ws + int64_t(o) * p.ws_obj;
    const int tid = int(threadIdx.x);
    if constexpr (STREAM)
        if (p.T == nullptr && fc != 0) return;  // only T is spread over the row chunks
    const int rank = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
    const int done = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
    const int32_t *piv = reinterpret_cast<const int32_t *>(ws + L.piv);
    const int32_t *St = reinterpret_cast<const int32_t *>(ws + L.st);
    const uint32_t *R = ws + L.r;
    // stored row t goes to T row (number of smaller pivots)
    for (int c = tid; c < k; c += 256) colrow[c] = -1;
    __syncthreads();
    for (int t = tid; t < rank; t += 256) colrow[piv[t]] = t;
    __syncthreads();
    const int seg = (k + 255) >> 8, c0 = min(tid * seg, k), c1 = min(c0 + seg, k);
    int n = 0;
    for (int c = c0; c < c1; ++c) n += colrow[c] >= 0 ? 1 : 0;
    cnt[tid] = n;
    __syncthreads();
    int pos = 0;
    for (int j = 0; j < tid; ++j) pos += cnt[j];
    for (int c = c0; c < c1; ++c)
        if (colrow[c] >= 0) ord[pos++] = colrow[c];
    __syncthreads();
    const int r0 = fc * kFinRows, r1 = min(r0 + kFinRows, k);
    uint8_t *T = p.T + int64_t(o) * p.T_obj;
    const bool want_T = !STREAM || p.T != nullptr;
    if (!want_T) {
        // a snapshot without T
    } else if ((m & 3) == 0 && (reinterpret_cast<uintptr_t>(T) & 3) == 0) {
        const int mw = m >> 2;
        uint32_t *Tw = reinterpret_cast<uint32_t *>(T);
        for (int idx = tid; idx < (r1 - r0) * mw; idx += 256) {
            const int r = r0 + idx / mw, c = idx % mw;
            Tw[int64_t(r) * mw + c] = r < rank ? R[int64_t(ord[r]) * D + kd + c] : 0u;
        }
    } else {
        const uint8_t *E = reinterpret_cast<const uint8_t *>(R) + 4 * kd;
        for (int idx = tid; idx < (r1 - r0) * m; idx += 256) {
            const int r = r0 + idx / m, c = idx % m;
            T[int64_t(r) * m + c] = r < rank ? E[int64_t(ord[r]) * 4 * D + c] : uint8_t(0);
        }
    }
    if (fc == 0) {
        if (!STREAM || p.status != nullptr)
            for (int t = tid; t < m; t += 256)
                p.status[int64_t(o) * m + t] =
                    t < done ? St[t] : int32_t(STREAM ? RLNC_STATUS_PENDING : RLNC_ERR_RECEIVED_ALL_PIECES);
        if (tid == 0 && (!STREAM || p.rank != nullptr)) p.rank[o] = rank;
    }
}

// ---- decode streams: the small launches around the blocks of a push --------------------------------------------------
// one thread per object

__global__ __launch_bounds__(256) void gf_rank_stream_init(uint32_t *ws, int64_t ws_obj, int nobj) {
    const int o = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (o < nobj) *reinterpret_cast<uint4 *>(ws + int64_t(o) * ws_obj) = make_uint4(0u, 0u, 0u, 0u);
}

// the latch: the push target rule of rank_state.hpp, written out (the host passes max_new <= m)
__global__ __launch_bounds__(256) void gf_rank_stream_latch(uint32_t *ws, int64_t ws_obj, int nobj,
                                                           const int32_t *avail, int m, int max_new) {
    const int o = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (o >= nobj) return;
    uint32_t *st = ws + int64_t(o) * ws_obj;
    const int done = int(st[kStDone]);
    int target = done;
    if (done >= 0 && done < m) target = min(min(max(avail[o], done), m), done + min(max_new, m - done));
    st[kStTarget] = uint32_t(target);
}

__global__ __launch_bounds__(256) void gf_rank_stream_progress(const uint32_t *ws, int64_t ws_obj, int nobj,
                                                              int32_t *rank, int32_t *answered) {
    const int o = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (o >= nobj) return;
    const uint32_t *st = ws + int64_t(o) * ws_obj;
    if (rank != nullptr) rank[o] = int32_t(st[kStRank]);
    if (answered != nullptr) answered[o] = int32_t(st[kStDone]);
}

// the 160 KiB dynamic-LDS attribute of the block step (both forms), once per device
hipError_t step_attr() {
    static MaxLdsAttr attr;
    return attr.set(&gf_rank_large_step<false>, &gf_rank_large_step<true>);
}

// the launches' common part: the shape and workspace checks, the step's LDS attribute, the parameters and the grids
struct LargeGrids {
    size_t step_lds;
    unsigned reduce, step, update, fin;
};
hipError_t large_setup(const RrefParams &rp, const void *ws, size_t ws_bytes, LargeParams &p, LargeGrids &g) {
    if (rp.objs != nullptr) return hipErrorInvalidValue;
    if (rank_state_check(rp.k, rp.m, rp.n_obj, ws, ws_bytes) != hipSuccess) return hipErrorInvalidValue;
    const LargeLayout L = large_layout(rp.k, rp.m);
    g.step_lds = kLargeStepFixedBytes + size_t(L.B) * size_t(L.D) * 4;
    if (g.step_lds > kRrefMaxLds) return hipErrorInvalidValue;
    p = LargeParams{};
    p.pieces = rp.pieces;
    p.obj_stride = rp.obj_stride;
    p.piece_stride = rp.piece_stride;
    p.T = rp.T;
    p.T_obj = rp.T_obj;
    p.status = rp.status;
    p.rank = rp.rank;
    p.ws = static_cast<uint32_t *>(const_cast<void *>(ws));
    p.ws_obj = int64_t(L.total);
    p.k = rp.k;
    p.m = rp.m;
    p.chunks = (L.D + kColChunk - 1) / kColChunk;
    p.row_chunks = (rp.k + kUpdRows - 1) / kUpdRows;
    p.fin_chunks = (rp.k + kFinRows - 1) / kFinRows;
    const int64_t nobj = rp.n_obj;
    const int64_t g_reduce = nobj * p.chunks, g_update = g_reduce * p.row_chunks, g_final = nobj * p.fin_chunks;
    if (g_update > 0x7FFFFFFF || g_final > 0x7FFFFFFF) return hipErrorInvalidValue;
    g.reduce = unsigned(g_reduce);
    g.step = unsigned(nobj);
    g.update = unsigned(g_update);
    g.fin = unsigned(g_final);
    return step_attr();
}

}  // namespace

hipError_t launch_rank_large(const RrefParams &rp, void *ws, size_t ws_bytes, hipStream_t s) {
    if (rp.n_obj <= 0) return hipSuccess;
    LargeParams p;
    LargeGrids g;
    hipError_t e = large_setup(rp, ws, ws_bytes, p, g);
    if (e != hipSuccess) return e;
    const int B = large_block(rp.k, rp.m);
    for (int t0 = 0; t0 < rp.m; t0 += B) {
        p.t0 = t0;
        p.b = rp.m - t0 < B ? rp.m - t0 : B;
        hipLaunchKernelGGL(gf_rank_large_reduce<false>, dim3(g.reduce), dim3(256), 0, s, p);
        hipLaunchKernelGGL(gf_rank_large_step<false>, dim3(g.step), dim3(256), g.step_lds, s, p);
        hipLaunchKernelGGL(gf_rank_large_update, dim3(g.update), dim3(256), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gf_rank_large_final<false>, dim3(g.fin), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rank_stream_init(int k, int m, int n_obj, void *state, size_t state_bytes, hipStream_t s) {
    if (n_obj <= 0) return hipSuccess;
    RrefParams rp{};
    rp.k = k;
    rp.m = m;
    rp.n_obj = n_obj;
    LargeParams p;
    LargeGrids g;
    hipError_t e = large_setup(rp, state, state_bytes, p, g);  // the grids of every later launch fit
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_rank_stream_init, dim3((unsigned(n_obj) + 255) / 256), dim3(256), 0, s, p.ws, p.ws_obj, n_obj);
    return hipGetLastError();
}

hipError_t launch_rank_stream_push(const RrefParams &rp, void *state, size_t state_bytes, const int32_t *avail,
                                   int max_new, int32_t *rank, int32_t *answered, hipStream_t s) {
    if (rp.n_obj <= 0 || max_new <= 0) return hipSuccess;
    if (avail == nullptr || rp.pieces == nullptr) return hipErrorInvalidValue;
    LargeParams p;
    LargeGrids g;
    hipError_t e = large_setup(rp, state, state_bytes, p, g);
    if (e != hipSuccess) return e;
    const int B = large_block(rp.k, rp.m);
    const int most = max_new < rp.m ? max_new : rp.m;
    const dim3 per_obj((unsigned(rp.n_obj) + 255) / 256);
    hipLaunchKernelGGL(gf_rank_stream_latch, per_obj, dim3(256), 0, s, p.ws, p.ws_obj, rp.n_obj, avail, rp.m, most);
    for (int t = 0; t < most; t += B) {  // every block: each object's own next pieces, from its state
        hipLaunchKernelGGL(gf_rank_large_reduce<true>, dim3(g.reduce), dim3(256), 0, s, p);
        hipLaunchKernelGGL(gf_rank_large_step<true>, dim3(g.step), dim3(256), g.step_lds, s, p);
        hipLaunchKernelGGL(gf_rank_large_update, dim3(g.update), dim3(256), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (rank != nullptr || answered != nullptr)
        hipLaunchKernelGGL(gf_rank_stream_progress, per_obj, dim3(256), 0, s, p.ws, p.ws_obj, rp.n_obj, rank, answered);
    return hipGetLastError();
}

hipError_t launch_rank_stream_snapshot(const RrefParams &rp, const void *state, size_t state_bytes, hipStream_t s) {
    if (rp.n_obj <= 0 || (rp.T == nullptr && rp.status == nullptr && rp.rank == nullptr)) return hipSuccess;
    LargeParams p;
    LargeGrids g;
    hipError_t e = large_setup(rp, state, state_bytes, p, g);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_rank_large_final<true>, dim3(g.fin), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace rlnc
