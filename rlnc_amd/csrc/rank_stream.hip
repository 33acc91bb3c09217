// rank_stream.hip — the LDS form of a decode stream's push (include/rlnc_hip.h, "Decode streams"; interface:
// rank_stream_kernels.hpp; the state buffer, its words and their protocol: rank_state.hpp; the workspace form:
// rank_large.hip).
//
// One launch per push.  Per object the kernel reads done, rank and avail[o] once, each through readfirstlane, and takes
// the target by rank_state.hpp's rule, b = target - done new slots:
//   b <= 0     the object is idle (the workgroup form returns before any barrier, the wave form after the one table
//              barrier);
//   rank = k   the slots done .. target - 1 are answered ReceivedAllPieces and done moves up, as in the workspace step;
//   otherwise  piv[0 .. rank) and R[0 .. rank)[D] come into LDS (the state's rows have rank.hip's layout, [c | e] of
//              D dwords in arrival order), the headers of the b new slots are staged (bytes past k zero), and rank.hip's
//              per-piece loop (reduce, pivot, insert) runs over them with unit(t) at the slot's own index t.  Rank k
//              inside the push: ReceivedAllPieces for the rest of it.  Then St[done .. target) goes back, piv[0 .. rank')
//              and R[0 .. rank')[D] too when a row was inserted (an insert rewrites the older rows), last the words.
// Q, X, the rows and pivots at or beyond rank' and the statuses at or beyond target are never touched.  rank / answered
// (when given) are written for every object.  avail[o] is read exactly once, here, so no latch launch is needed: the
// caller may rewrite avail once the call returned, and a captured push reads it anew at every replay.
//
// The LDS region of an object is rank.hip's (rank_lds_bytes): it holds m staged headers and m statuses, of which a push
// uses its b first.  TPO = threads per object, 256 (a workgroup per object) or 64 (a wave per object, four objects per
// workgroup over one table copy), as in rank.hip.  Rules kept: every branch around a barrier is uniform over the
// object's threads, on values read after the previous barrier and passed through readfirstlane (the state words:
// rank_state.hpp); no workgroup waits for another; plain vector loads and stores only.  The per-piece loop is a copy
// of rank.hip's.  Factored into one shared inline function it compiled the one-shot kernels to the same instructions,
// but with commuted operands, two registers renamed and one address computation moved; rank.hip stays as it is, so
// that its kernels keep their code to the byte.
#include "../../include/rlnc_hip.h"
#include "gf_perm.hpp"
#include "rref.hpp"
#include "rank_stream_kernels.hpp"

namespace rlnc {

namespace {

struct StreamLdsParams {
    const uint8_t *pieces;
    int64_t obj_stride, piece_stride;
    uint32_t *ws;
    int64_t ws_obj;  // dwords
    const int32_t *avail;
    int32_t *rank, *answered;  // each optional
    int k, m, n_obj, max_new;
    int off_piv, off_st, off_r;  // large_layout(k, m), dwords from the object's state words
    int D;                       // dwords of a row
    int obj_dw;                  // dwords of one object's LDS region
};

template <int TPO>
__global__ __launch_bounds__(256) void gf_rank_stream_push(StreamLdsParams p) {
    extern __shared__ uint32_t lds[];
    constexpr bool WG = TPO == 256;
    uint32_t *tab = lds;
    const int tid = int(threadIdx.x) % TPO;
    const int lane = lane_id();
    const int o = int(blockIdx.x) * (256 / TPO) + int(threadIdx.x) / TPO;
    const bool valid = o < p.n_obj;
    const int k = p.k, m = p.m;
    const int kd = (k + 3) >> 2, D = p.D;
    uint32_t *ws = p.ws + int64_t(valid ? o : 0) * p.ws_obj;
    int32_t *gpiv = reinterpret_cast<int32_t *>(ws + p.off_piv);
    int32_t *gSt = reinterpret_cast<int32_t *>(ws + p.off_st);
    uint32_t *R = ws + p.off_r;

    // the state, once; the push target rule of rank_state.hpp, written out (a rank below 0 leaves the object idle too)
    int done = 0, rank0 = 0, b = 0;
    if (valid) {
        done = __builtin_amdgcn_readfirstlane(int(ws[kStDone]));
        rank0 = __builtin_amdgcn_readfirstlane(int(ws[kStRank]));
        const int av = __builtin_amdgcn_readfirstlane(p.avail[o]);
        if (done >= 0 && done < m && rank0 >= 0) b = min(min(max(av, done), m), done + p.max_new) - done;
    }
    const int target = done + b;
    auto progress = [&](int rank) {
        if (p.rank != nullptr) p.rank[o] = rank;
        if (p.answered != nullptr) p.answered[o] = target;
    };
    // an object at rank k: its slots are consumed all the same (the snapshot tells them from pending ones)
    auto answer_full = [&]() {
        for (int t = tid; t < b; t += TPO) gSt[done + t] = RLNC_ERR_RECEIVED_ALL_PIECES;
        if (tid == 0) {
            store_state(ws, rank0, target);
            progress(rank0);
        }
    };
    if constexpr (WG) {
        if (b <= 0) {  // before any barrier
            if (tid == 0) progress(rank0);
            return;
        }
        if (rank0 >= k) {
            __syncthreads();  // every wave has read the state that thread 0 rewrites
            answer_full();
            return;
        }
    }

    uint32_t *rows = lds + kMulTabDw + size_t(int(threadIdx.x) / TPO) * size_t(p.obj_dw);
    uint8_t *rowsB = reinterpret_cast<uint8_t *>(rows);
    uint32_t *vb = rows + k * D;  // two scratch rows, alternating by piece
    uint32_t *Hw = vb + 2 * D;    // the staged headers of the new slots, kd dwords each (room for m)
    const uint8_t *HB = reinterpret_cast<const uint8_t *>(Hw);
    int32_t *St = reinterpret_cast<int32_t *>(Hw + m * kd);  // the new slots' statuses (room for m)
    int32_t *piv = St + m;
    uint8_t *qb = reinterpret_cast<uint8_t *>(piv + 2 * k);  // after rank.hip's order array, which a push does not need

    copy_table(tab);
    if (valid && b > 0 && rank0 < k) {
        {  // the stored rows, 16 bytes a lane and four loads in flight (both sides start on 16 bytes)
            const int nR = rank0 * D, n4 = nR >> 2;
            const uint4 *src = reinterpret_cast<const uint4 *>(R);
            uint4 *dst = reinterpret_cast<uint4 *>(rows);
            for (int i0 = tid; i0 < n4; i0 += 4 * TPO) {
                uint4 x4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x4[u] = i0 + TPO * u < n4 ? src[i0 + TPO * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + TPO * u < n4) dst[i0 + TPO * u] = x4[u];
            }
            for (int i = 4 * n4 + tid; i < nR; i += TPO) rows[i] = R[i];
            for (int t = tid; t < rank0; t += TPO) piv[t] = gpiv[t];
        }
        // the headers of slots done .. target - 1, 8 independent byte loads in flight per batch
        const uint8_t *base = p.pieces + int64_t(o) * p.obj_stride + int64_t(done) * p.piece_stride;
        uint8_t *hdst = reinterpret_cast<uint8_t *>(Hw);
        const int kb = 4 * kd, tot = b * kb;
        for (int e0 = 0; e0 < tot; e0 += TPO * 8) {
            uint8_t hb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + tid + TPO * u;
                const int s = e / kb, c = e - s * kb;
                hb[u] = (e < tot && c < k) ? base[int64_t(s) * p.piece_stride + c] : uint8_t(0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e0 + tid + TPO * u < tot) hdst[e0 + tid + TPO * u] = hb[u];
        }
    }
    __syncthreads();
    if constexpr (!WG) {  // whole waves, after the one workgroup barrier of this form
        if (!valid) return;
        if (b <= 0) {
            if (tid == 0) progress(rank0);
            return;
        }
        if (rank0 >= k) {
            answer_full();
            return;
        }
    }

    // the insert step's thread layout: lpr lanes per row (a power of two), rpp rows per pass
    int lpr = 1, sh = 0;
    while (lpr < D && lpr < TPO) {
        lpr <<= 1;
        ++sh;
    }
    const int sub = tid & (lpr - 1), rgrp = tid >> sh, rpp = TPO >> sh;

    // rank.hip's per-piece loop over the slots s = 0 .. b - 1 of the push, piece pi = done + s
    int rank = rank0, par = 0, s = 0;
    for (; s < b; ++s) {
        if (rank == k) break;
        const int pi = done + s;
        uint32_t *v = vb + par * D;
        const uint8_t *hb = HB + s * 4 * kd;
        // reduce
        for (int d0 = 0; d0 < D; d0 += TPO) {
            const int d = d0 + tid;
            const bool act = d < D;
            uint32_t acc = 0;
            if (act) acc = d < kd ? Hw[s * kd + d] : ((d - kd) == (pi >> 2) ? 1u << (8 * (pi & 3)) : 0u);
            // a wave with no dword of this chunk (rows narrower than the workgroup) skips the products
            const int nrows = ballot(act) != 0 ? rank : 0;
            for (int b0 = 0; b0 < nrows; b0 += 64) {
                const int i = b0 + lane;
                const uint32_t qv = i < rank ? uint32_t(hb[piv[i]]) : 0u;
                uint64_t mk = ballot(qv != 0);
                while (mk) {
                    const int j = __builtin_ctzll(mk);
                    mk &= mk - 1;
                    const uint32_t q = uint32_t(__builtin_amdgcn_readlane(int(qv), j));
                    const uint32_t x = act ? rows[(b0 + j) * D + d] : 0u;
                    acc ^= mul4(tab, q, x);
                }
            }
            if (act) v[d] = acc;
        }
        rsync<WG>();
        // pivot
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
            if (tid == 0) St[s] = RLNC_ERR_PIECE_NOT_USEFUL;
            par ^= 1;
            continue;
        }
        // insert
        const uint32_t inv = gfinv(tab, val);
        for (int t = tid; t < rank; t += TPO) qb[t] = rowsB[t * 4 * D + pc];
        if (tid == 0) {
            piv[rank] = pc;
            St[s] = RLNC_OK;
        }
        uint32_t *nr = rows + rank * D;
        for (int d = tid; d < D; d += TPO) nr[d] = mul4(tab, inv, v[d]);
        rsync<WG>();
        for (int r = rgrp; r < rank; r += rpp) {
            const uint32_t q = qb[r];
            if (q != 0u)
                for (int d = sub; d < D; d += lpr) rows[r * D + d] ^= mul4(tab, q, nr[d]);
        }
        ++rank;
        par ^= 1;
        rsync<WG>();
    }
    for (int t = s + tid; t < b; t += TPO) St[t] = RLNC_ERR_RECEIVED_ALL_PIECES;
    rsync<WG>();

    // back to the state: the new statuses; the pivots and all the rows when one was inserted; the state words last
    for (int t = tid; t < b; t += TPO) gSt[done + t] = St[t];
    if (rank > rank0) {
        for (int t = tid; t < rank; t += TPO) gpiv[t] = piv[t];
        const int nR = rank * D, n4 = nR >> 2;
        const uint4 *src = reinterpret_cast<const uint4 *>(rows);
        uint4 *dst = reinterpret_cast<uint4 *>(R);
        for (int i = tid; i < n4; i += TPO) dst[i] = src[i];
        for (int i = 4 * n4 + tid; i < nR; i += TPO) R[i] = rows[i];
    }
    if (tid == 0) {
        store_state(ws, rank, target);
        progress(rank);
    }
}

// the 160 KiB dynamic-LDS attribute of the workgroup form, once per device
hipError_t stream_attr() {
    static MaxLdsAttr attr;
    return attr.set(&gf_rank_stream_push<256>);
}

}  // namespace

bool rank_stream_lds_fits(size_t k, size_t m) {
    // beyond these the formula is far above the limit (k·D alone), and its int arguments would not hold the shape
    if (k == 0 || m == 0 || k > (size_t(1) << 20) || m > (size_t(1) << 20)) return false;
    return rank_lds_bytes(int(k), int(m)) <= kRrefMaxLds;
}

hipError_t launch_rank_stream_push_lds(const RrefParams &rp, void *state, size_t state_bytes, const int32_t *avail,
                                       int max_new, int32_t *rank, int32_t *answered, hipStream_t s) {
    if (rp.n_obj <= 0 || max_new <= 0) return hipSuccess;
    if (avail == nullptr || rp.pieces == nullptr || rp.objs != nullptr) return hipErrorInvalidValue;
    if (rank_state_check(rp.k, rp.m, rp.n_obj, state, state_bytes) != hipSuccess ||
        !rank_stream_lds_fits(size_t(rp.k), size_t(rp.m)))
        return hipErrorInvalidValue;
    const LargeLayout L = large_layout(rp.k, rp.m);
    const size_t lds = rank_lds_bytes(rp.k, rp.m);
    StreamLdsParams p{};
    p.pieces = rp.pieces;
    p.obj_stride = rp.obj_stride;
    p.piece_stride = rp.piece_stride;
    p.ws = static_cast<uint32_t *>(state);
    p.ws_obj = int64_t(L.total);
    p.avail = avail;
    p.rank = rank;
    p.answered = answered;
    p.k = rp.k;
    p.m = rp.m;
    p.n_obj = rp.n_obj;
    p.max_new = max_new < rp.m ? max_new : rp.m;
    p.off_piv = int(L.piv);
    p.off_st = int(L.st);
    p.off_r = int(L.r);
    p.D = L.D;
    p.obj_dw = int((lds - size_t(kMulTabDw) * 4) / 4);
    // many small objects: a workgroup per object leaves most of its lanes idle and the grid launch-bound
    if (rp.k <= 16 && L.D <= 16 && rp.n_obj >= 1024) {
        const size_t lds4 = size_t(kMulTabDw) * 4 + 4 * size_t(p.obj_dw) * 4;  // < 20 KiB
        hipLaunchKernelGGL(gf_rank_stream_push<64>, dim3((unsigned(rp.n_obj) + 3) / 4), dim3(256), lds4, s, p);
        return hipGetLastError();
    }
    const hipError_t e = stream_attr();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_rank_stream_push<256>, dim3(unsigned(rp.n_obj)), dim3(256), lds, s, p);
    return hipGetLastError();
}

}  // namespace rlnc
