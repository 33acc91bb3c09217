// rank.hip — the true-rank elimination on the device (RLNC_RANK_MODE_TRUE; see rank_kernels.hpp and the "Rank mode"
// block of include/rlnc_hip.h for the semantics).
//
// Per object the kernel keeps the useful pieces' rows [c | e] in LDS in arrival order, each with its pivot column, the
// coefficient parts always in reduced row-echelon form.  A row is kd = ceil(k/4) coefficient dwords followed by
// ceil(m/4) dwords of e (one byte per received piece).  Pushing piece p:
//   reduce   v = [h | unit(p)] ^ XOR_i h[piv_i] · row_i.  Thread t owns dwords t, t + TPO, ... of v; the quotients are
//            bytes of the staged header h itself (the RREF invariant), fetched 64 rows at a time, and only the nonzero
//            ones (a ballot) cost a product -- sparse coding vectors make this loop short.
//   pivot    every wave scans v's coefficient dwords with a ballot: all zero = PieceNotUseful, else the first nonzero
//            byte is the pivot column pc.
//   insert   the new row is v / v[pc]; the quotients row_i[pc] are snapshotted first, then the rows are updated
//            row_i ^= row_i[pc] · new, (row, dword) pairs spread over all the threads.
// T is written at the end, rows in pivot order (the permutation is counted from the pivot array).
//
// TPO = threads per object: 256 (one workgroup per object, workgroup barriers) or 64 (one wave per object, four
// objects per workgroup over one table copy; a wave's LDS operations execute in issue order, so a fence suffices).
// Every branch around a barrier depends on values all the threads of the object read from LDS after the previous
// barrier (rank, pc), taken through readfirstlane.
#include "../../include/rlnc_hip.h"
#include "gf_perm.hpp"
#include "rref.hpp"
#include "rank_kernels.hpp"

namespace rlnc {

namespace {

__host__ __device__ inline int rank_row_dwords(int k, int m) { return ((k + 3) >> 2) + ((m + 3) >> 2); }
// dwords of one object's LDS region (rank_kernels.hpp), a multiple of 4
__host__ __device__ inline size_t rank_obj_dwords(int k, int m) {
    const size_t kd = size_t((k + 3) >> 2), D = size_t(rank_row_dwords(k, m));
    const size_t n = size_t(k) * D + 2 * D + size_t(m) * kd + size_t(m) + 2 * size_t(k) + kd;
    return (n + 3) & ~size_t(3);
}

template <int TPO>
__global__ __launch_bounds__(256) void gf_true_rank_kernel(RrefParams p) {
    extern __shared__ uint32_t lds[];
    constexpr bool WG = TPO == 256;
    uint32_t *tab = lds;
    const int tid = int(threadIdx.x) % TPO;
    const int lane = lane_id();
    int o = int(blockIdx.x) * (256 / TPO) + int(threadIdx.x) / TPO;
    const bool valid = o < p.n_obj;
    if (p.objs != nullptr) {  // ragged batch: this workgroup's object, as object 0 of a one-object batch
        const RrefObj &d = p.objs[o];
        p.pieces = d.pieces;
        p.obj_stride = 0;
        p.piece_stride = d.piece_stride;
        p.k = __builtin_amdgcn_readfirstlane(d.k);
        p.m = __builtin_amdgcn_readfirstlane(d.m);
        p.T = d.T;
        p.T_obj = 0;
        p.status = d.status;
        p.rank = d.rank;
        o = 0;
    }
    const int k = p.k, m = p.m;
    const int kd = (k + 3) >> 2, D = rank_row_dwords(k, m);
    uint32_t *rows = lds + kMulTabDw + size_t(int(threadIdx.x) / TPO) * rank_obj_dwords(k, m);
    uint8_t *rowsB = reinterpret_cast<uint8_t *>(rows);
    uint32_t *vb = rows + k * D;  // two scratch rows, alternating by piece
    uint32_t *Hw = vb + 2 * D;    // m headers of kd dwords (bytes past k zero)
    const uint8_t *HB = reinterpret_cast<const uint8_t *>(Hw);
    int32_t *St = reinterpret_cast<int32_t *>(Hw + m * kd);
    int32_t *piv = St + m;
    int32_t *ord = piv + k;
    uint8_t *qb = reinterpret_cast<uint8_t *>(ord + k);

    copy_table(tab);
    if (valid) {  // all m headers, 8 independent byte loads in flight per batch
        const uint8_t *base = p.pieces + int64_t(o) * p.obj_stride;
        uint8_t *hdst = reinterpret_cast<uint8_t *>(Hw);
        const int kb = 4 * kd, tot = m * kb;
        for (int e0 = 0; e0 < tot; e0 += TPO * 8) {
            uint8_t hb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + tid + TPO * u;
                const int pi = e / kb, c = e - pi * kb;
                hb[u] = (e < tot && c < k) ? base[int64_t(pi) * p.piece_stride + c] : uint8_t(0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e0 + tid + TPO * u < tot) hdst[e0 + tid + TPO * u] = hb[u];
        }
    }
    __syncthreads();
    if (!valid) return;  // TPO = 64 only (whole waves past the last object); no workgroup barrier follows there

    // the insert step's thread layout: lpr lanes per row (a power of two), rpp rows per pass
    int lpr = 1, sh = 0;
    while (lpr < D && lpr < TPO) {
        lpr <<= 1;
        ++sh;
    }
    const int sub = tid & (lpr - 1), rgrp = tid >> sh, rpp = TPO >> sh;

    int rank = 0, par = 0, pi = 0;
    for (; pi < m; ++pi) {
        if (rank == k) break;
        uint32_t *v = vb + par * D;
        const uint8_t *hb = HB + pi * 4 * kd;
        // reduce
        for (int d0 = 0; d0 < D; d0 += TPO) {
            const int d = d0 + tid;
            const bool act = d < D;
            uint32_t acc = 0;
            if (act) acc = d < kd ? Hw[pi * kd + d] : ((d - kd) == (pi >> 2) ? 1u << (8 * (pi & 3)) : 0u);
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
                const int b = __builtin_ctz(word) >> 3;
                pc = (b0 + j) * 4 + b;
                val = (word >> (8 * b)) & 0xFFu;
                break;
            }
        }
        pc = __builtin_amdgcn_readfirstlane(pc);
        val = uni(val);
        if (pc < 0) {
            if (tid == 0) St[pi] = RLNC_ERR_PIECE_NOT_USEFUL;
            par ^= 1;
            continue;
        }
        // insert
        const uint32_t inv = gfinv(tab, val);
        for (int t = tid; t < rank; t += TPO) qb[t] = rowsB[t * 4 * D + pc];
        if (tid == 0) {
            piv[rank] = pc;
            St[pi] = RLNC_OK;
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
    for (int t = pi + tid; t < m; t += TPO) St[t] = RLNC_ERR_RECEIVED_ALL_PIECES;
    // stored row t goes to T row (number of smaller pivots)
    for (int t = tid; t < rank; t += TPO) {
        const int pv = piv[t];
        int pos = 0;
        for (int j = 0; j < rank; ++j) pos += piv[j] < pv ? 1 : 0;
        ord[pos] = t;
    }
    rsync<WG>();
    uint8_t *T = p.T + int64_t(o) * p.T_obj;
    if ((m & 3) == 0 && (reinterpret_cast<uintptr_t>(T) & 3) == 0) {
        const int mw = m >> 2;
        uint32_t *Tw = reinterpret_cast<uint32_t *>(T);
        for (int idx = tid; idx < k * mw; idx += TPO) {
            const int r = idx / mw, c = idx - r * mw;
            Tw[idx] = r < rank ? rows[ord[r] * D + kd + c] : 0u;
        }
    } else {
        const uint8_t *E = rowsB + 4 * kd;
        for (int idx = tid; idx < k * m; idx += TPO) {
            const int r = idx / m, c = idx - r * m;
            T[idx] = r < rank ? E[ord[r] * 4 * D + c] : uint8_t(0);
        }
    }
    for (int t = tid; t < m; t += TPO) p.status[int64_t(o) * m + t] = St[t];
    if (tid == 0) p.rank[o] = rank;
}

// the 160 KiB dynamic-LDS attribute of the workgroup form, once per device
hipError_t rank_attr() {
    static MaxLdsAttr attr;
    return attr.set(&gf_true_rank_kernel<256>);
}

}  // namespace

size_t rank_lds_bytes(int k, int m) { return size_t(kMulTabDw) * 4 + rank_obj_dwords(k, m) * 4; }

hipError_t launch_rank_batch(const RrefParams &p, hipStream_t s) {
    if (p.n_obj <= 0) return hipSuccess;
    if (p.objs != nullptr) return hipErrorInvalidValue;
    const size_t lds = rank_lds_bytes(p.k, p.m);
    if (lds > kRrefMaxLds) return hipErrorInvalidValue;
    // many small objects: a workgroup per object leaves most of its lanes idle and the grid launch-bound
    if (p.k <= 16 && rank_row_dwords(p.k, p.m) <= 16 && p.n_obj >= 1024) {
        const size_t lds4 = size_t(kMulTabDw) * 4 + 4 * rank_obj_dwords(p.k, p.m) * 4;  // < 20 KiB
        hipLaunchKernelGGL(gf_true_rank_kernel<64>, dim3((p.n_obj + 3) / 4), dim3(256), lds4, s, p);
        return hipGetLastError();
    }
    const hipError_t e = rank_attr();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_true_rank_kernel<256>, dim3(p.n_obj), dim3(256), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_rank_ragged(const RrefObj *objs, int n, size_t lds, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (lds > kRrefMaxLds) return hipErrorInvalidValue;
    const hipError_t e = rank_attr();
    if (e != hipSuccess) return e;
    RrefParams p{};
    p.objs = objs;
    p.n_obj = n;
    hipLaunchKernelGGL(gf_true_rank_kernel<256>, dim3(n), dim3(256), lds, s, p);
    return hipGetLastError();
}

}  // namespace rlnc
