// rref.hpp — launch interface of the device elimination (rref.hip; internal to librlnc_hip).  The true-rank
// eliminations (rank_kernels.hpp, rank_large_kernels.hpp) take the same parameters.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

namespace rlnc {

// Device replica of Decoder::decode over pieces 0..m-1 of every object (rref.hip).  Piece p of object o
// starts (coefficient header first) at pieces + o*obj_stride + p*piece_stride.  Outputs: status[o][p]
// (RLNC status of each decode() call), rank[o], T[o] (k × m, row-major, rows >= rank zero).
struct RrefParams {
    const uint8_t *pieces;
    int64_t obj_stride, piece_stride;
    int k, m, n_obj;
    uint8_t *T;
    int64_t T_obj;
    int32_t *status;
    int32_t *rank;
    int block_only;  // 1 = decode path 5: the blocked run (gf_rref_block_kernel), never the small-object kernel or the
                     // two-pass split; 0 = chosen by shape (launch_rref_one)
    const struct RrefObj *objs = nullptr;  // ragged batch: object o's shape and buffers (the fields above unused)
    // two-pass elimination when k + m > 256 (k <= 128): pass 1 (the blocked run) replays only the first m pieces of
    // each object with statuses / T at row stride m_stride (> m): an object full-ranked within them is exact
    // (decode() answers ReceivedAllPieces for every later piece and leaves the state alone, decoder.rs:97-99); pass 2
    // (the general kernel over all pieces) skips the objects pass 1 full-ranked (skip_full) and redoes the others
    int m_stride = 0;   // 0 = m
    int skip_full = 0;
    // optional (the small-object kernel only): also write T as the 1- / 2-wave bit-sliced program's block-offset
    // stream -- bsj_stream[o][j][i] = T[i][j] · bsj_block_bytes for i < bsj_tile_rows (0 past k) -- so the T × data
    // product needs no offset launch (MatmulParams::bsj_stream); launch_rref_batch reports whether it did
    uint32_t *bsj_stream = nullptr;
    uint32_t bsj_block_bytes = 0;
    int bsj_tile_rows = 0;
    // optional, with bsj_stream (same kernel): get_final_data_len (decoder.rs:162-177) decided from the last 64
    // payload bytes -- decoded row k - 1's last 64 bytes computed from T and the pieces' tails (tail_L = L, a multiple
    // of 4, >= 64; k and the object stride multiples of 4): tail_status / tail_len the object's status and final length when its last
    // nonzero byte lies there (or rank < k), else tail_need[o] = 1 (the product's workgroup scans the whole payload,
    // MatmulParams::scan_need)
    int32_t *tail_status = nullptr;
    int64_t *tail_len = nullptr;
    int32_t *tail_need = nullptr;
    int64_t tail_L = 0;
};
// One object of a ragged elimination launch (rlnc_decode_ragged): T is k x m row-major, status m entries.
struct RrefObj {
    const uint8_t *pieces;
    int64_t piece_stride;
    uint8_t *T;
    int32_t *status;
    int32_t *rank;
    int32_t k, m;      // m = received pieces (the row stride of T and of the statuses)
    int32_t m_first;   // > 0: the blocked pass replays only the first m_first pieces (see RrefParams::m_stride)
    int32_t two_pass;  // the general pass skips this object when the blocked pass full-ranked it
};
// ragged elimination: one workgroup per object of the device table objs (n objects, k + m <= 256 each when
// block = true -- the blocked clean run -- else the one-wave LDS kernel); lds = the largest object's need
hipError_t launch_rref_ragged(const RrefObj *objs, int n, bool block, size_t lds, int hdr_lds, hipStream_t s);
constexpr size_t kRrefMaxLds = 160 * 1024;
// hipFuncAttributeMaxDynamicSharedMemorySize = kRrefMaxLds for a call site's kernels, set once per device (function
// attributes are per device) under a lock: one static instance per call site, set() before the launch
struct MaxLdsAttr {
    std::mutex mu;
    bool done[64] = {};
    template <class... Kernels>
    hipError_t set(Kernels... kernels) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lock(mu);
        if (done[dev]) return hipSuccess;
        for (const void *f : {reinterpret_cast<const void *>(kernels)...}) {
            e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, int(kRrefMaxLds));
            if (e != hipSuccess) return e;
        }
        done[dev] = true;
        return hipSuccess;
    }
};
// dynamic LDS of the one-wave kernel, of the same with the piece headers staged in LDS, and of the blocked run
size_t rref_lds_bytes(int k, int m);
size_t rref_lds_bytes_staged(int k, int m);
size_t rref_block_lds_bytes(int k, int m);
// the blocked clean-run kernel (decode path 5, and what 0 / 2 pick) applies: a row fits one wave (k + m <= 256)
bool rref_block_eligible(int k, int m);
hipError_t launch_rref_batch(const RrefParams &p, hipStream_t s, bool *bsj_written = nullptr);

}  // namespace rlnc
