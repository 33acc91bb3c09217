// elementwise.hip — the element-wise vector primitives, the strided row copy and the decoder's marker scan (launch
// interface: kernels.hpp; internal to librlnc_hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/rlnc_hip.h"
#include "gf256.hpp"
#include "kernels.hpp"
#include "kernels_common.hpp"

namespace rlnc {

namespace {

// strided row copy (the coded pieces' coefficient headers, encoder.rs:246-248): one byte per thread
__global__ __launch_bounds__(256) void copy_rows_kernel(uint8_t *dst, int64_t dst_stride, const uint8_t *src,
                                                        int64_t src_stride, int64_t width, int64_t total) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t r = e / width, c = e % width;
    dst[r * dst_stride + c] = src[r * src_stride + c];
}

// ---------------------------------------------------------------------------------------------------
// element-wise primitives (simd/mod.rs:18-119); the scalar early-outs are taken on the host
// ---------------------------------------------------------------------------------------------------
template <int OP, bool ALIGNED>  // OP 0: v = c·v   1: d ^= s   2: d ^= c·s
__global__ __launch_bounds__(kThreads) void gf_vec_kernel(uint8_t *dst, const uint8_t *src, int64_t len, uint32_t t0lo,
                                                          uint32_t t0hi, uint32_t t1lo, uint32_t t1hi, uint32_t t2) {
    const int64_t stride = int64_t(gridDim.x) * kThreads * kBytesPerThread;
    for (int64_t off = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * kBytesPerThread; off < len; off += stride) {
        const int nb = int(min<int64_t>(kBytesPerThread, len - off));
        const uint4 x = load16<ALIGNED>((OP == 0 ? dst : src) + off, nb);
        uint4 r;
        if (OP == 1) {
            r = x;
        } else {
            const Sel s = selectors(x);
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = xor3(vperm(t0hi, t0lo, s.s0[q]), vperm(t1hi, t1lo, s.s1[q]), vperm(t2, t2, s.s2[q]));
            r = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (OP != 0) {
            const uint4 d = load16<ALIGNED>(dst + off, nb);
            r = make_uint4(r.x ^ d.x, r.y ^ d.y, r.z ^ d.z, r.w ^ d.w);
        }
        store16<ALIGNED>(dst + off, r, nb);
    }
}

template <int OP>
hipError_t launch_vec(uint8_t *dst, const uint8_t *src, int64_t len, uint8_t c, hipStream_t s) {
    if (len <= 0) return hipSuccess;
    const PermTable t = make_perm_table(c);
    const int64_t chunks = (len + kBytesPerThread - 1) / kBytesPerThread;
    const int blocks = int(std::min<int64_t>((chunks + kThreads - 1) / kThreads, 2048));
    const bool aligned = unaligned_vector_ok() || (al16(dst) && (OP == 0 || al16(src)));
    const auto kern = aligned ? &gf_vec_kernel<OP, true> : &gf_vec_kernel<OP, false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kThreads), 0, s, dst, src, len, t.t0lo, t.t0hi, t.t1lo, t.t1hi, t.t2);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// get_final_data_len on device (decoder.rs:162-177).  Equivalent formulation: the last nonzero byte of
// the padded payload must be the boundary marker and must not sit at index 0.
// ---------------------------------------------------------------------------------------------------
// 16 lanes per object (one DPP row, 64 B a lane) scan 1 KiB chunks from the END of the payload: for any padded object the last
// nonzero byte lies in the final k bytes (Encoder::new pads with < k zeros after the marker,
// encoder.rs:95-99), so the scan normally stops after one chunk — O(1) instead of a full re-read.  The same wave
// then checks the marker and writes the object's status and length (one launch; the round-3 form wrote the index
// to scratch for a second kernel: 5.5 us more per decode of configs[0]'s 4,096 objects).
// rank != nullptr: objects of rank < k are NotAllPiecesReceivedYet (decoder.rs:137-139); the rank is loaded beside
// the first chunk (their latencies overlap) and decides the outcome; invalid_code: the status of a payload without a
// valid marker.  The row maximum is a DPP ladder (row16_max), not __shfl_xor; 16 objects per workgroup: a quarter of
// the waves of the round-4 one-wave-per-object form.
// max over one 16-lane DPP row of a 32-bit key (every lane of the row ends with it): VALU row rotations only
__device__ __forceinline__ uint32_t row16_max(uint32_t a) {
    a = max(a, uint32_t(__builtin_amdgcn_update_dpp(0, int(a), 0x121, 0xf, 0xf, false)));  // row_ror:1
    a = max(a, uint32_t(__builtin_amdgcn_update_dpp(0, int(a), 0x122, 0xf, 0xf, false)));  // row_ror:2
    a = max(a, uint32_t(__builtin_amdgcn_update_dpp(0, int(a), 0x124, 0xf, 0xf, false)));  // row_ror:4
    a = max(a, uint32_t(__builtin_amdgcn_update_dpp(0, int(a), 0x128, 0xf, 0xf, false)));  // row_ror:8
    return a;
}

constexpr int kScanObjPerWg = 16;  // 16 lanes (one DPP row) per object, 16 objects per 256-thread workgroup

template <bool ALIGNED>
__global__ __launch_bounds__(256) void final_len_scan_kernel(const uint8_t *data, int64_t obj_stride, int64_t len,
                                                             int n_obj, const int32_t *rank, int k, int32_t *status,
                                                             int64_t *final_len, int32_t invalid_code) {
    const int tid = threadIdx.x, l = tid & 15;
    const int obj = blockIdx.x * kScanObjPerWg + (tid >> 4);
    const bool valid = obj < n_obj;
    const int32_t rk = (valid && rank != nullptr) ? rank[obj] : k;
    const uint8_t *d = data + int64_t(valid ? obj : 0) * obj_stride;
    int64_t c = (len + 1023) / 1024 - 1;  // this object's chunk, from the end
    bool done = !valid;
    int64_t hit = -1;  // index of the payload's last nonzero byte
    uint32_t byte = 0;
    for (;;) {
        // (index in the chunk + 1) << 8 | byte of the last nonzero byte of this lane's 64 B, 0 = none: the maximum
        // over the object's 16 lanes is the chunk's last nonzero byte with its value
        uint32_t mine = 0;
        if (!done) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t off = c * 1024 + l * 64 + u * kBytesPerThread;
                if (off < len) {
                    const int nb = int(min<int64_t>(kBytesPerThread, len - off));
                    const uint4 x = load16<ALIGNED>(d + off, nb);
                    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (w[q]) {
                            const int b = (31 - __builtin_clz(w[q])) / 8;
                            mine = (uint32_t(l * 64 + u * kBytesPerThread + 4 * q + b + 1) << 8) |
                                   ((w[q] >> (8 * b)) & 0xFFu);
                        }
                }
            }
        }
        const uint32_t best = row16_max(mine);
        if (!done) {
            if (best) {
                hit = c * 1024 + int64_t(best >> 8) - 1;
                byte = best & 0xFFu;
                done = true;
            } else if (rk < k || c == 0) {
                done = true;  // not decoded (nothing to scan), or an all-zero payload
            } else {
                --c;
            }
        }
        if (__ballot(!done) == 0) break;
    }
    if (valid && l == 0) {
        if (rk < k) {
            status[obj] = RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET;
            final_len[obj] = 0;
        } else {
            const bool ok = hit > 0 && byte == kBoundaryMarker;  // decoder.rs:162-177
            status[obj] = ok ? RLNC_OK : invalid_code;
            final_len[obj] = ok ? hit : 0;
        }
    }
}

// rank = nullptr: every object counts as decoded (k unused)
hipError_t launch_scan(const uint8_t *data, int64_t obj_stride, int64_t len, int n_obj, const int32_t *rank, int k,
                       int32_t *status, int64_t *final_len, int32_t invalid_code, hipStream_t s) {
    if (n_obj <= 0) return hipSuccess;
    const dim3 grid((n_obj + kScanObjPerWg - 1) / kScanObjPerWg);
    const bool aligned = unaligned_vector_ok() || (al16(data) && (n_obj == 1 || al16(obj_stride)));
    hipLaunchKernelGGL(aligned ? &final_len_scan_kernel<true> : &final_len_scan_kernel<false>, grid, dim3(256), 0, s, data,
                       obj_stride, len, n_obj, rank, k, status, final_len, invalid_code);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_copy_rows(uint8_t *dst, int64_t dst_stride, const uint8_t *src, int64_t src_stride, int64_t width,
                            int64_t rows, hipStream_t s) {
    const int64_t total = width * rows;
    if (total <= 0) return hipSuccess;
    if ((total + 255) / 256 > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, dst, dst_stride, src,
                       src_stride, width, total);
    return hipGetLastError();
}

hipError_t launch_mul_vec_by_scalar(uint8_t *vec, int64_t len, uint8_t scalar, hipStream_t s) {
    return launch_vec<0>(vec, nullptr, len, scalar, s);
}
hipError_t launch_add_vectors(uint8_t *dst, const uint8_t *src, int64_t len, hipStream_t s) {
    return launch_vec<1>(dst, src, len, 1, s);
}
hipError_t launch_mul_add(uint8_t *dst, const uint8_t *src, int64_t len, uint8_t scalar, hipStream_t s) {
    return launch_vec<2>(dst, src, len, scalar, s);
}

hipError_t launch_final_data_len(const uint8_t *data, int64_t obj_stride, int64_t len, int n_obj, int32_t *status,
                                 int64_t *final_len, int32_t invalid_code, hipStream_t s) {
    return launch_scan(data, obj_stride, len, n_obj, nullptr, 0, status, final_len, invalid_code, s);
}

hipError_t launch_final_data_len_ranked(const uint8_t *data, int64_t obj_stride, int64_t len, int n_obj, int k,
                                        const int32_t *rank, int32_t *status, int64_t *final_len, hipStream_t s) {
    return launch_scan(data, obj_stride, len, n_obj, rank, k, status, final_len,
                       int32_t(RLNC_ERR_INVALID_DECODED_DATA_FORMAT), s);
}

}  // namespace rlnc
