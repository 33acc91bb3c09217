// piece_call.hpp — the call-latency path of the object API (piece_call.cpp, kernel in piece.hip; internal to
// librlnc_hip): one synchronous product whose output rows land in the caller's host buffer.
#pragma once
#include <cstddef>
#include <cstdint>

#include "context.hpp"

namespace rlnc::eng {

// Encoder::code_with_buf / Recoder::recode_with_buf / Decoder::get_decoded_data take the path up to this much output (a
// pooled workspace keeps a coherent pinned output buffer as large as the largest piece it produced), the decoder up to
// this many multiply-adds too (the kernel reads every source chunk once per output row, so larger products go to the
// batch kernels instead; its 16-byte write-through stores across PCIe run at ~10 GB/s, so outputs of many MiB come
// back faster as one DMA: 16 MiB objects 0.63 ms that way against 0.92 through the kernel, 1 MiB objects 0.11 ms
// against 0.22 -- profiles/r04_object_api_bench_full_v1)
constexpr size_t kPieceMaxBytes = size_t(4) << 20;
constexpr size_t kPieceDecodeMaxMacs = size_t(1) << 31;

// rows of `width` bytes at a 16-byte-aligned stride with room for the last slot's whole 16 bytes
inline bool piece_eligible(const uint8_t *in, size_t in_row, size_t width) {
    return (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (in_row & 15) == 0 && in_row >= round16(width);
}

// out rows r < n_out: dst[r·dst_row + 0 : width) = XOR_j coef[r·coef_row + j] · in[j·in_row + 0 : width), j < n_in.
// coef: host memory; one row of at most kPieceInline bytes travels in the kernel arguments, more are read by the kernel
// from ws->pc_coef (coef may already point there).  Synchronous: returns once dst holds every row.
int piece_call(CallWs *ws, const uint8_t *in, size_t in_row, size_t n_in, size_t width, const uint8_t *coef,
               size_t coef_row, size_t n_out, uint8_t *dst, size_t dst_row);

}  // namespace rlnc::eng
