// piece_call.cpp — the call-latency path of the object API (piece_call.hpp): launch the kernel of piece.hip and copy
// its output rows from pinned memory into the caller's buffer chunk by chunk, as the device raises their flags.
#include "piece_call.hpp"

#include "piece.hpp"

namespace rlnc::eng {
namespace {

// workgroups per completion flag: 64 KiB of a row, which the host copies while the device writes on
// (profiles/r04_chunk_ab.txt, r06_piece_chunk_ab.txt)
constexpr int kPieceChunkBlocks = 64;

// RLNC_PIECE_TRACE=1: per-phase host time of the piece calls
PhaseTrace g_piece_trace("RLNC_PIECE_TRACE",
                         "{\"piece_trace\": {\"calls\": %zu, \"median_pre_us\": %.2f, \"median_launch_us\": %.2f, "
                         "\"median_to_first_flag_us\": %.2f, \"median_copies_and_rest_us\": %.2f}}\n");

// Spin until the kernel raises *f to epoch.  The stream is queried only once the wait is long (a faulted kernel never
// raises its flag: hipStreamQuery then reports the error).
int piece_wait(const uint32_t *f, uint32_t epoch, hipStream_t s) {
    if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == epoch) return RLNC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 1;; ++i) {
        if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == epoch) return RLNC_OK;
        __builtin_ia32_pause();
        if ((i & 4095) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipErrorNotReady) continue;
            if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == epoch) return RLNC_OK;
            if (q == hipSuccess) return set_error(RLNC_ERR_DEVICE, "piece kernel finished without raising its flag");
            return set_error(RLNC_ERR_DEVICE, "piece kernel: %s", hipGetErrorString(q));
        }
    }
}

}  // namespace

int piece_call(CallWs *ws, const uint8_t *in, size_t in_row, size_t n_in, size_t width, const uint8_t *coef,
               size_t coef_row, size_t n_out, uint8_t *dst, size_t dst_row) {
    const bool tr = g_piece_trace.on;
    const uint64_t t0 = tr ? now_ns() : 0;
    rlnc::PieceParams p{};
    p.in = in;
    p.in_row = int64_t(in_row);
    p.coef_row = int64_t(coef_row);
    if (n_out == 1 && n_in <= size_t(rlnc::kPieceInline)) {
        p.coef = nullptr;
        std::memcpy(p.coef_inline, coef, n_in);
    } else {
        if (int st = ws->pc_coef.ensure(n_out * coef_row)) return st;
        if (coef != ws->pc_coef.as<uint8_t>()) std::memcpy(ws->pc_coef.p, coef, n_out * coef_row);
        p.coef = ws->pc_coef.as<uint8_t>();
    }
    p.out_row = int64_t(round16(width));
    p.width = int64_t(width);
    p.n_in = int(n_in);
    p.n_out = int(n_out);
    const int64_t gx = (p.width + rlnc::kPieceCols - 1) / rlnc::kPieceCols;
    p.split = rlnc::piece_split(p.n_in, gx * int64_t(n_out));
    const int waves = rlnc::piece_waves((p.n_in + p.split - 1) / p.split);
    p.chunk_blocks = kPieceChunkBlocks;
    const size_t chunks = size_t(rlnc::piece_chunks(p));
    if (int st = ws->pc_out.ensure(n_out * size_t(p.out_row))) return st;
    if (chunks * 4 > ws->pc_flag.cap) {
        // completion is "flag == epoch" and every workspace counts its epochs from 1: a freshly allocated pinned
        // buffer may hold another (freed) workspace's flag values, so it starts zeroed (epochs are never 0)
        if (int st = ws->pc_flag.ensure(chunks * 4)) return st;
        std::memset(ws->pc_flag.p, 0, ws->pc_flag.cap);
    }
    if (chunks > ws->pc_count_words) {
        if (int st = ws->pc_count.ensure(chunks * 4)) return st;
        HIP_TRY(hipMemsetAsync(ws->pc_count.p, 0, chunks * 4, ws->stream));
        ws->pc_count_words = chunks;
    }
    if (p.split > 1) {
        const size_t blocks = size_t(gx) * n_out;
        if (int st = ws->pc_part.ensure(blocks * size_t(p.split) * 64 * 16)) return st;
        if (blocks > ws->pc_pcount_words) {
            if (int st = ws->pc_pcount.ensure(blocks * 4)) return st;
            HIP_TRY(hipMemsetAsync(ws->pc_pcount.p, 0, blocks * 4, ws->stream));
            ws->pc_pcount_words = blocks;
        }
        p.part = ws->pc_part.as<uint4>();
        p.pcount = ws->pc_pcount.as<uint32_t>();
    }
    p.out = ws->pc_out.as<uint8_t>();
    p.count = ws->pc_count.as<uint32_t>();
    p.flag = ws->pc_flag.as<uint32_t>();
    if (++ws->epoch == 0) ws->epoch = 1;
    p.epoch = ws->epoch;
    const uint64_t t1 = tr ? now_ns() : 0;
    HIP_TRY(rlnc::launch_piece(p, waves, ws->stream));
    const uint64_t t2 = tr ? now_ns() : 0;
    uint64_t t3 = 0;
    const size_t chunk_bytes = size_t(p.chunk_blocks) * size_t(rlnc::kPieceCols);
    const size_t cpr = chunks / n_out;
    for (size_t c = 0; c < chunks; ++c) {
        if (int st = piece_wait(p.flag + c, p.epoch, ws->stream)) {
            // a failed launch may leave counters part-way: wait for the stream and re-arm them
            (void)hipStreamSynchronize(ws->stream);
            ws->pc_count_words = 0;
            ws->pc_pcount_words = 0;
            return st;
        }
        if (c == 0 && tr) t3 = now_ns();
        const size_t r = c / cpr, c0 = (c % cpr) * chunk_bytes, c1 = std::min(width, c0 + chunk_bytes);
        std::memcpy(dst + r * dst_row + c0, p.out + r * size_t(p.out_row) + c0, c1 - c0);
    }
    if (tr) g_piece_trace.add((t1 - t0) / 1e3f, (t2 - t1) / 1e3f, (t3 - t2) / 1e3f, (now_ns() - t3) / 1e3f);
    return RLNC_OK;
}

}  // namespace rlnc::eng
