// decode_stream.cpp — the resumable device decode of librlnc_hip (include/rlnc_hip.h, "Decode streams"): the
// true-rank decoder state of many objects in a caller-owned device buffer, pushed forward as pieces arrive
// (rank_large.hip in its stream form, rank_large_kernels.hpp; for generations that fit LDS also the one-launch form of
// rank_stream.hip, rank_stream_kernels.hpp), compacted in place (rank_compact.hip, rank_compact_kernels.hpp), its
// finished objects delivered (stream_deliver.hip, stream_deliver_kernels.hpp), the pieces it holds recoded for a relay
// (stream_recode.hip, stream_recode_kernels.hpp), mixed arrivals accepted into their slots (stream_accept.hip,
// stream_accept_kernels.hpp), and the registry of initialised state buffers.  The state buffer itself: rank_state.hpp.
#include <mutex>
#include <tuple>
#include <vector>

#include "context.hpp"
#include "rank_compact_kernels.hpp"
#include "rank_stream_kernels.hpp"
#include "stream_accept_kernels.hpp"
#include "stream_deliver_kernels.hpp"
#include "stream_recode_kernels.hpp"

using namespace rlnc::eng;

namespace {

// State buffers initialised by rlnc_decode_stream_init (any context), by address: the device and the shape they were
// laid out for.  Push and snapshot take a buffer only with exactly those, as the planned products take a plan buffer.
struct StreamKey {
    int device;
    size_t k, m, nobj;
    auto tie() const { return std::tie(device, k, m, nobj); }
    bool operator==(const StreamKey &o) const { return tie() == o.tie(); }
};
std::mutex g_stream_mu;
std::vector<std::pair<const void *, StreamKey>> g_streams;  // (state buffer, key), most recent last
constexpr size_t kStreamRecs = 256;

void remember_stream(const void *state, const StreamKey &key) {
    std::lock_guard<std::mutex> lock(g_stream_mu);
    for (auto it = g_streams.begin(); it != g_streams.end(); ++it)
        if (it->first == state) {
            g_streams.erase(it);
            break;
        }
    if (g_streams.size() >= kStreamRecs) g_streams.erase(g_streams.begin());
    g_streams.emplace_back(state, key);
}

int stream_check(const void *state, const StreamKey &key) {
    std::lock_guard<std::mutex> lock(g_stream_mu);
    for (auto it = g_streams.rbegin(); it != g_streams.rend(); ++it)
        if (it->first == state) {
            if (it->second == key) return RLNC_OK;
            break;
        }
    return set_error(RLNC_ERR_INVALID_ARGUMENT,
                     "decode stream state %p was not initialised for this device and shape (k=%zu, m=%zu, %zu objects): "
                     "call rlnc_decode_stream_init with the arguments of this call",
                     state, key.k, key.m, key.nobj);
}

// what init, push and snapshot share: the handle, the state buffer, the shape, the rank mode
int stream_args(rlnc_context *ctx, const void *state, size_t state_bytes, size_t k, size_t m, size_t nobj) {
    CHECK_ARG(ctx != nullptr && state != nullptr);
    CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 15) == 0);
    if (ctx->rank_mode != RLNC_RANK_MODE_TRUE)
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "a decode stream has true-rank semantics: the context is in rank mode %d (rlnc_set_rank_mode)",
                         ctx->rank_mode);
    const size_t need = rlnc::rank_stream_state_bytes(k, m, nobj);
    if (need == 0)
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "a decode stream takes k <= %d, m <= %d and at least one object "
                         "(k=%zu, m=%zu, %zu objects)", rlnc::kLargeMaxK, rlnc::kLargeMaxM, k, m, nobj);
    CHECK_ARG(state_bytes >= need);
    return RLNC_OK;
}

// the shape of a stream call, as every launch on the state takes it (no pieces, no strides)
rlnc::RrefParams stream_shape(size_t k, size_t m, size_t nobj) {
    rlnc::RrefParams rp{};
    rp.k = int(k), rp.m = int(m), rp.n_obj = int(nobj);
    return rp;
}

// RLNC_STREAM_FORM_AUTO: the LDS form where it was measured faster than the workspace form by more than the two arms'
// spread on every line -- dense and density-4 vectors, one push of everything down to one piece per push, 32 to 4,096
// objects -- which is k <= 48 with m <= 64 (profiles/r14_stream_lds.jsonl).  From k = 64 on the
// workspace form wins some or most lines with several pieces per push; the object count did not decide any line.
constexpr size_t kStreamAutoLdsMaxK = 48, kStreamAutoLdsMaxM = 64;
bool stream_auto_lds(size_t k, size_t m) { return k <= kStreamAutoLdsMaxK && m <= kStreamAutoLdsMaxM; }

}  // namespace

extern "C" {

int rlnc_set_stream_form(rlnc_context *ctx, int form) {
    CHECK_ARG(ctx != nullptr && (form == RLNC_STREAM_FORM_AUTO || form == RLNC_STREAM_FORM_WORKSPACE ||
                                 form == RLNC_STREAM_FORM_LDS));
    ctx->stream_form = form;
    return RLNC_OK;
}

int rlnc_decode_stream_lds_fits(size_t k, size_t m) { return rlnc::rank_stream_lds_fits(k, m) ? 1 : 0; }

size_t rlnc_decode_stream_state_bytes(size_t k, size_t m, size_t nobj) {
    return rlnc::rank_stream_state_bytes(k, m, nobj);
}

int rlnc_decode_stream_init(rlnc_context *ctx, void *state, size_t state_bytes, size_t k, size_t m, size_t nobj) {
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st || (st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_rank_stream_init(int(k), int(m), int(nobj), state, state_bytes, ctx->stream));
    remember_stream(state, StreamKey{ctx->device, k, m, nobj});
    return RLNC_OK;
}

int rlnc_decode_stream_push(rlnc_context *ctx, void *state, size_t state_bytes, const uint8_t *pieces,
                            size_t obj_stride, size_t k, size_t L, size_t m, size_t nobj, const int32_t *avail,
                            size_t max_new, int32_t *rank_dev, int32_t *answered_dev) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (max_new == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(pieces != nullptr && avail != nullptr);
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st) return st;
    if (obj_stride == 0) obj_stride = m * (k + L);
    CHECK_ARG(obj_stride >= m * (k + L));
    if ((st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))) return st;
    const bool fits = rlnc::rank_stream_lds_fits(k, m);
    if (ctx->stream_form == RLNC_STREAM_FORM_LDS && !fits)  // no silent fallback to the workspace form
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "stream form %d (LDS) takes 8192 + 4*(k*D + 2*D + m*ceil(k/4) + m + 2*k + ceil(k/4)) <= %zu bytes, "
                         "D = ceil(k/4) + ceil(m/4): k=%zu, m=%zu takes %zu (rlnc_set_stream_form)",
                         RLNC_STREAM_FORM_LDS, rlnc::kRrefMaxLds, k, m, rlnc::rank_lds_bytes(int(k), int(m)));
    const bool lds = ctx->stream_form == RLNC_STREAM_FORM_LDS ||
                     (ctx->stream_form == RLNC_STREAM_FORM_AUTO && fits && stream_auto_lds(k, m));
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    rlnc::RrefParams rp = stream_shape(k, m, nobj);
    rp.pieces = pieces;
    rp.obj_stride = int64_t(obj_stride);
    rp.piece_stride = int64_t(k + L);
    if (lds)
        HIP_TRY(rlnc::launch_rank_stream_push_lds(rp, state, state_bytes, avail, int(std::min(max_new, m)), rank_dev,
                                                  answered_dev, ctx->stream));
    else
        HIP_TRY(rlnc::launch_rank_stream_push(rp, state, state_bytes, avail, int(std::min(max_new, m)), rank_dev,
                                              answered_dev, ctx->stream));
    return RLNC_OK;
}

int rlnc_decode_stream_compact(rlnc_context *ctx, void *state, size_t state_bytes, uint8_t *pieces, size_t obj_stride,
                               size_t k, size_t L, size_t m, size_t nobj, const int32_t *retire, int32_t *kept_dev,
                               int32_t *answered_dev) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (pieces != nullptr && L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (nobj == 0) return RLNC_OK;
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st) return st;
    rlnc::RrefParams rp = stream_shape(k, m, nobj);
    if (pieces != nullptr) {
        CHECK_ARG(L <= (size_t(1) << 40));  // m * (k + L) stays far inside 64 bits
        if (obj_stride == 0) obj_stride = m * (k + L);
        CHECK_ARG(obj_stride >= m * (k + L));
        rp.obj_stride = int64_t(obj_stride);
        rp.piece_stride = int64_t(k + L);
    }
    if ((st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))) return st;
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_rank_stream_compact(rp, pieces, state, state_bytes, retire, kept_dev, answered_dev,
                                             rlnc::unaligned_vector_ok(), ctx->stream));
    return RLNC_OK;
}

int rlnc_decode_stream_snapshot(rlnc_context *ctx, const void *state, size_t state_bytes, size_t k, size_t m,
                                size_t nobj, uint8_t *T_dev, int32_t *piece_status_dev, int32_t *rank_dev) {
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st || (st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))) return st;
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    rlnc::RrefParams rp = stream_shape(k, m, nobj);
    rp.T = T_dev;
    rp.T_obj = int64_t(k * m);
    rp.status = piece_status_dev;
    rp.rank = rank_dev;
    HIP_TRY(rlnc::launch_rank_stream_snapshot(rp, state, state_bytes, ctx->stream));
    return RLNC_OK;
}

size_t rlnc_decode_stream_deliver_plan_bytes(size_t k, size_t m, size_t nobj) {
    return rlnc::stream_deliver_plan_bytes(k, m, nobj);
}

int rlnc_decode_stream_deliver(rlnc_context *ctx, const void *state, size_t state_bytes, const uint8_t *pieces,
                               size_t obj_stride, size_t k, size_t L, size_t m, size_t nobj, const int32_t *select,
                               uint8_t *decoded, int32_t *object_status_dev, int64_t *data_len_dev, void *plan,
                               size_t plan_bytes) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (nobj == 0) return RLNC_OK;
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st || (st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))) return st;
    CHECK_ARG(L <= (size_t(1) << 40));  // m * (k + L) stays far inside 64 bits
    if (obj_stride == 0) obj_stride = m * (k + L);
    CHECK_ARG(obj_stride >= m * (k + L));
    CHECK_ARG(pieces != nullptr && decoded != nullptr && object_status_dev != nullptr && data_len_dev != nullptr);
    const size_t need = rlnc::stream_deliver_plan_bytes(k, m, nobj);
    if (plan == nullptr || (reinterpret_cast<uintptr_t>(plan) & 15) != 0 || plan_bytes < need)
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "the delivery's plan buffer must be non-null, 16-byte aligned and at least "
                         "rlnc_decode_stream_deliver_plan_bytes(k=%zu, m=%zu, %zu objects) = %zu bytes long (%p, %zu bytes)",
                         k, m, nobj, need, plan, plan_bytes);
    rlnc::DeliverParams p{};
    p.pieces = pieces;
    p.obj_stride = int64_t(obj_stride);
    p.k = int(k), p.m = int(m), p.n_obj = int(nobj);
    p.L = int64_t(L);
    p.select = select;
    p.decoded = decoded;
    p.status = object_status_dev;
    p.len = data_len_dev;
    p.plan = plan;
    if (!rlnc::stream_deliver_fits(p))
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "a delivery of %zu objects of k=%zu, m=%zu, L=%zu needs more than 2^31 - 1 workgroups in one "
                         "launch: deliver fewer objects per call", nobj, k, m, L);
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_stream_deliver(p, state, state_bytes, rlnc::unaligned_vector_ok(), ctx->stream));
    return RLNC_OK;
}

size_t rlnc_decode_stream_recode_plan_bytes(size_t k, size_t m, size_t count, size_t nobj) {
    return rlnc::stream_recode_plan_bytes(k, m, count, nobj);
}

int rlnc_decode_stream_recode(rlnc_context *ctx, const void *state, size_t state_bytes, const uint8_t *pieces,
                              size_t obj_stride, size_t k, size_t L, size_t m, size_t nobj, const int32_t *select,
                              const uint8_t *r, size_t count, uint8_t *out, int32_t *status_dev, int32_t *used_dev,
                              void *plan, size_t plan_bytes) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (count == 0 || nobj == 0) return RLNC_OK;
    int st = stream_args(ctx, state, state_bytes, k, m, nobj);
    if (st || (st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))) return st;
    CHECK_ARG(L <= (size_t(1) << 40));  // m * (k + L) and count * (k + L) stay far inside 64 bits
    if (obj_stride == 0) obj_stride = m * (k + L);
    CHECK_ARG(obj_stride >= m * (k + L));
    CHECK_ARG(pieces != nullptr && r != nullptr && out != nullptr && status_dev != nullptr);
    if (count > size_t(rlnc::kRecodeMaxCount))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "a stream recode takes 1 <= count <= %d recoded pieces per object "
                         "(count=%zu): recode in several calls", rlnc::kRecodeMaxCount, count);
    const size_t need = rlnc::stream_recode_plan_bytes(k, m, count, nobj);
    if (plan == nullptr || (reinterpret_cast<uintptr_t>(plan) & 15) != 0 || plan_bytes < need)
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "the recode's plan buffer must be non-null, 16-byte aligned and at least "
                         "rlnc_decode_stream_recode_plan_bytes(k=%zu, m=%zu, count=%zu, %zu objects) = %zu bytes long "
                         "(%p, %zu bytes)", k, m, count, nobj, need, plan, plan_bytes);
    rlnc::RecodeParams p{};
    p.pieces = pieces;
    p.obj_stride = int64_t(obj_stride);
    p.k = int(k), p.m = int(m), p.n_obj = int(nobj), p.count = int(count);
    p.L = int64_t(L);
    p.select = select;
    p.r = r;
    p.out = out;
    p.status = status_dev;
    p.used = used_dev;
    p.plan = plan;
    if (!rlnc::stream_recode_fits(p))
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "a recode of %zu objects of k=%zu, m=%zu, L=%zu, count=%zu needs more than 2^31 - 1 workgroups in "
                         "one launch: recode fewer objects per call", nobj, k, m, L, count);
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_stream_recode(p, state, state_bytes, rlnc::unaligned_vector_ok(), ctx->stream));
    return RLNC_OK;
}

size_t rlnc_decode_stream_accept_plan_bytes(size_t n, size_t nobj) { return rlnc::stream_accept_plan_bytes(n, nobj); }

int rlnc_decode_stream_accept(rlnc_context *ctx, const void *state, size_t state_bytes, const uint8_t *arrivals,
                              size_t arrival_stride, const int32_t *object, size_t n, const int32_t *count,
                              uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m, size_t nobj,
                              int32_t *avail, int32_t *slot_dev, int32_t *refused_dev, void *plan, size_t plan_bytes) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0) return RLNC_OK;
    int st;
    if (state != nullptr &&
        ((st = stream_args(ctx, state, state_bytes, k, m, nobj)) || (st = stream_check(state, StreamKey{ctx->device, k, m, nobj}))))
        return st;
    if (m == 0 || m > size_t(rlnc::kLargeMaxM) || k > size_t(rlnc::kLargeMaxK) || nobj > 0x7FFFFFFF)
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an accept takes k <= %d, 1 <= m <= %d and fewer than 2^31 objects "
                         "(k=%zu, m=%zu, %zu objects)", rlnc::kLargeMaxK, rlnc::kLargeMaxM, k, m, nobj);
    if (n > size_t(rlnc::kAcceptMaxArrivals))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an accept takes n <= %d arrivals (n=%zu): accept in several calls",
                         rlnc::kAcceptMaxArrivals, n);
    if (L > (size_t(1) << 40))  // m * (k + L) and n * (k + L) stay far inside 64 bits
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an accept takes L <= 2^40 bytes (L=%zu)", L);
    if (arrival_stride == 0) arrival_stride = k + L;
    if (arrival_stride < k + L || arrival_stride > (size_t(1) << 42))  // n * arrival_stride stays inside 64 bits
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "arrival_stride must be 0 or lie in [k + L, 2^42] = [%zu, %zu] "
                         "(arrival_stride=%zu)", k + L, size_t(1) << 42, arrival_stride);
    if (obj_stride == 0) obj_stride = m * (k + L);
    CHECK_ARG(obj_stride >= m * (k + L));
    CHECK_ARG(arrivals != nullptr && object != nullptr && pieces != nullptr && avail != nullptr);
    const size_t need = rlnc::stream_accept_plan_bytes(n, nobj);
    if (plan == nullptr || (reinterpret_cast<uintptr_t>(plan) & 15) != 0 || plan_bytes < need)
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "the accept's plan buffer must be non-null, 16-byte aligned and at least "
                         "rlnc_decode_stream_accept_plan_bytes(n=%zu, %zu objects) = %zu bytes long (%p, %zu bytes)",
                         n, nobj, need, plan, plan_bytes);
    rlnc::AcceptParams p{};
    p.arrivals = arrivals;
    p.arrival_stride = int64_t(arrival_stride);
    p.object = object;
    p.count = count;
    p.n = int(n);
    p.pieces = pieces;
    p.obj_stride = int64_t(obj_stride);
    p.piece = int64_t(k + L);
    p.k = int(k), p.m = int(m), p.n_obj = int(nobj);
    p.avail = avail;
    p.slot = slot_dev;
    p.refused = refused_dev;
    p.plan = plan;
    if (!rlnc::stream_accept_fits(p))
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "an accept of n=%zu arrivals of k + L = %zu bytes needs more than 2^31 - 1 workgroups in one "
                         "launch (n x floor((k + L) / %d)): accept fewer arrivals per call", n, k + L,
                         rlnc::kAcceptColChunk);
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_stream_accept(p, state, state_bytes, rlnc::unaligned_vector_ok(), ctx->stream));
    return RLNC_OK;
}

}  // extern "C"
