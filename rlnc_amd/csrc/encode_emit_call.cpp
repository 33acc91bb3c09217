// encode_emit_call.cpp — the sender's emit of librlnc_hip (include/rlnc_hip.h, rlnc_encode_emit): the argument checks and
// the call into encode_emit.hip (encode_emit_kernels.hpp).  The call takes a caller-owned plan buffer and no context
// workspace.
#include "context.hpp"
#include "encode_emit_kernels.hpp"

using namespace rlnc::eng;

extern "C" {

size_t rlnc_encode_emit_plan_bytes(size_t k, size_t max_per_object, size_t nobj, size_t n) {
    return rlnc::encode_emit_plan_bytes(k, max_per_object, nobj, n);
}

int rlnc_encode_emit(rlnc_context *ctx, const uint8_t *src, size_t src_obj_stride, size_t k, size_t L, size_t nobj,
                     const int32_t *want, size_t max_per_object, const uint8_t *r, size_t n, uint8_t *out,
                     size_t out_stride, int32_t *object_dev, int32_t *count_dev, int32_t *granted_dev, void *plan,
                     size_t plan_bytes) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0 || max_per_object == 0) return RLNC_OK;
    if (k > size_t(rlnc::kEmitMaxK))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an emit takes k <= %d (k=%zu)", rlnc::kEmitMaxK, k);
    if (max_per_object > size_t(rlnc::kEmitMaxPerObject))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an emit takes max_per_object <= %d packets per object "
                         "(max_per_object=%zu): emit in several calls", rlnc::kEmitMaxPerObject, max_per_object);
    if (n > size_t(rlnc::kEmitMaxPackets))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an emit takes n <= %d packets (n=%zu): emit in several calls",
                         rlnc::kEmitMaxPackets, n);
    if (nobj > size_t(rlnc::kEmitMaxObjects))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an emit takes num_objects <= %d (%zu objects): emit in several "
                         "calls", rlnc::kEmitMaxObjects, nobj);
    if (L > (size_t(1) << 40))  // k * L and n * (k + L) stay far inside 64 bits
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "an emit takes L <= 2^40 bytes (L=%zu)", L);
    if (out_stride == 0) out_stride = k + L;
    if (out_stride < k + L || out_stride > (size_t(1) << 42))  // n * out_stride stays inside 64 bits
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "out_stride must be 0 or lie in [k + L, 2^42] = [%zu, %zu] "
                         "(out_stride=%zu)", k + L, size_t(1) << 42, out_stride);
    if (src_obj_stride == 0) src_obj_stride = k * L;
    if (src_obj_stride < k * L || src_obj_stride > (size_t(1) << 62) / nobj)
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "src_obj_stride must be 0 or at least k * L = %zu, with "
                         "num_objects * src_obj_stride inside 2^62 (src_obj_stride=%zu)", k * L, src_obj_stride);
    CHECK_ARG(src != nullptr && want != nullptr && r != nullptr && out != nullptr && object_dev != nullptr &&
              count_dev != nullptr);
    const size_t need = rlnc::encode_emit_plan_bytes(k, max_per_object, nobj, n);
    if (plan == nullptr || (reinterpret_cast<uintptr_t>(plan) & 15) != 0 || plan_bytes < need)
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "the emit's plan buffer must be non-null, 16-byte aligned and at least "
                         "rlnc_encode_emit_plan_bytes(k=%zu, max_per_object=%zu, %zu objects, n=%zu) = %zu bytes long "
                         "(%p, %zu bytes)", k, max_per_object, nobj, n, need, plan, plan_bytes);
    rlnc::EmitParams p{};
    p.src = src;
    p.src_obj = int64_t(src_obj_stride);
    p.k = int(k), p.n_obj = int(nobj), p.max_per = int(max_per_object), p.n = int(n);
    p.L = int64_t(L);
    p.want = want;
    p.r = r;
    p.out = out;
    p.out_stride = int64_t(out_stride);
    p.object = object_dev;
    p.count = count_dev;
    p.granted = granted_dev;
    p.plan = plan;
    if (!rlnc::encode_emit_fits(p))
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "an emit of %zu objects of k=%zu, L=%zu, max_per_object=%zu needs more than 2^31 - 1 workgroups "
                         "in one launch: emit fewer objects per call", nobj, k, L, max_per_object);
    int st;
    if ((st = ctx->activate()) || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_encode_emit(p, rlnc::unaligned_vector_ok(), ctx->stream));
    return RLNC_OK;
}

}  // extern "C"
