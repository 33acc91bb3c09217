// engine.cpp — librlnc_hip's context and its stateless calls behind the C ABI of include/rlnc_hip.h: status text, the
// context calls, the L1 primitives (one GF(2^8) kernel launch each on the context stream) and the host-only handle on
// the decoder's elimination (elimination.hpp).  The object API is objects.cpp, the batch API batch.cpp.
#include <new>

#include "context.hpp"
#include "elimination.hpp"

using rlnc::Elimination;
using namespace rlnc::eng;

namespace rlnc::eng {
thread_local std::string g_last_error;
}  // namespace rlnc::eng

extern "C" {

// ------------------------------------------------------------------------------------------------------
// status text — errors.rs:3-58
// ------------------------------------------------------------------------------------------------------
const char *rlnc_status_name(int s) {
    static const char *names[] = {"Ok",
                                  "CodingVectorLengthMismatch",
                                  "DataLengthMismatch",
                                  "PieceCountZero",
                                  "DataLengthZero",
                                  "PieceLengthZero",
                                  "NotEnoughPiecesToRecode",
                                  "PieceLengthTooShort",
                                  "PieceNotUseful",
                                  "ReceivedAllPieces",
                                  "NotAllPiecesReceivedYet",
                                  "InvalidDecodedDataFormat",
                                  "InvalidPieceLength",
                                  "InvalidOutputBuffer"};
    if (s >= 0 && s <= 13) return names[s];
    switch (s) {
    case RLNC_ERR_INVALID_ARGUMENT: return "InvalidArgument";
    case RLNC_ERR_DEVICE: return "DeviceError";
    case RLNC_ERR_OUT_OF_MEMORY: return "OutOfMemory";
    case RLNC_ERR_NO_DEVICE: return "NoDevice";
    default: return "Unknown";
    }
}

const char *rlnc_status_message(int s) {
    static const char *msgs[] = {"Ok",
                                 "Coding vector length mismatch",
                                 "Data length mismatch",
                                 "Piece count is zero",
                                 "Data length is zero",
                                 "Piece length is zero",
                                 "Not enough pieces received to recode",
                                 "Piece length is too short",
                                 "Received piece is not useful",
                                 "Received all pieces",
                                 "Not all pieces are received yet",
                                 "Invalid decoded data format",
                                 "Invalid piece length",
                                 "Invalid output buffer"};
    if (s >= 0 && s <= 13) return msgs[s];
    return rlnc_status_name(s);
}

const char *rlnc_last_error(void) { return g_last_error.c_str(); }
const char *rlnc_version(void) { return "rlnc_hip 0.1.0 (gfx950; reference itzmeanjan/rlnc 0.8.5)"; }

// ------------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------------
int rlnc_context_create(int device, rlnc_context **out) {
    CHECK_ARG(out != nullptr);
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_error(RLNC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return set_error(RLNC_ERR_NO_DEVICE, "device %d out of range (%d)", device, count);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(RLNC_ERR_NO_DEVICE, "device %d is %s, librlnc_hip is built for gfx950 only", device,
                         prop.gcnArchName);
    (void)rlnc::probe_unaligned_vector_access(device);  // once per device: rows at any byte alignment on the vector path
    auto *c = new (std::nothrow) rlnc_context;
    if (!c) return set_error(RLNC_ERR_OUT_OF_MEMORY, "context allocation");
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return set_error(RLNC_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->stream = c->own;
    // the persistent product's claim counters: zero before the first launch, left zero by every launch (zeroed on the
    // context's own stream: a legacy-stream memset would invalidate a capture in progress on another stream)
    if (c->ws_claim.ensure(256) != RLNC_OK || hipMemsetAsync(c->ws_claim.p, 0, 256, c->own) != hipSuccess ||
        hipStreamSynchronize(c->own) != hipSuccess) {
        c->release();
        return set_error(RLNC_ERR_OUT_OF_MEMORY, "context workspace");
    }
    *out = c;
    return RLNC_OK;
}

// Drops the creator's reference; the context lives on while objects bound to it exist.
void rlnc_context_destroy(rlnc_context *ctx) {
    if (ctx) ctx->release();
}

int rlnc_context_set_stream(rlnc_context *ctx, void *s) {
    CHECK_ARG(ctx != nullptr);
    ctx->stream = static_cast<hipStream_t>(s);
    return RLNC_OK;
}

int rlnc_context_use_own_stream(rlnc_context *ctx) {
    CHECK_ARG(ctx != nullptr);
    ctx->stream = ctx->own;
    return RLNC_OK;
}

void *rlnc_context_get_stream(rlnc_context *ctx) { return ctx ? ctx->stream : nullptr; }
int rlnc_context_device(const rlnc_context *ctx) { return ctx ? ctx->device : -1; }
int rlnc_device_unaligned_vector_access(int device) { return rlnc::unaligned_vector_access(device); }

int rlnc_stream_is_capturing(void *hip_stream, int *capturing) {
    CHECK_ARG(capturing != nullptr);
    *capturing = 1;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(static_cast<hipStream_t>(hip_stream), &cs);
    if (e != hipSuccess)
        return set_error(RLNC_ERR_DEVICE, "hipStreamIsCapturing: %s", hipGetErrorString(e));
    *capturing = cs != hipStreamCaptureStatusNone;
    return RLNC_OK;
}

int rlnc_context_synchronize(rlnc_context *ctx) {
    CHECK_ARG(ctx != nullptr);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RLNC_OK;
}

// Decode paths: 0 auto, 1 host, 2 device, 5 device blocked run, 7 and 8 the true-rank kernels for every shape (rank
// mode 1).  3, 4 and 6 were the round-1 LDS / register forms, retired: invalid in every build.
int rlnc_set_decode_path(rlnc_context *ctx, int path) {
    CHECK_ARG(ctx != nullptr && (path == 0 || path == 1 || path == 2 || path == 5 ||
                                 path == RLNC_DECODE_PATH_DEVICE_ANY || path == RLNC_DECODE_PATH_LARGE));
    ctx->decode_path = path;
    return RLNC_OK;
}

int rlnc_set_rank_mode(rlnc_context *ctx, int mode) {
    CHECK_ARG(ctx != nullptr && (mode == RLNC_RANK_MODE_REFERENCE || mode == RLNC_RANK_MODE_TRUE));
    ctx->rank_mode = mode;
    return RLNC_OK;
}

int rlnc_get_rank_mode(const rlnc_context *ctx) { return ctx ? ctx->rank_mode : -1; }

int rlnc_set_kernel_variant(rlnc_context *ctx, int variant, int max_tile_rows) {
    CHECK_ARG(ctx != nullptr);
    // shipped: 0 perm, 1 nibble (the reference's tables, ablation), 6 (the unshared bit-sliced program, which also
    // serves <= 16-row products and a first use inside a graph capture), 7 and 8 (the bit-sliced default); 2-5 and 9
    // are the A/B history, in the diagnostic build only (kernels_ab.hip)
    CHECK_ARG(variant == 0 || variant == 1 || variant == 6 || variant == 7 || variant == 8 ||
              (rlnc::ab_build() && variant >= 2 && variant <= 9));
    CHECK_ARG(max_tile_rows == 0 || max_tile_rows == 1 || max_tile_rows == 2 || max_tile_rows == 4 ||
              max_tile_rows == 8 || max_tile_rows == 16 || max_tile_rows == 32);
    ctx->variant = static_cast<rlnc::MatmulVariant>(variant);
    ctx->max_tile_rows = max_tile_rows;
    return RLNC_OK;
}

int rlnc_set_persistent_tiles(rlnc_context *ctx, int mode, int max_workgroups) {
    CHECK_ARG(ctx != nullptr);
    CHECK_ARG(mode == rlnc::kBsjPersistAuto || mode == rlnc::kBsjPersistOff || mode == rlnc::kBsjPersistAlways);
    CHECK_ARG(max_workgroups == 0 || (max_workgroups >= 8 && max_workgroups <= 65536));  // one per counter at least
    ctx->persist_mode = mode;
    ctx->persist_max_wgs = max_workgroups;
    return RLNC_OK;
}

int rlnc_set_column_run(rlnc_context *ctx, int col_run) {
    CHECK_ARG(ctx != nullptr);
    CHECK_ARG(col_run >= 0 && col_run <= 64);
    ctx->col_run = col_run;
    return RLNC_OK;
}

// ------------------------------------------------------------------------------------------------------
// L1 primitives — simd/mod.rs:18-119 (early-outs on the host, exactly as the reference)
// ------------------------------------------------------------------------------------------------------
int rlnc_gf256_inplace_mul_vec_by_scalar(rlnc_context *ctx, uint8_t *vec, size_t len, uint8_t scalar) {
    CHECK_ARG(ctx != nullptr);
    if (len == 0) return RLNC_OK;  // :19-21
    CHECK_ARG(vec != nullptr);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    if (scalar == 0) {  // :22-25
        HIP_TRY(hipMemsetAsync(vec, 0, len, ctx->stream));
        return RLNC_OK;
    }
    if (scalar == 1) return RLNC_OK;  // :26-28
    HIP_TRY(rlnc::launch_mul_vec_by_scalar(vec, int64_t(len), scalar, ctx->stream));
    return RLNC_OK;
}

int rlnc_gf256_inplace_add_vectors(rlnc_context *ctx, uint8_t *dst, const uint8_t *src, size_t len) {
    CHECK_ARG(ctx != nullptr);
    if (len == 0) return RLNC_OK;
    CHECK_ARG(dst != nullptr && src != nullptr);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    HIP_TRY(rlnc::launch_add_vectors(dst, src, int64_t(len), ctx->stream));
    return RLNC_OK;
}

int rlnc_gf256_mul_vec_by_scalar_then_add_into_vec(rlnc_context *ctx, uint8_t *dst, const uint8_t *src, size_t len,
                                                   uint8_t scalar) {
    CHECK_ARG(ctx != nullptr);
    if (len == 0) return RLNC_OK;  // :90-92
    if (scalar == 0) return RLNC_OK;  // :93-95
    CHECK_ARG(dst != nullptr && src != nullptr);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    if (scalar == 1) {  // :96-99
        HIP_TRY(rlnc::launch_add_vectors(dst, src, int64_t(len), ctx->stream));
        return RLNC_OK;
    }
    HIP_TRY(rlnc::launch_mul_add(dst, src, int64_t(len), scalar, ctx->stream));
    return RLNC_OK;
}

// The raw descriptors' stride contract (rlnc_hip.h): an operand the call writes has strides >= 0 and rows that do not
// overlap -- [n_obj][n_rows] rows of `bytes` bytes, objects outside each other's rows or rows outside each other's
// objects (either nesting) -- and an operand it reads has strides >= 0 (0: one row or one object for all).
static bool written_strides_ok(int64_t obj, int64_t row, int64_t n_obj, int64_t n_rows, int64_t bytes) {
    if (obj < 0 || row < 0) return false;
    const bool rows = n_rows > 1, objs = n_obj > 1;
    if ((rows && row < bytes) || (objs && obj < bytes)) return false;
    if (!rows || !objs) return true;
    using i128 = __int128;
    return i128(n_rows - 1) * row + bytes <= i128(obj) || i128(n_obj - 1) * obj + bytes <= i128(row);
}

int rlnc_gf256_matmul(rlnc_context *ctx, const rlnc_matmul_desc *desc) {
    CHECK_ARG(ctx != nullptr && desc != nullptr);
    CHECK_ARG(desc->n_out >= 0 && desc->n_in >= 0 && desc->width >= 0 && desc->n_obj >= 0);
    if (desc->n_out == 0 || desc->width == 0 || desc->n_obj == 0) return RLNC_OK;
    CHECK_ARG(desc->n_in > 0 && desc->in && desc->coef && desc->out);
    CHECK_ARG(desc->in_obj_stride >= 0 && desc->in_row_stride >= 0 && desc->coef_obj_stride >= 0 &&
              desc->coef_row_stride >= 0);
    CHECK_ARG(written_strides_ok(desc->out_obj_stride, desc->out_row_stride, desc->n_obj, desc->n_out, desc->width));
    CHECK_ARG(desc->hdr == nullptr ||
              written_strides_ok(desc->hdr_obj_stride, desc->hdr_row_stride, desc->n_obj, desc->n_out, desc->n_in));
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    rlnc::MatmulParams p{};
    p.in = desc->in;
    p.in_obj = desc->in_obj_stride;
    p.in_row = desc->in_row_stride;
    p.coef = desc->coef;
    p.coef_obj = desc->coef_obj_stride;
    p.coef_row = desc->coef_row_stride;
    p.out = desc->out;
    p.out_obj = desc->out_obj_stride;
    p.out_row = desc->out_row_stride;
    p.hdr = desc->hdr;
    p.hdr_obj = desc->hdr_obj_stride;
    p.hdr_row = desc->hdr_row_stride;
    p.n_out = desc->n_out;
    p.n_in = desc->n_in;
    p.width = desc->width;
    p.n_obj = desc->n_obj;
    return ctx->matmul(p);
}

int rlnc_gf256_sparse_matmul(rlnc_context *ctx, const rlnc_sparse_matmul_desc *desc) {
    CHECK_ARG(ctx != nullptr && desc != nullptr);
    CHECK_ARG(desc->n_out >= 0 && desc->n_in >= 0 && desc->w >= 0 && desc->width >= 0 && desc->n_obj >= 0);
    if (desc->n_out == 0 || desc->width == 0 || desc->n_obj == 0) return RLNC_OK;
    CHECK_ARG(desc->n_in > 0 && desc->in && desc->out && (desc->w == 0 || (desc->idx && desc->val)));
    CHECK_ARG((reinterpret_cast<uintptr_t>(desc->idx) & 3) == 0 && (desc->idx_obj_stride & 3) == 0 &&
              (desc->idx_row_stride & 3) == 0);
    CHECK_ARG(desc->in_obj_stride >= 0 && desc->in_row_stride >= 0 && desc->idx_obj_stride >= 0 &&
              desc->idx_row_stride >= 0 && desc->val_obj_stride >= 0 && desc->val_row_stride >= 0);
    CHECK_ARG(written_strides_ok(desc->out_obj_stride, desc->out_row_stride, desc->n_obj, desc->n_out, desc->width));
    CHECK_ARG(desc->hdr == nullptr ||
              written_strides_ok(desc->hdr_obj_stride, desc->hdr_row_stride, desc->n_obj, desc->n_out, desc->n_in));
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    rlnc::SparseMatmulParams p{};
    p.in = desc->in;
    p.in_obj = desc->in_obj_stride;
    p.in_row = desc->in_row_stride;
    p.idx = desc->idx;
    p.idx_obj = desc->idx_obj_stride;
    p.idx_row = desc->idx_row_stride;
    p.val = desc->val;
    p.val_obj = desc->val_obj_stride;
    p.val_row = desc->val_row_stride;
    p.out = desc->out;
    p.out_obj = desc->out_obj_stride;
    p.out_row = desc->out_row_stride;
    p.hdr = desc->hdr;
    p.hdr_obj = desc->hdr_obj_stride;
    p.hdr_row = desc->hdr_row_stride;
    p.n_out = desc->n_out;
    p.n_in = desc->n_in;
    p.w = desc->w;
    p.n_obj = desc->n_obj;
    p.width = desc->width;
    return ctx->sparse_matmul(p);
}

// ------------------------------------------------------------------------------------------------------
// host-only access to the decoder's elimination engine (no device needed; CPU-testable host logic)
// ------------------------------------------------------------------------------------------------------
struct rlnc_elimination {
    Elimination e;
    explicit rlnc_elimination(size_t k, size_t fixed, int mode = 0) : e(k, fixed, mode) {}
};

int rlnc_elimination_new(size_t k, size_t fixed_slots, rlnc_elimination **out) {
    CHECK_ARG(out != nullptr);
    *out = nullptr;
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    *out = new (std::nothrow) rlnc_elimination(k, fixed_slots);
    return *out ? RLNC_OK : set_error(RLNC_ERR_OUT_OF_MEMORY, "elimination allocation");
}
int rlnc_elimination_new_mode(size_t k, size_t fixed_slots, int rank_mode, rlnc_elimination **out) {
    CHECK_ARG(out != nullptr);
    *out = nullptr;
    CHECK_ARG(rank_mode == RLNC_RANK_MODE_REFERENCE || rank_mode == RLNC_RANK_MODE_TRUE);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    *out = new (std::nothrow) rlnc_elimination(k, fixed_slots, rank_mode);
    return *out ? RLNC_OK : set_error(RLNC_ERR_OUT_OF_MEMORY, "elimination allocation");
}
void rlnc_elimination_free(rlnc_elimination *e) { delete e; }
int rlnc_elimination_push(rlnc_elimination *e, const uint8_t *coeffs, int32_t *slot, int32_t *keep) {
    CHECK_ARG(e != nullptr && coeffs != nullptr);
    int s = -1;
    bool k = false;
    const int st = e->e.push(coeffs, &s, &k);
    if (slot) *slot = s;
    if (keep) *keep = k ? 1 : 0;
    return st;
}
size_t rlnc_elimination_rank(const rlnc_elimination *e) { return e ? e->e.rank() : 0; }
size_t rlnc_elimination_slots(const rlnc_elimination *e) { return e ? e->e.slots() : 0; }
int rlnc_elimination_transform(const rlnc_elimination *e, uint8_t *T, size_t ld) {
    CHECK_ARG(e != nullptr && T != nullptr && ld >= e->e.slots());
    std::memset(T, 0, e->e.k() * ld);
    e->e.transform(T, ld);
    return RLNC_OK;
}
int rlnc_elimination_coefficients(const rlnc_elimination *e, uint8_t *C) {
    CHECK_ARG(e != nullptr && C != nullptr);
    for (size_t r = 0; r < e->e.rank(); ++r) std::memcpy(C + r * e->e.k(), e->e.row(r), e->e.k());
    return RLNC_OK;
}

}  // extern "C"
