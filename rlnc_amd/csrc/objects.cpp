// objects.cpp — the object API of librlnc_hip: Encoder / Recoder / Decoder behind the C ABI of include/rlnc_hip.h.
// Mirrors rlnc::full::{Encoder, Recoder, Decoder} (src/full/*.rs): same constructor validation order, same status for
// every error, same getters.  All GF(2^8) byte work on pieces runs on the device (piece.hip, kernels.hip, elementwise.hip); the host
// only runs the k×(k+slots) coefficient elimination of the decoder (elimination.hpp).
#include <memory>
#include <new>
#include <vector>

#include "context.hpp"
#include "elimination.hpp"
#include "gf256.hpp"
#include "host_copy.hpp"
#include "piece.hpp"
#include "piece_call.hpp"

using rlnc::Elimination;
using namespace rlnc::eng;

// Encoder / Recoder / Decoder hold a reference on their context (released when the object is freed, after the object's
// own members), so an object outlives the handle its creator held -- e.g. one built on a worker thread whose
// thread-local context has since been destroyed.
struct ContextRef {
    rlnc_context *ctx = nullptr;
    ~ContextRef() {
        if (ctx) ctx->release();
    }
};

struct rlnc_encoder : ContextRef {
    size_t k = 0, L = 0, stride = 0;
    uint8_t *src = nullptr;  // k rows × stride
    size_t src_cap = 0;      // bytes of the owned block
    bool owned = false;
    ObjUse use;  // code_batch_device launches reading src
    ~rlnc_encoder() {
        if (owned && src) ctx->obj_free(src, src_cap, &use);
    }
};

struct rlnc_recoder : ContextRef {
    size_t k = 0, n = 0, full = 0, stride = 0;
    uint8_t *pieces = nullptr;  // n rows × stride (coeffs ‖ data)
    size_t pieces_cap = 0;
    ObjUse use;  // recode_batch_device launches reading pieces
    ~rlnc_recoder() {
        if (pieces) ctx->obj_free(pieces, pieces_cap, &use);
    }
};

struct rlnc_decoder : ContextRef {
    size_t k = 0, L = 0, stride = 0;
    size_t received = 0, useful = 0;
    int rank_mode = 0;  // the context's rank mode when the decoder was created
    std::unique_ptr<Elimination> elim;
    uint8_t *store = nullptr;  // slot rows × stride (received data rows still referenced by E)
    size_t store_slots = 0, store_cap = 0;
    // the context's upload-ring slot of the last upload into store (Decoder::decode returns once its piece is staged,
    // before the DMA): every later use of store, on whichever stream, is ordered after it
    UpTicket up;
    int order(hipStream_t s) const { return ctx->upload_wait(up, s); }
    ~rlnc_decoder() {
        // every other use of the store is synchronous (decode_device, get_decoded_data*, clone): the uploads only
        (void)ctx->upload_sync(up);
        if (store) ctx->obj_free(store, store_cap, nullptr);
    }
};

namespace {

// a new object bound to ctx, or OutOfMemory ("<what> allocation")
template <class T>
int new_object(rlnc_context *ctx, const char *what, std::unique_ptr<T> &o) {
    o.reset(new (std::nothrow) T);
    if (!o) return set_error(RLNC_ERR_OUT_OF_MEMORY, "%s allocation", what);
    o->ctx = ctx;
    ctx->retain();
    return RLNC_OK;
}

// dst[0:width) = XOR_j coef[j] · in[j·stride + 0 : width), j < n_in, from host coefficients into host memory: the
// call-latency kernel for rows it takes, else staged through the lease's device buffers and the batch kernels.
// ordered: the rows may still be written by work on the context stream (a borrowed device source); rows uploaded by
// their object's constructor, which synchronised, need no ordering on the call-latency path.
// Thread-safe on one object (the reference's code(&self) on a Send + Sync Encoder): each call leases its own stream
// and buffers.
int one_row_product(rlnc_context *ctx, const uint8_t *in, size_t stride, size_t n_in, size_t width,
                    const uint8_t *coef, uint8_t *dst, bool ordered) {
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    Lease ws(ctx);
    if (width <= kPieceMaxBytes && piece_eligible(in, stride, width)) {
        if ((st = ws.acquire(ordered))) return st;
        return piece_call(ws.ws.get(), in, stride, n_in, width, coef, n_in, 1, dst, width);
    }
    if ((st = ws.acquire())) return st;
    if ((st = ws->coef.ensure(n_in)) || (st = ws->out.ensure(width))) return st;
    HIP_TRY(hipMemcpyAsync(ws->coef.p, coef, n_in, hipMemcpyHostToDevice, ws->stream));
    const auto p = product_params(in, 0, stride, n_in, width, ws->coef.as<uint8_t>(), 1, ws->out.as<uint8_t>(), 0,
                                  width, 1);
    if ((st = ctx->matmul(p, ws->stream, ws->idx, false))) return st;
    HIP_TRY(hipMemcpyAsync(dst, ws->out.p, width, hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    return RLNC_OK;
}

constexpr size_t kGridUploadMax = size_t(8) << 20;  // Recoder::new uploads up to this many bytes by the grid kernel

}  // namespace

int rlnc::eng::encoder_adopt_device(rlnc_context *ctx, uint8_t *img, size_t k, size_t L, size_t stride,
                                    rlnc_encoder **out) {
    std::unique_ptr<rlnc_encoder> e;
    if (int st = new_object(ctx, "encoder", e)) return st;
    e->k = k;
    e->L = L;
    e->stride = stride;
    e->src = img;
    e->src_cap = k * stride;
    e->owned = true;
    *out = e.release();
    return RLNC_OK;
}

extern "C" {

// ------------------------------------------------------------------------------------------------------
// Encoder — encoder.rs
// ------------------------------------------------------------------------------------------------------
static int encoder_from_host(rlnc_context *ctx, const uint8_t *data, size_t len, size_t k, bool pad, rlnc_encoder **out) {
    CHECK_ARG(ctx != nullptr && out != nullptr);
    *out = nullptr;
    if (len == 0) return RLNC_ERR_DATA_LENGTH_ZERO;  // encoder.rs:86-88 / :51-53
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;    // :89-91 / :54-56
    CHECK_ARG(data != nullptr);
    size_t L;
    if (pad) {
        L = (len + 1 + k - 1) / k;  // :93-95
    } else {
        L = len / k;
        if (L * k != len) return RLNC_ERR_DATA_LENGTH_MISMATCH;  // :58-64
    }
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    std::unique_ptr<rlnc_encoder> e;
    if ((st = new_object(ctx, "encoder", e))) return st;
    e->k = k;
    e->L = L;
    e->stride = round16(L);
    e->owned = true;
    if ((st = ctx->obj_alloc(k * e->stride, &e->src, &e->src_cap))) return st;
    Lease ws(ctx);
    if ((st = ws.acquire())) return st;
    // padded image: data, 0x81 marker, zeros (encoder.rs:98-99), laid out at a 16-B row stride
    if ((st = ws->pin_a.ensure(k * e->stride))) return st;
    uint8_t *h = ws->pin_a.as<uint8_t>();
    std::memset(h, 0, k * e->stride);
    for (size_t r = 0; r < k; ++r) {
        const size_t off = r * L;
        if (off < len) std::memcpy(h + r * e->stride, data + off, std::min(L, len - off));
    }
    if (pad) h[(len / L) * e->stride + (len % L)] = rlnc::kBoundaryMarker;
    HIP_TRY(hipMemcpyAsync(e->src, h, k * e->stride, hipMemcpyHostToDevice, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    *out = e.release();
    return RLNC_OK;
}

int rlnc_encoder_new(rlnc_context *ctx, const uint8_t *data, size_t len, size_t k, rlnc_encoder **out) {
    return encoder_from_host(ctx, data, len, k, true, out);
}

int rlnc_encoder_without_padding(rlnc_context *ctx, const uint8_t *data, size_t len, size_t k, rlnc_encoder **out) {
    return encoder_from_host(ctx, data, len, k, false, out);
}

int rlnc_encoder_from_device(rlnc_context *ctx, const uint8_t *pieces, size_t k, size_t L, size_t row_stride,
                             rlnc_encoder **out) {
    CHECK_ARG(ctx != nullptr && out != nullptr);
    *out = nullptr;
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_DATA_LENGTH_ZERO;
    CHECK_ARG(pieces != nullptr && row_stride >= L);
    std::unique_ptr<rlnc_encoder> e;
    if (int st = new_object(ctx, "encoder", e)) return st;
    e->k = k;
    e->L = L;
    e->stride = row_stride;
    e->src = const_cast<uint8_t *>(pieces);
    e->owned = false;
    *out = e.release();
    return RLNC_OK;
}

// #[derive(Clone)] (encoder.rs:18): an owned source is copied; a borrowed device source stays borrowed
int rlnc_encoder_clone(const rlnc_encoder *e, rlnc_encoder **out) {
    CHECK_ARG(e != nullptr && out != nullptr);
    *out = nullptr;
    int st = e->ctx->activate();
    if (st) return st;
    std::unique_ptr<rlnc_encoder> c;
    if ((st = new_object(e->ctx, "encoder", c))) return st;
    c->k = e->k;
    c->L = e->L;
    c->stride = e->stride;
    c->owned = e->owned;
    if (e->owned) {
        if ((st = e->ctx->obj_alloc(e->k * e->stride, &c->src, &c->src_cap))) return st;
        Lease ws(e->ctx);
        if ((st = ws.acquire())) return st;
        HIP_TRY(hipMemcpyAsync(c->src, e->src, e->k * e->stride, hipMemcpyDeviceToDevice, ws->stream));
        HIP_TRY(hipStreamSynchronize(ws->stream));
    } else {
        c->src = e->src;
    }
    *out = c.release();
    return RLNC_OK;
}

void rlnc_encoder_free(rlnc_encoder *e) { delete e; }
size_t rlnc_encoder_get_piece_count(const rlnc_encoder *e) { return e ? e->k : 0; }
size_t rlnc_encoder_get_piece_byte_len(const rlnc_encoder *e) { return e ? e->L : 0; }
size_t rlnc_encoder_get_full_coded_piece_byte_len(const rlnc_encoder *e) { return e ? e->k + e->L : 0; }

int rlnc_encoder_code_with_coding_vector(rlnc_encoder *e, const uint8_t *cv, size_t cv_len, uint8_t *coded,
                                         size_t coded_len) {
    CHECK_ARG(e != nullptr);
    if (cv_len != e->k) return RLNC_ERR_CODING_VECTOR_LENGTH_MISMATCH;  // encoder.rs:129-131
    if (coded_len != e->L) return RLNC_ERR_INVALID_OUTPUT_BUFFER;       // :132-134
    CHECK_ARG(cv != nullptr && coded != nullptr);
    // an owned source is immutable after Encoder::new; a borrowed one is ordered after the context stream's work
    return one_row_product(e->ctx, e->src, e->stride, e->k, e->L, cv, coded, !e->owned);
}

int rlnc_encoder_code_with_buf(rlnc_encoder *e, const uint8_t *rnd, size_t n_rnd, uint8_t *full, size_t full_len) {
    CHECK_ARG(e != nullptr);
    if (full_len != e->k + e->L) return RLNC_ERR_INVALID_OUTPUT_BUFFER;  // encoder.rs:242-244
    if (n_rnd != e->k) return RLNC_ERR_CODING_VECTOR_LENGTH_MISMATCH;    // fill_bytes fills exactly k bytes
    CHECK_ARG(rnd != nullptr && full != nullptr);
    std::memmove(full, rnd, e->k);  // :246-248
    return rlnc_encoder_code_with_coding_vector(e, full, e->k, full + e->k, e->L);
}

// n coded pieces: out[i] = cv[i] ‖ Σ_j cv[i][j] · src_j  (cv already on the device)
int rlnc_encoder_code_batch_device(rlnc_encoder *e, const uint8_t *coeffs_dev, size_t n, uint8_t *out_dev,
                                   size_t out_row_stride) {
    CHECK_ARG(e != nullptr);
    if (n == 0) return RLNC_OK;
    CHECK_ARG(coeffs_dev != nullptr && out_dev != nullptr && n <= 0x7FFFFFFF);
    const size_t row = out_row_stride ? out_row_stride : e->k + e->L;
    CHECK_ARG(row >= e->k + e->L);
    int st = e->ctx->activate();
    if (st || (st = e->ctx->note_capture())) return st;
    auto p = product_params(e->src, 0, e->stride, e->k, e->L, coeffs_dev, n, out_dev + e->k, 0, row, 1);
    p.hdr = out_dev;
    p.hdr_row = int64_t(row);
    if ((st = e->ctx->matmul(p))) return st;
    return e->owned ? e->use.note(e->ctx->stream) : RLNC_OK;
}

// the same from sparse coding vectors (sparse.hip): idx / val [n][w] -> out[i] = expanded cv[i] ‖ data
int rlnc_encoder_code_sparse_batch_device(rlnc_encoder *e, const int32_t *idx_dev, const uint8_t *val_dev, size_t w,
                                          size_t n, uint8_t *out_dev, size_t out_row_stride) {
    CHECK_ARG(e != nullptr);
    if (n == 0) return RLNC_OK;
    CHECK_ARG(out_dev != nullptr && n <= 0x7FFFFFFF && e->k <= 0x7FFFFFFF);
    CHECK_ARG(sparse_entries_ok(idx_dev, val_dev, w));
    const size_t row = out_row_stride ? out_row_stride : e->k + e->L;
    CHECK_ARG(row >= e->k + e->L);
    int st = e->ctx->activate();
    if (st || (st = e->ctx->note_capture())) return st;
    auto p = sparse_product_params(e->src, 0, e->stride, e->k, e->L, idx_dev, val_dev, w, n, out_dev + e->k, 0, row, 1);
    p.hdr = out_dev;
    p.hdr_row = int64_t(row);
    if ((st = e->ctx->sparse_matmul(p))) return st;
    return e->owned ? e->use.note(e->ctx->stream) : RLNC_OK;
}

// ------------------------------------------------------------------------------------------------------
// Recoder — recoder.rs
// ------------------------------------------------------------------------------------------------------
int rlnc_recoder_new(rlnc_context *ctx, const uint8_t *data, size_t len, size_t full, size_t k, rlnc_recoder **out) {
    CHECK_ARG(ctx != nullptr && out != nullptr);
    *out = nullptr;
    if (len == 0) return RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE;  // recoder.rs:69-71
    if (full == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;            // :72-74
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;                // :75-77
    if (full <= k) return RLNC_ERR_PIECE_LENGTH_TOO_SHORT;       // :78-80
    const size_t n = len / full;                                 // :83 (trailing bytes ignored, :88)
    if (n == 0) return RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE;     // reference: UB (unwrap_unchecked, :97)
    CHECK_ARG(data != nullptr && n <= 0x7FFFFFFF);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    std::unique_ptr<rlnc_recoder> r;
    if ((st = new_object(ctx, "recoder", r))) return st;
    r->k = k;
    r->n = n;
    r->full = full;
    r->stride = round16(full);
    if ((st = ctx->obj_alloc(n * r->stride, &r->pieces, &r->pieces_cap))) return st;
    Lease ws(ctx);
    if ((st = ws.acquire())) return st;
    if (full % 16 == 0 && full <= kPieceMaxBytes && n * full <= kGridUploadMax &&
        piece_eligible(r->pieces, r->stride, full)) {
        // small objects: staged through the lease's pinned buffer and copied by a kernel on the recode call's grid, so
        // the recode calls that follow find the pieces in the reading XCDs' L2 (piece.hip piece_upload_kernel;
        // against the DMA: profiles/r06_grid_upload_ab.txt)
        if ((st = ws->pc_coef.ensure(n * full))) return st;
        std::memcpy(ws->pc_coef.p, data, n * full);
        HIP_TRY(rlnc::launch_piece_upload(ws->pc_coef.as<uint8_t>(), int64_t(full), r->pieces, int64_t(r->stride),
                                          int64_t(full), int(n), ws->stream));
    } else {
        HIP_TRY(hipMemcpy2DAsync(r->pieces, r->stride, data, full, full, n, hipMemcpyHostToDevice, ws->stream));
    }
    HIP_TRY(hipStreamSynchronize(ws->stream));
    *out = r.release();
    return RLNC_OK;
}

// #[derive(Clone)] (recoder.rs:12)
int rlnc_recoder_clone(const rlnc_recoder *r, rlnc_recoder **out) {
    CHECK_ARG(r != nullptr && out != nullptr);
    *out = nullptr;
    int st = r->ctx->activate();
    if (st) return st;
    std::unique_ptr<rlnc_recoder> c;
    if ((st = new_object(r->ctx, "recoder", c))) return st;
    c->k = r->k;
    c->n = r->n;
    c->full = r->full;
    c->stride = r->stride;
    if ((st = r->ctx->obj_alloc(r->n * r->stride, &c->pieces, &c->pieces_cap))) return st;
    Lease ws(r->ctx);
    if ((st = ws.acquire())) return st;
    HIP_TRY(hipMemcpyAsync(c->pieces, r->pieces, r->n * r->stride, hipMemcpyDeviceToDevice, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    *out = c.release();
    return RLNC_OK;
}

void rlnc_recoder_free(rlnc_recoder *r) { delete r; }
size_t rlnc_recoder_get_original_num_pieces_coded_together(const rlnc_recoder *r) { return r ? r->k : 0; }
size_t rlnc_recoder_get_num_pieces_recoded_together(const rlnc_recoder *r) { return r ? r->n : 0; }
size_t rlnc_recoder_get_piece_byte_len(const rlnc_recoder *r) { return r ? r->full - r->k : 0; }
size_t rlnc_recoder_get_full_coded_piece_byte_len(const rlnc_recoder *r) { return r ? r->full : 0; }

// recoded piece = Σ_i r_i · (coeffs_i ‖ data_i): the coefficient fold of recoder.rs:133-144 and the data combination of
// :146-150 are the same linear map applied to different columns
int rlnc_recoder_recode_with_buf(rlnc_recoder *r, const uint8_t *rnd, size_t n_rnd, uint8_t *full, size_t full_len) {
    CHECK_ARG(r != nullptr);
    if (full_len != r->full) return RLNC_ERR_INVALID_OUTPUT_BUFFER;  // recoder.rs:123-125
    if (n_rnd != r->n) return RLNC_ERR_CODING_VECTOR_LENGTH_MISMATCH;  // fill_bytes fills exactly n bytes
    CHECK_ARG(rnd != nullptr && full != nullptr);
    // the received pieces are immutable after Recoder::new: no ordering
    return one_row_product(r->ctx, r->pieces, r->stride, r->n, r->full, rnd, full, false);
}

int rlnc_recoder_recode_batch_device(rlnc_recoder *r, const uint8_t *r_dev, size_t count, uint8_t *out_dev) {
    CHECK_ARG(r != nullptr);
    if (count == 0) return RLNC_OK;
    CHECK_ARG(r_dev != nullptr && out_dev != nullptr && count <= 0x7FFFFFFF);
    int st = r->ctx->activate();
    if (st || (st = r->ctx->note_capture())) return st;
    if ((st = r->ctx->matmul(product_params(r->pieces, 0, r->stride, r->n, r->full, r_dev, count, out_dev, 0, r->full, 1))))
        return st;
    return r->use.note(r->ctx->stream);
}

// ------------------------------------------------------------------------------------------------------
// Decoder — decoder.rs
// ------------------------------------------------------------------------------------------------------
int rlnc_decoder_new(rlnc_context *ctx, size_t L, size_t k, rlnc_decoder **out) {
    CHECK_ARG(ctx != nullptr && out != nullptr);
    *out = nullptr;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;  // decoder.rs:66-68
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;   // :69-71
    CHECK_ARG(k <= 0x7FFFFFFF);
    std::unique_ptr<rlnc_decoder> d;
    if (int st = new_object(ctx, "decoder", d)) return st;
    d->k = k;
    d->L = L;
    d->stride = round16(L);
    d->rank_mode = ctx->rank_mode;
    d->elim.reset(new (std::nothrow) Elimination(k, 0, d->rank_mode));
    if (!d->elim) return set_error(RLNC_ERR_OUT_OF_MEMORY, "decoder allocation");
    *out = d.release();
    return RLNC_OK;
}

// #[derive(Clone)] (decoder.rs:8): elimination state, counters and the stored data rows
int rlnc_decoder_clone(const rlnc_decoder *d, rlnc_decoder **out) {
    CHECK_ARG(d != nullptr && out != nullptr);
    *out = nullptr;
    int st = d->ctx->activate();
    if (st) return st;
    std::unique_ptr<rlnc_decoder> c;
    if ((st = new_object(d->ctx, "decoder", c))) return st;
    c->k = d->k;
    c->L = d->L;
    c->stride = d->stride;
    c->received = d->received;
    c->useful = d->useful;
    c->rank_mode = d->rank_mode;
    c->elim.reset(new (std::nothrow) Elimination(*d->elim));
    if (!c->elim) return set_error(RLNC_ERR_OUT_OF_MEMORY, "decoder allocation");
    if (d->store_slots) {
        if ((st = d->ctx->obj_alloc(d->store_slots * d->stride, &c->store, &c->store_cap))) return st;
        c->store_slots = d->store_slots;
        Lease ws(d->ctx);
        if ((st = ws.acquire()) || (st = d->order(ws->stream))) return st;
        HIP_TRY(hipMemcpyAsync(c->store, d->store, d->store_slots * d->stride, hipMemcpyDeviceToDevice, ws->stream));
        HIP_TRY(hipStreamSynchronize(ws->stream));
    }
    *out = c.release();
    return RLNC_OK;
}

void rlnc_decoder_free(rlnc_decoder *d) { delete d; }

int rlnc_decoder_get_rank_mode(const rlnc_decoder *d) { return d ? d->rank_mode : -1; }

// The store's block holds at least `slots` rows: a larger one takes over the rows stored so far, copied on s before
// the old block is returned.  staged: host pieces may still be staged for the old block (Decoder::decode), so they are
// flushed ahead of the copy.
static int decoder_store_reserve(rlnc_decoder *d, hipStream_t s, size_t slots, bool staged) {
    if (slots * d->stride <= d->store_cap) return RLNC_OK;
    uint8_t *n = nullptr;
    size_t cap = 0;
    if (int st = d->ctx->obj_alloc(slots * d->stride, &n, &cap)) return st;
    if (staged)
        if (int st = d->order(s)) return st;
    if (d->store) {
        HIP_TRY(hipMemcpyAsync(n, d->store, d->store_slots * d->stride, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        d->ctx->obj_free(d->store, d->store_cap, nullptr);
    }
    d->store = n;
    d->store_cap = cap;
    return RLNC_OK;
}

// s: the stream of the row copy (host pieces: the context's upload stream, where a store reallocation then also runs)
static int decoder_store_slot(rlnc_decoder *d, hipStream_t s, int slot, const uint8_t *src, hipMemcpyKind kind) {
    // device pieces: the row copy on s follows the decoder's staged host uploads (a host piece's upload runs on the
    // upload stream itself, behind every earlier one: no flush of the open ring slot per call)
    if (kind != hipMemcpyHostToDevice)
        if (int st = d->order(s)) return st;
    if (size_t(slot) >= d->store_slots) {
        const size_t ns = std::max(d->elim->slots(), size_t(slot) + 1);
        if (int st = decoder_store_reserve(d, s, ns, kind == hipMemcpyHostToDevice)) return st;
        d->store_slots = ns;
    }
    uint8_t *row = d->store + size_t(slot) * d->stride;
    if (kind == hipMemcpyHostToDevice)
        // staged through pinned memory: the caller may reuse the piece when the call returns, no synchronisation
        // (a pageable copy's cost 30 us per call for small pieces)
        return d->ctx->upload(row, src, d->L, d->stride, &d->up);
    HIP_TRY(hipMemcpyAsync(row, src, d->L, kind, s));
    HIP_TRY(hipStreamSynchronize(s));  // the caller may reuse the piece; the call is synchronous
    return RLNC_OK;
}

static int decoder_decode_impl(rlnc_decoder *d, hipStream_t s, const uint8_t *coeffs_host, const uint8_t *data,
                               hipMemcpyKind kind) {
    int slot = -1;
    bool keep = false;
    const int st = d->elim->push(coeffs_host, &slot, &keep);
    if (st == RLNC_ERR_RECEIVED_ALL_PIECES) return st;
    d->received += 1;                                     // decoder.rs:107
    if (st == RLNC_OK) d->useful = d->elim->rank();       // :115
    if (keep)
        if (int s2 = decoder_store_slot(d, s, slot, data, kind)) return s2;
    return st;
}

int rlnc_decoder_decode(rlnc_decoder *d, const uint8_t *piece, size_t len) {
    CHECK_ARG(d != nullptr);
    if (d->elim->decoded()) return RLNC_ERR_RECEIVED_ALL_PIECES;  // decoder.rs:97-99
    if (len != d->k + d->L) return RLNC_ERR_INVALID_PIECE_LENGTH; // :100-102
    CHECK_ARG(piece != nullptr);
    int st = d->ctx->activate();
    if (st) return st;
    hipStream_t s = nullptr;  // no call workspace: the piece goes through the context's upload ring
    if ((st = d->ctx->upload_stream(s))) return st;
    return decoder_decode_impl(d, s, piece, piece + d->k, hipMemcpyHostToDevice);
}

int rlnc_decoder_decode_device(rlnc_decoder *d, const uint8_t *piece_dev, size_t len) {
    CHECK_ARG(d != nullptr);
    if (d->elim->decoded()) return RLNC_ERR_RECEIVED_ALL_PIECES;
    if (len != d->k + d->L) return RLNC_ERR_INVALID_PIECE_LENGTH;
    CHECK_ARG(piece_dev != nullptr);
    int st = d->ctx->activate();
    if (st) return st;
    Lease ws(d->ctx);
    if ((st = ws.acquire()) || (st = ws->pin_c.ensure(d->k))) return st;
    HIP_TRY(hipMemcpyAsync(ws->pin_c.p, piece_dev, d->k, hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    std::vector<uint8_t> coeffs(ws->pin_c.as<uint8_t>(), ws->pin_c.as<uint8_t>() + d->k);
    return decoder_decode_impl(d, ws->stream, coeffs.data(), piece_dev + d->k, hipMemcpyDeviceToDevice);
}

int rlnc_decoder_is_already_decoded(const rlnc_decoder *d) { return d && d->elim->decoded() ? 1 : 0; }
size_t rlnc_decoder_get_num_pieces_coded_together(const rlnc_decoder *d) { return d ? d->k : 0; }
size_t rlnc_decoder_get_piece_byte_len(const rlnc_decoder *d) { return d ? d->L : 0; }
size_t rlnc_decoder_get_full_coded_piece_byte_len(const rlnc_decoder *d) { return d ? d->k + d->L : 0; }
size_t rlnc_decoder_get_received_piece_count(const rlnc_decoder *d) { return d ? d->received : 0; }
size_t rlnc_decoder_get_useful_piece_count(const rlnc_decoder *d) { return d ? d->useful : 0; }
size_t rlnc_decoder_get_remaining_piece_count(const rlnc_decoder *d) { return d ? d->k - d->useful : 0; }

// the store holds (at least) `slots` rows, on stream s (after the decoder's uploads); rows never stored are zeroed
// when `clear`
static int decoder_store_rows(rlnc_decoder *d, hipStream_t s, size_t slots, bool clear) {
    if (d->store_slots >= slots) return RLNC_OK;
    if (int st = decoder_store_reserve(d, s, slots, false)) return st;
    if (clear) HIP_TRY(hipMemsetAsync(d->store + d->store_slots * d->stride, 0, (slots - d->store_slots) * d->stride, s));
    d->store_slots = slots;
    return RLNC_OK;
}

// decoded rows = T × stored data rows, written to out_dev [k][L] on the lease's stream
static int decoder_apply(rlnc_decoder *d, CallWs *ws, uint8_t *out_dev) {
    const size_t slots = d->elim->slots();
    int st;
    if ((st = d->order(ws->stream))) return st;
    if ((st = ws->pin_b.ensure(d->k * slots)) || (st = ws->coef.ensure(d->k * slots))) return st;
    d->elim->transform(ws->pin_b.as<uint8_t>(), slots);
    HIP_TRY(hipMemcpyAsync(ws->coef.p, ws->pin_b.p, d->k * slots, hipMemcpyHostToDevice, ws->stream));
    // slots never stored were never referenced; give them zero rows so T × D is well defined
    if ((st = decoder_store_rows(d, ws->stream, slots, true))) return st;
    const auto p = product_params(d->store, 0, d->stride, slots, d->L, ws->coef.as<uint8_t>(), d->k, out_dev, 0, d->L, 1);
    return d->ctx->matmul(p, ws->stream, ws->idx, false);
}

int rlnc_decoder_get_decoded_data(rlnc_decoder *d, uint8_t *out, size_t cap, size_t *out_len) {
    CHECK_ARG(d != nullptr);
    if (!d->elim->decoded()) return RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET;  // decoder.rs:137-139
    CHECK_ARG(out != nullptr && out_len != nullptr && cap >= d->k * d->L);
    int st = d->ctx->activate();
    if (st) return st;
    Lease ws(d->ctx);
    const size_t slots = d->elim->slots();
    if (d->k * round16(d->L) <= kPieceMaxBytes && d->k * slots * d->L <= kPieceDecodeMaxMacs &&
        piece_eligible(d->store, d->stride, d->L)) {
        // T (k x slots) is read by the kernel from pinned memory and the rows land in pinned memory, copied into out
        // chunk by chunk as the device finishes them.  Store rows never stored are referenced by zero columns of T
        // only (0 · x = 0 for whatever they hold), so they need to exist, not to be cleared.
        if ((st = ws.acquire(false)) || (st = d->order(ws->stream))) return st;
        if ((st = decoder_store_rows(d, ws->stream, slots, false))) return st;
        if ((st = ws->pc_coef.ensure(d->k * slots))) return st;
        d->elim->transform(ws->pc_coef.as<uint8_t>(), slots);
        if ((st = piece_call(ws.ws.get(), d->store, d->stride, slots, d->L, ws->pc_coef.as<uint8_t>(), slots, d->k, out,
                             d->L)))
            return st;
    } else {
        if ((st = ws.acquire()) || (st = ws->out.ensure(d->k * d->L))) return st;
        if ((st = decoder_apply(d, ws.ws.get(), ws->out.as<uint8_t>()))) return st;
        if ((st = copy_out(ws.ws.get(), out, ws->out.as<uint8_t>(), d->k * d->L))) return st;
    }
    // get_final_data_len — decoder.rs:162-177: last nonzero byte must be the 0x81 marker, not at 0
    size_t n = d->k * d->L;
    while (n > 0 && out[n - 1] == 0) --n;
    if (n == 0 || out[n - 1] != rlnc::kBoundaryMarker || n - 1 == 0) return RLNC_ERR_INVALID_DECODED_DATA_FORMAT;
    *out_len = n - 1;
    return RLNC_OK;
}

int rlnc_decoder_get_decoded_data_device(rlnc_decoder *d, uint8_t *out_dev, size_t cap, size_t *out_len) {
    CHECK_ARG(d != nullptr);
    if (!d->elim->decoded()) return RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET;
    CHECK_ARG(out_dev != nullptr && out_len != nullptr && cap >= d->k * d->L);
    int st = d->ctx->activate();
    if (st) return st;
    Lease ws(d->ctx);
    if ((st = ws.acquire())) return st;
    if ((st = decoder_apply(d, ws.ws.get(), out_dev))) return st;
    if ((st = ws->status.ensure(4)) || (st = ws->len.ensure(8)) || (st = ws->pin_c.ensure(16))) return st;
    HIP_TRY(rlnc::launch_final_data_len(out_dev, 0, int64_t(d->k * d->L), 1, ws->status.as<int32_t>(),
                                        ws->len.as<int64_t>(), RLNC_ERR_INVALID_DECODED_DATA_FORMAT, ws->stream));
    int32_t status = 0;
    uint64_t len = 0;
    if ((st = read_results(ws->pin_c.as<uint8_t>(), ws->stream, 1, ws->status.p, ws->len.p, nullptr, 0, &status, &len,
                           nullptr)))
        return st;
    if (status) return status;
    *out_len = size_t(len);
    return RLNC_OK;
}

}  // extern "C"
