// batch.cpp — the stream-ordered batch API of librlnc_hip (include/rlnc_hip.h): encode, recode and decode of many
// objects per launch on the context stream, the registry of block-address streams written ahead for a product
// (the *_prepare / *_planned pairs), and the decode's device and host implementations.
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "context.hpp"
#include "elimination.hpp"

using rlnc::Elimination;
using namespace rlnc::eng;

namespace {

// coded pieces [nobj][n][k + L] of sources [nobj][k][L]: the data side, and the coefficient headers when `headers`
rlnc::MatmulParams encode_batch_params(const uint8_t *src, size_t k, size_t L, size_t nobj, const uint8_t *coeffs,
                                       size_t n, uint8_t *pieces, bool headers) {
    const size_t full = k + L;
    rlnc::MatmulParams p = product_params(src, k * L, L, k, L, coeffs, n, pieces + k, n * full, full, nobj);
    p.hdr = headers ? pieces : nullptr;
    p.hdr_obj = int64_t(n * full);
    p.hdr_row = int64_t(full);
    return p;
}

// The decode's data side: decoded [nobj][k][L] = T [nobj][k][m] × the received pieces' data
rlnc::MatmulParams decode_apply_params(const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                                       size_t nobj, const uint8_t *T, uint8_t *decoded) {
    return product_params(pieces + k, obj_stride, k + L, m, L, T, k, decoded, k * L, L, nobj);
}

// Block-address streams written ahead by rlnc_encode_batch_prepare (any context, any stream), by buffer: the product
// they were written for and their layout.  rlnc_encode_batch_data_planned uses one only for exactly that product.
// The decode's data side has the same pair (rlnc_decode_batch_apply_prepare / _planned): kind 1, with src = the
// received pieces, coeffs = T, out = the decoded output, n = m and the pieces' object stride.
struct PlanKey {
    int kind;  // 0 encode, 1 decode apply
    int device, variant;
    const uint8_t *src, *coeffs, *out;
    size_t k, L, nobj, n, obj_stride;
    auto tie() const { return std::tie(kind, device, variant, src, coeffs, out, k, L, nobj, n, obj_stride); }
    bool operator==(const PlanKey &o) const { return tie() == o.tie(); }
};
struct PlanRec {
    PlanKey key;
    rlnc::BsjStreamPlan plan;
};
std::mutex g_plan_mu;
std::vector<std::pair<const void *, PlanRec>> g_plans;  // (buffer, record), most recent last
constexpr size_t kPlanRecs = 64;

void remember_plan(const void *buf, const PlanRec &rec) {
    std::lock_guard<std::mutex> lock(g_plan_mu);
    for (auto it = g_plans.begin(); it != g_plans.end(); ++it)
        if (it->first == buf) {
            g_plans.erase(it);
            break;
        }
    if (g_plans.size() >= kPlanRecs) g_plans.erase(g_plans.begin());
    g_plans.emplace_back(buf, rec);
}

bool find_plan(const void *buf, PlanRec *rec) {
    std::lock_guard<std::mutex> lock(g_plan_mu);
    for (auto it = g_plans.rbegin(); it != g_plans.rend(); ++it)
        if (it->first == buf) {
            *rec = it->second;
            return true;
        }
    return false;
}

// write product p's stream into plan_buf on the context stream and record it under key
int plan_prepare(rlnc_context *ctx, const PlanKey &key, const rlnc::MatmulParams &p, void *plan_buf,
                 size_t plan_bytes) {
    PlanRec rec{key, {}};
    // the row-split tuning knob launches per row range, each with its own stream: nothing to write ahead
    if (!(ctx->max_tile_rows > 0 && p.n_out > ctx->max_tile_rows))
        HIP_TRY(rlnc::launch_bsj_stream(p, ctx->variant, ctx->stream, plan_buf, plan_bytes, rec.plan));
    remember_plan(plan_buf, rec);
    return RLNC_OK;
}

// attach the stream in plan_buf to p if it was prepared for exactly the product of key, else InvalidArgument
int plan_check(const PlanKey &key, const void *plan_buf, rlnc::MatmulParams &p) {
    PlanRec rec{};
    if (!find_plan(plan_buf, &rec) || !(rec.key == key))
        return set_error(RLNC_ERR_INVALID_ARGUMENT,
                         "%s plan %p was not prepared for this product (same buffers, shape, device and kernel "
                         "variant): call %s with the arguments of this call",
                         key.kind ? "decode" : "encode", plan_buf,
                         key.kind ? "rlnc_decode_batch_apply_prepare" : "rlnc_encode_batch_prepare");
    if (rec.plan.tile_rows > 0) {
        p.bsj_stream = plan_buf;
        p.bsj_stream_rows = rec.plan.tile_rows;
        p.bsj_stream_abs = rec.plan.abs;
    }
    return RLNC_OK;
}

PlanKey encode_plan_key(const rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj,
                        const uint8_t *coeffs, size_t n, const uint8_t *pieces) {
    return PlanKey{0, ctx->device, int(ctx->variant), src, coeffs, pieces, k, L, nobj, n, 0};
}

PlanKey decode_plan_key(const rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L,
                        size_t m, size_t nobj, const uint8_t *T, const uint8_t *decoded) {
    return PlanKey{1, ctx->device, int(ctx->variant), pieces, T, decoded, k, L, nobj, m, obj_stride};
}

int encode_batch_impl(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj, const uint8_t *coeffs,
                      size_t n, uint8_t *pieces, bool headers, const void *plan_buf = nullptr) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(src && coeffs && pieces && n <= 0x7FFFFFFF && k <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    rlnc::MatmulParams p = encode_batch_params(src, k, L, nobj, coeffs, n, pieces, headers);
    if (plan_buf)
        if ((st = plan_check(encode_plan_key(ctx, src, k, L, nobj, coeffs, n, pieces), plan_buf, p))) return st;
    return ctx->matmul(p);
}

// Device path: exact elimination on the device (rref.hip) → T × data (one matmul) → marker scan.
// Everything is enqueued on the context stream; outputs stay on the device.
// The elimination alone: reads only the k coefficient bytes of each piece; writes T [obj][k][m], the per-piece
// statuses and the ranks.
// tail (optional, with bsj): the small-object elimination also answers get_final_data_len from the payload tail
// (RrefParams::tail_status): {status, length, need-scan flags} device arrays
struct TailOut {
    int32_t *status = nullptr;
    int64_t *len = nullptr;
    int32_t *need = nullptr;
};

int decode_eliminate_impl(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                          size_t nobj, uint8_t *T, int32_t *pstat_dev, int32_t *rank_dev, uint32_t *bsj = nullptr,
                          int bsj_rows = 0, bool *bsj_written = nullptr, const TailOut *tail = nullptr) {
    const size_t full = k + L;
    rlnc::RrefParams rp{};
    rp.pieces = pieces;
    rp.obj_stride = int64_t(obj_stride);
    rp.piece_stride = int64_t(full);
    rp.k = int(k);
    rp.m = int(m);
    rp.n_obj = int(nobj);
    rp.T = T;
    rp.T_obj = int64_t(k * m);
    rp.status = pstat_dev;
    rp.rank = rank_dev;
    if (ctx->rank_mode == RLNC_RANK_MODE_TRUE) {  // the true-rank producer (rank.hip): no stream, no tail
        if (bsj_written) *bsj_written = false;
        if (int st = ctx->rank_mode_path_check()) return st;
        if (ctx->elim_large(k, m)) {  // paths 7 / 8: the state in a workspace, 3·ceil(m / B) + 1 launches (rank_large.hip)
            if (int st = rlnc_context::large_shape_check(k, m)) return st;
            const size_t need = rlnc::rank_large_workspace_bytes(k, m, nobj);
            if (int st = ctx->grow(ctx->ws_large, need)) return st;
            HIP_TRY(rlnc::launch_rank_large(rp, ctx->ws_large.p, ctx->ws_large.cap, ctx->stream));
            return RLNC_OK;
        }
        HIP_TRY(rlnc::launch_rank_batch(rp, ctx->stream));
        return RLNC_OK;
    }
    if (int st = ctx->rank_mode_path_check()) return st;  // paths 7 and 8 in mode 0
    rp.block_only = ctx->decode_path == 5 ? 1 : 0;
    if (ctx->decode_path == 5 && !rlnc::rref_block_eligible(int(k), int(m)))  // no silent fallback to another kernel
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "decode path 5 (blocked run) needs k + m <= 256 (k=%zu, m=%zu)", k, m);
    rp.bsj_stream = bsj;
    rp.bsj_block_bytes = rlnc::bsj_block_bytes();
    rp.bsj_tile_rows = bsj_rows;
    if (tail != nullptr) {
        rp.tail_status = tail->status;
        rp.tail_len = tail->len;
        rp.tail_need = tail->need;
        rp.tail_L = int64_t(L);
    }
    HIP_TRY(rlnc::launch_rref_batch(rp, ctx->stream, bsj_written));
    return RLNC_OK;
}

// The data side: product p (decode_apply_params, with its block-address stream if one was written), then the marker
// scan (decoder.rs:136-177).
int decode_apply_impl(rlnc_context *ctx, rlnc::MatmulParams p, size_t k, size_t L, size_t nobj,
                      const int32_t *rank_dev, int32_t *ostat_dev, int64_t *len_dev,
                      const int32_t *need_dev = nullptr) {
    // need_dev: the elimination already wrote every object's status and length from its payload tail; the objects
    // whose tail was all zero are scanned by their product workgroup when each object is one tile (configs[0]'s shape),
    // else the scan kernel runs over all of them
    bool scanned = false;
    if (need_dev != nullptr) {
        p.scan_status = ostat_dev;
        p.scan_need = need_dev;
        p.scan_len = len_dev;
        p.scan_k = int(k);
        p.scan_done = &scanned;
    }
    if (int st = ctx->matmul(p)) return st;
    if (!scanned)
        HIP_TRY(rlnc::launch_final_data_len_ranked(p.out, int64_t(k * L), int64_t(k * L), int(nobj), int(k), rank_dev,
                                                   ostat_dev, len_dev, ctx->stream));
    return RLNC_OK;
}

int decode_batch_device_impl(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                             size_t nobj, uint8_t *decoded, int32_t *pstat_dev, int32_t *ostat_dev, int64_t *len_dev,
                             int32_t *rank_dev) {
    int st;
    if ((st = ctx->grow(ctx->ws_coef, nobj * k * m))) return st;
    uint8_t *T = ctx->ws_coef.as<uint8_t>();
    // (Eliminating the later objects on a second stream beside the first objects' T x data product measured slower:
    // 8.3-8.6 ms against 7.99 for configs[4]'s 512 objects -- the concurrent elimination slows the product more
    // than it hides; profiles/r02_decode_pipeline_ab.txt.)
    // small objects (the one-wave elimination kernel, products in the 1- or 2-wave bit-sliced program): the elimination
    // also writes the product's block-offset stream, so the product needs no offset launch (configs[0] shape: -6 us)
    const int bsj_rows = rlnc::bsj_unshared_tile_rows(int(k));
    uint32_t *bsj = nullptr;
    if (bsj_rows > 0) {
        if ((st = ctx->grow(ctx->ws_bsj, nobj * m * size_t(bsj_rows) * 4 + 512))) return st;
        bsj = ctx->ws_bsj.as<uint32_t>();
    }
    // one-tile objects (k <= 16 x one 4 KiB column block): the elimination answers the marker scan from the payload
    // tail and the product's workgroups scan the rare all-zero tails (no scan launch: configs[0] shape; against the
    // separate scan launch: profiles/r05_tail_scan_ab.jsonl)
    TailOut tail;
    const bool want_tail = bsj != nullptr && L == 4096 && k % 4 == 0 && obj_stride % 4 == 0 &&
                           reinterpret_cast<uintptr_t>(pieces) % 4 == 0;
    if (want_tail) {
        if ((st = ctx->grow(ctx->ws_need, nobj * 4))) return st;
        tail.status = ostat_dev;
        tail.len = len_dev;
        tail.need = ctx->ws_need.as<int32_t>();
    }
    bool written = false;
    if ((st = decode_eliminate_impl(ctx, pieces, obj_stride, k, L, m, nobj, T, pstat_dev, rank_dev, bsj, bsj_rows,
                                    &written, want_tail ? &tail : nullptr)))
        return st;
    rlnc::MatmulParams p = decode_apply_params(pieces, obj_stride, k, L, m, nobj, T, decoded);
    if (written) {
        p.bsj_stream = bsj;
        p.bsj_stream_rows = bsj_rows;
    }
    return decode_apply_impl(ctx, p, k, L, nobj, rank_dev, ostat_dev, len_dev,
                             written && want_tail ? tail.need : nullptr);
}

// Host path (matrices too large for LDS): exact elimination on host threads (elimination.hpp).
int decode_batch_host_impl(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                           size_t nobj, uint8_t *decoded, int32_t *piece_status, int32_t *object_status,
                           uint64_t *data_len) {
    const size_t full = k + L;
    int st;
    // 1. coefficient headers → host (k bytes of each piece)
    if ((st = ctx->grow(ctx->pin_a, nobj * m * k))) return st;
    uint8_t *hdr = ctx->pin_a.as<uint8_t>();
    if (obj_stride == m * full) {
        HIP_TRY(hipMemcpy2DAsync(hdr, k, pieces, full, k, nobj * m, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        for (size_t o = 0; o < nobj; ++o)
            HIP_TRY(hipMemcpy2DAsync(hdr + o * m * k, k, pieces + o * obj_stride, full, k, m, hipMemcpyDeviceToHost,
                                     ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // 2. exact incremental elimination per object (decoder.rs:96-118 for pieces 0..m-1), host threads
    if ((st = ctx->grow(ctx->pin_b, nobj * k * m))) return st;
    uint8_t *T = ctx->pin_b.as<uint8_t>();
    std::vector<int32_t> ranks(nobj, 0);
    std::vector<int32_t> pst(nobj * m, 0);
    auto work = [&](size_t o0, size_t o1) {
        for (size_t o = o0; o < o1; ++o) {
            Elimination e(k, m, ctx->rank_mode);
            for (size_t p = 0; p < m; ++p) {
                int slot;
                bool keep;
                pst[o * m + p] = e.push(hdr + (o * m + p) * k, &slot, &keep);
            }
            ranks[o] = int32_t(e.rank());
            std::memset(T + o * k * m, 0, k * m);
            e.transform(T + o * k * m, m);
        }
    };
    const size_t hw = std::max<unsigned>(1, std::thread::hardware_concurrency());
    const size_t nth = std::min<size_t>({nobj, hw, 16});
    if (nth <= 1) {
        work(0, nobj);
    } else {
        std::vector<std::thread> th;
        const size_t per = (nobj + nth - 1) / nth;
        for (size_t t = 0; t < nth; ++t) {
            const size_t a = t * per, b = std::min(nobj, a + per);
            if (a < b) th.emplace_back(work, a, b);
        }
        for (auto &t : th) t.join();
    }
    // 3. T → device, decoded = T × received data rows (one launch for all objects), get_final_data_len on the device
    // (decoder.rs:162-177)
    if ((st = ctx->grow(ctx->ws_coef, nobj * k * m)) || (st = ctx->grow(ctx->ws_rank, nobj * 4)) ||
        (st = ctx->grow(ctx->ws_status, nobj * 4)) ||
        (st = ctx->grow(ctx->ws_len, nobj * 8)) || (st = ctx->grow(ctx->pin_c, nobj * 16)))
        return st;
    HIP_TRY(hipMemcpyAsync(ctx->ws_coef.p, T, nobj * k * m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->ws_rank.p, ranks.data(), nobj * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((st = decode_apply_impl(ctx, decode_apply_params(pieces, obj_stride, k, L, m, nobj, ctx->ws_coef.as<uint8_t>(), decoded),
                                k, L, nobj, ctx->ws_rank.as<int32_t>(), ctx->ws_status.as<int32_t>(),
                                ctx->ws_len.as<int64_t>())))
        return st;
    if ((st = read_results(ctx->pin_c.as<uint8_t>(), ctx->stream, nobj, ctx->ws_status.p, ctx->ws_len.p, nullptr, 0,
                           object_status, data_len, nullptr)))
        return st;
    if (piece_status) std::memcpy(piece_status, pst.data(), nobj * m * sizeof(int32_t));
    return RLNC_OK;
}

int decode_batch_check(rlnc_context *ctx, const uint8_t *pieces, size_t &obj_stride, size_t k, size_t L, size_t m,
                       size_t nobj, uint8_t *decoded) {
    CHECK_ARG(ctx != nullptr);
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    CHECK_ARG(pieces && decoded && m > 0 && m <= 0x7FFFFFFF && k <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    if (obj_stride == 0) obj_stride = m * (k + L);
    CHECK_ARG(obj_stride >= m * (k + L));
    int st = ctx->activate();
    if (st) return st;
    return ctx->note_capture();
}

}  // namespace

extern "C" {

int rlnc_encode_batch(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj, const uint8_t *coeffs,
                      size_t n, uint8_t *pieces) {
    return encode_batch_impl(ctx, src, k, L, nobj, coeffs, n, pieces, true);
}

int rlnc_encode_batch_data(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj,
                           const uint8_t *coeffs, size_t n, uint8_t *pieces) {
    return encode_batch_impl(ctx, src, k, L, nobj, coeffs, n, pieces, false);
}

size_t rlnc_encode_batch_plan_bytes(size_t k, size_t nobj, size_t n) {
    if (k == 0 || n == 0 || nobj == 0 || k > 0x7FFFFFFF || n > 0x7FFFFFFF || nobj > 0x7FFFFFFF) return 0;
    return rlnc::bsj_stream_bytes_bound(int(nobj), int(n), int(k));
}

int rlnc_encode_batch_prepare(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj,
                              const uint8_t *coeffs, size_t n, uint8_t *pieces, void *plan_buf, size_t plan_bytes) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(src && coeffs && pieces && plan_buf && n <= 0x7FFFFFFF && k <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    CHECK_ARG(plan_bytes >= rlnc_encode_batch_plan_bytes(k, nobj, n));
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    return plan_prepare(ctx, encode_plan_key(ctx, src, k, L, nobj, coeffs, n, pieces),
                        encode_batch_params(src, k, L, nobj, coeffs, n, pieces, false), plan_buf, plan_bytes);
}

int rlnc_encode_batch_data_planned(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj,
                                   const uint8_t *coeffs, size_t n, uint8_t *pieces, const void *plan_buf) {
    CHECK_ARG(plan_buf != nullptr);
    return encode_batch_impl(ctx, src, k, L, nobj, coeffs, n, pieces, false, plan_buf);
}

int rlnc_encode_batch_headers(rlnc_context *ctx, const uint8_t *coeffs, size_t k, size_t L, size_t nobj, size_t n,
                              uint8_t *pieces) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(coeffs && pieces);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    // pieces[o][i][0..k) = coeffs[o][i] (encoder.rs:246-248): one strided copy (a kernel: the runtime's 2D
    // blit took 36 µs for 1,024 rows of 32 B)
    HIP_TRY(rlnc::launch_copy_rows(pieces, int64_t(k + L), coeffs, int64_t(k), int64_t(k), int64_t(n * nobj),
                                   ctx->stream));
    return RLNC_OK;
}

// recoded piece = Σ_i r_i · (coeffs_i ‖ data_i): the coefficient fold of recoder.rs:133-144 and the data combination of
// :146-150 are the same linear map applied to different columns
int rlnc_recode_batch(rlnc_context *ctx, const uint8_t *pieces, size_t k, size_t L, size_t n, size_t nobj,
                      const uint8_t *r, size_t count, uint8_t *out) {
    CHECK_ARG(ctx != nullptr);
    if (n == 0) return RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE;
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_TOO_SHORT;
    if (count == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(pieces && r && out && n <= 0x7FFFFFFF && count <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    const size_t full = k + L;
    return ctx->matmul(product_params(pieces, n * full, full, n, full, r, count, out, count * full, full, nobj));
}

// the sparse twins of rlnc_encode_batch and rlnc_recode_batch (sparse.hip): same checks in the same order, then the
// entries'
int rlnc_encode_batch_sparse(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t nobj, const int32_t *idx,
                             const uint8_t *val, size_t w, size_t n, uint8_t *pieces) {
    CHECK_ARG(ctx != nullptr);
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_ZERO;
    if (n == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(src && pieces && n <= 0x7FFFFFFF && k <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    CHECK_ARG(sparse_entries_ok(idx, val, w));
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    const size_t full = k + L;
    rlnc::SparseMatmulParams p =
        sparse_product_params(src, k * L, L, k, L, idx, val, w, n, pieces + k, n * full, full, nobj);
    p.hdr = pieces;
    p.hdr_obj = int64_t(n * full);
    p.hdr_row = int64_t(full);
    return ctx->sparse_matmul(p);
}

int rlnc_recode_batch_sparse(rlnc_context *ctx, const uint8_t *pieces, size_t k, size_t L, size_t n, size_t nobj,
                             const int32_t *idx, const uint8_t *val, size_t w, size_t count, uint8_t *out) {
    CHECK_ARG(ctx != nullptr);
    if (n == 0) return RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE;
    if (k == 0) return RLNC_ERR_PIECE_COUNT_ZERO;
    if (L == 0) return RLNC_ERR_PIECE_LENGTH_TOO_SHORT;
    if (count == 0 || nobj == 0) return RLNC_OK;
    CHECK_ARG(pieces && out && n <= 0x7FFFFFFF && count <= 0x7FFFFFFF && nobj <= 0x7FFFFFFF);
    CHECK_ARG(sparse_entries_ok(idx, val, w));
    int st = ctx->activate();
    if (st || (st = ctx->note_capture())) return st;
    const size_t full = k + L;
    return ctx->sparse_matmul(
        sparse_product_params(pieces, n * full, full, n, full, idx, val, w, count, out, count * full, full, nobj));
}

int rlnc_decode_batch(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                      size_t nobj, uint8_t *decoded, int32_t *piece_status, int32_t *object_status,
                      uint64_t *data_len) {
    if (nobj == 0 && ctx) return RLNC_OK;
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, decoded);
    if (st) return st;
    if ((st = ctx->rank_mode_path_check())) return st;
    const bool fits = ctx->elim_on_device(k, m);
    if (ctx->decode_path >= 2 && !fits)
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "device elimination forced but k=%zu, m=%zu exceed LDS", k, m);
    if (!fits || ctx->decode_path == 1)
        return decode_batch_host_impl(ctx, pieces, obj_stride, k, L, m, nobj, decoded, piece_status, object_status,
                                      data_len);
    if ((st = ctx->grow(ctx->ws_pstat, nobj * m * 4)) || (st = ctx->grow(ctx->ws_status, nobj * 4)) ||
        (st = ctx->grow(ctx->ws_len, nobj * 8)) || (st = ctx->grow(ctx->ws_rank, nobj * 4)) ||
        (st = ctx->grow(ctx->pin_c, nobj * (m * 4 + 16))))
        return st;
    if ((st = decode_batch_device_impl(ctx, pieces, obj_stride, k, L, m, nobj, decoded, ctx->ws_pstat.as<int32_t>(),
                                       ctx->ws_status.as<int32_t>(), ctx->ws_len.as<int64_t>(),
                                       ctx->ws_rank.as<int32_t>())))
        return st;
    return read_results(ctx->pin_c.as<uint8_t>(), ctx->stream, nobj, ctx->ws_status.p, ctx->ws_len.p, ctx->ws_pstat.p, m,
                        object_status, data_len, piece_status);
}

int rlnc_decode_batch_device(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                             size_t nobj, uint8_t *decoded, int32_t *piece_status_dev, int32_t *object_status_dev,
                             int64_t *data_len_dev) {
    if (nobj == 0 && ctx) return RLNC_OK;
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, decoded);
    if (st) return st;
    CHECK_ARG(piece_status_dev && object_status_dev && data_len_dev);
    if ((st = ctx->rank_mode_path_check())) return st;
    if (!ctx->elim_on_device(k, m))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "k=%zu, m=%zu exceed the device elimination's LDS budget; use "
                         "rlnc_decode_batch", k, m);
    if ((st = ctx->grow(ctx->ws_rank, nobj * 4))) return st;
    return decode_batch_device_impl(ctx, pieces, obj_stride, k, L, m, nobj, decoded, piece_status_dev,
                                    object_status_dev, data_len_dev, ctx->ws_rank.as<int32_t>());
}

int rlnc_decode_batch_eliminate(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L,
                                size_t m, size_t nobj, uint8_t *T_dev, int32_t *piece_status_dev, int32_t *rank_dev) {
    if (nobj == 0 && ctx) return RLNC_OK;
    CHECK_ARG(T_dev != nullptr);
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, T_dev);
    if (st) return st;
    CHECK_ARG(piece_status_dev && rank_dev);
    if ((st = ctx->rank_mode_path_check())) return st;
    if (!ctx->elim_on_device(k, m))
        return set_error(RLNC_ERR_INVALID_ARGUMENT, "k=%zu, m=%zu exceed the device elimination's LDS budget; use "
                         "rlnc_decode_batch", k, m);
    return decode_eliminate_impl(ctx, pieces, obj_stride, k, L, m, nobj, T_dev, piece_status_dev, rank_dev);
}

int rlnc_decode_batch_apply(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L, size_t m,
                            size_t nobj, const uint8_t *T_dev, const int32_t *rank_dev, uint8_t *decoded,
                            int32_t *object_status_dev, int64_t *data_len_dev) {
    if (nobj == 0 && ctx) return RLNC_OK;
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, decoded);
    if (st) return st;
    CHECK_ARG(T_dev && rank_dev && object_status_dev && data_len_dev);
    return decode_apply_impl(ctx, decode_apply_params(pieces, obj_stride, k, L, m, nobj, T_dev, decoded), k, L, nobj,
                             rank_dev, object_status_dev, data_len_dev);
}

size_t rlnc_decode_large_workspace_bytes(size_t k, size_t m, size_t nobj) {
    return rlnc::rank_large_workspace_bytes(k, m, nobj);
}

size_t rlnc_decode_batch_apply_plan_bytes(size_t k, size_t m, size_t nobj) {
    if (k == 0 || m == 0 || nobj == 0 || k > 0x7FFFFFFF || m > 0x7FFFFFFF || nobj > 0x7FFFFFFF) return 0;
    return rlnc::bsj_stream_bytes_bound(int(nobj), int(k), int(m));
}

int rlnc_decode_batch_apply_prepare(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L,
                                    size_t m, size_t nobj, const uint8_t *T_dev, uint8_t *decoded, void *plan_buf,
                                    size_t plan_bytes) {
    if (nobj == 0 && ctx) return RLNC_OK;
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, decoded);
    if (st) return st;
    CHECK_ARG(T_dev && plan_buf && plan_bytes >= rlnc_decode_batch_apply_plan_bytes(k, m, nobj));
    return plan_prepare(ctx, decode_plan_key(ctx, pieces, obj_stride, k, L, m, nobj, T_dev, decoded),
                        decode_apply_params(pieces, obj_stride, k, L, m, nobj, T_dev, decoded), plan_buf, plan_bytes);
}

int rlnc_decode_batch_apply_planned(rlnc_context *ctx, const uint8_t *pieces, size_t obj_stride, size_t k, size_t L,
                                    size_t m, size_t nobj, const uint8_t *T_dev, const int32_t *rank_dev,
                                    uint8_t *decoded, int32_t *object_status_dev, int64_t *data_len_dev,
                                    const void *plan_buf) {
    if (nobj == 0 && ctx) return RLNC_OK;
    int st = decode_batch_check(ctx, pieces, obj_stride, k, L, m, nobj, decoded);
    if (st) return st;
    CHECK_ARG(T_dev && rank_dev && object_status_dev && data_len_dev && plan_buf);
    rlnc::MatmulParams p = decode_apply_params(pieces, obj_stride, k, L, m, nobj, T_dev, decoded);
    if ((st = plan_check(decode_plan_key(ctx, pieces, obj_stride, k, L, m, nobj, T_dev, decoded), plan_buf, p)))
        return st;
    return decode_apply_impl(ctx, p, k, L, nobj, rank_dev, object_status_dev, data_len_dev);
}

}  // extern "C"
