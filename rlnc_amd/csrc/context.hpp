// context.hpp — librlnc_hip internals shared by the host sources (engine.cpp, piece_call.cpp, objects.cpp, batch.cpp,
// host_stream.cpp, host_copy.cpp) and wire.hip: error reporting, the environment reader and the phase trace, the
// grow-only device / pinned buffers, the per-call workspace pool, struct rlnc_context (include/rlnc_hip.h), the matmul
// parameter builder and the result readback.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/rlnc_hip.h"
#include "kernels.hpp"
#include "rank_kernels.hpp"
#include "rref.hpp"
#include "rank_large_kernels.hpp"
#include "sparse_kernels.hpp"

namespace rlnc::eng {

extern thread_local std::string g_last_error;

inline int set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            return ::rlnc::eng::set_error(e_ == hipErrorOutOfMemory ? RLNC_ERR_OUT_OF_MEMORY : RLNC_ERR_DEVICE, \
                                          "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                                          __LINE__);                                                     \
        }                                                                                                \
    } while (0)

#define CHECK_ARG(cond)                                                                                     \
    do {                                                                                                    \
        if (!(cond)) return ::rlnc::eng::set_error(RLNC_ERR_INVALID_ARGUMENT, "invalid argument: %s", #cond); \
    } while (0)

inline size_t round16(size_t v) { return (v + 15) & ~size_t(15); }

// the integer value of environment variable `name`, or dflt when it is unset (callers read once, into a static)
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

inline uint64_t now_ns() {
    return uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(
                        std::chrono::steady_clock::now().time_since_epoch()).count());
}

// A diagnostic switched on by environment variable `env` = 1 (read once; it selects no path): four host times per
// call, in us, and their medians through `fmt` (the call count, then the four) on stderr at exit.
struct PhaseTrace {
    const bool on;
    const char *const fmt;
    std::mutex mu;
    std::vector<float> v[4];
    PhaseTrace(const char *env, const char *f) : on(env_int(env, 0) != 0), fmt(f) {}
    void add(float a, float b, float c, float d) {
        std::lock_guard<std::mutex> lock(mu);
        v[0].push_back(a);
        v[1].push_back(b);
        v[2].push_back(c);
        v[3].push_back(d);
    }
    static float med(std::vector<float> &x) {
        std::nth_element(x.begin(), x.begin() + x.size() / 2, x.end());
        return x[x.size() / 2];
    }
    ~PhaseTrace() {
        if (on && !v[0].empty()) std::fprintf(stderr, fmt, v[0].size(), med(v[0]), med(v[1]), med(v[2]), med(v[3]));
    }
};

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return RLNC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        HIP_TRY(hipMalloc(&p, std::max<size_t>(bytes, 256)));
        cap = std::max<size_t>(bytes, 256);
        return RLNC_OK;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

// grow-only pinned host buffer
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;  // hipHostMallocCoherent: read / written by a running kernel
    int ensure(size_t bytes) {
        if (bytes <= cap) return RLNC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        HIP_TRY(hipHostMalloc(&p, std::max<size_t>(bytes, 256), flags));
        cap = std::max<size_t>(bytes, 256);
        return RLNC_OK;
    }
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};


// Workspace of one object-API call (Encoder/Recoder/Decoder on host buffers): its own stream, scratch and
// staging buffers, leased from the context's pool for the duration of the call.  Concurrent calls on one
// context (e.g. Encoder::code(&self) from many threads, encoder.rs:264 -- the reference type is Send + Sync)
// therefore never share a buffer.
struct CallWs {
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    DevBuf coef, out, idx, status, len;
    PinBuf pin_a, pin_b, pin_c;
    // the call-latency kernel (piece.hip): coefficients read and output rows written by the kernel in host memory,
    // per-chunk completion flags raised to the call's epoch, and the chunks' workgroup counters on the device
    PinBuf pc_coef, pc_out, pc_flag;
    DevBuf pc_count;
    size_t pc_count_words = 0;  // zeroed words of pc_count
    DevBuf pc_part, pc_pcount;  // split products (piece.hpp): partial slabs and per-block counters
    size_t pc_pcount_words = 0;  // zeroed words of pc_pcount
    uint32_t epoch = 0;
    // large copy-outs to host (Decoder::get_decoded_data): a ring of pinned chunks the DMA fills while host threads
    // copy the previous chunks into the caller's buffer (host_copy.cpp copy_out)
    static constexpr int kOutRing = 4;
    PinBuf pin_out;
    hipEvent_t out_ev[kOutRing] = {};
    CallWs() { pc_coef.flags = pc_out.flags = pc_flag.flags = hipHostMallocCoherent; }
    ~CallWs() {
        for (hipEvent_t e : out_ev)
            if (e) (void)hipEventDestroy(e);
        if (ev) (void)hipEventDestroy(ev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Staging ring of the object API's host -> device piece uploads (Decoder::decode): a call copies its piece into the
// open pinned slot and returns.  A slot collects pieces until it is full or one of its decoders needs its rows on the
// device; then it is flushed -- one DMA per run of consecutive store rows, queued on the context's one upload stream
// -- and its event recorded.  All DMAs run on that one stream, so a slot's event, whenever it was last recorded,
// follows every upload flushed before it.  Pieces larger than a slot take several.
struct UpRun {
    uint8_t *dst;
    size_t off, len;  // bytes [off, off + len) of the slot go to dst
};
struct UpSlot {
    PinBuf buf;
    hipEvent_t ev = nullptr;  // the slot's last flush (the slot may be rewritten once it has run)
    std::vector<UpRun> runs;  // staged, not yet flushed
    size_t used = 0;
    unsigned gen = 0;  // bumped each time the slot is reopened
    bool open = false;
    ~UpSlot() {
        if (ev) (void)hipEventDestroy(ev);
    }
};
// The stream-ordered uses of an object's device block (the *_batch_device calls, queued on whatever stream the
// context had then): the block may be reused by another object only after the last of them.  Synchronous uses (the
// object API on host buffers, the decoder's uploads) are complete when their call returns and need no record.
struct ObjUse {
    hipEvent_t ev = nullptr;  // recorded after the latest stream-ordered use, and after every earlier one
    hipStream_t last = nullptr;
    bool used = false;
    bool captured = false;  // a use inside a HIP graph capture: the graph may replay it at any time
    ~ObjUse() {
        if (ev) (void)hipEventDestroy(ev);
    }
    int note(hipStream_t s) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) {
            captured = true;
            return RLNC_OK;
        }
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        // a use on another stream than the previous one: the event re-recorded on s must still follow that earlier
        // use (it may run after this one), so s waits for the event's previous recording first
        if (used && s != last) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        HIP_TRY(hipEventRecord(ev, s));
        last = s;
        used = true;
        return RLNC_OK;
    }
};

constexpr int kUpSlots = 8;
constexpr size_t kUpChunk = size_t(4) << 20;
constexpr size_t kUpRuns = 256;  // runs per slot before it is flushed
// where a decoder's last piece was staged: ring slot and its generation then
struct UpTicket {
    int slot = -1;
    unsigned gen = 0;
};

}  // namespace rlnc::eng

using rlnc::eng::set_error;

struct rlnc_context {
    using DevBuf = rlnc::eng::DevBuf;
    using PinBuf = rlnc::eng::PinBuf;
    using CallWs = rlnc::eng::CallWs;
    std::atomic<int> refs{1};  // the creator's reference + one per Encoder/Decoder/Recoder bound to it
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    // variant 9 (static column runs, A/B build) is faster for an isolated encode launch but slower in the bench's
    // pipelined step, where static runs unbalance the tail (profiles/r17_persistent_bound.txt); variant 8's persistent
    // tiles (ws_claim below) remove the same prologue with run-time claims and are faster in both
    rlnc::MatmulVariant variant = rlnc::MatmulVariant::BitSlicedJumpShared8;
    int max_tile_rows = 0;
    int col_run = 0;  // column blocks per workgroup of variant 9 (0 = chosen per launch; rlnc_set_column_run)
    int decode_path = 0;  // 0 auto (device when it fits LDS), 1 host elimination, 2 device elimination,
                          // 5 blocked clean run, 7 device for every shape (rank mode 1: rank.hip where it fits LDS,
                          // rank_large.hip beyond), 8 rank_large.hip for every shape (3, 4, 6: retired, never set)
    int rank_mode = 0;  // RLNC_RANK_MODE_*: 0 the reference's diagonal-pivot replica, 1 true rank (rank.hip, elimination.hpp)
    int stream_form = 0;  // RLNC_STREAM_FORM_*: which kernels rlnc_decode_stream_push runs (decode_stream.cpp)
    // the device elimination of this context's rank mode fits LDS
    bool elim_fits(size_t k, size_t m) const {
        return (rank_mode == RLNC_RANK_MODE_TRUE ? rlnc::rank_lds_bytes(int(k), int(m)) : rlnc::rref_lds_bytes(int(k), int(m))) <=
               rlnc::kRrefMaxLds;
    }
    // the elimination of this shape runs in the workspace-resident true-rank kernels (rank_large.hip): path 8 always,
    // path 7 beyond LDS (rank mode 1 only: rank_mode_path_check refuses both paths in mode 0)
    bool elim_large(size_t k, size_t m) const {
        return decode_path == RLNC_DECODE_PATH_LARGE || (decode_path == RLNC_DECODE_PATH_DEVICE_ANY && !elim_fits(k, m));
    }
    // the elimination of this shape can run on the device
    bool elim_on_device(size_t k, size_t m) const { return elim_fits(k, m) || elim_large(k, m); }
    // decode path 5 names a reference-mode kernel, 7 and 8 true-rank kernels: no silent fallback in the other mode
    int rank_mode_path_check() const {
        const bool large = decode_path == RLNC_DECODE_PATH_DEVICE_ANY || decode_path == RLNC_DECODE_PATH_LARGE;
        if (rank_mode == RLNC_RANK_MODE_TRUE && decode_path >= 3 && !large)
            return set_error(RLNC_ERR_INVALID_ARGUMENT,
                             "decode path %d is a reference-mode kernel: rank mode 1 takes paths 0, 1, 2, 7 and 8",
                             decode_path);
        if (rank_mode != RLNC_RANK_MODE_TRUE && large)
            return set_error(RLNC_ERR_INVALID_ARGUMENT,
                             "decode path %d is a true-rank kernel: rank mode 0 takes paths 0, 1, 2 and 5", decode_path);
        return RLNC_OK;
    }
    // the shape limits of rank_large.hip, by name
    static int large_shape_check(size_t k, size_t m) {
        if (rlnc::large_block(int64_t(std::min<size_t>(k, 0x7FFFFFFF)), int64_t(std::min<size_t>(m, 0x7FFFFFFF))) == 0)
            return set_error(RLNC_ERR_INVALID_ARGUMENT,
                             "decode paths 7 and 8 take k <= %d and m <= %d beyond LDS (k=%zu, m=%zu)", rlnc::kLargeMaxK,
                             rlnc::kLargeMaxM, k, m);
        return RLNC_OK;
    }
    // workspaces of the stream-ordered batch / _device API (one caller thread per context at a time)
    DevBuf ws_bsj;   // the small-object decode's block-offset stream, written by its elimination
    DevBuf ws_need;  // ... and its per-object "payload tail all zero" flags (RrefParams::tail_need)
    DevBuf ws_coef, ws_out, ws_status, ws_len, ws_pstat, ws_rank, ws_idx;
    DevBuf ws_large;  // the state of the workspace-resident true-rank elimination (rank_large.hip)
    // the claim counters of the persistent 64-row product (kernels.hpp BsjPersist), zeroed once at creation.  One set
    // per context is enough: only the batch calls on the context's stream use it, two of them are ordered by that
    // stream, and each launch leaves the counters zero; contexts on other streams have their own.
    DevBuf ws_claim;
    int persist_mode = 0, persist_max_wgs = 0;  // rlnc_set_persistent_tiles
    PinBuf pin_a, pin_b, pin_c;
    // set once a batch call ran inside a HIP stream capture: the graph holds the workspace addresses, so
    // they must never move again (grow() refuses instead of reallocating)
    std::atomic<bool> graph_bound{false};
    std::mutex pool_mu;
    std::vector<std::unique_ptr<CallWs>> pool;
    // host-stream pipeline (host_stream.cpp): per-slot window buffers and the two copy streams, kept between calls.
    // Few streams on purpose: HIP multiplexes streams over GPU_MAX_HW_QUEUES (4) hardware queues, and a copy
    // stream sharing a queue with another stage serialises behind it.
    struct HsSlot {
        DevBuf din, dcoef, dout, dst;
        PinBuf hin, hout, hst;
    };
    std::vector<std::unique_ptr<HsSlot>> hs_slots;
    hipStream_t hs_h2d = nullptr, hs_d2h = nullptr;
    DevBuf ws_tab;  // descriptor tables of the wire-format / ragged calls (wire.hip), uploaded from pin_tab
    // a ring of pinned staging buffers, each with the event of its last upload (it may be rewritten once that has
    // run): a ragged decode stages three tables per call, and with one buffer its third upload waited on the host for
    // the second's copy, queued behind the whole elimination
    static constexpr int kTabRing = 4;
    PinBuf pin_tab[kTabRing];
    hipEvent_t tab_ev[kTabRing] = {};
    int tab_next = 0;
    // descriptor tables of calls captured into HIP graphs: bump-allocated, never reused or moved (a replay rewrites
    // exactly its captured bytes); reserved by eager calls, since nothing may be allocated inside a capture
    std::vector<std::unique_ptr<DevBuf>> cap_arenas;
    size_t cap_used = 0;
    rlnc::eng::UpSlot up[rlnc::eng::kUpSlots];
    int up_cur = 0;       // the slot being filled
    std::mutex up_mu;     // guards the ring and the upload stream
    hipStream_t up_stream = nullptr;
    // device blocks of dropped encoders / recoders / decoders, reused by the next object of a similar size: a
    // hipMalloc + hipFree pair costs 0.1-0.6 ms per object, as much as a small object's whole decode
    std::mutex blk_mu;
    std::vector<std::pair<size_t, void *>> blk;  // (bytes, block), oldest first
    size_t blk_bytes = 0;
    static constexpr size_t kBlkCacheBytes = size_t(1) << 30;
    static constexpr size_t kBlkCacheCount = 32;

    void retain() { refs.fetch_add(1, std::memory_order_relaxed); }
    void release() {
        if (refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (hipStream_t x : {hs_h2d, hs_d2h})
            if (x) {
                (void)hipStreamSynchronize(x);
                (void)hipStreamDestroy(x);
            }
        hs_slots.clear();
        if (up_stream) {
            (void)hipStreamSynchronize(up_stream);
            (void)hipStreamDestroy(up_stream);
        }
        for (auto &b : blk) (void)hipFree(b.second);
        for (hipEvent_t e : tab_ev)
            if (e) (void)hipEventDestroy(e);
        if (own) (void)hipStreamDestroy(own);
        delete this;  // the buffers' destructors free on this device
    }
    int activate() const {
        HIP_TRY(hipSetDevice(device));
        return RLNC_OK;
    }
    // batch API: note a stream capture in progress (freezes the workspaces)
    int note_capture() {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(stream, &cs));
        if (cs != hipStreamCaptureStatusNone) graph_bound = true;
        return RLNC_OK;
    }
    int grow(DevBuf &b, size_t bytes) {
        if (bytes <= b.cap) return RLNC_OK;
        if (graph_bound)
            return set_error(RLNC_ERR_INVALID_ARGUMENT,
                             "this context's workspaces are bound to a captured HIP graph and cannot grow to %zu "
                             "bytes: capture the largest shape first, or use another context",
                             bytes);
        return b.ensure(bytes);
    }
    int grow(PinBuf &b, size_t bytes) {
        if (bytes <= b.cap) return RLNC_OK;
        if (graph_bound)
            return set_error(RLNC_ERR_INVALID_ARGUMENT,
                             "this context's workspaces are bound to a captured HIP graph and cannot grow");
        return b.ensure(bytes);
    }
    // an object's device block of at least n bytes (*cap = its size): a cached one when one fits (at most twice n
    // plus 1 MiB), else hipMalloc -- after emptying the cache into the device if that fails
    int obj_alloc(size_t n, uint8_t **p, size_t *cap) {
        {
            std::lock_guard<std::mutex> lock(blk_mu);
            int best = -1;
            for (int i = 0; i < int(blk.size()); ++i)
                if (blk[i].first >= n && blk[i].first <= 2 * n + (size_t(1) << 20) &&
                    (best < 0 || blk[i].first < blk[best].first))
                    best = i;
            if (best >= 0) {
                *p = static_cast<uint8_t *>(blk[best].second);
                *cap = blk[best].first;
                blk_bytes -= *cap;
                blk.erase(blk.begin() + best);
                return RLNC_OK;
            }
        }
        const size_t bytes = std::max<size_t>(n, 256);
        if (hipMalloc(reinterpret_cast<void **>(p), bytes) != hipSuccess) {
            (void)hipGetLastError();
            {
                std::lock_guard<std::mutex> lock(blk_mu);
                for (auto &b : blk) (void)hipFree(b.second);
                blk.clear();
                blk_bytes = 0;
            }
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), bytes));
        }
        *cap = bytes;
        return RLNC_OK;
    }
    // return an object's block: once its stream-ordered uses (u; nullptr = none) have run it joins the cache; a block
    // a captured graph may still use is freed (hipFree waits for the device), as is a large one
    void obj_free(void *p, size_t cap, const rlnc::eng::ObjUse *u) {
        if (!p) return;
        if (cap > kBlkCacheBytes / 4 || (u && u->captured) || (u && u->used && hipEventSynchronize(u->ev) != hipSuccess)) {
            (void)hipFree(p);
            return;
        }
        std::lock_guard<std::mutex> lock(blk_mu);
        blk.emplace_back(cap, p);
        blk_bytes += cap;
        while (blk_bytes > kBlkCacheBytes || blk.size() > kBlkCacheCount) {
            (void)hipFree(blk.front().second);
            blk_bytes -= blk.front().first;
            blk.erase(blk.begin());
        }
    }
    int upload_stream_locked() {
        if (!up_stream) HIP_TRY(hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking));
        return RLNC_OK;
    }
    int upload_stream(hipStream_t &s) {
        std::lock_guard<std::mutex> lock(up_mu);
        if (int st = upload_stream_locked()) return st;
        s = up_stream;
        return RLNC_OK;
    }
    int upload_flush_locked(rlnc::eng::UpSlot &u) {
        if (!u.open) return RLNC_OK;
        u.open = false;
        for (const auto &r : u.runs)
            HIP_TRY(hipMemcpyAsync(r.dst, u.buf.as<uint8_t>() + r.off, r.len, hipMemcpyHostToDevice, up_stream));
        u.runs.clear();
        HIP_TRY(hipEventRecord(u.ev, up_stream));
        return RLNC_OK;
    }
    // host -> device copy of n bytes to dst through the staging ring: returns once the bytes are staged (src may then
    // be reused).  pitch >= n: the destination row's size -- a piece landing right after the previous one's row
    // joins its DMA (the pad bytes between rows are copied too).  *t = where the last byte was staged.
    int upload(uint8_t *dst, const uint8_t *src, size_t n, size_t pitch, rlnc::eng::UpTicket *t) {
        using namespace rlnc::eng;
        std::lock_guard<std::mutex> lock(up_mu);
        if (int st = upload_stream_locked()) return st;
        for (size_t o = 0; o < n; o += kUpChunk) {
            const size_t c = std::min(kUpChunk, n - o);
            const size_t span = (c == n && pitch <= kUpChunk) ? pitch : c;  // staged bytes incl. the row's pad
            UpSlot *u = &up[up_cur];
            if (!u->open || u->used + span > kUpChunk || u->runs.size() >= kUpRuns) {
                if (int st = upload_flush_locked(*u)) return st;
                up_cur = (up_cur + 1) % kUpSlots;
                u = &up[up_cur];
                if (!u->ev)
                    HIP_TRY(hipEventCreateWithFlags(&u->ev, hipEventDisableTiming));
                else
                    HIP_TRY(hipEventSynchronize(u->ev));  // the slot's last flush has read it
                if (int st = u->buf.ensure(kUpChunk)) return st;
                u->used = 0;
                u->gen += 1;
                u->open = true;
            }
            std::memcpy(u->buf.as<uint8_t>() + u->used, src + o, c);
            UpRun *last = u->runs.empty() ? nullptr : &u->runs.back();
            if (last && last->dst + last->len == dst + o && last->off + last->len == u->used)
                last->len += span;
            else
                u->runs.push_back(UpRun{dst + o, u->used, span});
            u->used += span;
            t->slot = up_cur;
            t->gen = u->gen;
        }
        return RLNC_OK;
    }
    // flush the ticket's slot if it still holds the staged piece; *ev = nullptr when nothing was ever staged
    int upload_flush(const rlnc::eng::UpTicket &t, hipEvent_t *ev) {
        *ev = nullptr;
        if (t.slot < 0) return RLNC_OK;
        std::lock_guard<std::mutex> lock(up_mu);
        rlnc::eng::UpSlot &u = up[t.slot];
        if (u.gen == t.gen)
            if (int st = upload_flush_locked(u)) return st;
        *ev = u.ev;  // this flush, or a later one of the same slot (after it on the upload stream)
        return RLNC_OK;
    }
    // order stream s after every upload up to the ticket's
    int upload_wait(const rlnc::eng::UpTicket &t, hipStream_t s) {
        hipEvent_t ev = nullptr;
        if (int st = upload_flush(t, &ev)) return st;
        if (!ev) return RLNC_OK;
        std::lock_guard<std::mutex> lock(up_mu);  // the event is not re-recorded while waited on
        HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        return RLNC_OK;
    }
    int upload_sync(const rlnc::eng::UpTicket &t) {
        hipEvent_t ev = nullptr;
        if (int st = upload_flush(t, &ev)) return st;
        if (!ev) return RLNC_OK;
        HIP_TRY(hipEventSynchronize(ev));
        return RLNC_OK;
    }
    // a call workspace; ordered: after the work already enqueued on the context stream (a call that reads
    // memory the caller's stream-ordered work may still write, e.g. a borrowed device source)
    int lease(std::unique_ptr<CallWs> &ws, bool ordered = true) {
        {
            std::lock_guard<std::mutex> lock(pool_mu);
            if (!pool.empty()) {
                ws = std::move(pool.back());
                pool.pop_back();
            }
        }
        if (!ws) {
            ws.reset(new (std::nothrow) CallWs);
            if (!ws) return set_error(RLNC_ERR_OUT_OF_MEMORY, "call workspace allocation");
            HIP_TRY(hipStreamCreateWithFlags(&ws->stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming));
        }
        if (!ordered) return RLNC_OK;
        HIP_TRY(hipEventRecord(ws->ev, stream));
        HIP_TRY(hipStreamWaitEvent(ws->stream, ws->ev, 0));
        return RLNC_OK;
    }
    void unlease(std::unique_ptr<CallWs> ws) {
        if (!ws) return;
        std::lock_guard<std::mutex> lock(pool_mu);
        pool.push_back(std::move(ws));
    }
    // the GF(2^8) matmul on stream s with index scratch idx (batch API: the context's; object API: the lease's)
    int matmul(rlnc::MatmulParams p, hipStream_t s, DevBuf &idx, bool batch) {
        if (max_tile_rows > 0 && p.n_out > max_tile_rows) {
            // split the output rows into launches of at most max_tile_rows rows (tuning knob)
            const int total = p.n_out;
            for (int r0 = 0; r0 < total; r0 += max_tile_rows) {
                rlnc::MatmulParams q = p;
                q.bsj_stream = nullptr;   // laid out for all the rows
                q.scan_status = nullptr;  // rows split over launches: no workgroup holds a whole object
                q.n_out = std::min(max_tile_rows, total - r0);
                q.coef = p.coef + int64_t(r0) * p.coef_row;
                q.out = p.out + int64_t(r0) * p.out_row;
                if (p.hdr) q.hdr = p.hdr + int64_t(r0) * p.hdr_row;
                if (int st = launch(q, s, idx, batch)) return st;
            }
            return RLNC_OK;
        }
        return launch(p, s, idx, batch);
    }
    int matmul(const rlnc::MatmulParams &p) { return matmul(p, stream, ws_idx, true); }
    // the sparse product (sparse.hip) on the context stream; it takes no workspace
    int sparse_matmul(const rlnc::SparseMatmulParams &p) {
        if (rlnc::sparse_matmul_workgroups(p) > 0x7FFFFFFF)
            return set_error(RLNC_ERR_INVALID_ARGUMENT, "sparse product of %d objects x %d rows x %lld bytes needs more "
                             "than 2^31 - 1 workgroups", p.n_obj, p.n_out, static_cast<long long>(p.width));
        HIP_TRY(rlnc::launch_sparse_matmul(p, stream));
        return RLNC_OK;
    }
    int launch(rlnc::MatmulParams p, hipStream_t s, DevBuf &idx, bool batch) {
        const rlnc::MatmulVariant v = variant;
        p.col_run = col_run;
        const size_t need = rlnc::matmul_scratch_bytes(p, v);
        if (need)
            if (int st = batch ? grow(idx, need) : idx.ensure(need)) return st;
        rlnc::BsjPersist pt;
        pt.counters = batch && s == stream ? ws_claim.as<uint32_t>() : nullptr;  // leased calls run on streams of their own
        pt.mode = persist_mode;
        pt.max_wgs = persist_max_wgs;
        HIP_TRY(rlnc::launch_matmul(p, s, v, idx.p, idx.cap, pt));
        return RLNC_OK;
    }
};

namespace rlnc::eng {
// RAII lease of a call workspace
struct Lease {
    rlnc_context *ctx;
    std::unique_ptr<CallWs> ws;
    explicit Lease(rlnc_context *c) : ctx(c) {}
    int acquire(bool ordered = true) { return ctx->lease(ws, ordered); }
    CallWs *operator->() const { return ws.get(); }
    ~Lease() { ctx->unlease(std::move(ws)); }
};

// n_obj products out[i][0:width) = XOR_j coef[i][j] · in[j][0:width) (i < n_out, j < n_in): rows at in_row / out_row,
// objects at in_obj / out_obj, each object's coefficients dense ([n_out][n_in])
inline rlnc::MatmulParams product_params(const uint8_t *in, size_t in_obj, size_t in_row, size_t n_in, size_t width,
                                         const uint8_t *coef, size_t n_out, uint8_t *out, size_t out_obj,
                                         size_t out_row, size_t n_obj) {
    rlnc::MatmulParams p{};
    p.in = in;
    p.in_obj = int64_t(in_obj);
    p.in_row = int64_t(in_row);
    p.coef = coef;
    p.coef_obj = int64_t(n_out * n_in);
    p.coef_row = int64_t(n_in);
    p.out = out;
    p.out_obj = int64_t(out_obj);
    p.out_row = int64_t(out_row);
    p.n_out = int(n_out);
    p.n_in = int(n_in);
    p.width = int64_t(width);
    p.n_obj = int(n_obj);
    return p;
}

// the sparse form of product_params: each object's entries dense ([n_out][w] indices and values)
inline rlnc::SparseMatmulParams sparse_product_params(const uint8_t *in, size_t in_obj, size_t in_row, size_t n_in,
                                                      size_t width, const int32_t *idx, const uint8_t *val, size_t w,
                                                      size_t n_out, uint8_t *out, size_t out_obj, size_t out_row,
                                                      size_t n_obj) {
    rlnc::SparseMatmulParams p{};
    p.in = in;
    p.in_obj = int64_t(in_obj);
    p.in_row = int64_t(in_row);
    p.idx = idx;
    p.idx_obj = int64_t(n_out * w * 4);
    p.idx_row = int64_t(w * 4);
    p.val = val;
    p.val_obj = int64_t(n_out * w);
    p.val_row = int64_t(w);
    p.out = out;
    p.out_obj = int64_t(out_obj);
    p.out_row = int64_t(out_row);
    p.n_out = int(n_out);
    p.n_in = int(n_in);
    p.w = int(w);
    p.n_obj = int(n_obj);
    p.width = int64_t(width);
    return p;
}
// idx / val of a sparse call: both present unless w == 0, idx readable as int32
inline bool sparse_entries_ok(const int32_t *idx, const uint8_t *val, size_t w) {
    return w <= 0x7FFFFFFF && (w == 0 || (idx != nullptr && val != nullptr)) &&
           (reinterpret_cast<uintptr_t>(idx) & 3) == 0;
}

// The results of nobj objects, device -> pin (nobj · (16 + 4m) bytes of pinned memory) -> the caller's arrays, any of
// which may be null: object statuses, data lengths and, with pstat_dev, the m piece statuses of each.  Waits for s.
inline int read_results(uint8_t *pin, hipStream_t s, size_t nobj, const void *status_dev, const void *len_dev,
                        const void *pstat_dev, size_t m, int32_t *object_status, uint64_t *data_len,
                        int32_t *piece_status) {
    HIP_TRY(hipMemcpyAsync(pin, status_dev, nobj * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(pin + nobj * 8, len_dev, nobj * 8, hipMemcpyDeviceToHost, s));
    if (pstat_dev) HIP_TRY(hipMemcpyAsync(pin + nobj * 16, pstat_dev, nobj * m * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (object_status) std::memcpy(object_status, pin, nobj * 4);
    if (data_len) std::memcpy(data_len, pin + nobj * 8, nobj * 8);
    if (pstat_dev && piece_status) std::memcpy(piece_status, pin + nobj * 16, nobj * m * 4);
    return RLNC_OK;
}
}  // namespace rlnc::eng

struct rlnc_encoder;
namespace rlnc::eng {
// an Encoder owning the padded image img (k rows of L bytes at `stride`, hipMalloc'd; freed with the encoder)
int encoder_adopt_device(rlnc_context *ctx, uint8_t *img, size_t k, size_t L, size_t stride, rlnc_encoder **out);
}  // namespace rlnc::eng
