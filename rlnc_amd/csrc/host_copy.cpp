// host_copy.cpp — parallel host copies and the large device -> host copy-out built on them (host_copy.hpp).
#include "host_copy.hpp"

#include <sys/mman.h>

#include <condition_variable>
#include <thread>

#include "context.hpp"

namespace rlnc::eng {
namespace {

constexpr size_t kMinSlice = size_t(1) << 20;  // below this per thread the hand-off costs more than it saves
constexpr size_t kPage = 4096;

// one store into every 4 KiB page that dst[a, b) intersects
void touch(uint8_t *dst, size_t a, size_t b) {
    if (a >= b) return;
    volatile uint8_t *v = dst;
    v[a] = 0;
    for (size_t i = (a + kPage - reinterpret_cast<uintptr_t>(dst + a) % kPage); i < b; i += kPage) v[i] = 0;
}

// Persistent workers (created on first use, detached: they sleep on the condition variable between copies and die
// with the process).  One copy at a time; concurrent callers serialise on `call_mu` (a copy of many MiB is
// bandwidth-bound, two at once would not finish sooner).
class Pool {
   public:
    // src == nullptr: touch instead of copy (one zero byte in each 4 KiB page of each slice)
    void run(uint8_t *dst, const uint8_t *src, size_t n, int threads) {
        std::lock_guard<std::mutex> call(call_mu_);
        ensure(threads - 1);
        // slice boundaries on page boundaries of the destination ADDRESS (dst + offset), whatever dst's alignment:
        // slice 0 runs to the first page boundary past its share, every later slice starts on one, so no two threads
        // fault the same page
        const size_t per = ((n + threads - 1) / threads + kPage - 1) & ~(kPage - 1);
        const size_t lead = (kPage - reinterpret_cast<uintptr_t>(dst) % kPage) % kPage;
        {
            std::lock_guard<std::mutex> lock(mu_);
            dst_ = dst;
            src_ = src;
            n_ = n;
            per_ = per;
            lead_ = lead;
            next_ = 1;  // slice 0 is the caller's
            slices_ = n > lead + per ? (n - lead + per - 1) / per : 1;
            pending_ = slices_ - 1;
        }
        cv_.notify_all();
        copy_slice(0);
        std::unique_lock<std::mutex> lock(mu_);
        // the caller takes slices too until none is left unclaimed, then waits for the workers' last ones
        while (next_ < slices_) {
            const size_t s = next_++;
            lock.unlock();
            copy_slice(s);
            lock.lock();
            --pending_;
        }
        done_.wait(lock, [&] { return pending_ == 0; });
    }

   private:
    // slice s = [bound(s), bound(s + 1)): bound(0) = 0, bound(s) = lead + s * per (a page boundary of dst + offset)
    size_t bound(size_t s) const { return s == 0 ? 0 : std::min(n_, lead_ + s * per_); }
    void copy_slice(size_t s) {
        const size_t a = bound(s), b = s + 1 == slices_ ? n_ : bound(s + 1);
        if (src_ != nullptr) {
            std::memcpy(dst_ + a, src_ + a, b - a);
        } else {
            touch(dst_, a, b);
        }
    }
    void ensure(int workers) {
        while (int(workers_) < workers) {
            std::thread([this] { loop(); }).detach();
            ++workers_;
        }
    }
    void loop() {
        std::unique_lock<std::mutex> lock(mu_);
        for (;;) {
            cv_.wait(lock, [&] { return next_ < slices_; });
            const size_t s = next_++;
            lock.unlock();
            copy_slice(s);
            lock.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_;
    size_t workers_ = 0;
    uint8_t *dst_ = nullptr;
    const uint8_t *src_ = nullptr;
    size_t n_ = 0, per_ = 0, lead_ = 0, next_ = 0, slices_ = 0, pending_ = 0;
};

Pool &pool() {
    static Pool *p = new Pool;  // never destroyed: detached workers may still wait on it at exit
    return *p;
}

}  // namespace

void par_touch(void *dst, size_t n, int threads) {
    threads = int(std::min<size_t>(size_t(std::max(1, threads)), n / kMinSlice));
    if (threads <= 1) {
        touch(static_cast<uint8_t *>(dst), 0, n);
        return;
    }
    pool().run(static_cast<uint8_t *>(dst), nullptr, n, threads);
}

int copy_threads() {
    static const int t = std::max(
        1, env_int("RLNC_COPY_THREADS", int(std::min<unsigned>(8, std::thread::hardware_concurrency()))));
    return t;
}

void par_copy(void *dst, const void *src, size_t n, int threads) {
    threads = int(std::min<size_t>(size_t(std::max(1, threads)), n / kMinSlice));
    if (threads <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    pool().run(static_cast<uint8_t *>(dst), static_cast<const uint8_t *>(src), n, threads);
}

namespace {
constexpr size_t kOutChunk = size_t(4) << 20;
constexpr size_t kOutParallelMin = size_t(8) << 20;  // below this one pageable DMA is as fast (profiles/r05_copyout*)

// RLNC_COPY_TRACE=1: per-call host time of copy_out's phases
PhaseTrace g_copy_trace("RLNC_COPY_TRACE",
                        "{\"copy_trace\": {\"calls\": %zu, \"median_total_us\": %.1f, \"median_event_wait_us\": %.1f, "
                        "\"median_host_copy_us\": %.1f, \"median_first_chunk_wait_us\": %.1f}}\n");

// The whole 2 MiB-aligned pages inside dst[0, n) may be backed by transparent huge pages (a hint, where the host's
// THP mode is "madvise"): a fresh buffer then faults in 2 MiB at a time instead of 4 KiB.  The advice changes the
// flags of the caller's mapping (they outlive the buffer in its allocator's arena), so the library gives it only when
// the caller opts in with RLNC_COPY_HUGEPAGE=1 (read once).  A caller that owns a fresh result buffer advises it
// itself: the C++ mirror's get_decoded_data does (include/rlnc/full.hpp), which is where the 32 MB rows' huge-page
// gain is measured.
void advise_huge(uint8_t *dst, size_t n) {
    static const bool on = env_int("RLNC_COPY_HUGEPAGE", 0) != 0;
    constexpr uintptr_t kHuge = uintptr_t(2) << 20;
    const uintptr_t a = (reinterpret_cast<uintptr_t>(dst) + kHuge - 1) & ~(kHuge - 1);
    const uintptr_t b = (reinterpret_cast<uintptr_t>(dst) + n) & ~(kHuge - 1);
    if (on && b > a) (void)madvise(reinterpret_cast<void *>(a), b - a, MADV_HUGEPAGE);
}

// whether dst's pages are already mapped (a heap block the caller's allocator reused, zeroed on the caller's thread):
// mincore on its first, middle and last pages -- a fresh mapping has none of them
bool pages_resident(const uint8_t *dst, size_t n) {
    for (size_t off : {size_t(0), n / 2, n - 1}) {
        unsigned char v = 0;
        void *a = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(dst + off) & ~(kPage - 1));
        if (mincore(a, kPage, &v) != 0 || !(v & 1)) return false;
    }
    return true;
}
}  // namespace

int copy_out(CallWs *ws, uint8_t *dst, const uint8_t *src_dev, size_t n) {
    const int threads = copy_threads();
    if (n < kOutParallelMin || threads <= 1) {
        HIP_TRY(hipMemcpyAsync(dst, src_dev, n, hipMemcpyDeviceToHost, ws->stream));
        HIP_TRY(hipStreamSynchronize(ws->stream));
        return RLNC_OK;
    }
    constexpr int R = CallWs::kOutRing;
    if (int st = ws->pin_out.ensure(size_t(R) * kOutChunk)) return st;
    for (hipEvent_t &e : ws->out_ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint8_t *stage = ws->pin_out.as<uint8_t>();
    advise_huge(dst, n);
    const size_t chunks = (n + kOutChunk - 1) / kOutChunk;
    auto issue = [&](size_t c) -> int {
        const size_t off = c * kOutChunk, len = std::min(kOutChunk, n - off);
        HIP_TRY(hipMemcpyAsync(stage + (c % R) * kOutChunk, src_dev + off, len, hipMemcpyDeviceToHost, ws->stream));
        HIP_TRY(hipEventRecord(ws->out_ev[c % R], ws->stream));
        return RLNC_OK;
    };
    for (size_t c = 0; c < std::min<size_t>(R, chunks); ++c)
        if (int st = issue(c)) return st;
    // while the device runs the product and the first chunks' DMAs: fault the caller's pages in, in parallel (a fresh
    // buffer's page faults were most of the host copies' time: profiles/r05_copyout_trace*)
    if (!pages_resident(dst, n)) par_touch(dst, n, threads);
    const bool tr = g_copy_trace.on;
    const uint64_t t0 = tr ? now_ns() : 0;
    uint64_t tw = 0, tc = 0, tf = 0;
    for (size_t c = 0; c < chunks; ++c) {
        const uint64_t a = tr ? now_ns() : 0;
        HIP_TRY(hipEventSynchronize(ws->out_ev[c % R]));
        const uint64_t b = tr ? now_ns() : 0;
        const size_t off = c * kOutChunk, len = std::min(kOutChunk, n - off);
        par_copy(dst + off, stage + (c % R) * kOutChunk, len, threads);
        if (tr) {
            tw += b - a;
            tc += now_ns() - b;
            if (c == 0) tf = b - a;
        }
        if (c + R < chunks)
            if (int st = issue(c + R)) return st;
    }
    if (tr) g_copy_trace.add((now_ns() - t0) / 1e3f, tw / 1e3f, tc / 1e3f, tf / 1e3f);
    return RLNC_OK;
}

}  // namespace rlnc::eng
