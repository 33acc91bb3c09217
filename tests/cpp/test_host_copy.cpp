// The host copy pool (rlnc_amd/csrc/host_copy.cpp: par_copy / par_touch) on destinations off a page boundary and odd
// lengths.  Stand-alone: linked with host_copy.cpp and host_copy_stubs.cpp (the engine's error string and aborting
// stand-ins for the HIP entry points of copy_out, which is never called), makes no HIP call and needs no GPU.
// tests/test_host_copy.py builds and runs it, plain and under the address and thread sanitizers.
//
// par_copy(dst, src, n, threads): every byte of dst[0, n) equals src, the 4 KiB before and after are untouched.
// par_touch(dst, n, threads): "one zero byte written per 4 KiB" -- dst[0] and the first byte of every 4 KiB page of the
// destination ADDRESS inside (dst, dst + n) become zero; every other byte, inside and outside, keeps its value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rlnc_amd/csrc/host_copy.hpp"

namespace {

constexpr size_t kPage = 4096, kGuard = 4096, MiB = size_t(1) << 20;

int failures = 0;

void fail(const char *what, size_t off, size_t n, int threads, const uint8_t *got, const uint8_t *want, size_t len,
          ptrdiff_t origin) {
    size_t i = 0;
    while (i < len && got[i] == want[i]) ++i;
    std::fprintf(stderr, "FAIL %s: page offset %zu, n %zu, %d threads: first difference at dst%+td (got 0x%02X, want 0x%02X)\n",
                 what, off, n, threads, ptrdiff_t(i) - origin, got[i], want[i]);
    ++failures;
}

// bytes that are never zero and never repeat with a page's period
void pattern(std::vector<uint8_t> &v, uint64_t seed) {
    uint64_t x = seed;
    for (uint8_t &b : v) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        b = uint8_t(x >> 32) | 1u;
    }
}

}  // namespace

int main() {
    const size_t offsets[] = {0, 1, 17, 4095};
    const size_t lengths[] = {8 * MiB, 8 * MiB + 1, 9 * MiB - 4097, 3 * MiB + 5};
    const int thread_counts[] = {1, 2, 3, 8};
    const size_t max_n = 9 * MiB;
    const size_t span = kGuard + kPage + max_n + kGuard;  // guard | page offset | n | guard

    std::vector<uint8_t> src(max_n + 16), fill(span), want(span);
    pattern(src, 0x9E3779B97F4A7C15ull);
    pattern(fill, 0xD1B54A32D192ED03ull);
    uint8_t *buf = static_cast<uint8_t *>(std::aligned_alloc(kPage, (span + kPage - 1) / kPage * kPage));
    if (buf == nullptr) return 2;

    int cases = 0;
    for (size_t off : offsets)
        for (size_t n : lengths)
            for (int threads : thread_counts) {
                uint8_t *dst = buf + kGuard + off;  // buf is page-aligned: dst is `off` bytes past a page boundary
                const size_t used = kGuard + off + n + kGuard;
                const uint8_t *s = src.data() + (cases % 2 ? 3 : 0);  // the source off an 8-byte boundary too

                std::memcpy(buf, fill.data(), used);
                rlnc::eng::par_copy(dst, s, n, threads);
                std::memcpy(want.data(), fill.data(), used);
                std::memcpy(want.data() + kGuard + off, s, n);
                if (std::memcmp(buf, want.data(), used) != 0)
                    fail("par_copy", off, n, threads, buf, want.data(), used, ptrdiff_t(kGuard + off));

                std::memcpy(buf, fill.data(), used);
                rlnc::eng::par_touch(dst, n, threads);
                std::memcpy(want.data(), fill.data(), used);
                want[kGuard + off] = 0;
                for (size_t a = (kGuard + off) / kPage * kPage + kPage; a < kGuard + off + n; a += kPage) want[a] = 0;
                if (std::memcmp(buf, want.data(), used) != 0)
                    fail("par_touch", off, n, threads, buf, want.data(), used, ptrdiff_t(kGuard + off));
                ++cases;
            }
    // below one slice per thread the copy stays on the calling thread; n = 0 and n = 1 touch nothing else
    for (size_t n : {size_t(0), size_t(1), size_t(4097), MiB - 1}) {
        uint8_t *dst = buf + kGuard + 4095;
        const size_t used = kGuard + 4095 + n + kGuard;
        std::memcpy(buf, fill.data(), used);
        rlnc::eng::par_copy(dst, src.data(), n, 8);
        std::memcpy(want.data(), fill.data(), used);
        std::memcpy(want.data() + kGuard + 4095, src.data(), n);
        if (std::memcmp(buf, want.data(), used) != 0) fail("par_copy (small)", 4095, n, 8, buf, want.data(), used, kGuard + 4095);
        std::memcpy(buf, fill.data(), used);
        rlnc::eng::par_touch(dst, n, 8);
        std::memcpy(want.data(), fill.data(), used);
        if (n > 0) want[kGuard + 4095] = 0;
        for (size_t a = 2 * kGuard; a < kGuard + 4095 + n; a += kPage) want[a] = 0;
        if (std::memcmp(buf, want.data(), used) != 0) fail("par_touch (small)", 4095, n, 8, buf, want.data(), used, kGuard + 4095);
        ++cases;
    }
    std::free(buf);
    if (failures) {
        std::fprintf(stderr, "%d of %d cases failed\n", failures, cases);
        return 1;
    }
    std::printf("host copy pool ok: %d cases\n", cases);
    return 0;
}
