// gf_perm.hpp — the device GF(2^8) helpers of the elimination kernels (rref_kernels.hpp, rank.hip, rank_large.hip;
// internal to librlnc_hip): the compile-time v_perm multiplier table, the products that read a copy of it, and the
// wave helpers.  Nothing of any elimination lives here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gf256.hpp"

namespace rlnc {
namespace {

constexpr int kTabDw = 8;  // dwords per multiplier: t0lo t0hi t1lo t1hi t2 inv - -

// The 512 × kTabDw table, built at compile time: entry c < 256 = make_perm_table's layout of multiplier c plus
// c^-1 = c^254 in dword 5; entry 256 + c = the layout of c^-1 (0 for c = 0), so that "multiply by the
// inverse of the pivot" is one table read (the register path's normalisation).
constexpr int kTabEntries = 512;
constexpr int kMulTabDw = 256 * kTabDw;  // the multipliers 0..255 alone (8 KiB): what copy_table brings into LDS
struct RrefTable {
    uint32_t v[kTabEntries * kTabDw];
};
constexpr void fill_perm_entry(uint32_t *e, uint8_t c) {
    uint8_t m[8] = {};
    m[0] = c;
    for (int b = 1; b < 8; ++b) m[b] = gf_xtime(m[b - 1]);
    uint32_t t0lo = 0, t0hi = 0, t1lo = 0, t1hi = 0, t2 = 0;
    for (int x = 0; x < 8; ++x) {
        uint8_t a = 0, h = 0;
        for (int b = 0; b < 3; ++b)
            if (x & (1 << b)) {
                a = uint8_t(a ^ m[b]);
                h = uint8_t(h ^ m[b + 3]);
            }
        if (x < 4) {
            t0lo |= uint32_t(a) << (8 * x);
            t1lo |= uint32_t(h) << (8 * x);
        } else {
            t0hi |= uint32_t(a) << (8 * (x - 4));
            t1hi |= uint32_t(h) << (8 * (x - 4));
        }
    }
    for (int x = 0; x < 4; ++x) {
        uint8_t a = 0;
        for (int b = 0; b < 2; ++b)
            if (x & (1 << b)) a = uint8_t(a ^ m[b + 6]);
        t2 |= uint32_t(a) << (8 * x);
    }
    e[0] = t0lo;
    e[1] = t0hi;
    e[2] = t1lo;
    e[3] = t1hi;
    e[4] = t2;
}
constexpr RrefTable build_rref_table() {
    RrefTable t{};
    // inverses by the generator-3 logarithm (gf256.rs:16-44, 88-108): c^-1 = 3^(255 - log3 c)
    uint8_t ex[256] = {}, lg[256] = {};
    uint8_t x = 1;
    for (int i = 0; i < 255; ++i) {
        ex[i] = x;
        lg[x] = uint8_t(i);
        x = uint8_t(x ^ gf_xtime(x));  // x·3
    }
    for (int c = 0; c < 256; ++c) {
        const uint8_t inv = c ? ex[(255 - lg[c]) % 255] : uint8_t(0);
        fill_perm_entry(t.v + c * kTabDw, uint8_t(c));
        t.v[c * kTabDw + 5] = inv;
        fill_perm_entry(t.v + (256 + c) * kTabDw, inv);
    }
    return t;
}
__device__ const RrefTable kRrefTable = build_rref_table();
// spot checks against the field (gf256.rs:16-44): identity tables of c = 1, 2^-1 = 0x8D, 3^-1 = 0xF6
static_assert(build_rref_table().v[1 * kTabDw + 0] == 0x03020100u && build_rref_table().v[1 * kTabDw + 1] == 0x07060504u,
              "c = 1 low table");
static_assert(build_rref_table().v[2 * kTabDw + 5] == 0x8Du && build_rref_table().v[3 * kTabDw + 5] == 0xF6u,
              "inverses");
static_assert(build_rref_table().v[(256 + 1) * kTabDw + 0] == 0x03020100u, "1^-1 = 1");

__device__ __forceinline__ uint32_t mul4(const uint32_t *tab, uint32_t q, uint32_t x) {
    const uint4 t = *reinterpret_cast<const uint4 *>(tab + q * kTabDw);
    const uint32_t t2 = tab[q * kTabDw + 4];
    return __builtin_amdgcn_perm(t.y, t.x, x & 0x07070707u) ^ __builtin_amdgcn_perm(t.w, t.z, (x >> 3) & 0x07070707u) ^
           __builtin_amdgcn_perm(t2, t2, (x >> 6) & 0x03030303u);
}
__device__ __forceinline__ uint32_t mul4t(uint4 t, uint32_t t2, uint32_t x) {
    return __builtin_amdgcn_perm(t.y, t.x, x & 0x07070707u) ^ __builtin_amdgcn_perm(t.w, t.z, (x >> 3) & 0x07070707u) ^
           __builtin_amdgcn_perm(t2, t2, (x >> 6) & 0x03030303u);
}
__device__ __forceinline__ uint32_t gfmul(const uint32_t *tab, uint32_t a, uint32_t b) {
    return mul4(tab, a, b) & 0xFFu;
}
__device__ __forceinline__ uint32_t gfinv(const uint32_t *tab, uint32_t a) { return tab[a * kTabDw + 5]; }

// lane within the wave: single-wave code also runs in one wave of a multi-object workgroup
__device__ __forceinline__ int lane_id() { return int(threadIdx.x & 63u); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }

// WG: a workgroup barrier; else the code runs in one wave only (the other waves of the workgroup are elsewhere and
// must not be waited for): a compiler fence suffices, a wave's LDS operations execute in issue order
template <bool WG>
__device__ __forceinline__ void rsync() {
    if constexpr (WG) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// a wave-uniform value as a scalar
__device__ __forceinline__ uint32_t uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }

// the multipliers 0..255 of kRrefTable (8 KiB) into LDS by a workgroup of 256 threads, both halves of the copy in
// flight at once
__device__ __forceinline__ void copy_table(uint32_t *tab) {
    const uint4 *src = reinterpret_cast<const uint4 *>(kRrefTable.v);
    uint4 *dst = reinterpret_cast<uint4 *>(tab);
    const uint4 a = src[threadIdx.x], b = src[threadIdx.x + 256];
    dst[threadIdx.x] = a;
    dst[threadIdx.x + 256] = b;
}

}  // namespace
}  // namespace rlnc
