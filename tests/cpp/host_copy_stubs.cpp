// What rlnc_amd/csrc/host_copy.cpp references outside itself, for the stand-alone program of test_host_copy.cpp:
// engine.cpp's error string, and the HIP runtime entry points of copy_out (the device -> host copy, which the program
// never calls).  The stubs abort: the program makes no HIP call, and would say so if it ever did.  A new reference
// from host_copy.cpp into the engine shows up as an undefined symbol when the program is linked.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>

namespace rlnc::eng {
thread_local std::string g_last_error;
}

namespace {
[[noreturn]] void no_hip(const char *name) {
    std::fprintf(stderr, "test_host_copy: unexpected HIP call %s\n", name);
    std::abort();
}
}  // namespace

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned) { no_hip("hipEventCreateWithFlags"); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { no_hip("hipEventRecord"); }
hipError_t hipEventSynchronize(hipEvent_t) { no_hip("hipEventSynchronize"); }
const char *hipGetErrorString(hipError_t) { no_hip("hipGetErrorString"); }
hipError_t hipHostFree(void *) { no_hip("hipHostFree"); }
hipError_t hipHostMalloc(void **, size_t, unsigned int) { no_hip("hipHostMalloc"); }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { no_hip("hipMemcpyAsync"); }
hipError_t hipStreamSynchronize(hipStream_t) { no_hip("hipStreamSynchronize"); }
}
