// host_copy.hpp — a small pool of host threads that copies large buffers in parallel (internal to librlnc_hip).
//
// Decoder::get_decoded_data hands its output to a caller buffer the caller has just allocated (the reference builds a
// fresh `vec![0u8; k·L]`, decoder.rs:141-142).  At many MiB such a buffer is a fresh mapping whose pages fault in on
// first write, and one thread copying (and faulting) 32 MiB is what bounded the copy-out (round 4: 5.8 ms of a 7 ms
// decode).  The pool splits a copy into page-aligned slices of the destination, one per thread, so the page faults
// and the bytes are spread over several cores.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rlnc::eng {

// dst[0, n) = src[0, n) with up to `threads` threads (the caller's included); returns when done.  Small copies stay on
// the calling thread.
void par_copy(void *dst, const void *src, size_t n, int threads);
// the pages of dst[0, n) faulted in (one zero byte written per 4 KiB) by up to `threads` threads: a caller buffer
// fresh from calloc is then warm when the device's bytes arrive (call it while the device works)
void par_touch(void *dst, size_t n, int threads);
// the thread count par_copy callers use: RLNC_COPY_THREADS (sizes the pool to the host, read once), else
// min(8, hardware threads)
int copy_threads();

// Device -> caller host memory for large outputs, synchronous on ws->stream: chunks DMA'd into a ring of pinned buffers
// (ws->pin_out), each copied into dst by the pool while the next chunks are in flight.  The caller's buffer is
// typically fresh (the reference returns a new vec![0u8; k·L], decoder.rs:141-142): the pool's threads also share its
// page faults, which one thread paid alone in the runtime's pageable copy (round 4: 5.8 ms for 32 MiB).
struct CallWs;
int copy_out(CallWs *ws, uint8_t *dst, const uint8_t *src_dev, size_t n);

}  // namespace rlnc::eng
