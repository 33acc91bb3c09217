/*
 * rlnc_hip.h — C ABI of librlnc_hip.so, the MI355X (gfx950) engine for the RLNC hot path of
 * itzmeanjan/rlnc 0.8.5.
 *
 * Drop-in boundary.  The reference exposes exactly three types plus one error enum
 * (rlnc::full::{Encoder, Decoder, Recoder}, rlnc::RLNCError — src/lib.rs:127-130, src/full/mod.rs:9-11);
 * its internal seam is the three src/common/simd functions (simd/mod.rs:18,58,89).  Every entry point
 * below names the reference item it replaces.  The Rust-side binding a maintainer would add is in
 * INTEGRATION.md.
 *
 * Conventions
 *   - Plain C: pointers + sizes, no exceptions across the ABI, no torch types.
 *   - Return value: RLNC_OK (0) or a status code.  Codes 1..13 are RLNCError discriminant + 1
 *     (src/common/errors.rs:3-32, same order); >= 100 are engine/device errors (rlnc_last_error() has
 *     the message, thread-local).
 *   - Randomness stays with the caller (the reference draws coefficients with rng.fill_bytes,
 *     encoder.rs:248 / recoder.rs:131): functions that the reference feeds from an RNG take those
 *     bytes explicitly, so outputs are bit-exact given the same coefficient bytes.
 *   - "_device" / batch functions take device pointers (hipMalloc'd memory on the context's device) and
 *     are asynchronous on the context's stream; the object API (encoder/decoder/recoder on host buffers)
 *     is synchronous, like the Rust API it mirrors.
 *   - Threading.  The object API (Encoder/Decoder/Recoder on host buffers) is safe to call from many host
 *     threads on one context: every call leases its own stream and buffers from the context's pool, so
 *     rlnc_encoder_code_with_buf on ONE encoder from many threads at once is safe, like the reference's
 *     code(&self) on a Send + Sync Encoder (encoder.rs:264).  A decoder or recoder must not be used by two
 *     threads at the same time (the reference's &mut self).  The stream-ordered batch / _device calls use the
 *     context's own workspaces: one caller thread per context at a time (one context per stream).
 *   - Lifetime.  Objects hold a reference on the context that created them: rlnc_context_destroy drops the
 *     creator's reference and the context is freed when its last object is freed, so an object may outlive
 *     the thread (and thread-local context) that created it.  Freeing an object waits only for its own
 *     stream-ordered uses (its _batch_device / _device launches, on whichever streams the context had then),
 *     not for other work queued on the context's stream; its device memory is reused only after them.
 *   - HIP graphs.  Once a batch call on a context has been captured into a HIP graph, the graph holds that
 *     context's workspace addresses: they are frozen, and a later call that would need a larger workspace
 *     fails with RLNC_ERR_INVALID_ARGUMENT instead of moving them (run the largest shape eagerly before
 *     capturing, or use another context for other shapes).
 *   - Rank mode.  RLNC_RANK_MODE_REFERENCE (0, the default) replays the crate's DecoderMatrix::rref bit for bit,
 *     including its quirk: it pivots only on the diagonal, so sparse or structured coding vectors can be counted
 *     useful when they are linearly dependent.  RLNC_RANK_MODE_TRUE (1) is NOT the crate's
 *     behaviour on such input: the decoder keeps the useful pieces' rows [c | e] (c: k coefficient bytes, e: one
 *     byte per received-piece slot) in reduced row-echelon form with free pivot columns.  Pushing piece p with
 *     coefficients h: (1) rank == k answers ReceivedAllPieces and changes nothing; (2) v = [h | unit(p)], and for
 *     every stored row i, v ^= h[pivot_i] · row_i; (3) v[0:k] all zero answers PieceNotUseful and changes nothing;
 *     (4) pc = first nonzero column of v, v is scaled by 1 / v[pc], every stored row gets row_i ^= row_i[pc] · v,
 *     and v is stored with pivot pc: Ok.  rank = number of rows; T row r (r < rank) is the e part of the row with
 *     the r-th smallest pivot column, rows >= rank are zero.  A piece is therefore useful exactly when it is
 *     independent of the useful pieces before it; at rank k, T × data is the source as in mode 0.  On dense random
 *     coefficients the two modes answer alike.  The device kernel of mode 1 applies when
 *     8192 + 4·(k·D + 2·D + m·ceil(k/4) + m + 2·k + ceil(k/4)) <= 160 KiB with D = ceil(k/4) + ceil(m/4);
 *     beyond that each call does what it does in mode 0 beyond LDS (host elimination, or the same error) -- unless
 *     decode path 7 is set (rlnc_set_decode_path): then a second set of kernels keeps the same rows in a device
 *     workspace, takes the pieces B <= 32 at a time (three launches per block, one at the end, none synchronising) and
 *     produces the same T, statuses and rank for k <= 4096, m <= 8192.
 *   - Decode streams.  rlnc_decode_stream_* keep the rank-mode-1 decoder state of num_objects objects (the rows,
 *     pivots, statuses and counters of "Rank mode") in a caller-owned device buffer between calls: a receiver pushes
 *     pieces as they arrive, per object, instead of re-running an elimination over every prefix.  Slot t of object o
 *     is piece t of that object in the caller's pieces [obj][m][k+L] buffer; the caller fills slots in order and says,
 *     in an int32 device array, how many of each object are filled.  A push advances every object to that count
 *     (capped by m and by max_new pieces per object and call) and leaves exactly the state a fresh mode-1 decoder has
 *     after decode() of the same slots in order -- the same statuses, rank and T, however the pieces were split over
 *     pushes.  A push has two forms (rlnc_set_stream_form).  The workspace form runs the kernels of decode paths 7
 *     and 8 with the block taken per object from the state (rlnc_amd/csrc/rank_large.hip): k <= 4096, m <= 8192, one
 *     latch launch and three launches per block of B <= 32 pieces.  The LDS form (rlnc_amd/csrc/rank_stream.hip) is one
 *     launch per push, for the generations whose rows fit one workgroup's LDS -- the condition of "Rank mode" above,
 *     rlnc_decode_stream_lds_fits: an object's rows and pivots come from the state into LDS, the per-piece loop of the
 *     mode-1 LDS kernel runs over the new slots only, and the rows go back.  Both leave the same state, byte for byte
 *     in everything a later call reads, so they may be mixed from push to push on one state buffer (its layout and
 *     state words: rlnc_amd/csrc/rank_state.hpp).
 *     rlnc_decode_stream_compact (rlnc_amd/csrc/rank_compact.hip) reclaims the slots of useless arrivals and retires
 *     finished objects in place, on the device: the useful pieces move to the first slots, the columns of the stored
 *     rows are renumbered to match, and the state is a fresh stream's after the kept pieces -- so m bounds the pieces
 *     an object holds, not the arrivals it sees, and a place is reused while its neighbours go on.
 *     rlnc_decode_stream_deliver (rlnc_amd/csrc/stream_deliver.hip) hands over the decoded data of the objects whose
 *     rank is k, chosen on the device, at the cost of those objects' products alone.
 *     rlnc_decode_stream_recode (rlnc_amd/csrc/stream_recode.hip) is the relay's call: every selected object that
 *     holds a useful piece gets count recoded pieces over exactly its useful pieces -- the slots compact would keep --
 *     found on the device, so a relay forwards without leaving the push -> deliver -> compact loop.
 *     rlnc_decode_stream_accept (rlnc_amd/csrc/stream_accept.hip) is the step before the push: arrivals for many
 *     objects, interleaved in one staging buffer, go into their objects' next free slots in arrival order, with the
 *     slot decided on the device from avail and the rank, so the loop needs no host decision.  Not covered: the
 *     reference rank mode has no stream form (a context in mode 0 is refused).  Measured on one MI355X
 *     (profiles/r12_decode_stream.jsonl, profiles/r14_stream_lds.jsonl, profiles/r16_stream_compact.jsonl): see
 *     DESIGN.md §4.2.4.
 *   - Sparse coding vectors.  The *_sparse calls take a coefficient matrix as two arrays with a fixed number w of
 *     entries per output row: idx int32 [obj][n_out][w], the source-row index of each entry, and val uint8
 *     [obj][n_out][w], its coefficient.  The dense row c they stand for is c[j] = XOR of val[t] over all t with
 *     idx[t] == j.  An entry with val == 0 contributes nothing: it is padding.  An entry whose index is not in
 *     [0, n_in) contributes nothing either, and no source row is read for it; that is a guard, not an error report
 *     (the arrays are device-resident and cannot be validated without a synchronise).  Duplicate indices accumulate
 *     by XOR in the header and, by linearity, in the data.  w == 0 is allowed (idx / val may then be NULL): every
 *     output row, header included, is zero.  Every sparse call therefore writes, byte for byte, what the
 *     corresponding dense call writes on the expanded matrix.  The coded pieces keep the crate's wire format, dense
 *     coefficients ‖ data, so any decoder reads them (this library's in either rank mode; a sparse sender wants a
 *     rank-mode-1 receiver).  The sparse calls always run the sparse kernel (rlnc_amd/csrc/sparse.hip: w source rows
 *     gathered per output row, no workspace), never the dense engine; they are asynchronous on the context's stream,
 *     never synchronise and can be captured into a HIP graph.  When to prefer the dense call on the expanded matrix
 *     (measured on one MI355X, profiles/r08_sparse_product.jsonl, dense time / sparse time on the same input):
 *     k = 1,024 (rows of 32 KiB): sparse 11.0x, 8.0x, 4.9x faster at w = 4, 8, 16, and by its slope (0.0102 ms per
 *     entry against the dense call's flat 1.08 ms) up to w of about 100, a density of 1/10; k = 128 (256 KiB rows):
 *     2.2x, 1.8x, 1.2x faster at w = 2, 4, 8 and 0.76x at w = 16 -- prefer the dense call above a density of about
 *     1/12; k = 32 and k = 16: the dense call is faster at every w (0.79x at w = 2 of k = 32, 0.19x at w = k), because
 *     the dense programs read each source row once per row tile where the gather reads it once per entry.
 */
#ifndef RLNC_HIP_H
#define RLNC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: errors.rs:3-32 (discriminant + 1) ------------------------------------------- */
#define RLNC_OK 0
#define RLNC_ERR_CODING_VECTOR_LENGTH_MISMATCH 1 /* errors.rs:6  */
#define RLNC_ERR_DATA_LENGTH_MISMATCH 2          /* errors.rs:8  */
#define RLNC_ERR_PIECE_COUNT_ZERO 3              /* errors.rs:10 */
#define RLNC_ERR_DATA_LENGTH_ZERO 4              /* errors.rs:12 */
#define RLNC_ERR_PIECE_LENGTH_ZERO 5             /* errors.rs:14 */
#define RLNC_ERR_NOT_ENOUGH_PIECES_TO_RECODE 6   /* errors.rs:17 */
#define RLNC_ERR_PIECE_LENGTH_TOO_SHORT 7        /* errors.rs:19 */
#define RLNC_ERR_PIECE_NOT_USEFUL 8              /* errors.rs:22 */
#define RLNC_ERR_RECEIVED_ALL_PIECES 9           /* errors.rs:24 */
#define RLNC_ERR_NOT_ALL_PIECES_RECEIVED_YET 10  /* errors.rs:26 */
#define RLNC_ERR_INVALID_DECODED_DATA_FORMAT 11  /* errors.rs:28 */
#define RLNC_ERR_INVALID_PIECE_LENGTH 12         /* errors.rs:30 */
#define RLNC_ERR_INVALID_OUTPUT_BUFFER 13        /* errors.rs:31 */
/* engine errors (no reference counterpart) */
#define RLNC_ERR_INVALID_ARGUMENT 100 /* null handle/pointer, size overflow, misuse of the ABI */
#define RLNC_ERR_DEVICE 101           /* HIP runtime / launch failure */
#define RLNC_ERR_OUT_OF_MEMORY 102    /* device or pinned-host allocation failed */
#define RLNC_ERR_NO_DEVICE 103        /* no usable gfx950 device */

const char *rlnc_status_name(int status); /* "Ok", "PieceNotUseful", ... (errors.rs:34-58 variant names) */
const char *rlnc_status_message(int status); /* Display text, errors.rs:34-58 */
const char *rlnc_last_error(void);        /* detail of the last engine error on this thread */
const char *rlnc_version(void);

/* ---- context: device + HIP stream + workspace ----------------------------------------------------- */
typedef struct rlnc_context rlnc_context;
int rlnc_context_create(int device, rlnc_context **out);
void rlnc_context_destroy(rlnc_context *ctx);
/* Launch on an external hipStream_t, taken literally: NULL is HIP's null (default) stream, which is what
 * torch.cuda.current_stream().cuda_stream returns for torch's default stream.  The caller keeps ownership. */
int rlnc_context_set_stream(rlnc_context *ctx, void *hip_stream);
/* Go back to the context's own non-blocking stream (the initial state). */
int rlnc_context_use_own_stream(rlnc_context *ctx);
void *rlnc_context_get_stream(rlnc_context *ctx);
int rlnc_context_synchronize(rlnc_context *ctx);
int rlnc_context_device(const rlnc_context *ctx);
/* *capturing = 1 when `hip_stream` (NULL: the null stream) is inside a HIP stream capture, else 0, asked of the HIP
 * runtime this library is linked against (the one a host framework such as torch shares).  On any runtime error it
 * returns RLNC_ERR_DEVICE and sets *capturing = 1 (a caller deciding whether it may synchronise assumes the worst). */
int rlnc_stream_is_capturing(void *hip_stream, int *capturing);
/* 1 when 16-byte vector loads/stores (and LDS-DMA) at any byte address return the right bytes on `device` (the
 * queue's unaligned memory mode, checked by a probe kernel when the first context on the device is created):
 * piece rows at any alignment (odd L from Encoder::new, data at byte k of a (k + L)-byte coded piece) then take the
 * vector kernels directly; 0: misaligned rows are copied through 16-byte-aligned scratch around them (same results).
 * -1 before a context exists on the device.  RLNC_ASSUME_ALIGNED_ONLY=1 in the environment forces 0 and skips the
 * probe.  The probe's misaligned accesses return wrong bytes in the "dword" alignment mode (detected: 0) but fault
 * the process under a strict alignment mode: on a queue configured that way (not the ROCm default for compute
 * queues) set RLNC_ASSUME_ALIGNED_ONLY=1 before the first rlnc_context_create. */
int rlnc_device_unaligned_vector_access(int device);

/* ---- L1: vector primitives on device buffers (src/common/simd/mod.rs) --------------------------------
 * Same scalar early-outs as the reference (0 → zero-fill / no-op, 1 → no-op / plain XOR). */
int rlnc_gf256_inplace_mul_vec_by_scalar(rlnc_context *ctx, uint8_t *vec_dev, size_t len, uint8_t scalar); /* :18-47 */
int rlnc_gf256_inplace_add_vectors(rlnc_context *ctx, uint8_t *dst_dev, const uint8_t *src_dev, size_t len); /* :58-76 */
int rlnc_gf256_mul_vec_by_scalar_then_add_into_vec(rlnc_context *ctx, uint8_t *dst_dev, const uint8_t *src_dev,
                                                   size_t len, uint8_t scalar); /* :89-119 */

/* ---- L2: the matrix-level hot operator (device buffers) -----------------------------------------------
 * out[o][i][0:width) = XOR_j coef[o][i][j] · in[o][j][0:width)   (i < n_out, j < n_in, o < n_obj)
 * Replaces the loop of gf256_mul_vec_by_scalar_then_add_into_vec calls in
 * Encoder::code_with_coding_vector (encoder.rs:138-141), batched over n_out coding vectors and n_obj
 * independent objects.  All strides in bytes.  hdr (optional, may be NULL) also receives the coefficient
 * rows, hdr[o][i][0:n_in) — the coeffs‖data framing of a full coded piece (encoder.rs:246-248).
 * Strides (this descriptor and rlnc_sparse_matmul_desc), checked before any launch, else RLNC_ERR_INVALID_ARGUMENT:
 *   - no stride is negative.  Any magnitude is addressed with 64 bits: objects or rows may lie more than 4 GiB apart
 *     (the bit-sliced programs take row strides below 2^32; a product with a larger one runs on the perm kernels).
 *   - what the call writes must not overlap, or its workgroups would race: with n_out > 1 the row stride of out is at
 *     least width, with n_obj > 1 its object stride is at least width, and with both the objects lie outside each
 *     other's rows, (n_out - 1) · row + width <= obj, or the rows outside each other's objects, (n_obj - 1) · obj +
 *     width <= row.  The same for hdr (when not NULL) with n_in bytes in place of width.  The stride of a dimension of
 *     one element is not used and may be anything >= 0.  out and hdr overlapping each other is not checked.
 *   - what the call reads (in, coef; idx, val) may have stride 0: one source row, one source object, one coefficient
 *     row or one coefficient matrix for all.
 * n_obj is limited by the launch alone (n_obj · row tiles · column blocks below 2^31): 65,536 objects and more are one
 * call. */
typedef struct rlnc_matmul_desc {
    const uint8_t *in;
    int64_t in_obj_stride, in_row_stride;
    const uint8_t *coef;
    int64_t coef_obj_stride, coef_row_stride;
    uint8_t *out;
    int64_t out_obj_stride, out_row_stride;
    uint8_t *hdr;
    int64_t hdr_obj_stride, hdr_row_stride;
    int32_t n_out, n_in;
    int64_t width;
    int32_t n_obj;
} rlnc_matmul_desc;
int rlnc_gf256_matmul(rlnc_context *ctx, const rlnc_matmul_desc *desc);
/* The same operator on a sparse coefficient matrix ("Sparse coding vectors" above):
 * out[o][i][0:width) = XOR_t val[o][i][t] · in[o][idx[o][i][t]][0:width)   (t < w), and hdr (optional) receives the
 * expanded dense rows hdr[o][i][0:n_in).  Strides in bytes; idx must be 4-byte aligned and its strides multiples of 4
 * (else RLNC_ERR_INVALID_ARGUMENT).  Any byte alignment of in / out / hdr and any width. */
typedef struct rlnc_sparse_matmul_desc {
    const uint8_t *in;
    int64_t in_obj_stride, in_row_stride;
    const int32_t *idx;
    int64_t idx_obj_stride, idx_row_stride;
    const uint8_t *val;
    int64_t val_obj_stride, val_row_stride;
    uint8_t *out;
    int64_t out_obj_stride, out_row_stride;
    uint8_t *hdr;
    int64_t hdr_obj_stride, hdr_row_stride;
    int32_t n_out, n_in, w, n_obj;
    int64_t width;
} rlnc_sparse_matmul_desc;
int rlnc_gf256_sparse_matmul(rlnc_context *ctx, const rlnc_sparse_matmul_desc *desc);
/* Kernel variant of the GF(2^8) matmul (all bit-identical; the switch exists for A/B measurement):
 *   0 = perm       3-bit split tables in LDS consumed by v_perm_b32
 *   1 = nibble     the reference's 4-bit LOW/HIGH tables looked up from LDS byte-wise (ablation)
 *   6 = bitsliced-jump  bit-plane transpose; each (row, source) is one call into a code block specialised for the
 *                  coefficient (16 v_bitop3_b32 XOR3s of plane combinations); full 4 KiB column blocks of 16-byte
 *                  aligned operands with >= 4 output rows, the rest goes to perm
 *   7 = bitsliced-jump-shared  as 6; in 32-row tiles each of the 4 waves builds one quarter of every source
 *                  row's plane combinations and the quarters are exchanged through LDS
 *   8 = bitsliced-jump-shared-8w  as 7; above 32 output rows, 64-row tiles of 8 waves (one workgroup per CU):
 *                  waves 0-3 stage the source and build the combinations three rows ahead, waves 4-7 only
 *                  read them and call; a barrier every third row -- the default
 * Other values fail with RLNC_ERR_INVALID_ARGUMENT, except in the diagnostic A/B build (make -C rlnc_amd/csrc ab:
 * librlnc_hip_ab.so), which keeps the measured history: 2 perm3, 3/4 wide2/wide4, 5 bitsliced with
 * register-indexed XORs, 9 column runs.
 * max_tile_rows caps the output rows per launch/workgroup (0 = automatic, else 1/2/4/8/16/32). */
int rlnc_set_kernel_variant(rlnc_context *ctx, int variant, int max_tile_rows);
/* Persistent tiles of the 64-row product (variant 8 above 32 output rows, batch calls on the context's stream): 0 =
 * chosen per launch (from two tiles per compute unit on), 1 = never (the one-tile-per-workgroup grid), 2 = every launch
 * the program takes, however few its tiles (tests).  max_workgroups: 0 = one workgroup per compute unit, else (8 or
 * more) at most that many, so that a small product gives each workgroup several tiles (tests).  Bit-identical for every
 * value. */
int rlnc_set_persistent_tiles(rlnc_context *ctx, int mode, int max_workgroups);
/* Column blocks per workgroup of variant 9 (A/B build only; 0 = automatic, else 1..64).  Bit-identical for every
 * value. */
int rlnc_set_column_run(rlnc_context *ctx, int col_run);
/* Where rlnc_decode_batch runs the coefficient elimination: 0 = auto (device when it fits LDS, default),
 * 1 = host threads, 2 = device, 5 = device, blocked clean run (k + m <= 256, else RLNC_ERR_INVALID_ARGUMENT; what 0
 * and 2 use when it applies).  All of these are exact replicas; the switch exists for A/B tests.  Every other value
 * is RLNC_ERR_INVALID_ARGUMENT and leaves the path as it was (3, 4 and 6 once named forms that are retired).
 * Rank mode 1 only (in mode 0 every decode call under them returns RLNC_ERR_INVALID_ARGUMENT, no silent fallback):
 * RLNC_DECODE_PATH_DEVICE_ANY (7) = the device for every shape -- the LDS kernel where it fits, beyond that the
 * workspace-resident true-rank kernels (rlnc_amd/csrc/rank_large.hip), so rlnc_decode_batch makes no host round trip
 * for the elimination, rlnc_decode_batch_device / _eliminate accept the shape, and a ragged decode with such objects
 * stays on the stream and can be captured; RLNC_DECODE_PATH_LARGE (8) = those kernels for every shape, small ones
 * included (tests and A/Bs).  Their limits: k <= 4096, m <= 8192, else RLNC_ERR_INVALID_ARGUMENT. */
#define RLNC_DECODE_PATH_DEVICE_ANY 7
#define RLNC_DECODE_PATH_LARGE 8
int rlnc_set_decode_path(rlnc_context *ctx, int path);
/* Device workspace, in bytes, that decode paths 7 and 8 keep in the context for num_objects objects of k x m beyond LDS
 * (it grows on the first eager call of a shape; under a HIP graph capture a grow is refused, see "HIP graphs").  0 for a
 * shape outside their limits.  Pure: needs no context and no GPU. */
size_t rlnc_decode_large_workspace_bytes(size_t k, size_t m, size_t num_objects);
/* Rank mode of the context (see "Rank mode" above): governs rlnc_decode_batch, rlnc_decode_batch_device,
 * rlnc_decode_batch_eliminate, rlnc_decode_ragged and rlnc_decode_host_stream, and is snapshotted by rlnc_decoder_new.
 * Other values: RLNC_ERR_INVALID_ARGUMENT.  In mode 1 decode paths 0 and 2 use the true-rank device kernel when it
 * fits, path 1 the host, paths 7 and 8 the device for every shape (rlnc_set_decode_path); path 5 names a
 * reference-mode kernel and makes the decode calls return RLNC_ERR_INVALID_ARGUMENT (no silent fallback). */
#define RLNC_RANK_MODE_REFERENCE 0
#define RLNC_RANK_MODE_TRUE 1
int rlnc_set_rank_mode(rlnc_context *ctx, int mode);
int rlnc_get_rank_mode(const rlnc_context *ctx); /* -1 for a null context */

/* ---- Encoder: src/full/encoder.rs ----------------------------------------------------------------- */
typedef struct rlnc_encoder rlnc_encoder;
/* Encoder::new (encoder.rs:85-106): pads with the 0x81 marker + zeros; data is host memory (copied). */
int rlnc_encoder_new(rlnc_context *ctx, const uint8_t *data, size_t data_len, size_t piece_count, rlnc_encoder **out);
/* Encoder::without_padding (encoder.rs:50-71). */
int rlnc_encoder_without_padding(rlnc_context *ctx, const uint8_t *data, size_t data_len, size_t piece_count,
                                 rlnc_encoder **out);
/* Device-resident source: piece_count rows of piece_len bytes at row_stride (borrowed, not copied; must
 * outlive the encoder). */
int rlnc_encoder_from_device(rlnc_context *ctx, const uint8_t *pieces_dev, size_t piece_count, size_t piece_len,
                             size_t row_stride, rlnc_encoder **out);
/* #[derive(Clone)] (encoder.rs:18): an independent copy (an owned source is copied on the device; a borrowed
 * device source stays borrowed). */
int rlnc_encoder_clone(const rlnc_encoder *enc, rlnc_encoder **out);
void rlnc_encoder_free(rlnc_encoder *enc);
size_t rlnc_encoder_get_piece_count(const rlnc_encoder *enc);              /* encoder.rs:27-29 */
size_t rlnc_encoder_get_piece_byte_len(const rlnc_encoder *enc);           /* encoder.rs:32-34 */
size_t rlnc_encoder_get_full_coded_piece_byte_len(const rlnc_encoder *enc); /* encoder.rs:37-39 */
/* Encoder::code_with_coding_vector (encoder.rs:128-144), host buffers. */
int rlnc_encoder_code_with_coding_vector(rlnc_encoder *enc, const uint8_t *coding_vector, size_t cv_len,
                                         uint8_t *coded_data, size_t coded_len);
/* Encoder::code_with_buf (encoder.rs:241-250): random_bytes are the piece_count bytes rng.fill_bytes
 * would have written into the coefficient prefix (n_random must equal piece_count, else
 * CodingVectorLengthMismatch); the output length is checked first, like the reference. */
int rlnc_encoder_code_with_buf(rlnc_encoder *enc, const uint8_t *random_bytes, size_t n_random,
                               uint8_t *full_coded_piece, size_t full_len);
/* n coded pieces in one launch, device buffers: coeffs_dev [n][k] → out_dev [n][k+L] (coeffs‖data,
 * row stride out_row_stride >= k+L; pass 0 for k+L). */
int rlnc_encoder_code_batch_device(rlnc_encoder *enc, const uint8_t *coeffs_dev, size_t n, uint8_t *out_dev,
                                   size_t out_row_stride);
/* The sparse twin: idx_dev int32 [n][w], val_dev uint8 [n][w] ("Sparse coding vectors") → out_dev [n][k+L], the
 * expanded dense coefficients ‖ data. */
int rlnc_encoder_code_sparse_batch_device(rlnc_encoder *enc, const int32_t *idx_dev, const uint8_t *val_dev, size_t w,
                                          size_t n, uint8_t *out_dev, size_t out_row_stride);

/* ---- Recoder: src/full/recoder.rs ---------------------------------------------------------------- */
typedef struct rlnc_recoder rlnc_recoder;
/* Recoder::new (recoder.rs:68-108); data = concatenated full coded pieces (host, copied). */
int rlnc_recoder_new(rlnc_context *ctx, const uint8_t *data, size_t data_len, size_t full_coded_piece_byte_len,
                     size_t num_pieces_coded_together, rlnc_recoder **out);
int rlnc_recoder_clone(const rlnc_recoder *rec, rlnc_recoder **out); /* #[derive(Clone)], recoder.rs:12 */
void rlnc_recoder_free(rlnc_recoder *rec);
size_t rlnc_recoder_get_original_num_pieces_coded_together(const rlnc_recoder *rec); /* recoder.rs:26-28 */
size_t rlnc_recoder_get_num_pieces_recoded_together(const rlnc_recoder *rec);       /* recoder.rs:31-33 */
size_t rlnc_recoder_get_piece_byte_len(const rlnc_recoder *rec);                    /* recoder.rs:36-38 */
size_t rlnc_recoder_get_full_coded_piece_byte_len(const rlnc_recoder *rec);         /* recoder.rs:41-43 */
/* Recoder::recode_with_buf (recoder.rs:122-153): random_bytes = the n recoding coefficients that
 * rng.fill_bytes would have drawn (n_random must equal n, else CodingVectorLengthMismatch). */
int rlnc_recoder_recode_with_buf(rlnc_recoder *rec, const uint8_t *random_bytes, size_t n_random,
                                 uint8_t *full_recoded_piece, size_t full_len);
/* count recoded pieces in one launch: r_dev [count][n] → out_dev [count][k+L] (device). */
int rlnc_recoder_recode_batch_device(rlnc_recoder *rec, const uint8_t *r_dev, size_t count, uint8_t *out_dev);

/* ---- Decoder: src/full/decoder.rs ----------------------------------------------------------------- */
typedef struct rlnc_decoder rlnc_decoder;
/* Decoder::new(piece_byte_len, required_piece_count) (decoder.rs:65-80; note the argument order). */
int rlnc_decoder_new(rlnc_context *ctx, size_t piece_byte_len, size_t required_piece_count, rlnc_decoder **out);
/* #[derive(Clone)] (decoder.rs:8): elimination state, counters and the received data rows are copied. */
int rlnc_decoder_clone(const rlnc_decoder *dec, rlnc_decoder **out);
/* The rank mode the decoder took from its context when it was created (a clone keeps it; a later
 * rlnc_set_rank_mode on the context does not change it).  -1 for a null decoder. */
int rlnc_decoder_get_rank_mode(const rlnc_decoder *dec);
void rlnc_decoder_free(rlnc_decoder *dec);
/* Decoder::decode (decoder.rs:96-118): Ok / PieceNotUseful / ReceivedAllPieces / InvalidPieceLength.
 * The accept/reject answer is immediate (exact replica of the diagonal-pivot RREF on the coefficient
 * block); the data rows are combined on the device when the data is requested.  The piece's data bytes are
 * staged in pinned memory before the call returns (the caller may reuse its buffer at once); staged pieces are
 * copied to the device in batches on the context's upload stream, at the latest when the decoder's rows are next
 * used (get_decoded_data, clone, drop), which is ordered after them. */
int rlnc_decoder_decode(rlnc_decoder *dec, const uint8_t *full_coded_piece, size_t len);
/* Same, piece already in HBM (only its k coefficient bytes are read back to the host). */
int rlnc_decoder_decode_device(rlnc_decoder *dec, const uint8_t *piece_dev, size_t len);
int rlnc_decoder_is_already_decoded(const rlnc_decoder *dec);                   /* decoder.rs:121-123 */
size_t rlnc_decoder_get_num_pieces_coded_together(const rlnc_decoder *dec);     /* decoder.rs:25-27 */
size_t rlnc_decoder_get_piece_byte_len(const rlnc_decoder *dec);                /* decoder.rs:30-32 */
size_t rlnc_decoder_get_full_coded_piece_byte_len(const rlnc_decoder *dec);     /* decoder.rs:35-37 */
size_t rlnc_decoder_get_received_piece_count(const rlnc_decoder *dec);          /* decoder.rs:40-42 */
size_t rlnc_decoder_get_useful_piece_count(const rlnc_decoder *dec);            /* decoder.rs:45-47 */
size_t rlnc_decoder_get_remaining_piece_count(const rlnc_decoder *dec);         /* decoder.rs:50-52 */
/* Decoder::get_decoded_data (decoder.rs:136-177) into host memory: out must hold k*L bytes (the padded
 * size); *out_len receives the unpadded length.  Does not consume the decoder (the C caller frees it). */
int rlnc_decoder_get_decoded_data(rlnc_decoder *dec, uint8_t *out, size_t out_cap, size_t *out_len);
/* Same into device memory (out_dev holds k*L bytes). */
int rlnc_decoder_get_decoded_data_device(rlnc_decoder *dec, uint8_t *out_dev, size_t out_cap, size_t *out_len);

/* ---- multi-object batch API (device-resident) -------------------------------
 * Layouts (bytes, contiguous): src [obj][k][L]; coeffs [obj][n][k]; pieces [obj][n][k+L] (coeffs‖data). */
/* n coded pieces for each of num_objects objects (encoder.rs:241-250 × n × objects). */
int rlnc_encode_batch(rlnc_context *ctx, const uint8_t *src_dev, size_t k, size_t L, size_t num_objects,
                      const uint8_t *coeffs_dev, size_t n, uint8_t *pieces_dev);
/* rlnc_encode_batch in two parts, for pipelining a decoder's elimination against the data work (bench.py):
 * the coefficient headers alone (pieces[o][i][0..k) = coeffs[o][i], one strided copy) and the data alone
 * (pieces[o][i][k..k+L)).  Together they write exactly what rlnc_encode_batch writes. */
int rlnc_encode_batch_headers(rlnc_context *ctx, const uint8_t *coeffs_dev, size_t k, size_t L, size_t num_objects,
                              size_t n, uint8_t *pieces_dev);
int rlnc_encode_batch_data(rlnc_context *ctx, const uint8_t *src_dev, size_t k, size_t L, size_t num_objects,
                           const uint8_t *coeffs_dev, size_t n, uint8_t *pieces_dev);
/* rlnc_encode_batch_data with the kernel's per-coefficient code-block address stream written ahead: _prepare runs
 * the (coefficient-only) address launch on ITS context's stream into plan_dev (device memory of at least
 * rlnc_encode_batch_plan_bytes bytes), e.g. on a side stream beside other work; _data_planned, with the same
 * arguments and the same kernel variant, then runs the product without that launch (the caller orders it after the
 * prepare, e.g. with an event).  A plan buffer serves the product it was prepared for.  The library remembers each
 * prepare by the plan buffer's address with its arguments (buffers, shape, device, kernel variant) and
 * _data_planned returns InvalidArgument when those arguments differ.  What it cannot see is the memory itself: the
 * caller keeps the plan buffer alive and unwritten, and the coefficient bytes unchanged, from the prepare to the
 * product.  A plan buffer freed and reallocated at the same address, or coefficients rewritten in place, must be
 * prepared again: the product takes the buffer's entries as code addresses, so a stale plan gives wrong bytes and
 * a plan buffer overwritten with other data is undefined behaviour, like a dangling pointer.  Writes exactly what
 * rlnc_encode_batch_data writes. */
size_t rlnc_encode_batch_plan_bytes(size_t k, size_t num_objects, size_t n);
int rlnc_encode_batch_prepare(rlnc_context *ctx, const uint8_t *src_dev, size_t k, size_t L, size_t num_objects,
                              const uint8_t *coeffs_dev, size_t n, uint8_t *pieces_dev, void *plan_dev,
                              size_t plan_bytes);
int rlnc_encode_batch_data_planned(rlnc_context *ctx, const uint8_t *src_dev, size_t k, size_t L, size_t num_objects,
                                   const uint8_t *coeffs_dev, size_t n, uint8_t *pieces_dev, const void *plan_dev);

/* What rlnc_encode_emit writes in object_dev for a packet index at or beyond the emitted count. */
#define RLNC_EMIT_NONE (-1)
/* Bytes of rlnc_encode_emit's plan buffer: two int32 arrays of num_objects entries (an object's first packet, its
 * grant), the sums of the chunks of 1,024 objects and the total, each rounded up to 16 bytes, and for
 * max_per_object >= 4 the block-address streams of the product, ceil(max_per_object / tile rows) x k x tile rows
 * entries of 8 bytes per object (tile rows = 8, 16, 32 or 64: the program of max_per_object rows) plus 512.  A
 * multiple of 16, non-decreasing in each argument inside the limits; 0 when an argument is 0, k > 4,096,
 * max_per_object > 4,096, num_objects > 1,048,576 or n > 1,048,576.  Pure: needs no context and no GPU. */
size_t rlnc_encode_emit_plan_bytes(size_t k, size_t max_per_object, size_t num_objects, size_t n);
/* The sender's call: want_dev[o] coded pieces per object, read on the device, written as one packed run of packets
 * with an object id per packet and a device-side count.  (out_dev, object_dev, count_dev) go into
 * rlnc_decode_stream_accept(arrivals_dev, object_dev, ..., count_dev) unchanged, so that emit -> wire -> (accept, push,
 * deliver, compact) runs with no host decision on either end.  src_dev is [obj][k][L] with src_obj_stride bytes between
 * objects (0 = k*L); r_dev is uint8 [n][k], packet i's random bytes: the random bytes are indexed by packet, not by
 * object, so a caller supplies n x k bytes whatever the split.  n is the host-known packet capacity of out_dev,
 * object_dev and r_dev.  Packet i starts at out_dev + i * out_stride (0 = k + L), at any byte address.
 *   Let w_o = min(max(want_dev[o], 0), max_per_object), each entry read once; base_o = min(sum of w_o' for o' < o, n)
 *   (object-major order); g_o = min(w_o, n - base_o); total = min(sum of w_o, n).  Every running sum saturates at n:
 *   with n <= 2^20 and w <= 4,096 no sum needs more than int32.
 *   Packet i with base_o <= i < base_o + g_o belongs to object o: object_dev[i] = o, out[i][0..k) = r_dev[i][0..k),
 *   out[i][k..k+L) = XOR_j r_dev[i][j] . src[o][j][0..L).
 *   object_dev[i] = RLNC_EMIT_NONE for total <= i < n; every entry of object_dev is written.  *count_dev = total.
 *   granted_dev (int32 [num_objects], may be NULL): granted_dev[o] = g_o.
 * Truncation: when the wants exceed n the low-numbered objects are served first and granted_dev says who was cut;
 * fairness under truncation is the caller's (e.g. subtract granted from want and call again).
 * Equivalence: byte for byte packet i is Encoder::code_with_buf of object o with the random bytes r_dev[i]
 * (encoder.rs:241-250), and what rlnc_encode_batch writes for that coding vector.
 * Footprint.  Written: the k + L bytes of packets [0, total); object_dev[0 .. n); *count_dev; granted_dev[0 ..
 * num_objects); the plan buffer.  Never written: any byte of out_dev from packet total on; the bytes between k + L and
 * out_stride; src_dev, want_dev, r_dev (rows of r_dev at or beyond total are not read either).  plan_dev is caller-owned
 * scratch, 16-byte aligned and at least rlnc_encode_emit_plan_bytes long; its contents after the call are unspecified.
 * Launches: at most six on the context's stream -- scan (a workgroup per 1,024 objects: w_o and its prefix inside the
 * chunk), base (one workgroup: the prefix over the chunk sums, base_o, g_o, granted_dev, *count_dev; no atomics, no
 * workgroup waits for another, so the split is deterministic), label (object_dev and the k header bytes), the
 * block-address streams of the objects with g_o >= 4, the bit-sliced product over the whole 4 KiB column blocks of L
 * (objects x row tiles x column blocks; the program of max_per_object rows serves the whole call, so a sender in its
 * late rounds passes a small max_per_object), and the perm product over the rest: L mod 4,096, all of L for objects
 * with 1 <= g_o < 4 (the tile programs take products of >= 4 rows; the grant is known on the device only) and for
 * every object when the operands are not the program's (a row stride of 2^32 or more; misaligned operands where
 * rlnc_device_unaligned_vector_access is 0).  The call never synchronises and grows no context workspace, but for the
 * shared programs' one block-table probe per device: the call can be captured after one eager call on the device, as
 * deliver and recode; a first call inside a capture runs every column in the perm product, the same bytes.
 * Checks, in rlnc_encode_batch's order first: a null handle RLNC_ERR_INVALID_ARGUMENT; k == 0 PieceCountZero; L == 0
 * PieceLengthZero; n == 0, num_objects == 0 or max_per_object == 0 RLNC_OK, nothing launched and nothing written; then
 * k <= 4,096; max_per_object <= 4,096; n <= 1,048,576; num_objects <= 1,048,576; L <= 2^40; out_stride 0 or in
 * [k + L, 2^42]; src_obj_stride 0 or >= k*L (and num_objects * src_obj_stride within 2^62); src_dev, want_dev, r_dev, out_dev, object_dev and count_dev non-null;
 * plan_dev non-null, aligned and long enough; every launch within 2^31 - 1 workgroups.  Each failure is
 * RLNC_ERR_INVALID_ARGUMENT, names the limit in rlnc_last_error and writes nothing.  Measurements: DESIGN.md §4.2.5. */
int rlnc_encode_emit(rlnc_context *ctx, const uint8_t *src_dev, size_t src_obj_stride, size_t k, size_t L,
                     size_t num_objects, const int32_t *want_dev, size_t max_per_object, const uint8_t *r_dev, size_t n,
                     uint8_t *out_dev, size_t out_stride, int32_t *object_dev, int32_t *count_dev,
                     int32_t *granted_dev, void *plan_dev, size_t plan_bytes);

/* count recoded pieces per object from n received pieces: r [obj][count][n] → out [obj][count][k+L]
 * (recoder.rs:122-153; coefficient header and data are one linear combination of the full pieces). */
int rlnc_recode_batch(rlnc_context *ctx, const uint8_t *pieces_dev, size_t k, size_t L, size_t n,
                      size_t num_objects, const uint8_t *r_dev, size_t count, uint8_t *out_dev);
/* The sparse twins ("Sparse coding vectors"): idx int32 [obj][n][w], val uint8 [obj][n][w] → pieces [obj][n][k+L],
 * the expanded dense header ‖ data: exactly what rlnc_encode_batch writes on the expanded coefficients.  Checks in
 * rlnc_encode_batch's order; w above 0x7FFFFFFF or a misaligned idx: RLNC_ERR_INVALID_ARGUMENT. */
int rlnc_encode_batch_sparse(rlnc_context *ctx, const uint8_t *src_dev, size_t k, size_t L, size_t num_objects,
                             const int32_t *idx_dev, const uint8_t *val_dev, size_t w, size_t n, uint8_t *pieces_dev);
/* idx over the n received pieces: idx / val [obj][count][w] → out [obj][count][k+L] (one linear map over the k+L
 * bytes of the full pieces, as rlnc_recode_batch).  Checks in rlnc_recode_batch's order. */
int rlnc_recode_batch_sparse(rlnc_context *ctx, const uint8_t *pieces_dev, size_t k, size_t L, size_t n,
                             size_t num_objects, const int32_t *idx_dev, const uint8_t *val_dev, size_t w,
                             size_t count, uint8_t *out_dev);
/* Feeds pieces 0..m-1 of every object, in order, to a fresh Decoder (decoder.rs:96-118) and extracts the
 * data (decoder.rs:136-177).  decoded_dev [obj][k][L] receives the padded payload rows in the reference's
 * row order.  pieces_obj_stride = bytes between objects' first pieces (0 = m*(k+L), i.e. dense; a larger
 * stride decodes from the first m of more coded pieces in place).  Host outputs (each may be NULL): piece_status [obj][m] (status of each decode() call),
 * object_status [obj] (Ok / NotAllPiecesReceivedYet / InvalidDecodedDataFormat of get_decoded_data),
 * data_len [obj] (unpadded length when Ok).  data_len is written for every object: 0 for one that is not Ok (rank < k
 * or no valid marker), here and in rlnc_decode_batch_device, rlnc_decode_batch_apply / _apply_planned and
 * rlnc_decode_ragged.  Synchronous. */
int rlnc_decode_batch(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k, size_t L,
                      size_t m, size_t num_objects, uint8_t *decoded_dev, int32_t *piece_status,
                      int32_t *object_status, uint64_t *data_len);

/* Fully asynchronous variant: everything stays on the device (statuses int32 [obj][m] and [obj], unpadded
 * lengths int64 [obj], all device pointers).  The exact elimination runs on the device (one wave per
 * object, LDS-resident [coeffs | E]; requires (k+1)·4·ceil_pow2((k+m)/4) + 8 KiB <= 160 KiB). */
int rlnc_decode_batch_device(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k,
                             size_t L, size_t m, size_t num_objects, uint8_t *decoded_dev, int32_t *piece_status_dev,
                             int32_t *object_status_dev, int64_t *data_len_dev);

/* rlnc_decode_batch_device in two parts (same results): the exact elimination, which reads only the k
 * coefficient bytes of each piece — T_dev [obj][k][m] (decoded rows = T × received data rows; rows >= rank
 * zero), per-piece statuses, ranks int32 [obj] — and the data side (T × data + the marker scan).  The two may
 * run on different contexts/streams; the caller orders them (e.g. a HIP event). */
int rlnc_decode_batch_eliminate(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k,
                                size_t L, size_t m, size_t num_objects, uint8_t *T_dev, int32_t *piece_status_dev,
                                int32_t *rank_dev);
int rlnc_decode_batch_apply(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k,
                            size_t L, size_t m, size_t num_objects, const uint8_t *T_dev, const int32_t *rank_dev,
                            uint8_t *decoded_dev, int32_t *object_status_dev, int64_t *data_len_dev);
/* rlnc_decode_batch_apply with the T x data product's code-block address stream written ahead, the decode's form of
 * rlnc_encode_batch_prepare / _data_planned: _prepare runs the (T-only) address launch on ITS context's stream into
 * plan_dev (device memory of at least rlnc_decode_batch_apply_plan_bytes bytes) once T is final -- e.g. on the
 * elimination's stream right behind rlnc_decode_batch_eliminate -- and _planned, with the same arguments and kernel
 * variant, runs the product and the marker scan without it (the caller orders it after the prepare).  The plan
 * contract is the encode plan's: prepares are remembered by the plan buffer's address with their arguments and
 * _planned returns InvalidArgument when those differ; the caller keeps the plan buffer alive and unwritten and T
 * unchanged from the prepare to the product.  Writes exactly what rlnc_decode_batch_apply writes. */
size_t rlnc_decode_batch_apply_plan_bytes(size_t k, size_t m, size_t num_objects);
int rlnc_decode_batch_apply_prepare(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k,
                                    size_t L, size_t m, size_t num_objects, const uint8_t *T_dev, uint8_t *decoded_dev,
                                    void *plan_dev, size_t plan_bytes);
int rlnc_decode_batch_apply_planned(rlnc_context *ctx, const uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k,
                                    size_t L, size_t m, size_t num_objects, const uint8_t *T_dev,
                                    const int32_t *rank_dev, uint8_t *decoded_dev, int32_t *object_status_dev,
                                    int64_t *data_len_dev, const void *plan_dev);

/* ---- decode streams: the device decode, resumable ("Decode streams" above) ----------------------------------------
 * A slot of a stream's status array that no push has answered yet. */
#define RLNC_STATUS_PENDING (-1)
/* Bytes of the state buffer of num_objects objects of generation size k with m piece slots each: a multiple of 16;
 * 0 outside the limits, exactly where rlnc_decode_large_workspace_bytes is 0.  Pure: needs no context and no GPU. */
size_t rlnc_decode_stream_state_bytes(size_t k, size_t m, size_t num_objects);
/* Starts a stream in state_dev (caller-owned device memory, 16-byte aligned, state_bytes >= the above): rank, pieces
 * answered and target of every object become 0.  One asynchronous launch on the context's stream.  The library
 * remembers each init by the state buffer's address with (device, k, m, num_objects), as it remembers plan buffers;
 * push and snapshot with other values, or on a buffer never initialised, return RLNC_ERR_INVALID_ARGUMENT (it keeps
 * the 256 most recently initialised buffers: a stream is many objects, a process needs few of them).  What it
 * cannot see is the caller's contract: the state buffer stays alive and unwritten by anyone else between the calls
 * (a buffer freed and reallocated at the same address must be initialised again), and the slots below avail are not
 * rewritten once they have been pushed.  All three calls return RLNC_ERR_INVALID_ARGUMENT on a context in rank mode 0
 * (no silent fallback), for a null handle or state, a misaligned or short state buffer and a shape outside the
 * limits; the decode path setting is irrelevant. */
int rlnc_decode_stream_init(rlnc_context *ctx, void *state_dev, size_t state_bytes, size_t k, size_t m,
                            size_t num_objects);
/* Which kernels rlnc_decode_stream_push runs on this context (per context, like rlnc_set_decode_path; any other value
 * is RLNC_ERR_INVALID_ARGUMENT and leaves the form as it was):
 *   RLNC_STREAM_FORM_WORKSPACE  the workspace form, every shape a stream takes: 1 + 3 * ceil(min(max_new, m) / B)
 *                               launches, plus one when rank_dev or answered_dev is asked for.
 *   RLNC_STREAM_FORM_LDS        the LDS form: one launch per push, rank_dev / answered_dev included; avail_dev is read
 *                               once per object in that launch.  An object with nothing new has no byte of its state
 *                               written.  A push of a shape for which rlnc_decode_stream_lds_fits is 0 returns
 *                               RLNC_ERR_INVALID_ARGUMENT and names the limit (no silent fallback to the other form).
 *   RLNC_STREAM_FORM_AUTO       the default: the LDS form for k <= 48 with m <= 64, the workspace form otherwise.  That
 *                               is where the LDS form was faster on every measured line (1.3-4x; dense and density-4
 *                               vectors, one push of everything down to one piece per push, 32 to 4,096 objects).
 *                               From k = 64 up the workspace form wins pushes of many pieces (2.5x for one push of
 *                               everything at k = 200) and the LDS form pushes of one to three (2-3x): a receiver
 *                               of such generations that pushes piece by piece sets RLNC_STREAM_FORM_LDS itself.
 *                               One MI355X, profiles/r14_stream_lds.jsonl, DESIGN.md §4.2.4.
 * The state buffer, init, snapshot and rlnc_decode_stream_state_bytes are the same for all three, and the forms may
 * alternate from push to push on one state buffer: the state after a push does not depend on the forms used so far. */
#define RLNC_STREAM_FORM_AUTO 0
#define RLNC_STREAM_FORM_WORKSPACE 1
#define RLNC_STREAM_FORM_LDS 2
int rlnc_set_stream_form(rlnc_context *ctx, int form);
/* 1 when the LDS form takes generation size k with m piece slots: 8192 + 4*(k*D + 2*D + m*ceil(k/4) + m + 2*k +
 * ceil(k/4)) <= 160 KiB with D = ceil(k/4) + ceil(m/4), the condition of the mode-1 LDS kernel ("Rank mode" above);
 * k = 200 with m = 210 fits, and so does k = 4 with m = 8192 (rows of more than 256 dwords).  0 otherwise, and for
 * k == 0 or m == 0.  Pure: needs no context and no GPU. */
int rlnc_decode_stream_lds_fits(size_t k, size_t m);
/* Object o advances from done_o, the slots answered so far, to min(max(avail_dev[o], done_o), m, done_o + max_new):
 * those slots of pieces_dev (addressed as in rlnc_decode_batch_eliminate: object stride in bytes, 0 = m*(k+L)) are
 * pushed to its decoder in order.  An avail below done_o changes nothing; one above m is clamped.  Asynchronous on
 * the context's stream, never synchronises and grows no context workspace, so it can be captured into a HIP graph
 * and replayed while avail_dev changes between replays.  avail_dev (int32 [num_objects]) is read by the call's first
 * launch only: the caller may overwrite it as soon as the call returns.  In the workspace form 1 + 3 *
 * ceil(min(max_new, m) / B) launches (B <= 32 pieces per block), plus one when rank_dev or answered_dev (int32
 * [num_objects], each may be NULL) are asked for: every object's rank and done_o after the push; in the LDS form one
 * launch in all (rlnc_set_stream_form).  An object whose rank is k still consumes its slots
 * (ReceivedAllPieces).  k == 0 PieceCountZero, then L == 0 PieceLengthZero; max_new == 0 or num_objects == 0: RLNC_OK,
 * nothing launched. */
int rlnc_decode_stream_push(rlnc_context *ctx, void *state_dev, size_t state_bytes, const uint8_t *pieces_dev,
                            size_t pieces_obj_stride, size_t k, size_t L, size_t m, size_t num_objects,
                            const int32_t *avail_dev, size_t max_new, int32_t *rank_dev, int32_t *answered_dev);
/* Reclaims the slots of useless arrivals and retires objects in place, so that m bounds the pieces an object holds
 * and not the arrivals it has seen, and a finished object's place takes the next generation while the others go on.
 * rank, done_o and the statuses are taken as the last push left them: the caller orders the call after that push (the
 * context's stream does).  Per object o:
 *   retired  (retire_dev != NULL and retire_dev[o] != 0) the four state words become 0, as init leaves them; nothing
 *            else of the object's state and no byte of its pieces is written; kept_dev[o][*] = -1, answered_dev[o] = 0.
 *   else     let u_0 < u_1 < ... < u_{r-1} be the slots below done_o whose status is Ok (r = rank).  The piece in slot
 *            u_j moves to slot j, all k + L bytes; byte j of every stored row's e part becomes the old byte u_j and the
 *            bytes from r on 0; the statuses of slots 0 .. r - 1 become Ok; the state words become {r, r, r, r}.
 *            kept_dev[o][j] = u_j for j < r and -1 from r on; answered_dev[o] = r, the slot the object's next arrival
 *            goes into: the caller's avail restarts from there.
 *   idle     an object that is not retired and has no useless slot below done_o (done_o == rank, 0 included): no byte
 *            of its state or pieces is written; kept_dev (the identity below r) and answered_dev are.
 * pieces_dev == NULL: only the state is compacted, L and the stride are ignored -- for callers that keep their pieces
 * behind an indirection of their own and move them by kept_dev.
 * Equivalence: after the call the live state -- state words 0 and 2, piv[0 .. rank), St[0 .. done), R[0 .. rank)[D] --
 * holds exactly the bytes a freshly initialised stream of the same shape holds after one push of the kept pieces in
 * order (a useless piece left a zero column of e in every stored row, and the stored rows are the unique reduced rows
 * of the span, so nothing is eliminated again: the call renumbers columns).  Later pushes (either form, alternating
 * freely), snapshot and apply need no change and answer as a decoder that had seen the kept pieces and then whatever is
 * pushed next.
 * Footprint.  Written: the four state words; St[0 .. r); the e part of the stored rows 0 .. r - 1, all ceil(m/4)
 * dwords; the state's Q region (scratch: the list u); the pieces slots j < r with u_j != j; the outputs.  Never
 * written: piv; the rows' coefficient part; rows and statuses at or beyond r; pieces slots at or beyond r; the bytes
 * between m*(k+L) and the object stride; retire_dev.
 * Four launches (three without pieces) on the context's stream, whichever push form wrote the state, every shape a
 * stream takes; never synchronises and grows no context workspace, so (compact, push) is capturable as a linear
 * graph.  The piece move takes 16-byte accesses at any byte address where rlnc_device_unaligned_vector_access is 1,
 * single bytes otherwise.  Checks in the order of push: a null handle RLNC_ERR_INVALID_ARGUMENT; k == 0
 * PieceCountZero; with pieces_dev, L == 0 PieceLengthZero; num_objects == 0 RLNC_OK, nothing launched; then the state
 * and shape checks of push (rank mode 0, a buffer never initialised or initialised for another shape) and
 * pieces_obj_stride (0 = m*(k+L)) >= m*(k+L): RLNC_ERR_INVALID_ARGUMENT, nothing written. */
int rlnc_decode_stream_compact(rlnc_context *ctx, void *state_dev, size_t state_bytes, uint8_t *pieces_dev,
                               size_t pieces_obj_stride, size_t k, size_t L, size_t m, size_t num_objects,
                               const int32_t *retire_dev, int32_t *kept_dev, int32_t *answered_dev);
/* What the stream holds now, in the layout of rlnc_decode_batch_eliminate (one launch; any output may be NULL; the
 * state is not modified and a later push continues from it): T_dev [obj][k][m], rows in pivot order, rows >= rank
 * and columns >= done_o zero; piece_status_dev [obj][m], the decoder's answer for the slots below done_o and
 * RLNC_STATUS_PENDING for the others; rank_dev [obj].  T_dev and rank_dev go straight into rlnc_decode_batch_apply
 * (NotAllPiecesReceivedYet for an object below rank k). */
int rlnc_decode_stream_snapshot(rlnc_context *ctx, const void *state_dev, size_t state_bytes, size_t k, size_t m,
                                size_t num_objects, uint8_t *T_dev, int32_t *piece_status_dev, int32_t *rank_dev);
/* Bytes of rlnc_decode_stream_deliver's plan buffer: the T extract [obj][k][m] and the block-address stream of the
 * product (8 bytes per entry of ceil(k / tile rows) * tile rows x m coefficients per object, tile rows = 8, 16, 32 or 64
 * by k).  A multiple of 16, at least num_objects * k * m; 0 exactly where rlnc_decode_stream_state_bytes is 0.  Pure:
 * needs no context and no GPU. */
size_t rlnc_decode_stream_deliver_plan_bytes(size_t k, size_t m, size_t num_objects);
/* Delivers the finished objects of a stream, and only those, chosen on the device: the receive loop's middle call,
 * push -> deliver -> compact(retire).  rank and done_o are taken as the last push or compaction left them (the
 * context's stream orders the calls).  Per object o:
 *   unselected   (select_dev != NULL and select_dev[o] == 0) nothing of the object is written: no byte of
 *                decoded_dev[o], neither object_status_dev[o] nor data_len_dev[o].
 *   rank < k     object_status_dev[o] = NotAllPiecesReceivedYet, data_len_dev[o] = 0; no byte of decoded_dev[o] is
 *                written and no product work is done for it (its workgroups return on reading the state).
 *   rank == k    decoded_dev[o] ([obj][k][L], all k * L bytes) = T_o x the data rows of slots 0 .. done_o - 1;
 *                object_status_dev[o] and data_len_dev[o] exactly what rlnc_decode_batch_apply writes for the object: Ok
 *                with the marker index, or InvalidDecodedDataFormat with 0.
 * The state, the pieces and select_dev are only read: a later push continues from the state unchanged.  plan_dev is
 * caller-owned scratch, 16-byte aligned and at least rlnc_decode_stream_deliver_plan_bytes long; its contents after the
 * call are unspecified.
 * Columns.  A delivering object's product takes done_o source rows, read on the device, not m (T's columns from done_o
 * on are zero).  After rlnc_decode_stream_compact done_o = rank = k: the minimal k x k x L product.  Without a
 * compaction it costs done_o / k of that, so a receiver with many useless arrivals calls compact, then deliver.
 * Launches: at most five on the context's stream -- the snapshot's T extract, the block-address streams of the
 * delivering objects, the bit-sliced product over the whole 4 KiB column blocks of L (the program of the batch
 * products, one workgroup per object x row tile x column block), a perm-multiply product over what that does not take
 * (L mod 4096; everything for k < 4 or operands the program refuses), the marker scan of the selected objects.  The
 * call never synchronises and grows no context workspace, so (push, deliver, compact) can be captured as a linear HIP
 * graph -- after one eager deliver on the device: the 32- and 64-row programs look up their block table once per
 * device, synchronously, and a first deliver inside a capture runs every column in the perm-multiply kernel instead
 * (the same bytes, slower).
 * Checks in the order of push and compact: a null handle RLNC_ERR_INVALID_ARGUMENT; k == 0 PieceCountZero; L == 0
 * PieceLengthZero; num_objects == 0 RLNC_OK, nothing launched; then the state and shape checks of push (rank mode 0, a
 * buffer never initialised or initialised for another shape); pieces_obj_stride (0 = m*(k+L)) >= m*(k+L); pieces_dev,
 * decoded_dev, object_status_dev and data_len_dev non-null; plan_dev non-null, aligned and long enough; every launch
 * within 2^31 - 1 workgroups.  Each failure is RLNC_ERR_INVALID_ARGUMENT, names the limit in rlnc_last_error and
 * writes nothing.  rlnc_decode_stream_snapshot + rlnc_decode_batch_apply remain the way to the product over every
 * object; measurements of both: DESIGN.md §4.2.4, "Delivery". */
int rlnc_decode_stream_deliver(rlnc_context *ctx, const void *state_dev, size_t state_bytes, const uint8_t *pieces_dev,
                               size_t pieces_obj_stride, size_t k, size_t L, size_t m, size_t num_objects,
                               const int32_t *select_dev, uint8_t *decoded_dev, int32_t *object_status_dev,
                               int64_t *data_len_dev, void *plan_dev, size_t plan_bytes);

/* Bytes of rlnc_decode_stream_recode's plan buffer: the expanded coefficients C [obj][count][m] and the block-address
 * stream of the product (8 bytes per entry of ceil(count / tile rows) * tile rows x m coefficients per object, tile rows
 * = 8, 16, 32 or 64 by count).  A multiple of 16, non-decreasing in count; 0 exactly where
 * rlnc_decode_stream_state_bytes is 0 or count is outside [1, 4096].  Pure: needs no context and no GPU. */
size_t rlnc_decode_stream_recode_plan_bytes(size_t k, size_t m, size_t count, size_t num_objects);
/* Recodes for a relay from the pieces a stream's objects hold, found on the device: count recoded pieces per selected
 * object, each a random combination of the object's useful pieces.  rank and done_o are taken as the last push or
 * compaction left them (the context's stream orders the calls).  Let u_0 < ... < u_{r-1} be the slots below done_o
 * whose status is Ok, r = rank: the list rlnc_decode_stream_compact keeps.  Pieces answered PieceNotUseful or
 * ReceivedAllPieces are left out -- they add nothing to the span.  r_dev is uint8 [obj][count][k], the bytes
 * rng.fill_bytes would draw (recoder.rs:131), supplied by the caller as in every other call here; out_dev is
 * [obj][count][k+L], contiguous; status_dev int32 [obj]; used_dev int32 [obj], may be NULL.  Per object o:
 *   unselected   (select_dev != NULL and select_dev[o] == 0) nothing of the object is written: no byte of out_dev[o],
 *                neither status_dev[o] nor used_dev[o].
 *   rank 0       (nothing pushed, or only zero vectors) status_dev[o] = NotEnoughPiecesToRecode, what Recoder::new
 *                answers for no pieces; used_dev[o] = 0; no byte of out_dev[o] is written and no product work is done
 *                (its workgroups return on reading the state).
 *   rank r > 0   out_dev[o][i][0 .. k+L) = XOR over j < r of r_dev[o][i][j] * pieces[o][u_j][0 .. k+L) for i < count:
 *                header and data are one linear map over the full piece, as in rlnc_recode_batch.  The bytes
 *                r_dev[o][i][r .. k) are ignored.  status_dev[o] = RLNC_OK, used_dev[o] = r.  Byte for byte
 *                Recoder::new over the useful pieces in arrival order followed by recode_with_buf with the random bytes
 *                r_dev[o][i][0 .. r), count times.
 * The state, the pieces, select_dev and r_dev are only read: a later push, compact or deliver continues unchanged.
 * plan_dev is caller-owned scratch, 16-byte aligned and at least rlnc_decode_stream_recode_plan_bytes long; its
 * contents after the call are unspecified.
 * Columns.  A recoding object's product takes done_o source rows, read on the device: a useless slot below done_o is a
 * zero column of the expanded coefficients, so the product costs done_o / r of the minimal count x r x (k+L) one.
 * After rlnc_decode_stream_compact u_j = j and done_o = r: the minimal product.  A relay with many useless arrivals
 * compacts, then recodes.
 * Launches: at most four on the context's stream -- the expansion (a workgroup per object and 16 rows of C: numbers the Ok
 * slots, writes C[o][i][u_j] = r_dev[o][i][j] and zero elsewhere below done_o into the plan, and status_dev and used_dev), the
 * block-address streams of the recoding objects, the bit-sliced product over the whole 4 KiB column blocks of k+L (the
 * program of the batch products, 8, 16, 32 or 64 rows a workgroup by count), a perm-multiply product over what that
 * does not take ((k+L) mod 4096; everything for count < 4 or operands the program refuses).  The call never
 * synchronises and grows no context workspace, so (push, recode) can be captured as a linear HIP graph -- after one
 * eager recode or deliver on the device: the 32- and 64-row programs look up their block table once per device,
 * synchronously, and a first such call inside a capture runs every column in the perm-multiply kernel instead (the
 * same bytes, slower).
 * Checks in deliver's order: a null handle RLNC_ERR_INVALID_ARGUMENT; k == 0 PieceCountZero; L == 0 PieceLengthZero;
 * count == 0 or num_objects == 0 RLNC_OK, nothing launched; then the state and shape checks of push (rank mode 0, a
 * buffer never initialised or initialised for another shape); pieces_obj_stride (0 = m*(k+L)) >= m*(k+L); pieces_dev,
 * r_dev, out_dev and status_dev non-null; count <= 4096; plan_dev non-null, aligned and long enough; every launch
 * within 2^31 - 1 workgroups.  Each failure is RLNC_ERR_INVALID_ARGUMENT, names the limit in rlnc_last_error and
 * writes nothing.  Measurements: DESIGN.md §4.2.4, "Recoding". */
int rlnc_decode_stream_recode(rlnc_context *ctx, const void *state_dev, size_t state_bytes, const uint8_t *pieces_dev,
                              size_t pieces_obj_stride, size_t k, size_t L, size_t m, size_t num_objects,
                              const int32_t *select_dev, const uint8_t *r_dev, size_t count, uint8_t *out_dev,
                              int32_t *status_dev, int32_t *used_dev, void *plan_dev, size_t plan_bytes);

/* What rlnc_decode_stream_accept answers in slot_dev for an arrival that it did not place. */
#define RLNC_ACCEPT_NO_ROOM (-1)   /* the object's m slots are filled */
#define RLNC_ACCEPT_NO_OBJECT (-2) /* object id outside [0, num_objects) */
#define RLNC_ACCEPT_FINISHED (-3)  /* state_dev given and the object's rank is k */
#define RLNC_ACCEPT_ABSENT (-4)    /* index at or beyond the device count */
/* Bytes of rlnc_decode_stream_accept's plan buffer: five int32 arrays, four of n entries (an arrival's rank among the
 * equal ids of its chunk of 1,024, its chunk's first equal id, that id's count in the chunk, the slot the chunk's first
 * one takes) and one of num_objects (the next free slot), each rounded up to 16 bytes.  A multiple
 * of 16, non-decreasing in both arguments; 0 for n == 0, n > 1,048,576 and num_objects == 0 (or beyond 2^31 - 1).
 * Pure: needs no context and no GPU. */
size_t rlnc_decode_stream_accept_plan_bytes(size_t n, size_t num_objects);
/* Accepts mixed arrivals into their objects' slots, decided on the device: the receive loop's first call,
 * compact(answered = avail) -> accept(arrivals, object, avail) -> push(avail) -> deliver.  arrivals_dev holds n full
 * coded pieces of k + L bytes for many objects, interleaved as they came: arrival i starts at arrivals_dev + i *
 * arrival_stride (0 = k + L), at any byte address, and belongs to object object_dev[i] (int32 [n]).  count_dev may be
 * NULL; otherwise it points to one device int32, read by the rank and the base launch and written by neither, and the
 * call takes the first n' = min(max(*count_dev, 0), n)
 * arrivals (NULL: n' = n), so that a captured call replays with another number of arrivals each time.  n is the
 * host-known capacity, at most 1,048,576: a receiver with more arrivals calls again.  What rlnc_encode_emit writes as
 * (out_dev, object_dev, count_dev) goes in as (arrivals_dev, object_dev, count_dev) unchanged.  avail_dev (int32 [num_objects]) is
 * the array push takes, and what rlnc_decode_stream_compact writes as answered_dev goes in as it is.  Per object o:
 *   let a = min(max(avail_dev[o], 0), m), read once, and i_0 < i_1 < ... the arrivals below n' whose id is o, in
 *   arrival order (the assignment is stable: no slot is claimed with an atomic).
 *   finished     (state_dev != NULL and rank_o == k, the rank as the last push or compaction left it: the context's
 *                stream orders the calls) slot_dev[i_j] = RLNC_ACCEPT_FINISHED for every j; no byte of the object's
 *                pieces is written and avail_dev[o] keeps its value; refused_dev[o] = 0.
 *   else         arrival i_j goes to slot a + j while a + j < m: all k + L bytes are copied to pieces_dev[o][a + j] and
 *                slot_dev[i_j] = a + j.  The arrivals from j = m - a on get RLNC_ACCEPT_NO_ROOM and are not copied.
 *                avail_dev[o] = min(a + count_o, m); refused_dev[o] = the number of its arrivals that found no room.  An
 *                object with no arrival in the call still has avail_dev[o] rewritten with a, and refused_dev[o] = 0.
 * An id outside [0, num_objects) gets RLNC_ACCEPT_NO_OBJECT, an index in [n', n) RLNC_ACCEPT_ABSENT.  slot_dev (int32
 * [n]) and refused_dev (int32 [num_objects]) may each be NULL; when given, every entry is written.  state_dev == NULL:
 * no finished filter, the registry of initialised state buffers is not consulted and state_bytes is ignored (k and m
 * still say where a piece goes).
 * Equivalence: after the call the pieces and avail_dev hold exactly what a host loop of one copy per arrival into
 * pieces[o][filled[o]++] leaves after the same arrivals in the same order, with the arrivals beyond m dropped; a
 * following push(avail_dev) answers as a decoder fed those pieces in arrival order.
 * Footprint.  Written: the k + L bytes of every slot assigned in this call; avail_dev[0 .. num_objects) (but a finished
 * object's entry); slot_dev[0 .. n); refused_dev[0 .. num_objects); the plan buffer.  Never written: the slots below a
 * or at and beyond the new avail; the bytes between m*(k+L) and the object stride; the arrivals, object_dev, count_dev;
 * any byte of the state.  plan_dev is caller-owned scratch, 16-byte aligned and at least
 * rlnc_decode_stream_accept_plan_bytes long; its contents after the call are unspecified.
 * Launches: three on the context's stream -- rank (a workgroup per 1,024 arrivals: every arrival's place among the equal
 * ids of its chunk), base (one workgroup: the chunks in order, ceil(n' / 1024) dependent steps, the call's only serial
 * part; avail_dev and refused_dev), move (arrival x 4 KiB of a piece: the copy, 16-byte accesses at any byte address
 * where rlnc_device_unaligned_vector_access is 1, single bytes otherwise; slot_dev).  The call never synchronises and
 * grows no context workspace, so (compact, accept, push, deliver) can be captured as a linear HIP graph.
 * Checks in the order of push and deliver: a null handle RLNC_ERR_INVALID_ARGUMENT; k == 0 PieceCountZero; L == 0
 * PieceLengthZero; n == 0 or num_objects == 0 RLNC_OK, nothing launched; with state_dev the state and shape checks of
 * push (rank mode 0, a buffer never initialised or initialised for another shape); 1 <= m <= 8192 and k <= 4096 even
 * without a state; n <= 1,048,576; L <= 2^40; arrival_stride 0 or in [k + L, 2^42]; pieces_obj_stride (0 = m*(k+L))
 * >= m*(k+L); arrivals_dev, object_dev, pieces_dev and avail_dev non-null; plan_dev non-null, aligned and long enough; every launch
 * within 2^31 - 1 workgroups.  Each failure is RLNC_ERR_INVALID_ARGUMENT, names the limit in rlnc_last_error and
 * writes nothing.  Measurements: DESIGN.md §4.2.4, "Accepting arrivals". */
int rlnc_decode_stream_accept(rlnc_context *ctx, const void *state_dev, size_t state_bytes,
                              const uint8_t *arrivals_dev, size_t arrival_stride, const int32_t *object_dev,
                              size_t n, const int32_t *count_dev,
                              uint8_t *pieces_dev, size_t pieces_obj_stride, size_t k, size_t L, size_t m,
                              size_t num_objects, int32_t *avail_dev, int32_t *slot_dev, int32_t *refused_dev,
                              void *plan_dev, size_t plan_bytes);

/* ---- wire formats on the device ------------------------------------------------------------
 * Encoder::new's padded image (encoder.rs:85-106, BOUNDARY_MARKER consts.rs:5) built by a kernel from a byte
 * string already in HBM: out[r][c] (r < k, c < L = ceil((data_len+1)/k), row stride out_row_stride, 0 = L) =
 * data[r·L + c] below data_len, 0x81 at data_len, zeros after.  Errors as Encoder::new (DataLengthZero before
 * PieceCountZero).  Asynchronous on the context stream; data may be unaligned. */
typedef struct rlnc_pad_desc {
    const uint8_t *data;
    size_t data_len;
    size_t k;
    uint8_t *out;
    size_t out_row_stride;
} rlnc_pad_desc;
size_t rlnc_padded_piece_byte_len(size_t data_len, size_t k); /* encoder.rs:93-95 (0 when k == 0) */
int rlnc_pad_device(rlnc_context *ctx, const uint8_t *data_dev, size_t data_len, size_t k, uint8_t *out_dev,
                    size_t out_row_stride);
/* One launch for count descriptors; count <= 65,535 (RLNC_PAD_BATCH_MAX), else RLNC_ERR_INVALID_ARGUMENT and nothing
 * is written: a caller with more splits its batch. */
#define RLNC_PAD_BATCH_MAX 65535
int rlnc_pad_batch_device(rlnc_context *ctx, const rlnc_pad_desc *descs, size_t count);
/* Encoder::new from a device byte string: the encoder owns its padded image (built on the device). */
int rlnc_encoder_new_device(rlnc_context *ctx, const uint8_t *data_dev, size_t data_len, size_t piece_count,
                            rlnc_encoder **out);
/* Ragged batches: every object with its own shape and buffers (device pointers; strides 0 = dense), as a sender or
 * receiver holding pieces of many objects has them.  Each kernel stage is one launch over a device-side descriptor
 * table, whatever the number of objects and shapes (the matmul stage: <= 6 launches -- block addresses, the
 * bit-sliced program for <= 8, <= 16, <= 32 and > 32 output rows, the perm kernel for < 4 KiB tails -- and for
 * misaligned operands on a device without unaligned vector access, rlnc_device_unaligned_vector_access).
 * Asynchronous on the context stream.  Error checks run over all descriptors before anything is launched.
 * rlnc_encode_ragged: n coded pieces coeffs ‖ data per object (encoder.rs:241-250 × n). */
typedef struct rlnc_object_desc {
    const uint8_t *src;      /* k source pieces of L bytes */
    size_t src_row_stride;   /* >= L, 0 = L */
    const uint8_t *coeffs;   /* n × k coding vectors */
    uint8_t *pieces;         /* n full coded pieces */
    size_t piece_row_stride; /* >= k + L, 0 = k + L */
    size_t k, L, n;
} rlnc_object_desc;
int rlnc_encode_ragged(rlnc_context *ctx, const rlnc_object_desc *objs, size_t count);
/* Recoder::recode_with_buf (recoder.rs:122-153) × n_recoded per object: out[i] = Σ_j r[i][j] · pieces[j] over the
 * full pieces (coefficient header and data are one linear map).  Checks in Recoder::new's order (recoder.rs:69-80):
 * n == 0 NotEnoughPiecesToRecode, k + L == 0 PieceLengthZero, k == 0 PieceCountZero, L == 0 PieceLengthTooShort. */
typedef struct rlnc_recode_object_desc {
    const uint8_t *pieces;   /* n received full pieces of k + L bytes */
    size_t piece_row_stride; /* >= k + L, 0 = k + L */
    const uint8_t *r;        /* n_recoded × n recoding coefficients (rng.fill_bytes draws them, recoder.rs:131) */
    uint8_t *out;            /* n_recoded full recoded pieces */
    size_t out_row_stride;   /* >= k + L, 0 = k + L */
    size_t k, L, n, n_recoded;
} rlnc_recode_object_desc;
int rlnc_recode_ragged(rlnc_context *ctx, const rlnc_recode_object_desc *objs, size_t count);
/* Decoder::decode for pieces 0..m-1 of every object + get_decoded_data (decoder.rs:96-177), like
 * rlnc_decode_batch_device per object: decoded [k][L] (padded payload rows in the reference's row order),
 * piece_status_dev int32 [Σ m] (object order, each object's m statuses of its decode() calls), object_status_dev
 * int32 [count] (Ok / NotAllPiecesReceivedYet / InvalidDecodedDataFormat), data_len_dev int64 [count] (unpadded
 * length when Ok).  The exact elimination runs on the device when an object's [coeffs | E] fits LDS, else on host
 * threads (then the call is not capturable).  L == 0 PieceLengthZero, k == 0 PieceCountZero (decoder.rs:66-71). */
typedef struct rlnc_decode_object_desc {
    const uint8_t *pieces;   /* m received full pieces, coeffs ‖ data */
    size_t piece_row_stride; /* >= k + L, 0 = k + L */
    uint8_t *decoded;        /* k × L bytes */
    size_t k, L, m;
} rlnc_decode_object_desc;
int rlnc_decode_ragged(rlnc_context *ctx, const rlnc_decode_object_desc *objs, size_t count, int32_t *piece_status_dev,
                       int32_t *object_status_dev, int64_t *data_len_dev);

/* ---- host-resident pieces (a socket or a file) ---------------------------------------------
 * The batch API above for host buffers: objects stream through the device in windows of `window` objects (0 =
 * automatic, >= 32 MiB of input per window) as a three-stage pipeline on three streams (host-to-device copies, the
 * encode/decode on the context's stream, device-to-host copies; windows rotate over three slots of device buffers,
 * ordered by events), so that window w+1's copy in, window w's encode/decode and window w-1's copy out overlap.
 * Pinned host buffers (hipHostMalloc / hipHostRegister) are copied by DMA directly; pageable ones are staged through
 * pinned buffers by host threads.  Same results as the device-resident calls (they run them).  Synchronous; like the
 * batch calls, one caller thread per context at a time (the slot buffers and copy streams belong to the context). */
/* src [obj][k][L], coeffs [obj][n][k] → pieces [obj][n][k+L] (rlnc_encode_batch). */
int rlnc_encode_host_stream(rlnc_context *ctx, const uint8_t *src, size_t k, size_t L, size_t num_objects,
                            const uint8_t *coeffs, size_t n, uint8_t *pieces, size_t window);
/* pieces: the first m pieces of each object (object stride in bytes, 0 = m*(k+L)) → decoded [obj][k][L], host
 * statuses as rlnc_decode_batch (each may be NULL). */
int rlnc_decode_host_stream(rlnc_context *ctx, const uint8_t *pieces, size_t pieces_obj_stride, size_t k, size_t L,
                            size_t m, size_t num_objects, uint8_t *decoded, int32_t *piece_status,
                            int32_t *object_status, uint64_t *data_len, size_t window);

/* ---- host-only: the decoder's exact coefficient elimination (no device needed) ---------------------------
 * The diagonal-pivot RREF of DecoderMatrix (decoder_matrix.rs:99-244) replicated on [coeffs | E] where E
 * tracks every row as a combination of received pieces; data rows = E × received data (elimination.hpp).
 * fixed_slots > 0: piece p owns E column p; 0: columns are recycled once unreferenced. */
typedef struct rlnc_elimination rlnc_elimination;
int rlnc_elimination_new(size_t k, size_t fixed_slots, rlnc_elimination **out);
/* The same engine in a rank mode (rlnc_elimination_new is mode 0).  In mode 1 a piece that is not useful keeps no slot
 * (keep = 0), recycled slots never exceed k, and rlnc_elimination_coefficients returns the RREF rows in pivot order. */
int rlnc_elimination_new_mode(size_t k, size_t fixed_slots, int rank_mode, rlnc_elimination **out);
void rlnc_elimination_free(rlnc_elimination *e);
/* Decoder::decode on the k coefficient bytes: Ok / PieceNotUseful / ReceivedAllPieces. */
int rlnc_elimination_push(rlnc_elimination *e, const uint8_t *coeffs, int32_t *slot, int32_t *keep);
size_t rlnc_elimination_rank(const rlnc_elimination *e);
size_t rlnc_elimination_slots(const rlnc_elimination *e);
int rlnc_elimination_transform(const rlnc_elimination *e, uint8_t *T, size_t ld); /* k × ld, zero-filled */
int rlnc_elimination_coefficients(const rlnc_elimination *e, uint8_t *C);        /* rank × k */

#ifdef __cplusplus
}
#endif
#endif /* RLNC_HIP_H */
