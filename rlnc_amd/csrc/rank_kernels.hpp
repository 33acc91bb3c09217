// rank_kernels.hpp — launch interface of the true-rank elimination (rank.hip; internal to librlnc_hip).
//
// RLNC_RANK_MODE_TRUE: a second producer of {T, status, rank} from RrefParams / RrefObj.  Where the default device
// elimination (rref.hip) replays the reference's diagonal-pivot RREF bit for bit, this one keeps [coeffs | E] in
// reduced row-echelon form with free pivot columns, so a piece is useful exactly when it is linearly independent of
// the useful pieces before it (include/rlnc_hip.h, "Rank mode").  It reads k, m, n_obj, pieces, the strides, T,
// T_obj, status, rank and objs of RrefParams; it writes neither bsj_stream nor the tail_* outputs and ignores
// block_only, m_stride, skip_full (RrefObj: m_first, two_pass).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "rref.hpp"

namespace rlnc {

// LDS of one object's workgroup: the 8 KiB multiplier table, k rows of D = ceil(k/4) + ceil(m/4) dwords, two scratch
// rows, the m staged headers (ceil(k/4) dwords each), m statuses, the pivot and order arrays and k quotient bytes:
//   8192 + 4·(k·D + 2·D + m·ceil(k/4) + m + 2·k + ceil(k/4))  bytes.
// The kernel applies when this is <= kRrefMaxLds (160 KiB): k = 200, m = 210 takes 135 KiB, k = 300, m = 310 does not fit.
size_t rank_lds_bytes(int k, int m);
// batch form (p.objs == nullptr): one workgroup of 4 waves per object, or -- k <= 16, rows of <= 16 dwords and
// >= 1024 objects -- one wave per object, 4 objects per workgroup over one table copy
hipError_t launch_rank_batch(const RrefParams &p, hipStream_t s);
// ragged form: one workgroup per object of the device table objs; lds = the largest object's rank_lds_bytes
hipError_t launch_rank_ragged(const RrefObj *objs, int n, size_t lds, hipStream_t s);

}  // namespace rlnc
