// Stage geometry shared by the "one wave per SIMD, every wave stages and consumes" kernels (cost_tile256.hip: 256 x 256
// pair tiles of the single-GPU loss; cost_rows.hip: the row block of a batch-sharded rank; cost_bwd_q256.hip: the video
// gradient on the same tile).  The split, the fragment reads and the six-product MFMA chain are bf16x3.h's.
//
// LDS stage = 3 planes (h, m, l) x NROWS rows x 32 bytes (16 bf16: the pairs (k, k+1) of eight float4 column pieces of a
// 32-column load granule; the odd step of the granule holds the pairs (k+2, k+3)).  A fragment is rows 32 r .. 32 r + 31,
// lane l reading 16 bytes at row (l & 31), column half (l >> 5): contiguous 1 KB per plane, conflict-free.
#pragma once
#include "common.h"
#include "bf16x3.h"

namespace kccot {

constexpr int QROWB = 32;                  // bytes of one row of one plane of a 16-k step
constexpr int QG = 32;                     // columns per load granule = two steps
// Granules per K-chunk.  The chunk length is bounded by the ACCUMULATION, not by occupancy: an MFMA accumulation loses
// ~0.02 ulp of the running sum (addends are truncated when aligned to it; measured: 2.3e-5 low after 14 000 accumulations of
// all-positive terms in the 128-tile kernel, 1.5e-5 of a distance with 2300), so one partial tile holds at most
// Q_MAX_GRAN granules = 1536 columns = 576 accumulations (a distance within 4e-6); the fp64 reduction adds the tiles up.
constexpr int Q_MAX_GRAN = 48;

}  // namespace kccot
