// block -> (batch, tile_m, tile_n), XCD aware: all tiles of one batch index on one XCD (blockIdx % 8), back to back.
// Shared by the fp32-MFMA kernels (gemm.hip) and the bf16x3 engine (x3_engine.h); each keeps its own grid_blocks, the
// grid that this map expects: ceil(nbatch / 8) * 8 * tiles_m * tiles_n workgroups.
#pragma once
#include <hip/hip_runtime.h>

namespace mk {

struct TileId {
    int batch, tm, tn;
    bool valid;
};
__device__ __forceinline__ TileId decode_block(int nbatch, int tiles_m, int tiles_n) {
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = bid >> 3;
    const int T = tiles_m * tiles_n;
    TileId t;
    t.batch = (q / T) * 8 + xcd;
    const int r = q % T;
    t.tm = r / tiles_n;
    t.tn = r - t.tm * tiles_n;
    t.valid = t.batch < nbatch;
    return t;
}

}  // namespace mk
