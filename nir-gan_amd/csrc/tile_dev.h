// The geometry that the overlapping-tile entries share (tileblend.hip: nirgan_tile_count_ov / _gather_ov / nirgan_tile_blend;
// scenepredict.hip: nirgan_scene_tile_invalid / _gather / nirgan_scene_finish): the reflected read index and the tiles of one axis.
#pragma once
#include "common.h"

// ng_reflect continued periodically (period 2 (n - 1)): the same index wherever ng_reflect is defined (one reflection), and an index
// inside [0, n) for every i -- a tile that is much larger than the scene reads rows more than one reflection away.
__host__ __device__ __forceinline__ int tb_reflect(int i, int n) {
    int r = ng_reflect(i, n);
    if (r < 0 || r >= n) {
        const int period = 2 * (n - 1);
        if (period == 0) return 0;
        r = i % period;
        if (r < 0) r += period;
        if (r >= n) r = period - r;
    }
    return r;
}

inline int tiles_per_axis(int extent, int core, int stride) { return extent <= core ? 1 : (extent - core + stride - 1) / stride + 1; }
