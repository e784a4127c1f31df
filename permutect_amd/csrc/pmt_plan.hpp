// The packing rule of the group planners (pmt_plan.hip): next-fit over consecutive read sets -- a set that does not fit the open group, or
// would be its (PMT_GROUP_MAX_SETS + 1)-th, closes it, and the closed group's ref and alt tiles advance the tile base.  The kernels index
// LDS tables of PMT_GROUP_MAX_SETS rows on the strength of it.  The fit predicate is host and device code's alike (T: long long on the
// host, any int32 counts; int on the device).  NextFit is the HOST planners' (pmt_plan_groups, pmt_plan_groups_split, pmt_pack_order);
// plan_chunk_wave of pmt_plan_groups_device repeats its statements by hand, because through the struct its two kernels took 15 % longer
// (profiles/host_split_device_asm_sha256.txt), and tests/test_balancer_gpu.py holds it to the host plan.  Counts are never negative.
#pragma once
#include <hip/hip_runtime.h>

#include "permutect_amd.h"

// ref tiles and alt tiles go to disjoint waves, PMT_GROUP_TILES / PMT_GROUP_WAVES tiles per wave (pmt_device.hpp: group_fits, group_geometry)
template <typename T>
__host__ __device__ inline bool group_fits_reads(T ref_reads, T alt_reads) {
    const T per = PMT_GROUP_TILES / PMT_GROUP_WAVES;
    const T tr = (ref_reads + 15) >> 4, ta = (alt_reads + 15) >> 4;
    return (tr + per - 1) / per + (ta + per - 1) / per <= PMT_GROUP_WAVES;
}

template <typename T>
struct NextFit {
    T ref = 0, alt = 0;  // reads of the open group
    int sets = 0;        // its read sets
    T tile_base = 0;     // tiles of every group closed so far
    bool takes(T r, T a) const { return sets < PMT_GROUP_MAX_SETS && group_fits_reads(ref + r, alt + a); }
    bool closes(T r, T a) const { return sets > 0 && !takes(r, a); }
    void add(T r, T a) { ref += r; alt += a; ++sets; }
    T close() {  // -> the tile base of the next group
        tile_base += ((ref + 15) >> 4) + ((alt + 15) >> 4);
        ref = alt = 0;
        sets = 0;
        return tile_base;
    }
};
