// api_walk.hip.h -- the launch plan of a per-lane query walk (bvh_walk.hip.h), for closest_launch, all_hits_launch, near_launch and sphere_cast_launch.  Part of api.hip's
// translation unit.
#pragma once

// blocks per CU of a walk's grid: at the default 16 LDS levels a block's stack is 32 KB with 8-byte entries, 16 KB with 4-byte ones
static const int kWalkBlocksPerCu = 5;

struct WalkLaunch {
    bool wide;                  // the 4-wide tree, else the binary one
    int entries, lds_entries;   // the bound of the stack ("The walk the queries share"), and how much of it is in LDS
    int blocks;                 // the grid of the call's largest launch: the spill has a column per thread of these
    size_t lds;                 // dynamic LDS bytes of a launch
    StreamScratch spill_scratch;
    void *spill = nullptr;      // the levels above lds_entries, on the caller's stream; nullptr when there are none
    // entry_bytes: of a stack entry; lds_levels: the call's knob, read per call; per_launch: the most queries one launch of the call takes
    int plan(const gnxr_scene *r, size_t entry_bytes, int lds_levels, long long per_launch, hipStream_t st) {
        wide = r->wide_ok;
        entries = wide ? r->cs.stack4_need + 1 : r->cs.bvh_max_depth + 2;   // (children - 1) per node of the deepest path, and one of slack
        lds_entries = std::min(entries, lds_levels);
        blocks = grid_for(per_launch, kWalkBlocksPerCu);
        lds = (size_t)lds_entries * kBlock * entry_bytes;
        if (entries > lds_entries) {
            HIP_TRY(spill_scratch.alloc((size_t)(entries - lds_entries) * (size_t)blocks * kBlock * entry_bytes, st));
            spill = spill_scratch.p;
        }
        return GNXR_OK;
    }
    // the grid of a launch over cnt queries: never more blocks than the spill has columns for
    int grid(long long cnt) const { return std::min(blocks, grid_for(cnt, kWalkBlocksPerCu)); }
};
