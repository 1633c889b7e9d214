// fused_host.h -- the host side the fused optimizer rounds share (fused_round.cpp): row classes, the layout
// prefix and a family's knobs.  No device code; fused_round.h adds the kernel and its launch.
#pragma once
#include <stdint.h>

namespace mx {
namespace fused {

struct Cls {
    int ns, tile, tw;    // row class, layout tile (columns), work-item width
};
// the LDS bytes of mix_bf16.hip's classes (x' is parked as fp32 in every family): 8 / 16 rows are worked
// in 512-column halves of a 1024-column layout tile (16 / 32 KB of LDS per workgroup)
Cls pick(int n_slots);

// mx_*_layout: the tile prefix of the segments; `who` names the entry point in the error text
int layout(const char* who, const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);

// A family's knobs (mx_*_set / _get); every family owns an instance.  Speed only, never bits.
struct Tune {
    int nontemporal = 2;   // 1 / 0: streaming hints on / off; 2 = auto (off for rounds moving 32-320 MB, as mix.hip)
    int wgpc = 0;          // 8 / 16 rows, flat grid: workgroups per CU cap (dynamic LDS); 0 = as many as fit
    int blocks_per_cu = 2; // persistent grids (32 / 64 rows, or more work items than flat_small x the grid)
    int flat_small = 256;  // 8 / 16 rows: one workgroup per work item up to flat_small x CUs x blocks_per_cu items
    int grid = 0;          // > 0: exact persistent grid size (tests: few workgroups looping over many work items)
    int store_policy = 0;  // 16-byte stores of the streaming 8- / 16-row launches (mx::StorePolicy): 1 nt, 2 sc1,
                           // 3 sc1 nt forced at every size; 0 = auto: kAutoPolicy for rounds moving > 320 MB, nt below
                           // (nt: write-through measured 0.5-4 % slower in all four families on 8 x 25.6M,
                           // tools/store_policy_ab.py, profiles/store_policy_ab.json "fused")
    static constexpr int kAutoPolicy = 1;

    int set(const char* who, const char* key, int value);
    int get(const char* who, const char* key) const;
    // streaming hints for a round whose arrays hold `bytes_per_elem` bytes per (row, column)
    bool streaming(int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const;
    // the store policy of that round's launch (plain without streaming hints)
    int policy(bool nt, int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const;
    // the grid of `work` work items of an `ns`-row class: one workgroup each (flat; `wgpc` then caps the
    // workgroups per CU) or a persistent grid looping over them
    int64_t grid_of(int ns, int64_t work, bool* flat) const;
};

}  // namespace fused
}  // namespace mx
