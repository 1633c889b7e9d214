// fused_round.cpp -- the host side the fused optimizer rounds share: row classes, the layout prefix, the
// knobs and the grid choice (see fused_host.h).
#include "fused_host.h"
#include "mx_common.h"

namespace mx {
namespace fused {

Cls pick(int n_slots) {
    if (n_slots < 1) return {0, 0, 0};
    if (n_slots <= 8) return {8, 1024, 512};
    if (n_slots <= 16) return {16, 1024, 512};
    if (n_slots <= 32) return {32, 512, 512};
    if (n_slots <= 64) return {64, 256, 256};
    return {0, 0, 0};
}

int layout(const char* who, const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host) {
    MX_CHECK(seg_len_host && tile_off_host && nseg >= 1, "%s: bad arguments", who);
    const int tile = pick(n_slots).tile;
    MX_CHECK(tile > 0, "%s: n_slots=%d outside [1, 64]", who, n_slots);
    return mx::tile_prefix(who, tile, seg_len_host, nseg, tile_off_host);
}

// the six knobs of one family's instance
static void knobs_of(Tune& t, Knob (&k)[6]) {
    k[0] = knob_tri("nontemporal", &t.nontemporal);
    k[1] = knob_range("wgpc", &t.wgpc, 0, 32);
    k[2] = knob_range("blocks_per_cu", &t.blocks_per_cu, 1, 64);
    k[3] = knob_range("flat_small", &t.flat_small, 0, 4096);
    k[4] = knob_range("grid", &t.grid, 0, 65536);
    k[5] = knob_range("store_policy", &t.store_policy, 0, mx::kStoreSc1Nt);
}

int Tune::set(const char* who, const char* key, int value) {
    Knob k[6];
    knobs_of(*this, k);
    return knob_set(who, k, 6, key, value);
}

int Tune::get(const char* who, const char* key) const {
    Knob k[6];
    knobs_of(const_cast<Tune&>(*this), k);
    return knob_get(who, k, 6, key);
}

// bytes the round moves
static int64_t moved(int64_t total_tiles, int tile, int n_local, int bytes_per_elem) {
    return total_tiles * (int64_t)tile * n_local * bytes_per_elem;
}

bool Tune::streaming(int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const {
    return nontemporal == 2 ? mx::streams(moved(total_tiles, tile, n_local, bytes_per_elem)) : nontemporal != 0;
}

int Tune::policy(bool nt, int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const {
    if (!nt) return mx::kStorePlain;
    return mx::store_policy_of(store_policy, moved(total_tiles, tile, n_local, bytes_per_elem), kAutoPolicy);
}

int64_t Tune::grid_of(int ns, int64_t work, bool* flat) const {
    const int64_t target = grid > 0 ? (int64_t)grid : (int64_t)cu_count() * blocks_per_cu;
    *flat = ns <= 16 && grid == 0 && flat_small > 0 && work <= (int64_t)flat_small * target;
    const int64_t n = *flat ? work : (work < target ? work : target);
    return n < 1 ? 1 : n;
}

}  // namespace fused
}  // namespace mx
