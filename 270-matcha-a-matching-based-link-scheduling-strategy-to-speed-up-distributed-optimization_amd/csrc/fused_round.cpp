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

int Tune::set(const char* who, const char* key, int value) {
    MX_CHECK(key, "%s: null key", who);
    if (!strcmp(key, "nontemporal")) {
        nontemporal = value == 2 ? 2 : (value ? 1 : 0);
    } else if (!strcmp(key, "wgpc")) {
        MX_CHECK(value >= 0 && value <= 32, "%s: wgpc %d", who, value);
        wgpc = value;
    } else if (!strcmp(key, "blocks_per_cu")) {
        MX_CHECK(value >= 1 && value <= 64, "%s: blocks_per_cu %d", who, value);
        blocks_per_cu = value;
    } else if (!strcmp(key, "flat_small")) {
        MX_CHECK(value >= 0 && value <= 4096, "%s: flat_small %d", who, value);
        flat_small = value;
    } else if (!strcmp(key, "grid")) {
        MX_CHECK(value >= 0 && value <= 65536, "%s: grid %d", who, value);
        grid = value;
    } else if (!strcmp(key, "store_policy")) {
        MX_CHECK(value >= 0 && value <= mx::kStoreSc1Nt, "%s: store_policy %d", who, value);
        store_policy = value;
    } else {
        MX_CHECK(false, "%s: unknown key '%s'", who, key);
    }
    return MX_OK;
}

int Tune::get(const char* who, const char* key) const {
    if (!key) return MX_ERR_INVALID;
    if (!strcmp(key, "nontemporal")) return nontemporal;
    if (!strcmp(key, "wgpc")) return wgpc;
    if (!strcmp(key, "blocks_per_cu")) return blocks_per_cu;
    if (!strcmp(key, "flat_small")) return flat_small;
    if (!strcmp(key, "grid")) return grid;
    if (!strcmp(key, "store_policy")) return store_policy;
    mx::set_error("%s: unknown key '%s'", who, key);
    return MX_ERR_INVALID;
}

bool Tune::streaming(int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const {
    if (nontemporal != 2) return nontemporal != 0;
    const int64_t ws = total_tiles * (int64_t)tile * n_local * bytes_per_elem;   // bytes the round moves
    return ws <= ((int64_t)32 << 20) || ws > ((int64_t)320 << 20);
}

int Tune::policy(bool nt, int64_t total_tiles, int tile, int n_local, int bytes_per_elem) const {
    if (!nt) return mx::kStorePlain;
    if (store_policy > 0) return store_policy;
    const int64_t ws = total_tiles * (int64_t)tile * n_local * bytes_per_elem;
    return ws > mx::kStoreAutoBytes ? kAutoPolicy : mx::kStoreNt;
}

int64_t Tune::grid_of(int ns, int64_t work, bool* flat) const {
    const int64_t target = grid > 0 ? (int64_t)grid : (int64_t)cu_count() * blocks_per_cu;
    *flat = ns <= 16 && grid == 0 && flat_small > 0 && work <= (int64_t)flat_small * target;
    const int64_t n = *flat ? work : (work < target ? work : target);
    return n < 1 ? 1 : n;
}

}  // namespace fused
}  // namespace mx
