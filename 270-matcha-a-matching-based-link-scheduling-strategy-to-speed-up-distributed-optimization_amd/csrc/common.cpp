// common.cpp -- library identity and error plumbing for the C ABI.
#include <stdarg.h>

#include "mx_common.h"

namespace mx {
static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int g_mean_wgpc = 3;
int g_store_policy = 0;

int cu_count() {
    static int v = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 256;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 256;
        return n > 0 ? n : 256;
    }();
    return v;
}

int tile_prefix(const char* who, int tile, const int64_t* seg_len_host, int nseg, int64_t* tile_off_host) {
    tile_off_host[0] = 0;
    for (int s = 0; s < nseg; ++s) {
        MX_CHECK(seg_len_host[s] >= 0, "%s: negative length", who);
        tile_off_host[s + 1] = tile_off_host[s] + (seg_len_host[s] + tile - 1) / tile;
    }
    return MX_OK;
}

int lds_per_cu() {
    static int v = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 160 * 1024;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || n <= 0)
            return 160 * 1024;
        return n;
    }();
    return v;
}

size_t lds_cap_pad(int static_bytes, int wg_per_cu) {
    if (wg_per_cu <= 0 || static_bytes <= 0) return 0;
    const int cap = lds_per_cu();
    const int want = (cap / (wg_per_cu + 1) + cap / wg_per_cu) / 2 / 256 * 256;
    return want > static_bytes ? (size_t)(want - static_bytes) : 0;
}

static const Knob* knob_find(const Knob* table, int n, const char* key) {
    for (int i = 0; i < n; ++i)
        if (!strcmp(table[i].key, key)) return table + i;
    return nullptr;
}

int knob_set(const char* who, const Knob* table, int n, const char* key, int value) {
    MX_CHECK(key, "%s: null key", who);
    const Knob* k = knob_find(table, n, key);
    MX_CHECK(k && !k->read_only, "%s: unknown key '%s'", who, key);
    bool ok = true;
    if (k->kind == Knob::kRange) ok = value >= k->v[0] && value <= k->v[1];
    else if (k->kind == Knob::kOneOf) ok = value == k->v[0] || value == k->v[1] || value == k->v[2] || value == k->v[3];
    else value = (k->kind == Knob::kTri && value == 2) ? 2 : (value ? 1 : 0);
    MX_CHECK(ok, "%s: %s %d", who, key, value);
    *k->slot = value;
    return MX_OK;
}

int knob_get(const char* who, const Knob* table, int n, const char* key) {
    if (!key) return MX_ERR_INVALID;
    const Knob* k = knob_find(table, n, key);
    MX_CHECK(k, "%s: unknown key '%s'", who, key);
    return *k->slot;
}
}  // namespace mx

extern "C" const char* mx_version(void) { return "matcha-gossip gfx950 0.1"; }
extern "C" const char* mx_last_error(void) { return mx::g_err; }

// the host-side validator of the per-parameter-group run tables (mx_param_runs, see the header)
extern "C" int mx_param_runs_check(const int64_t* seg_len_host, int nseg, const int32_t* run_off_host,
                                   const int64_t* run_end_host, const float* wd_host, const float* lr_scale_host) {
    MX_CHECK(seg_len_host && run_off_host && run_end_host && wd_host && lr_scale_host,
             "mx_param_runs_check: null argument");
    MX_CHECK(nseg >= 1, "mx_param_runs_check: nseg=%d < 1", nseg);
    MX_CHECK(run_off_host[0] == 0, "mx_param_runs_check: run_off[0]=%d != 0", run_off_host[0]);
    for (int s = 0; s < nseg; ++s) {
        const int a = run_off_host[s], b = run_off_host[s + 1];
        MX_CHECK(seg_len_host[s] >= 0, "mx_param_runs_check: segment %d has a negative length", s);
        MX_CHECK(b >= a, "mx_param_runs_check: run_off descends at segment %d", s);
        if (seg_len_host[s] == 0) {
            MX_CHECK(b == a, "mx_param_runs_check: segment %d is empty but has runs (an empty run)", s);
            continue;
        }
        MX_CHECK(b > a, "mx_param_runs_check: segment %d has no runs", s);
        int64_t prev = 0;
        for (int r = a; r < b; ++r) {
            const int64_t e = run_end_host[r];
            MX_CHECK(e != prev, "mx_param_runs_check: run %d of segment %d is empty", r - a, s);
            MX_CHECK(e > prev, "mx_param_runs_check: run ends of segment %d are not ascending at run %d", s, r - a);
            prev = e;
            const float wd = wd_host[r], sc = lr_scale_host[r];
            // x - x is 0 for finite x only (NaN for NaN and the infinities): no <cmath> needed
            MX_CHECK(wd >= 0.0f && wd - wd == 0.0f, "mx_param_runs_check: weight decay of run %d of segment %d is "
                     "negative or not finite", r - a, s);
            MX_CHECK(sc >= 0.0f && sc - sc == 0.0f, "mx_param_runs_check: lr scale of run %d of segment %d is "
                     "negative or not finite", r - a, s);
        }
        MX_CHECK(prev == seg_len_host[s], "mx_param_runs_check: the last run of segment %d ends at %lld, not at the "
                 "segment's length %lld", s, (long long)prev, (long long)seg_len_host[s]);
    }
    return MX_OK;
}
