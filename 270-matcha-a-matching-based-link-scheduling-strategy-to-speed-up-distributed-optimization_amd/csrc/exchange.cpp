// exchange.cpp -- cross-GPU transport over RCCL (xGMI within a node).
//
// The reference moves every active edge's full parameter vector with a pickled, blocking
// comm.sendrecv in ascending matching order (communicator.py:99-112).  Here one process drives
// one GPU holding a contiguous block of workers; per round, every active matching edge that
// crosses GPUs becomes an ncclSend of the local row plus an ncclRecv of the partner's row into
// a receive slab, all inside ONE ncclGroupStart/End so the <= 7 peers of a GPU stream over
// their own xGMI links concurrently.  Edges inside a GPU are not moved at all: the mixing
// kernel reads those rows straight from HBM.
//
// Each row crosses a link at most once per round: a local worker whose active partners include
// several workers on one peer GPU (different matchings) is sent to that peer once, and the peer
// receives it into one slab slot that all its local partners read.  Posting order (both
// directions): first appearance of the (worker, destination GPU) pair in (matching ascending,
// sender worker id ascending) order -- identical to the receive-slot numbering of plan_kernel
// (plan.hip), so slab slot k of the round always holds the row the plan expects.  Sends to /
// receives from one peer pair up in posting order, as RCCL point-to-point requires.
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mx_common.h"
#include "row_sum.h"

#define MX_NCCL(call)                                                                       \
    do {                                                                                    \
        ncclResult_t r_ = (call);                                                           \
        if (r_ != ncclSuccess) {                                                            \
            ::mx::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
            return MX_ERR_RCCL;                                                             \
        }                                                                                   \
    } while (0)

static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");

extern "C" int mx_rccl_unique_id(void* id_out) {
    MX_CHECK(id_out, "mx_rccl_unique_id: null pointer");
    ncclUniqueId id;
    MX_NCCL(ncclGetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return MX_OK;
}

// ---------------------------------------------------------------------------------- deadlines
// A peer that never arrives (a dead rank, a rank that skipped a collective) must not hang the
// process: the communicator is created NON-blocking (ncclConfig_t.blocking = 0), so
// ncclCommInitRankConfig, ncclGroupEnd and the collectives return at once (ncclInProgress) and
// wait_comm() polls ncclCommGetAsyncError against a deadline.  On expiry the call returns
// MX_ERR_RCCL ("timed out"); a timed-out init is aborted here, a timed-out operation leaves the
// communicator to the caller (mx_rccl_abort).  The deadline is the init call's timeout_ms, kept
// per process (MX_RCCL_TIMEOUT_S or 300 s for mx_rccl_init).
namespace {
std::atomic<int64_t> g_op_timeout_ms{300000};

int64_t env_timeout_ms() {
    const char* e = getenv("MX_RCCL_TIMEOUT_S");
    if (e && *e) {
        const double s = atof(e);
        if (s > 0) return (int64_t)(s * 1000.0);
    }
    return 300000;
}

// ncclSuccess once every operation issued on `comm` is enqueued (non-blocking communicators), the
// async error if one occurred, ncclInProgress if the deadline passed first.
ncclResult_t wait_comm(ncclComm_t comm, int64_t timeout_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        ncclResult_t st = ncclSuccess;
        const ncclResult_t r = ncclCommGetAsyncError(comm, &st);
        if (r != ncclSuccess) return r;
        if (st != ncclInProgress) return st;
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if (ms >= timeout_ms) return ncclInProgress;
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(spin > 4096 ? 1000 : 20));
    }
}

// `r` is what an RCCL call on `comm` returned: wait for ncclInProgress to resolve.
int finish(ncclComm_t comm, ncclResult_t r, const char* what) {
    if (r == ncclInProgress) r = wait_comm(comm, g_op_timeout_ms.load());
    if (r == ncclInProgress) {
        mx::set_error("%s: timed out after %lld ms (a peer rank never joined)", what, (long long)g_op_timeout_ms.load());
        return MX_ERR_RCCL;
    }
    if (r != ncclSuccess) {
        mx::set_error("%s -> %s", what, ncclGetErrorString(r));
        return MX_ERR_RCCL;
    }
    return MX_OK;
}
}  // namespace

#define MX_NCCL_ON(comm, call)                                   \
    do {                                                         \
        int rc_ = finish((comm), (call), #call);                 \
        if (rc_ != MX_OK) return rc_;                            \
    } while (0)

extern "C" int mx_rccl_init_timeout(const void* id, int nranks, int rank, int64_t timeout_ms, void** comm_out,
                                    int* nonblocking_out) {
    MX_CHECK(id && comm_out, "mx_rccl_init_timeout: null pointer");
    MX_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "mx_rccl_init_timeout: rank %d of %d", rank, nranks);
    MX_CHECK(timeout_ms > 0, "mx_rccl_init_timeout: timeout_ms %lld", (long long)timeout_ms);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclResult_t r = ncclCommInitRankConfig(&comm, nranks, uid, rank, &cfg);
    if (r == ncclInProgress || (r == ncclSuccess && comm)) {
        r = wait_comm(comm, timeout_ms);
        if (r != ncclSuccess) {
            (void)ncclCommAbort(comm);
            if (r == ncclInProgress)
                mx::set_error("mx_rccl_init: rank %d of %d: no complete communicator within %lld ms (a peer rank "
                              "never joined)", rank, nranks, (long long)timeout_ms);
            else
                mx::set_error("mx_rccl_init: ncclCommInitRankConfig -> %s", ncclGetErrorString(r));
            return MX_ERR_RCCL;
        }
        g_op_timeout_ms.store(timeout_ms);
        if (nonblocking_out) *nonblocking_out = 1;
        *comm_out = comm;
        return MX_OK;
    }
    if (comm) (void)ncclCommAbort(comm);          // a half-built communicator is not leaked
    mx::set_error("mx_rccl_init: ncclCommInitRankConfig(blocking = 0) -> %s", ncclGetErrorString(r));
    return MX_ERR_RCCL;
}

extern "C" int mx_rccl_init(const void* id, int nranks, int rank, void** comm_out) {
    return mx_rccl_init_timeout(id, nranks, rank, env_timeout_ms(), comm_out, nullptr);
}

extern "C" int mx_rccl_count(void* comm, int* nranks_out) {
    MX_CHECK(comm && nranks_out, "mx_rccl_count: null pointer");
    MX_NCCL(ncclCommCount(reinterpret_cast<ncclComm_t>(comm), nranks_out));
    return MX_OK;
}

// The deadlines above cover getting an operation ENQUEUED (a peer that never joins an init or a
// group's connection setup).  Once the point-to-point connections exist, a peer that dies or skips
// an exchange leaves the RCCL kernel waiting on the GPU, and the hang would surface at the next
// stream / event synchronisation, which has no limit.  mx_rccl_wait is that synchronisation with
// the deadline: an event recorded on `stream` behind everything enqueued so far, polled
// (hipEventQuery) until it completes or timeout_ms passes; on expiry the communicator is aborted
// (ncclCommAbort: its kernels see the abort flag and exit, the stream drains) and MX_ERR_RCCL
// "timed out" is returned -- the caller must not use the communicator again.
static constexpr int64_t kDrainMs = 2000;       // after an abort: how long the stream may take to drain

extern "C" int mx_rccl_wait(void* comm, void* stream, int64_t timeout_ms) {
    MX_CHECK(comm, "mx_rccl_wait: null communicator");
    if (timeout_ms <= 0) timeout_ms = g_op_timeout_ms.load();
    hipEvent_t ev;
    MX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, mx::as_stream(stream));
    if (e != hipSuccess) {
        (void)hipEventDestroy(ev);
        mx::set_error("mx_rccl_wait: hipEventRecord -> %s", hipGetErrorString(e));
        return MX_ERR_HIP;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        e = hipEventQuery(ev);
        if (e != hipErrorNotReady) break;
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if (ms >= timeout_ms) {
            (void)ncclCommAbort(reinterpret_cast<ncclComm_t>(comm));
            // the aborted kernels should leave the stream; wait for that against a second, short
            // deadline (never an unbounded hipEventSynchronize: a kernel that misses the abort flag,
            // or another long kernel behind it, would hang here)
            const auto t1 = std::chrono::steady_clock::now();
            bool drained = false;
            for (;;) {
                const hipError_t q = hipEventQuery(ev);
                if (q != hipErrorNotReady) { drained = true; break; }
                if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t1)
                        .count() >= kDrainMs)
                    break;
                std::this_thread::sleep_for(std::chrono::microseconds(500));
            }
            if (drained) (void)hipEventDestroy(ev);   // else the event stays: destroying it could block
            mx::set_error("mx_rccl_wait: the stream did not drain within %lld ms (a peer rank died or skipped an "
                          "exchange); the communicator was aborted%s", (long long)timeout_ms,
                          drained ? "" : " and the stream was still busy 2 s later");
            return MX_ERR_RCCL;
        }
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(spin > 4096 ? 1000 : 20));
    }
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) {
        mx::set_error("mx_rccl_wait: hipEventQuery -> %s", hipGetErrorString(e));
        return MX_ERR_HIP;
    }
    return MX_OK;
}

extern "C" int mx_rccl_abort(void* comm) {
    if (!comm) return MX_OK;
    MX_NCCL(ncclCommAbort(reinterpret_cast<ncclComm_t>(comm)));
    return MX_OK;
}

extern "C" int mx_rccl_destroy(void* comm_v) {
    if (!comm_v) return MX_OK;
    ncclComm_t comm = reinterpret_cast<ncclComm_t>(comm_v);
    // drain what is still queued, then release; a communicator whose peers are gone is aborted
    if (finish(comm, ncclCommFinalize(comm), "ncclCommFinalize") != MX_OK) {
        (void)ncclCommAbort(comm);
        return MX_ERR_RCCL;
    }
    const ncclResult_t r = ncclCommDestroy(comm);       // local once finalized
    if (r != ncclSuccess && r != ncclInProgress) {
        mx::set_error("ncclCommDestroy -> %s", ncclGetErrorString(r));
        return MX_ERR_RCCL;
    }
    return MX_OK;
}

extern "C" int mx_exchange_plan(const uint8_t* flags_row, int M, const int32_t* partner, int n_global,
                                const int32_t* owner, int my_rank, int row_base, int n_local,
                                int32_t* ops, int cap, int* n_ops) {
    MX_CHECK(flags_row && partner && owner && n_ops, "mx_exchange_plan: null pointer");
    MX_CHECK(M >= 1 && n_global >= 1 && n_local >= 1 && row_base >= 0 && row_base + n_local <= n_global,
             "mx_exchange_plan: M=%d n=%d block [%d, %d)", M, n_global, row_base, row_base + n_local);
    auto is_local = [&](int w) { return w >= row_base && w < row_base + n_local; };
    std::vector<uint8_t> sent((size_t)n_local * (size_t)(n_global > 0 ? n_global : 1), 0);  // [row][peer]
    std::vector<uint8_t> got((size_t)n_global, 0);                                         // by worker
    int cnt = 0, remote = 0;
    for (int g = 0; g < M; ++g) {
        if (!flags_row[g]) continue;
        for (int p = 0; p < n_global; ++p) {      // p = sender, ascending
            const int q = partner[g * n_global + p];
            if (q < 0) continue;
            MX_CHECK(q < n_global && partner[g * n_global + q] == p,
                     "mx_exchange_plan: matching %d is not symmetric at %d", g, p);
            const bool pl = is_local(p), ql = is_local(q);
            if (pl == ql) continue;
            const int peer = pl ? owner[q] : owner[p];
            MX_CHECK(peer >= 0 && peer != my_rank && peer < n_global,
                     "mx_exchange_plan: worker owned by bad rank %d", peer);
            if (pl) {                               // send p's row to peer once per round
                uint8_t& done = sent[(size_t)(p - row_base) * n_global + peer];
                if (done) continue;
                done = 1;
            } else {                                // receive p's row once per round
                if (got[p]) continue;
                got[p] = 1;
            }
            if (ops) {
                MX_CHECK(cnt < cap, "mx_exchange_plan: more than %d operations", cap);
                int32_t* o = ops + 4 * cnt;
                o[0] = pl ? 0 : 1;                  // 0 = send our row p, 1 = receive p's row
                o[1] = peer;
                o[2] = pl ? p - row_base : remote;  // local row / receive slab slot
                o[3] = p;                           // the worker whose row travels
            }
            if (!pl) ++remote;
            ++cnt;
        }
    }
    *n_ops = cnt;
    return MX_OK;
}

extern "C" int mx_exchange_post(void* comm_v, const int32_t* ops, int n_ops, void* const* rows, int n_rows,
                                void* slab, int64_t slab_ld_bytes, int64_t row_bytes, void* stream) {
    MX_CHECK(comm_v && (ops || n_ops == 0) && n_ops >= 0, "mx_exchange_post: bad arguments");
    MX_CHECK(row_bytes > 0 && row_bytes % 4 == 0, "mx_exchange_post: row_bytes %lld", (long long)row_bytes);
    if (n_ops == 0) return MX_OK;
    int nranks = 0;
    MX_NCCL(ncclCommCount(reinterpret_cast<ncclComm_t>(comm_v), &nranks));
    for (int i = 0; i < n_ops; ++i) {                     // validate everything before posting
        const int32_t* o = ops + 4 * i;
        MX_CHECK(o[0] == 0 || o[0] == 1, "mx_exchange_post: op %d kind %d", i, o[0]);
        MX_CHECK(o[1] >= 0 && o[1] < nranks, "mx_exchange_post: op %d peer %d outside the communicator's %d ranks",
                 i, o[1], nranks);
        if (o[0] == 0)
            MX_CHECK(rows && o[2] >= 0 && o[2] < n_rows && rows[o[2]], "mx_exchange_post: op %d row %d of %d", i,
                     o[2], n_rows);
        else
            MX_CHECK(slab && o[2] >= 0 && slab_ld_bytes >= row_bytes, "mx_exchange_post: op %d slab slot %d", i, o[2]);
    }
    ncclComm_t comm = reinterpret_cast<ncclComm_t>(comm_v);
    hipStream_t st = mx::as_stream(stream);
    const size_t count = (size_t)(row_bytes / 4);
    MX_NCCL(ncclGroupStart());
    for (int i = 0; i < n_ops; ++i) {
        const int32_t* o = ops + 4 * i;
        ncclResult_t r;
        if (o[0] == 0) {
            r = ncclSend(rows[o[2]], count, ncclFloat32, o[1], comm, st);
        } else {
            r = ncclRecv(static_cast<char*>(slab) + (int64_t)o[2] * slab_ld_bytes, count, ncclFloat32,
                         o[1], comm, st);
        }
        if (r != ncclSuccess && r != ncclInProgress) {
            (void)finish(comm, ncclGroupEnd(), "ncclGroupEnd");
            mx::set_error("%s: %s", o[0] == 0 ? "ncclSend" : "ncclRecv", ncclGetErrorString(r));
            return MX_ERR_RCCL;
        }
    }
    MX_NCCL_ON(comm, ncclGroupEnd());
    return MX_OK;
}

extern "C" int mx_exchange_round(void* comm_v, const uint8_t* flags_row, int M,
                                 const int32_t* partner, int n_global, const int32_t* owner,
                                 int my_rank, int row_base, int n_local, void* const* rows,
                                 void* slab, int64_t slab_ld_bytes, int64_t row_bytes,
                                 int* n_remote_out, void* stream) {
    MX_CHECK(comm_v && rows, "mx_exchange_round: null pointer");
    int nops = 0;
    int rc = mx_exchange_plan(flags_row, M, partner, n_global, owner, my_rank, row_base, n_local,
                              nullptr, 0, &nops);
    if (rc != MX_OK) return rc;
    std::vector<int32_t> ops(4 * (size_t)(nops > 0 ? nops : 1));
    rc = mx_exchange_plan(flags_row, M, partner, n_global, owner, my_rank, row_base, n_local,
                          ops.data(), nops, &nops);
    if (rc != MX_OK) return rc;
    int remote = 0;
    for (int i = 0; i < nops; ++i) remote += ops[4 * i] == 1;
    if (n_remote_out) *n_remote_out = remote;
    return mx_exchange_post(comm_v, ops.data(), nops, rows, n_local, slab, slab_ld_bytes, row_bytes, stream);
}

namespace {
__global__ void div_kernel(float* __restrict__ x, int64_t n, float d) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        x[i] = x[i] / d;
}

// out[i] = (sum of rows[0..nrows)[i] in the reference's order) / nrows, fp32 adds, one rounding
// each (no contraction: -ffp-contract=off), then one correctly rounded division -- the
// centralizedCommunicator's comm.allreduce(obj, MPI.SUM) + div_(size) (communicator.py:61-62):
//   TREE = 1  mpi4py's default object all-reduce (rc.fast_reduce), a binomial-tree reduction to
//             rank 0, then a broadcast: row_sum.h's tree_order
//   TREE = 0  rank order (mpi4py with fast_reduce off): row_sum.h's rank_order
// The two orders are written once, in row_sum.h, which the SlowMo outer step (slowmo.hip) includes too.
// MAXR bounds nrows; the tree runs over a register array with compile-time indices.
//   TREE = 2  the same binomial tree for any nrows, row by row: a binary counter of partial sums
//             (stack[l] = the sum of the last complete block of 2^l rows; pushing a row merges
//             stack[l] + carry while bit l of the count is set) and a right-to-left fold of the
//             stack at the end -- ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + x6) for 7 rows, exactly
//             the mask loop's order (checked against it for 1..300 rows in tests/reforder.py).
// The mean written to ndst destination rows (dst + d * dst_ld; mx_mean_rows: one): the all-reduce
// of centralizedCommunicator for workers held as rows of one arena (every worker's row becomes the
// mean) in ONE pass -- each lane reads a column of every row, then writes that column of every
// destination row, so dst == rows (in place) is safe.  Scalar form (any row count, order,
// alignment); the 16-byte forms are mean4_kernel and mean_tile_kernel below.
typedef float f4v __attribute__((ext_vector_type(4)));

template <typename V, int TREE, int MAXR>
__global__ __launch_bounds__(256) void mean_to_kernel(const V* rows, int nrows, int64_t ld, int64_t count,
                                                      float size, V* dst, int ndst, int64_t dst_ld) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        V acc;
        if (TREE == 2) {                          // binary counter of partial sums (above)
            constexpr int L = 24;
            V stack[L];
#pragma unroll
            for (int l = 0; l < L; ++l) stack[l] = V(0.0f);
            for (int r = 0; r < nrows; ++r) {
                V p = rows[(int64_t)r * ld + i];
                bool carry = true;
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const bool set = (r >> l) & 1;
                    if (carry && set) p = stack[l] + p;
                    else if (carry) { stack[l] = p; carry = false; }
                }
            }
            bool have = false;
            acc = V(0.0f);
#pragma unroll
            for (int l = 0; l < L; ++l)
                if ((nrows >> l) & 1) {
                    acc = have ? stack[l] + acc : stack[l];
                    have = true;
                }
        } else if (TREE) {
            V v[MAXR];
#pragma unroll
            for (int r = 0; r < MAXR; ++r)
                v[r] = r < nrows ? __builtin_nontemporal_load(rows + (int64_t)r * ld + i) : V(0.0f);
            mx::rowsum::tree_sum<MAXR>(v, nrows);
            acc = v[0];
        } else {
            acc = __builtin_nontemporal_load(rows + i);
            for (int r = 1; r < nrows; ++r) acc = acc + __builtin_nontemporal_load(rows + (int64_t)r * ld + i);
        }
        const V m = acc / size;
        for (int d = 0; d < ndst; ++d) __builtin_nontemporal_store(m, dst + (int64_t)d * dst_ld + i);
    }
}

// The 16-byte path with U columns (4-float vectors) per lane per step, U loads per row in flight:
// columns base + u * 256 + lane of a U * 256-column block; blocks strided over the grid.
template <int TREE, int U>
__global__ __launch_bounds__(256) void mean4_kernel(const f4v* rows, int nrows, int64_t ld, int64_t count,
                                                    float size, f4v* dst, int ndst, int64_t dst_ld) {
    for (int64_t b0 = (int64_t)blockIdx.x * (U * 256); b0 < count; b0 += (int64_t)gridDim.x * (U * 256)) {
        f4v acc[U];
        if (TREE) {
            f4v v[8][U];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t i = b0 + u * 256 + threadIdx.x;
                    v[r][u] = (r < nrows && i < count) ? __builtin_nontemporal_load(rows + (int64_t)r * ld + i)
                                                       : f4v(0.0f);
                }
            mx::rowsum::tree_order<8>(nrows, [&](int i, int j) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < U; ++u) v[i][u] = v[i][u] + v[j][u];
            });
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = v[0][u];
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = b0 + u * 256 + threadIdx.x;
                acc[u] = i < count ? __builtin_nontemporal_load(rows + i) : f4v(0.0f);
            }
            for (int r = 1; r < nrows; ++r)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t i = b0 + u * 256 + threadIdx.x;
                    acc[u] = acc[u] + (i < count ? __builtin_nontemporal_load(rows + (int64_t)r * ld + i) : f4v(0.0f));
                }
        }
        for (int d = 0; d < ndst; ++d)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = b0 + u * 256 + threadIdx.x;
                if (i < count) __builtin_nontemporal_store(acc[u] / size, dst + (int64_t)d * dst_ld + i);
            }
    }
}

// The mixing kernel's tile geometry for up to 8 rows: one workgroup per 512-column tile (128
// 4-float vectors).  The rows' 2 KB pieces are staged in LDS with 16-byte loads (each wave load is
// 1 KB of one row), then every lane sums its column in the same order as mean4_kernel<TREE> (the
// same adds, the same division: identical bits) and stores every other destination row under the
// store policy SP (mx::StorePolicy, mx_mix_set "store_policy").
template <int TREE, int SP = mx::kStoreNt>
__global__ __launch_bounds__(256) void mean_tile_kernel(const f4v* rows, int nrows, int64_t ld, float size,
                                                        f4v* dst, int ndst, int64_t dst_ld) {
    constexpr int C4 = 128;
    __shared__ f4v lds[8 * C4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * C4;
    f4v R[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = wave * 64 + 256 * j;                 // wave-uniform row e / C4
        R[j] = e / C4 < nrows ? __builtin_nontemporal_load(rows + (int64_t)(e / C4) * ld + c0 + e % C4 + lane)
                              : f4v(0.0f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) lds[wave * 64 + 256 * j + lane] = R[j];
    __syncthreads();
    const int c = tid % C4, h = tid / C4;
    f4v v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = lds[r * C4 + c];
    const auto add = [&](int i, int j) __attribute__((always_inline)) { v[i] = v[i] + v[j]; };
    if (TREE) mx::rowsum::tree_order<8>(nrows, add);
    else mx::rowsum::rank_order<8>(nrows, add);
    const f4v m = v[0] / size;
    for (int d = h; d < ndst; d += 2) mx::store16<SP>(dst + (int64_t)d * dst_ld + c0 + c, m);
}

inline unsigned grid_of(int64_t count) {
    int64_t g = (count + 255) / 256;
    return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
}  // namespace

extern "C" int mx_allreduce_mean(void* comm_v, float* buf, int64_t count, int nranks, void* stream) {
    MX_CHECK(comm_v && (buf || count == 0) && nranks >= 1, "mx_allreduce_mean: bad arguments");
    if (count == 0) return MX_OK;
    hipStream_t st = mx::as_stream(stream);
    ncclComm_t comm = reinterpret_cast<ncclComm_t>(comm_v);
    MX_NCCL_ON(comm, ncclAllReduce(buf, buf, (size_t)count, ncclFloat32, ncclSum, comm, st));
    hipLaunchKernelGGL(div_kernel, dim3(grid_of(count)), dim3(256), 0, st, buf, count, (float)nranks);
    MX_LAUNCH_CHECK();
    return MX_OK;
}

extern "C" int mx_mean_rows_to(const float* rows, int nrows, int64_t ld, int64_t count, int order, float* dst,
                               int ndst, int64_t dst_ld, void* stream);

// mx_mean_rows_to's 16-byte path: everything 16-byte aligned and the <= 8-row tree or rank order
// (shared with mx_mean_kernel_name, so the name reported is the kernel launched)
static bool mean_vec_path(const float* rows, int nrows, int64_t ld, int64_t count, int order, const float* dst,
                          int ndst, int64_t dst_ld) {
    return count >= 4 && ld % 4 == 0 && (ndst <= 1 || dst_ld % 4 == 0) &&
           ((uintptr_t)rows | (uintptr_t)dst) % 16 == 0 && (order == 1 || nrows <= 8);
}

// One destination row: the same kernels as mx_mean_rows_to (identical summation order and bits).
extern "C" int mx_mean_rows(const float* rows, int nrows, int64_t ld, int64_t count, int order, float* out,
                            void* stream) {
    MX_CHECK(rows && out && nrows >= 1 && nrows <= (1 << 24) && ld >= count && count >= 0,
             "mx_mean_rows: nrows=%d (1..2^24) ld=%lld count=%lld", nrows, (long long)ld, (long long)count);
    MX_CHECK(order == 0 || order == 1, "mx_mean_rows: order %d (0 tree, 1 rank order)", order);
    return mx_mean_rows_to(rows, nrows, ld, count, order, out, 1, count, stream);
}

extern "C" int mx_mean_rows_to(const float* rows, int nrows, int64_t ld, int64_t count, int order, float* dst,
                               int ndst, int64_t dst_ld, void* stream) {
    MX_CHECK(rows && dst && nrows >= 1 && nrows <= (1 << 24) && ld >= count && count >= 0 && ndst >= 0 &&
                 (ndst <= 1 || dst_ld >= count),
             "mx_mean_rows_to: nrows=%d ld=%lld count=%lld ndst=%d dst_ld=%lld", nrows, (long long)ld,
             (long long)count, ndst, (long long)dst_ld);
    MX_CHECK(order == 0 || order == 1, "mx_mean_rows_to: order %d (0 tree, 1 rank order)", order);
    MX_CHECK(dst == rows ? (dst_ld == ld || ndst <= 1) : true, "mx_mean_rows_to: in place needs dst_ld == ld");
    if (count == 0 || ndst == 0) return MX_OK;
    {
        // every kernel reads a column of every row before writing that column: a destination that
        // overlaps the rows is safe only when each destination element sits in the same column of
        // the rows' frame (offset and stride whole multiples of ld); anything else is refused
        const uintptr_t r0 = (uintptr_t)rows, r1 = (uintptr_t)(rows + (int64_t)(nrows - 1) * ld + count);
        const uintptr_t d0 = (uintptr_t)dst, d1 = (uintptr_t)(dst + (int64_t)(ndst - 1) * (ndst > 1 ? dst_ld : 0) + count);
        const bool overlap = d0 < r1 && r0 < d1;
        const int64_t off = (int64_t)(dst - rows);
        MX_CHECK(!overlap || (off % ld == 0 && (ndst <= 1 || dst_ld % ld == 0)),
                 "mx_mean_rows_to: dst overlaps rows at a column offset (only whole-row aliasing is supported)");
    }
    hipStream_t st = mx::as_stream(stream);
    const float d = (float)nrows;
    const bool vec = mean_vec_path(rows, nrows, ld, count, order, dst, ndst, dst_ld);
    if (vec) {
        const int64_t c4 = count / 4, tail = count - 4 * c4;
        if (tail) {                               // the last 1-3 columns: scalar lanes, same order
            const int64_t o = 4 * c4;
            if (order == 1)
                hipLaunchKernelGGL((mean_to_kernel<float, 0, 1>), dim3(1), dim3(256), 0, st, rows + o, nrows, ld,
                                   tail, d, dst + o, ndst, dst_ld);
            else
                hipLaunchKernelGGL((mean_to_kernel<float, 1, 8>), dim3(1), dim3(256), 0, st, rows + o, nrows, ld,
                                   tail, d, dst + o, ndst, dst_ld);
            MX_LAUNCH_CHECK();
        }
        const f4v* r4 = reinterpret_cast<const f4v*>(rows);
        f4v* d4 = reinterpret_cast<f4v*>(dst);
        // a flat grid, 4 vectors per lane (16 loads in flight per lane for 4 rows): 0.285 ms for
        // 8 x 25.6M in place = 0.72 of 8 TB/s, against 0.322 ms for a 4096-block persistent grid
        // with one vector per lane per step, 0.287 with two, 0.31 with two on CUs x 8 blocks
        // (tools/mean_ab.py, profiles/r04b_mean_rows_geometry.log)
        // up to 8 rows: whole 512-column tiles through LDS (mean_tile_kernel: 0.2768 vs 0.2838 ms
        // for 8 x 25.6M in place, 0.74 vs 0.72 of 8 TB/s, 3 interleaved repeats,
        // profiles/r04ac_mean_tile_ab.log); the remaining vectors (< 128) as before
        int64_t done4 = 0;
        if (nrows <= 8 && c4 >= 128) {
            const int64_t nt = c4 / 128;
            // large rounds at mean_wgpc workgroups per CU (dynamic LDS cap): every load of a tile
            // is issued at kernel start, so a few tiles in flight per CU stream best -- 8 x 25.6M in
            // place 0.2796 -> 0.2590 ms at 3 per CU (0.73 -> 0.79 of 8 TB/s; tools/occ_sweep.py)
            const size_t pad = (int64_t)nrows * count * 4 > ((int64_t)64 << 20)
                                   ? mx::lds_cap_pad(8 * 128 * (int)sizeof(f4v), mx::g_mean_wgpc) : 0;
            // store policy: forced, or auto -- the chosen policy above 320 MB of rows, nt below
            const int pol = mx::store_policy_of(mx::g_store_policy, (int64_t)nrows * count * 4, mx::kStoreAutoPolicy);
#define MX_MEAN_TILE(T, P)                                                                                    \
    hipLaunchKernelGGL((mean_tile_kernel<T, P>), dim3((unsigned)nt), dim3(256), pad, st, r4, nrows, ld / 4, d, d4, \
                       ndst, dst_ld / 4)
#define MX_MEAN_POL(T)                                                     \
    do {                                                                   \
        if (pol == mx::kStoreSc1) MX_MEAN_TILE(T, mx::kStoreSc1);          \
        else if (pol == mx::kStoreSc1Nt) MX_MEAN_TILE(T, mx::kStoreSc1Nt); \
        else if (pol == mx::kStoreSc0Sc1) MX_MEAN_TILE(T, mx::kStoreSc0Sc1); \
        else MX_MEAN_TILE(T, mx::kStoreNt);                                \
    } while (0)
            if (order == 1) MX_MEAN_POL(0);
            else MX_MEAN_POL(1);
#undef MX_MEAN_POL
#undef MX_MEAN_TILE
            MX_LAUNCH_CHECK();
            done4 = nt * 128;
        }
        if (done4 < c4) {
        constexpr int U = 4;
        const int64_t rest = c4 - done4;
        const int64_t gg = (rest + U * 256 - 1) / (U * 256);
        if (order == 1)
            hipLaunchKernelGGL((mean4_kernel<0, U>), dim3((unsigned)gg), dim3(256), 0, st, r4 + done4, nrows, ld / 4, rest, d,
                               d4 + done4, ndst, dst_ld / 4);
        else
            hipLaunchKernelGGL((mean4_kernel<1, U>), dim3((unsigned)gg), dim3(256), 0, st, r4 + done4, nrows, ld / 4, rest, d,
                               d4 + done4, ndst, dst_ld / 4);
        }
    } else if (order == 1) {
        hipLaunchKernelGGL((mean_to_kernel<float, 0, 1>), dim3(grid_of(count)), dim3(256), 0, st, rows, nrows, ld,
                           count, d, dst, ndst, dst_ld);
    } else if (nrows <= 8) {
        hipLaunchKernelGGL((mean_to_kernel<float, 1, 8>), dim3(grid_of(count)), dim3(256), 0, st, rows, nrows, ld,
                           count, d, dst, ndst, dst_ld);
    } else if (nrows <= 64) {
        hipLaunchKernelGGL((mean_to_kernel<float, 1, 64>), dim3(grid_of(count)), dim3(256), 0, st, rows, nrows, ld,
                           count, d, dst, ndst, dst_ld);
    } else {
        hipLaunchKernelGGL((mean_to_kernel<float, 2, 1>), dim3(grid_of(count)), dim3(256), 0, st, rows, nrows, ld,
                           count, d, dst, ndst, dst_ld);
    }
    MX_LAUNCH_CHECK();
    return MX_OK;
}

// The kernel that moves the bulk of the mx_mean_rows_to call with the same arguments -- the same
// dispatch as above, alignment included (nothing is launched or dereferenced), for reports
// (bench.py's centralized figure).
extern "C" const char* mx_mean_kernel_name(const float* rows, int nrows, int64_t ld, int64_t count, int order,
                                           const float* dst, int ndst, int64_t dst_ld) {
    if (nrows < 1 || count < 0 || ld < count || (order != 0 && order != 1)) return "invalid";
    if (mean_vec_path(rows, nrows, ld, count, order, dst, ndst, dst_ld)) {
        if (nrows <= 8 && count / 4 >= 128) return order == 1 ? "mean_tile_kernel<0>" : "mean_tile_kernel<1>";
        return order == 1 ? "mean4_kernel<0, 4>" : "mean4_kernel<1, 4>";
    }
    if (order == 1) return "mean_to_kernel<float, 0, 1>";
    if (nrows <= 8) return "mean_to_kernel<float, 1, 8>";
    if (nrows <= 64) return "mean_to_kernel<float, 1, 64>";
    return "mean_to_kernel<float, 2, 1>";
}

extern "C" int mx_allgather(void* comm_v, const float* send, int64_t count, float* gather, void* stream) {
    MX_CHECK(comm_v && count >= 0 && (count == 0 || (send && gather)), "mx_allgather: bad arguments");
    if (count == 0) return MX_OK;
    ncclComm_t comm = reinterpret_cast<ncclComm_t>(comm_v);
    MX_NCCL_ON(comm, ncclAllGather(send, gather, (size_t)count, ncclFloat32, comm, mx::as_stream(stream)));
    return MX_OK;
}

extern "C" int mx_allreduce_mean_ordered(void* comm_v, float* buf, int64_t count, float* gather, int order,
                                         void* stream) {
    MX_CHECK(comm_v && (count == 0 || (buf && gather)), "mx_allreduce_mean_ordered: bad arguments");
    if (count == 0) return MX_OK;
    int nranks = 0;
    MX_NCCL(ncclCommCount(reinterpret_cast<ncclComm_t>(comm_v), &nranks));
    int rc = mx_allgather(comm_v, buf, count, gather, stream);
    if (rc != MX_OK) return rc;
    return mx_mean_rows(gather, nranks, count, count, order, buf, stream);
}

// ---------------------------------------------------------------------------------- pull transport
// Device buffers shared between the processes of one node (one per GPU): each rank publishes a
// snapshot of its rows in a buffer of its own, the peers map it (IPC, dmabuf) and the mixing
// kernel reads a partner's row straight from the peer's HBM over xGMI -- no RCCL FIFO copies,
// no receive slab.  See engine.PullTransport for the round protocol (double-buffered snapshots,
// one barrier per round).
static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is expected to be 64 bytes");

extern "C" int mx_ipc_handle_bytes(void) { return (int)sizeof(hipIpcMemHandle_t); }

// Export accounting and the one refusal the runtime produces.  hipIpcGetMemHandle returns
// "invalid argument" for a fresh hipMalloc block that lands on the address range this process
// released moments before by closing a peer's IPC import (hipIpcCloseMemHandle): pinned by
// tools/ipc_reuse_probe.py (two ranks; re-export after closing the imports: 8 of 120 refused, with a
// device synchronize 9, after a 50 ms sleep 5; while the import is still open: 0 --
// profiles/r06t_ipc_reuse_probe.json).  That is the sequence of a group's close() followed by the
// next group's bind(), the round-5 and round-6 suite failures.  So a refused block is kept while a
// second one is allocated -- necessarily elsewhere -- and exported; then the first is freed (knob
// "hold", default on; 21 of 21 refusals recovered in the probe, 0 final).  Counted process-wide and
// read back by engine.PullTransport.bind: every export call, every refusal of a first block that a
// second one recovered (mx_ipc_get "recovered"), and every mx_ipc_alloc that still failed
// (mx_ipc_stats' `refused`: the bench line's ipc_refused, zero in every multi-process test).  Sizes
// are rounded up to the export granule (default 2 MiB, knob "granule").
namespace {
std::atomic<int64_t> g_ipc_granule{(int64_t)2 << 20};
std::atomic<int> g_ipc_exports{0};     // hipIpcGetMemHandle calls
std::atomic<int> g_ipc_refused{0};     // mx_ipc_alloc calls that returned no exported block
std::atomic<int> g_ipc_hold{1};        // on a refusal: keep the refused block, allocate another, export it
std::atomic<int> g_ipc_recovered{0};   // first blocks refused whose second block exported
}  // namespace

extern "C" int mx_ipc_set(const char* key, int64_t value) {
    MX_CHECK(key, "mx_ipc_set: null key");
    if (!strcmp(key, "granule")) {
        MX_CHECK(value >= 1 && value <= ((int64_t)1 << 30), "mx_ipc_set: granule %lld (1 .. 1 GiB)", (long long)value);
        g_ipc_granule = value;
        return MX_OK;
    }
    if (!strcmp(key, "hold")) {
        g_ipc_hold = value ? 1 : 0;
        return MX_OK;
    }
    mx::set_error("mx_ipc_set: unknown key '%s' (granule)", key);
    return MX_ERR_INVALID;
}

extern "C" int64_t mx_ipc_get(const char* key) {
    if (key && !strcmp(key, "granule")) return g_ipc_granule.load();
    if (key && !strcmp(key, "hold")) return g_ipc_hold.load();
    if (key && !strcmp(key, "recovered")) return g_ipc_recovered.load();
    return -1;
}

extern "C" int mx_ipc_stats(int* exports, int* refused) {
    MX_CHECK(exports && refused, "mx_ipc_stats: null pointer");
    *exports = g_ipc_exports.load();
    *refused = g_ipc_refused.load();
    return MX_OK;
}

extern "C" int mx_ipc_alloc(int64_t bytes, void** ptr_out, void* handle_out) {
    MX_CHECK(bytes > 0 && ptr_out && handle_out, "mx_ipc_alloc: bad arguments");
    const size_t gran = (size_t)g_ipc_granule.load();
    const size_t n = ((size_t)bytes + gran - 1) / gran * gran;
    void* p = nullptr;
    MX_HIP(hipMalloc(&p, n));
    // zero-filled (the pull header's epoch starts at 0) and complete before the handle is shared; on
    // a private stream waited for alone -- a device-wide synchronize would also wait for other groups'
    // rounds (a pull gate may be spinning on a peer for its whole deadline)
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemsetAsync(p, 0, n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (st) (void)hipStreamDestroy(st);
    if (e != hipSuccess) {
        (void)hipFree(p);
        mx::set_error("mx_ipc_alloc: zero fill -> %s", hipGetErrorString(e));
        return MX_ERR_HIP;
    }
    hipIpcMemHandle_t h;
    ++g_ipc_exports;
    e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess && g_ipc_hold.load()) {
        (void)hipGetLastError();
        void* q = nullptr;
        hipError_t e2 = hipMalloc(&q, n);
        if (e2 == hipSuccess) e2 = hipMemset(q, 0, n);
        if (e2 == hipSuccess) {
            ++g_ipc_exports;
            e2 = hipIpcGetMemHandle(&h, q);
        }
        (void)hipFree(p);
        if (e2 == hipSuccess) {
            ++g_ipc_recovered;
            memcpy(handle_out, &h, sizeof(h));
            *ptr_out = q;
            return MX_OK;
        }
        if (q) (void)hipFree(q);
        p = nullptr;
        e = e2;
    }
    if (e != hipSuccess) {
        ++g_ipc_refused;
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        fprintf(stderr, "[matcha_gossip] mx_ipc_alloc: hipIpcGetMemHandle refused a %zu-byte allocation (%s)\n", n,
                hipGetErrorString(e));
        mx::set_error("mx_ipc_alloc: hipIpcGetMemHandle -> %s (%zu bytes)", hipGetErrorString(e), n);
        return MX_ERR_HIP;
    }
    memcpy(handle_out, &h, sizeof(h));
    *ptr_out = p;
    return MX_OK;
}

extern "C" int mx_ipc_open(const void* handle, void** ptr_out) {
    MX_CHECK(handle && ptr_out, "mx_ipc_open: bad arguments");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void* p = nullptr;
    MX_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    *ptr_out = p;
    return MX_OK;
}

extern "C" int mx_ipc_close(void* ptr) {
    if (!ptr) return MX_OK;
    MX_HIP(hipIpcCloseMemHandle(ptr));
    return MX_OK;
}

extern "C" int mx_ipc_free(void* ptr) {
    if (!ptr) return MX_OK;
    MX_HIP(hipFree(ptr));
    return MX_OK;
}
