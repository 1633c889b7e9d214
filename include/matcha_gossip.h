/*
 * matcha_gossip.h -- C ABI of the MI355X (gfx950) gossip hot path.
 *
 * Plain pointers and sizes only.  "dev" pointers are HIP device pointers; "host" pointers are
 * ordinary host memory.  `stream` is a hipStream_t passed as void* (0 = legacy default).
 * Every entry point returns MX_OK (0) or a negative MX_ERR_* code; mx_last_error() returns
 * a thread-local message describing the last failure.
 *
 * The reference is pure Python over mpi4py.  Each entry point names the
 * reference function(s) it replaces; the binding a maintainer would add on the reference side
 * (a ctypes stub) is in INTEGRATION.md.
 */
#ifndef MATCHA_GOSSIP_H
#define MATCHA_GOSSIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_INVALID (-1)   /* bad argument (shape, alignment, range)               */
#define MX_ERR_HIP (-2)       /* HIP runtime error                                     */
#define MX_ERR_RCCL (-3)      /* RCCL error                                            */
#define MX_ERR_RNG (-4)       /* MT19937 word stream exhausted by resample events      */
#define MX_ERR_UNSUPPORTED (-5)

/* ---------------------------------------------------------------- library */
const char* mx_version(void);
const char* mx_last_error(void);

/* ---------------------------------------------------------------- schedule (L2)
 * Per-iteration activation flags on the GPU, bit-exact with numpy's legacy global RNG.
 *
 * mx_flags_binomial replaces MatchaProcessor.set_flags (graph_manager.py:298-309):
 *   for m in 0..M-1: flags[:, m] = np.random.binomial(1, p[m], T)   (matching-major draws)
 * and, with M == 1 and the output ignored, the discarded draw of FixedProcessor.set_flags
 * (graph_manager.py:213).
 *   key_in/pos_in   numpy MT19937 state (np.random.get_state()[1:3]) before the draws (host)
 *   p               activation probabilities (host, float64[M]); NaN / negative -> 0 as
 *                   graph_manager.py:305-306 does; values > 1 are rejected
 *   flags_dev       uint8 [T][M] output, row t = active_flags[t]
 *   key_out/pos_out MT19937 state after the draws (host) -- hand back to np.random.set_state
 * Blocking (synchronises `stream`).
 */
int mx_flags_binomial(const uint32_t* key_in, int pos_in, const double* p, int M, int64_t T,
                      uint8_t* flags_dev, uint32_t* key_out, int* pos_out, void* stream);

/* Same, but forces the sequential (resample-aware) walk; used by tests to pin the fix-up path. */
int mx_flags_binomial_sequential(const uint32_t* key_in, int pos_in, const double* p, int M,
                                 int64_t T, uint8_t* flags_dev, uint32_t* key_out, int* pos_out,
                                 void* stream);

/* ---------------------------------------------------------------- round plans
 * Precomputes, for every iteration t of a device-resident flag table, the per-row neighbour
 * walk of decenCommunicator.averaging (communicator.py:99-117): for each local row r
 * (global worker row_base + r) the source slots of its active partners in ascending matching
 * order, its degree and selfweight f32(1 - degree * alpha).  Partners held by another rank
 * get receive-slab slots numbered in (matching asc, sender id asc) order -- the same order
 * mx_exchange_round posts its RCCL receives in.
 *   partner_dev  int32 [M][n_global]   (GraphProcessor.neighbors_info, graph_manager.py:157-180)
 *   owner_dev    int32 [n_global]      rank owning each worker; NULL = all local
 *   plan_dev     int32 [T][mx_plan_words(n_local, M)]
 * Plan record layout (int32 words): [0] any flag set, [1] n_remote, [2] mode
 *   bits (0 after mx_plan_build): bit 0 idle-row mode (mx_plan_set_idle), bit 1 receive slots in
 *   peer GPUs' memory (mx_plan_set_peer_reads), [3] 1 if the round has more than 156 distinct
 *   remote partners (not representable: mx_plan_build then returns MX_ERR_INVALID after one
 *   4-byte read-back and a stream synchronize at build time),
 *   [4, 4+n_local) degree, [4+n_local, 4+2n_local) selfweight (f32 bits),
 *   [4+2n_local + r*M + e] source slot of row r's e-th partner (slot < n_local: local row,
 *   slot >= n_local: receive slab row slot - n_local).
 */
int64_t mx_plan_words(int n_local, int M);
int mx_plan_build(const uint8_t* flags_dev, int64_t T, int M, const int32_t* partner_dev,
                  int n_global, const int32_t* owner_dev, int my_rank, int row_base,
                  int n_local, double alpha, int32_t* plan_dev, void* stream);

/* Idle rows of an active round (degree 0 while some matching is active).  The reference still
 * runs them through averaging: recv = zeros; recv.add_(x, alpha=1 - 0*alpha) (communicator.py:
 * 113-117), i.e. x = 0 + 1.0 * x, which is x itself except that -0.0 becomes +0.0 (and a
 * signalling NaN is quieted).  mode 0 (mx_plan_build's default): such rows are not touched -- no
 * HBM traffic for them, equal to the reference under IEEE ==.  mode 1: they are streamed and
 * rewritten as fma(1.0f, x, 0.0f), bit-identical to the reference.  Sets word [2] of every
 * record of a plan table built by mx_plan_build. */
int mx_plan_set_idle(int32_t* plan_dev, int64_t T, int n_local, int M, int mode, void* stream);

/* ---------------------------------------------------------------- the hot path
 * One decentralized averaging round, in place, for every local worker:
 *   y_r = fma(f32(1-d_r*alpha), x_r, fma(f32(alpha), x_{j_d}, ... fma(f32(alpha), x_{j_1}, 0)))
 * with the partners j_1..j_d in ascending matching order -- decenCommunicator.averaging +
 * prepare_comm_buffer + reset_model (communicator.py:87-131), with flatten_tensors /
 * unflatten_tensors (comm_helpers.py:12-56) fused away: the kernel reads and writes the
 * workers' tensors where they live.
 *   seg_ptrs_dev  float* [nseg][n_slots] device table: worker slot k's copy of tensor s.
 *                 Slots [0, n_local) are the local workers (read + written in place);
 *                 slots [n_local, n_slots) are receive-slab rows (read only).
 *   seg_len_dev   int64 [nseg] floats per tensor;  tile_off_dev int64 [nseg+1] prefix of
 *                 ceil(len / mx_mix_tile(n_slots)) per tensor (see mx_mix_layout);
 *                 total_tiles = tile_off[nseg] (host copy, sizes the grid)
 *   seg_vec_dev   uint8 [nseg]: 1 if every slot pointer of that tensor is 16-byte aligned
 *   plan_dev      plan table from mx_plan_build; iter selects the record
 * Rows with degree 0 are neither read nor written (unless mx_plan_set_idle asked for the
 * reference's 0 + 1.0 * x).  No-op when the record's flags are all 0.  1-156 slots (> 64, or
 * M > 32 matchings: the untuned mix_kernel_wide); mx_mix_tile returns 0 above that.
 */
int mx_mix_tile(int n_slots);
/* Tuning knobs of the mixing kernel (process-wide), by name:
 *   blocks_per_cu  persistent workgroups per CU (grid = CUs x this, capped by the tile count)
 *   unroll         16-byte accesses per lane per slot per iteration, n_slots <= 8: 1, 2 or 4
 *                  (register-indexed kernel), 1 or 2 (LDS kernel)
 *   nontemporal    streaming (non-temporal) load/store hints: 1 on, 0 off, 2 = auto (default: the row
 *                  kernel drops them for rows of 32-320 MB, about the Infinity Cache)
 *   prefetch       issue the next iteration's loads before mixing/storing the current one
 *   regidx         register-indexed kernel (no LDS) instead of the LDS-column one, n_slots <= 8
 *   chunked        single-segment layouts: equal contiguous chunk per workgroup (1) or tile stride (0)
 *   grid           > 0: exact persistent grid size (overrides blocks_per_cu); 0 = CUs x blocks_per_cu
 *   readlane_min   LDS kernel: slot-count classes >= this (16 / 32 / 64) fetch one step's slots with
 *                  one LDS read + v_readlane and keep short chains by select (default 32)
 *   rows           row-per-wave kernel (tile staged in LDS, each wave walks whole rows' own
 *                  partner lists): 2 = every slot count (default; <= 8 slots needs unroll 1 or 2),
 *                  1 = 9-64 slots only, 0 = never
 *   split          row kernel: sub-tiles of 256+ columns per layout tile, so short rows still
 *                  give every persistent workgroup work, and 2 for 8-16 slots on flat grids:
 *                  0 = auto (default), 1 / 2 / 4 = forced
 *                  (capped at 4 for 8/16 slots, 2 for 32, 1 for 64); layouts are unaffected
 *   flat_small     row kernel, 8-16 slots: rounds of at most flat_small x (CUs x blocks_per_cu) work items
 *                  launch one workgroup per item instead of the persistent grid (default 256;
 *                  0 = always persistent; ignored when grid > 0)
 *   mid_bpc        row kernel, 8 slots, rows of at most mid_tiles x CUs layout tiles (0.4-2M params): a
 *   mid_tiles      persistent grid of mid_bpc workgroups per CU instead of the flat one (defaults 4 / 8;
 *                  mid_bpc 0 = off)
 *   spec           row kernel, 8 local slots (no receive slots), flat grid, streaming hints, rounds
 *                  moving > 64 MB (with the auto hints: > 320 MB, e.g. 8 rows of > 10.5M params): a
 *                  round whose active local
 *                  rows the caller passed (mx_gossip_mix_packed's need_host) issues their first tile's
 *                  loads before it reads the plan record (1 on, default; 0 off)
 *   spec_wgpc      ... and runs at this many workgroups per CU, capped with dynamic LDS (default 5;
 *                  0 = as many as fit): fewer tiles in flight, each issued at once -- the headline
 *                  round 0.2700 -> 0.2637 ms on one box (tools/occ_sweep.py)
 *   spec_glds      ... staging those tiles by LDS-DMA (global_load_lds_dwordx4) instead of registers,
 *                  512-column sub-tiles (default 1; headline 0.2627 -> 0.2591 ms)
 *   mean_wgpc      mx_mean_rows_to's tile kernel on rounds moving > 64 MB: workgroups per CU (default
 *                  3; 0 = as many as fit) -- 8 x 25.6M in place 0.2796 -> 0.2590 ms (tools/occ_sweep.py)
 *   store_policy   cache policy of the 16-byte row stores of the streaming (non-temporal) launches of the
 *                  row kernel's 8- and 16-slot classes and of mx_mean_rows_to's tile kernel: 1 = nt (the
 *                  line stays dirty in the write-back L2 until evicted), 2 = sc1, 3 = sc1 nt, 4 = sc0 sc1
 *                  (written through, the line dropped), forced at every size; 0 = auto (default): sc1 nt
 *                  for rounds moving > 320 MB, nt below (rows the caches hold are found there by the next
 *                  round).  Element tails, rows that are not 16-byte aligned, launches without streaming
 *                  hints and every other kernel keep their stores.  Never changes a bit.  In one process,
 *                  nt -> sc1 nt: 8 x 25.6M 0.2616 -> 0.2565 ms, 8 x 36.5M 0.3725 -> 0.3673 ms, the mean
 *                  of 8 x 25.6M 0.2629 -> 0.2584 ms (tools/store_policy_ab.py)
 *   spec_launches  (mx_mix_get only) SPEC launches so far in this process, modulo 2^31
 *   ns48           33-48 slots: 1 = a 48-slot row-kernel class instead of the 64-slot one (default 0)
 *   rows_pf2       row kernel, persistent grids of 32-64 slots: two tiles' loads in flight instead of
 *                  one -- 1 on, 0 off, 2 auto (default): when at most 5/8 of the class's slots are
 *                  staged (a GPU's share of a big topology: few local rows, many received ones)
 *   rows_tpb       row kernel, 32-64-slot classes on unsplit tiles: workgroup size 256 (default) / 512 /
 *                  1024 -- the tile's items dealt to 4 / 8 / 16 waves (measured neutral, r3)
 *   wide_tpb       wide kernel: workgroup size 256 / 512 / 1024 (default 1024: 16 waves walk the rows of
 *                  one staged piece)
 *   wide_pf2       wide kernel, 1024-thread workgroups: two pieces' loads in flight (default 1)
 *   wide_lds_kb    wide kernel: LDS budget per staged piece, 8-158 KB (default 158: 64 x 4 columns of
 *                  every slot up to 156 slots); smaller -> narrower pieces, more workgroups per CU
 *   wide_per_cu    wide kernel: workgroups per CU cap, 0 = auto (LDS- and wave-limited, <= 4)
 *   wide_plan_lds  wide kernel: copy the round's plan record to LDS when that costs no occupancy
 *                  (default 1)
 * "unroll" changes the tile size: rebuild layouts (mx_mix_layout) after setting it.
 * mx_mix_get returns the current value (negative on an unknown key).
 * mx_mix_kernel_name: the kernel mx_gossip_mix launches for n_slots under the current knobs
 * ("mix_kernel_rows", "mix_kernel_reg", "mix_kernel" for <= 64 slots and <= 32 matchings;
 * "mix_kernel_wide" for 65-156 slots -- also used for any slot count when M > 32; "" when
 * n_slots > 156). */
int mx_mix_set(const char* key, int value);
int mx_mix_get(const char* key);
const char* mx_mix_kernel_name(int n_slots);
int mx_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_gossip_mix(float* const* seg_ptrs_dev, const int64_t* seg_len_dev,
                  const int64_t* tile_off_dev, const uint8_t* seg_vec_dev, int nseg,
                  int64_t total_tiles, int n_slots, const int32_t* plan_dev, int64_t iter,
                  int n_local, int M, float alpha, void* stream);
/* The same call with its per-group arguments packed once (a round of a launch-bound row pays the
 * host cost of converting 13 arguments per call, ~1 us of a ~4 us launch from Python): `call` is
 * an mx_mix_call the caller built and keeps alive; the same bits as mx_gossip_mix.
 *   need_host  optional (NULL = none): host uint64 [n_iters], bit r set when local row r is read
 *              and written in round t (degree > 0, or any row of an active round in idle mode 1)
 *              -- the plan record's own row set, known on the host from its copy of the flags.
 *              With it, 8-slot rounds of large rows load those rows' first tile before the plan
 *              record arrives (mx_mix_set "spec" / "spec_wgpc"); a bit missing or extra costs time,
 *              never bits (the record still decides what is mixed).  iter must be < n_iters. */
typedef struct mx_mix_call {
    float* const* seg_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const uint8_t* seg_vec_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha;
    int32_t pad_;
    const uint64_t* need_host;
    int64_t n_iters;
} mx_mix_call;
int mx_gossip_mix_packed(const mx_mix_call* call, int64_t iter, void* stream);
/* Graph-replayable form: the round is read on the device from *iter_dev (int64) when the kernel
 * runs, so one captured launch (hipStreamBeginCapture / torch.cuda.graph) serves every
 * iteration; a counter outside [0, n_iters) makes the launch a no-op.  mx_iter_advance adds `by`
 * to the counter on the stream (capture it after the mix). */
int mx_gossip_mix_at(float* const* seg_ptrs_dev, const int64_t* seg_len_dev,
                     const int64_t* tile_off_dev, const uint8_t* seg_vec_dev, int nseg,
                     int64_t total_tiles, int n_slots, const int32_t* plan_dev, const int64_t* iter_dev,
                     int64_t n_iters, int n_local, int M, float alpha, void* stream);
int mx_iter_advance(int64_t* iter_dev, int64_t by, void* stream);
/* K rounds per replay with one bookkeeping launch: ctrs[j] = *iter_dev + j (j < n), then
 * *iter_dev += n, all on the device; the n mx_gossip_mix_at launches captured after it read
 * &ctrs[0] .. &ctrs[n-1].  Same rounds as n (mix_at + advance-by-1) pairs, half the launches. */
int mx_iter_expand(int64_t* iter_dev, int64_t* ctrs, int n, void* stream);

/* ---------------------------------------------------------------- the hot path, bfloat16 rows
 * The same round (decenCommunicator.averaging + prepare_comm_buffer + reset_model,
 * communicator.py:87-131) for worker rows held in bfloat16, one GPU, every partner local:
 *   acc = 0.0f;  for each active partner j (ascending matching): acc = fmaf(alpha, f32(x_j), acc)
 *   acc = fmaf(selfweight_r, f32(x_r), acc);  x_r = bf16_rne(acc)
 * f32() is the exact widening (bits << 16); alpha and selfweight are the plan record's fp32 values;
 * the fp32 chain is rounded to bfloat16 once, to nearest even, at the store (a NaN stays a NaN, payload
 * unspecified).  This is NOT what the reference's recv_buffer.add_(alpha, recv_tmp)
 * (communicator.py:92-122) would compute on bf16 tensors -- it would round after every partner;
 * see DESIGN.md §4.  Plan tables (mx_plan_build, mx_plan_set_idle) are the fp32 path's, unchanged.
 * Pointers are to 16-bit elements and every length is in elements:
 *   seg_ptrs_dev  uint16* [nseg][n_slots]; n_slots == n_local (no receive slots), 1-64 slots,
 *                 M <= 32 matchings -- anything else is MX_ERR_INVALID and nothing is launched
 *   tile_off_dev  prefix of ceil(len / mx_mix_bf16_tile(n_slots)) per tensor (mx_mix_bf16_layout);
 *                 tiles are 2048 / 2048 / 1024 / 512 columns for the 8 / 16 / 32 / 64-slot classes
 *                 (twice the fp32 classes' columns in the same LDS bytes); 0 for n_slots > 64
 *   seg_vec_dev   unused (16-byte accesses wherever a row pointer is 16-byte aligned and the 8
 *                 elements are in range, 2-byte accesses elsewhere); may be NULL
 * mx_gossip_mix_bf16_packed takes the fp32 call record unchanged (its float* table read as uint16*
 * pointers); need_host is the same load hint: rows named there are loaded before the plan record
 * arrives, and a wrong mask costs time, never bits.  mx_gossip_mix_bf16_at is the graph-replayable
 * form (round = *iter_dev, a no-op outside [0, n_iters)), as mx_gossip_mix_at.
 * mx_mix_bf16_set / _get: "nontemporal" (1 / 0 / 2 = auto as mx_mix_set's), "wgpc" (8 / 16 slots on
 * the flat grid: workgroups per CU, 0 = as many as fit), "blocks_per_cu" (persistent grids),
 * "flat_small" (8 / 16 slots: one workgroup per 1024-column work item up to this many x the
 * persistent grid), "grid" (> 0: exact persistent grid size), "split" (8 / 16 slots: work items per 2048-column layout tile, 1 / 2 / 4;
 * 0 = the default, 2 -- layouts are unaffected).  Speed only, never bits. */
int mx_mix_bf16_tile(int n_slots);
int mx_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_mix_bf16_set(const char* key, int value);
int mx_mix_bf16_get(const char* key);
int mx_gossip_mix_bf16_packed(const mx_mix_call* call, int64_t iter, void* stream);
int mx_gossip_mix_bf16_at(uint16_t* const* seg_ptrs_dev, const int64_t* seg_len_dev,
                          const int64_t* tile_off_dev, const uint8_t* seg_vec_dev, int nseg,
                          int64_t total_tiles, int n_slots, const int32_t* plan_dev, const int64_t* iter_dev,
                          int64_t n_iters, int n_local, int M, float alpha, void* stream);

/* ---------------------------------------------------------------- the hot path, SGD step fused in
 * One training iteration's optimizer.step(), optimizer.zero_grad() and communicator.communicate(model)
 * (train_mpi.py:131-142) for every local worker in ONE launch, fp32 rows, one GPU, every partner local.
 * Per row r and column c, with x, g, m the parameter, gradient and momentum-buffer elements
 * (torch.optim.SGD, dampening 0):
 *   d  = (wd != 0) ? fmaf(wd, x, g) : g                       g.add(p, alpha=wd)
 *   if mom != 0:  m = fadd(fmul(mom, m), d)                   buf.mul_(mom).add_(d_p): two roundings
 *                 d = nesterov ? fmaf(mom, m, d) : m
 *   x' = fmaf(-lr, d, x)                                      p.add_(d_p, alpha=-lr)
 * and then the round of mx_gossip_mix (decenCommunicator.averaging + prepare_comm_buffer + reset_model,
 * communicator.py:87-131) on the x' values: same plan record, alpha, selfweight, ascending-matching
 * partner order, self term last.  Rows the record reads and writes (degree > 0, or every row of an
 * active round in idle mode 1) get that FMA chain; every other row, and every row of a round whose
 * flags are all zero, gets x' stored as it is -- an all-zero round is the SGD step alone, NOT a no-op.
 * The momentum buffer starts as zeros and the momentum line always runs, with no first-step case:
 * fadd(fmul(mom, 0), d) equals torch's first-step buf = clone(d_p) under IEEE == and differs only in
 * the sign of a zero (d = -0.0 gives m = +0.0).  lr, wd and mom are the fp32 roundings of the Python
 * floats.  Traffic: 20 bytes per element (24 with zero_grads; 12 / 16 without momentum).
 * mx_sgd_mix_call, built once and kept alive by the caller (pointer tables and plan on the device):
 *   x_ptrs_dev / g_ptrs_dev / m_ptrs_dev   float* [nseg][n_local]: row r's copy of tensor s, its gradient
 *                 and its momentum buffer; m_ptrs_dev is NULL exactly when mom == 0.  x and m are
 *                 updated in place; g is read only, or overwritten with zeros when zero_grads != 0.
 *                 Nothing is written at or past seg_len of a row in any of the three.
 *   seg_len_dev   int64 [nseg] floats per tensor; tile_off_dev int64 [nseg+1] prefix of
 *                 ceil(len / mx_sgd_mix_tile(n_slots)) per tensor (mx_sgd_mix_layout); total_tiles =
 *                 tile_off[nseg].  Tiles are 1024 / 1024 / 512 / 256 columns for the 8 / 16 / 32 / 64-row
 *                 classes; 0 for n_slots > 64.
 *   plan_dev      plan table of mx_plan_build / mx_plan_set_idle, unchanged
 *   n_slots == n_local (no receive slots), 1-64 rows, M <= 32 matchings: anything else is
 *   MX_ERR_INVALID and nothing is launched.  A record with the peer-reads bit (mx_plan_set_peer_reads)
 *   is not this kernel's either: the bit lives in device memory, so it is the launch that refuses it --
 *   it writes nothing.
 * 16-byte accesses where the x, g and m pointers of a (segment, row) are all 16-byte aligned and the 4
 * elements are in range, 4-byte accesses elsewhere.
 * mx_sgd_mix(call, iter, lr, lr_dev, stream): round `iter` of the plan table; a non-NULL lr_dev (device
 * float) overrides lr and is read when the kernel runs.
 * mx_sgd_mix_at: the graph-replayable form (as mx_gossip_mix_at): the round is *iter_dev; a counter
 * outside [0, n_iters) makes the whole launch a no-op -- x, g and m are not written, the SGD step
 * included.  With lr_dev one captured launch serves every iteration and every learning rate.
 * mx_sgd_mix_set / _get: "nontemporal" (1 / 0 / 2 = auto as mx_mix_set's, on the bytes the round moves),
 * "wgpc" (8 / 16 rows on the flat grid: workgroups per CU, 0 = as many as fit), "blocks_per_cu"
 * (persistent grids), "flat_small" (8 / 16 rows: one workgroup per 512-column work item up to this many
 * x the persistent grid), "grid" (> 0: exact persistent grid size), "store_policy" (the 16-byte stores
 * of x, m, v and the masters in the streaming launches of the 8- and 16-row classes, as mx_mix_set's:
 * 1 = nt, 2 = sc1, 3 = sc1 nt forced at every size, 0 = auto; the 8-byte bf16 stores stay nt).  Speed
 * only, never bits; none of them changes the tile. */
typedef struct mx_sgd_mix_call {
    float* const* x_ptrs_dev;
    float* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, mom;
    int32_t nesterov, zero_grads, pad_;
} mx_sgd_mix_call;
int mx_sgd_mix_tile(int n_slots);
int mx_sgd_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_sgd_mix_set(const char* key, int value);
int mx_sgd_mix_get(const char* key);
int mx_sgd_mix(const mx_sgd_mix_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_at(const mx_sgd_mix_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                  const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, mixed-precision SGD fused in
 * mx_sgd_mix for models held in bfloat16: the optimizer works on fp32 MASTER rows, the master rows are
 * what the round mixes, and the bfloat16 model row is the rounded image of its master, rewritten by every
 * launch (csrc/sgd_mix_bf16.hip).  Per (segment, row) four arrays, every length in elements:
 *   w  float*    fp32 master, read and written in place
 *   g  uint16_t* bfloat16 gradient, read; overwritten with zeros when zero_grads != 0
 *   m  float*    fp32 momentum buffer, read and written; no table (NULL) exactly when mom == 0
 *   p  uint16_t* bfloat16 model row, WRITE ONLY: the kernel never reads it
 * Arithmetic contract, per row and column (torch.optim.SGD, dampening 0, on the masters):
 *   g32 = f32(g)                                  exact widening, bits << 16
 *   d   = (wd != 0) ? fmaf(wd, w, g32) : g32
 *   m   = fadd(fmul(mom, m), d);  d = nesterov ? fmaf(mom, m, d) : m      [mom != 0]; m is rounded twice
 *   w'  = fmaf(-lr, d, w)
 *   w   = mx_sgd_mix's round on the w' values (same plan record, alpha, selfweight, ascending
 *         matchings, self term last; a row the record leaves alone, and every row of an all-zero
 *         round, keeps w' as it is)
 *   p   = bf16_rne(w)                             one rounding, to nearest even, of the value stored to w;
 *                                                 NaN stays NaN, payload unspecified
 * p is written for every row in every launch that runs, rows the round leaves alone included (their w
 * changed by the SGD step).  Nothing is written at or past seg_len of a row in any of the four arrays.
 * Traffic: 20 bytes per element (22 with zero_grads; 10 / 12 without momentum) against 64 unfused.
 * Alignment rule: a lane holds 4 elements; where w and m of a (segment, row) are 16-byte aligned, g and
 * p are 8-byte aligned and the 4 elements are in range, the accesses are 16 bytes on w / m and 8 bytes
 * on g / p; elsewhere they are per element (4 / 2 bytes), zero-filled past the end.
 * mx_sgd_mix_bf16_call is mx_sgd_mix_call with the four tables above; the other fields, the tile
 * (mx_sgd_mix_bf16_tile: 1024 / 1024 / 512 / 256 columns, 0 above 64 rows), the layout prefix, the
 * host-side refusals (MX_ERR_INVALID, nothing launched: n_slots != n_local, more than 64 rows, M outside
 * [1, 32], a momentum table that does not match mom, nesterov without momentum, a null table -- p
 * included) and the launch-side no-ops (a peer-reads plan record; for _at a counter outside
 * [0, n_iters): none of the four arrays is written, the SGD step included) are mx_sgd_mix's.
 * mx_sgd_mix_bf16_set / _get: "nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid", "store_policy", as
 * mx_sgd_mix_set's and independent of them.  Speed only, never bits; none of them changes the tile. */
typedef struct mx_sgd_mix_bf16_call {
    float* const* w_ptrs_dev;
    uint16_t* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    uint16_t* const* p_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, mom;
    int32_t nesterov, zero_grads, pad_;
} mx_sgd_mix_bf16_call;
int mx_sgd_mix_bf16_tile(int n_slots);
int mx_sgd_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_sgd_mix_bf16_set(const char* key, int value);
int mx_sgd_mix_bf16_get(const char* key);
int mx_sgd_mix_bf16(const mx_sgd_mix_bf16_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_bf16_at(const mx_sgd_mix_bf16_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                       const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, AdamW / Adam step fused in
 * mx_sgd_mix with torch.optim.AdamW's (decoupled != 0) or torch.optim.Adam's (decoupled == 0) update in
 * place of SGD's (csrc/adamw_mix.hip): fp32 rows, one GPU, every partner local, one launch per training
 * iteration.  No amsgrad, no maximize.  Per row and column, with x, g, m, v the parameter, gradient,
 * exp_avg and exp_avg_sq elements, every operation ONE IEEE fp32 rounding (explicit fmas, correctly
 * rounded square root and division, denormals kept):
 *   decay = fmaf(-lr, wd, 1.0f)                              once per launch
 *   x1 = (wd != 0 &&  decoupled) ? fmul(x, decay) : x        AdamW: p.mul_(1 - lr*wd)
 *   g1 = (wd != 0 && !decoupled) ? fmaf(wd, x, g) : g        Adam:  g.add(p, alpha=wd)
 *   m' = fmaf(omb1, fsub(g1, m), m)                          exp_avg.lerp_(g, 1 - beta1)
 *   v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))            exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
 *   den = fadd(fdiv(fsqrt(v'), bc2s), eps)
 *   ss  = fdiv(lr, bc1)                                      once per launch
 *   x'  = fmaf(-ss, fdiv(m', den), x1)
 * and then mx_sgd_mix's round on the x' values (same plan record, alpha, selfweight, ascending
 * matchings, self term last; a row the record leaves alone, and every row of an all-zero round, keeps
 * x' as it is -- an all-zero round is the optimizer step alone, NOT a no-op).  wd, eps and beta2 are the
 * fp32 roundings of the Python floats, omb1 / omb2 the fp32 roundings of the fp64 values 1 - beta1 and
 * 1 - beta2; m and v start as zeros.
 * Bias correction: (bc1, bc2s) of optimizer step t >= 1 are bias_dev[min(t, n_bias) - 1], bias_dev being
 * float [n_bias][2] with entry t-1 = (f32(1 - beta1**t), f32(sqrt(1 - beta2**t))) computed by the host in
 * double precision, as torch does, and ending at the first entry where both are exactly 1.0f (every
 * later step uses it, exactly).  Nothing computes pow on the device, so a launch is bit-reproducible
 * and graph-replayable.
 * Traffic: 28 bytes per element (32 with zero_grads) against 88 for the torch op sequence + the round.
 * mx_adamw_mix_call is mx_sgd_mix_call with four tables -- x / g / m / v_ptrs_dev, float* [nseg][n_local];
 * x, m and v are updated in place, g is read only or overwritten with zeros when zero_grads != 0, and
 * nothing is written at or past seg_len of a row in any of the four -- plus the bias table.  The tile
 * (mx_adamw_mix_tile: 1024 / 1024 / 512 / 256 columns for the 8 / 16 / 32 / 64-row classes, 0 above 64
 * rows), the layout prefix and the host-side refusals (MX_ERR_INVALID, nothing launched:
 * n_slots != n_local, more than 64 rows, M outside [1, 32], a null table, n_bias < 1) are mx_sgd_mix's.
 * 16-byte accesses where the x, g, m and v pointers of a (segment, row) are all 16-byte aligned and the 4
 * elements are in range, 4-byte accesses elsewhere.
 * mx_adamw_mix(call, iter, step, lr, lr_dev, stream): round `iter` at optimizer step `step`; step < 1 is
 * MX_ERR_INVALID and nothing is launched.  A non-NULL lr_dev (device float) overrides lr and is read
 * when the kernel runs.
 * mx_adamw_mix_at: the graph-replayable form: round *iter_dev, step *step_dev (both device int64,
 * advanced by the caller, e.g. mx_iter_advance).  An iteration counter outside [0, n_iters) or a step
 * below 1 makes the launch a complete no-op: none of x, g, m, v is written.  So does a plan record with
 * the peer-reads bit, in either form.
 * mx_adamw_mix_set / _get: "nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid", "store_policy", as
 * mx_sgd_mix_set's and independent of them.  Speed only, never bits; none of them changes the tile. */
typedef struct mx_adamw_mix_call {
    float* const* x_ptrs_dev;
    float* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    float* const* v_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    const float* bias_dev;
    int64_t total_tiles;
    int64_t n_bias;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, omb1, beta2, omb2, eps;
    int32_t decoupled, zero_grads;
} mx_adamw_mix_call;
int mx_adamw_mix_tile(int n_slots);
int mx_adamw_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_adamw_mix_set(const char* key, int value);
int mx_adamw_mix_get(const char* key);
int mx_adamw_mix(const mx_adamw_mix_call* call, int64_t iter, int64_t step, float lr, const float* lr_dev,
                 void* stream);
int mx_adamw_mix_at(const mx_adamw_mix_call* call, const int64_t* iter_dev, int64_t n_iters,
                    const int64_t* step_dev, float lr, const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, mixed-precision AdamW / Adam fused in
 * mx_adamw_mix for models held in bfloat16 (csrc/adamw_mix_bf16.hip): the optimizer works on fp32 MASTER
 * rows with fp32 exp_avg / exp_avg_sq, the master rows are what the round mixes, and the bfloat16 model
 * row is the rounded image of its master, rewritten by every launch.  Per (segment, row) five arrays,
 * every length in elements:
 *   w  float*    fp32 master, read and written in place
 *   g  uint16_t* bfloat16 gradient, read; overwritten with zeros when zero_grads != 0
 *   m  float*    fp32 exp_avg, read and written
 *   v  float*    fp32 exp_avg_sq, read and written
 *   p  uint16_t* bfloat16 model row, WRITE ONLY: the kernel never reads it
 * Arithmetic contract, per row and column, every line ONE IEEE fp32 rounding (explicit fmas, correctly
 * rounded square root and division, denormals kept):
 *   g32 = f32(g)                                             exact widening, bits << 16
 *   decay = fmaf(-lr, wd, 1.0f)                              once per launch
 *   w1 = (wd != 0 &&  decoupled) ? fmul(w, decay) : w
 *   g1 = (wd != 0 && !decoupled) ? fmaf(wd, w, g32) : g32
 *   m' = fmaf(omb1, fsub(g1, m), m)
 *   v' = fmaf(omb2, fmul(g1, g1), fmul(beta2, v))
 *   den = fadd(fdiv(fsqrt(v'), bc2s), eps)
 *   ss  = fdiv(lr, bc1)                                      once per launch
 *   w'  = fmaf(-ss, fdiv(m', den), w1)
 *   w   = mx_sgd_mix's round on the w' values (same plan record, alpha, selfweight, ascending
 *         matchings, self term last; a row the record leaves alone, and every row of an all-zero
 *         round, keeps w' as it is)
 *   p   = bf16_rne(w)                                        one rounding, to nearest even, of the value
 *                                                            stored to w; NaN stays NaN, payload unspecified
 * (bc1, bc2s) are mx_adamw_mix's: bias_dev[min(t, n_bias) - 1]; nothing computes pow on the device.
 * p is written for every row in every launch that runs, rows the round leaves alone included (their w
 * changed by the optimizer step).  Nothing is written at or past seg_len of a row in any of the five.
 * Traffic: 28 bytes per element (30 with zero_grads) against 100 for g.float(), the torch op sequence,
 * the fp32 round and the cast back.
 * Alignment rule: a lane holds 4 elements; where w, m and v of a (segment, row) are 16-byte aligned, g
 * and p are 8-byte aligned and the 4 elements are in range, the accesses are 16 bytes on w / m / v and
 * 8 bytes on g / p; elsewhere they are per element (4 / 2 bytes), zero-filled past the end.
 * mx_adamw_mix_bf16_call is mx_adamw_mix_call with the five tables above; the other fields, the tile
 * (mx_adamw_mix_bf16_tile: 1024 / 1024 / 512 / 256 columns, 0 above 64 rows), the layout prefix, the
 * host-side refusals (MX_ERR_INVALID, nothing launched: n_slots != n_local, more than 64 rows, M outside
 * [1, 32], n_bias < 1, step < 1, a null table -- p included) and the launch-side no-ops (a peer-reads
 * plan record; for _at an iteration counter outside [0, n_iters) or a step counter below 1: none of the
 * five arrays is written) are mx_adamw_mix's.
 * mx_adamw_mix_bf16_set / _get: "nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid", "store_policy", as
 * mx_adamw_mix_set's and independent of them.  Speed only, never bits; none of them changes the tile. */
typedef struct mx_adamw_mix_bf16_call {
    float* const* w_ptrs_dev;
    uint16_t* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    float* const* v_ptrs_dev;
    uint16_t* const* p_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    const float* bias_dev;
    int64_t total_tiles;
    int64_t n_bias;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, omb1, beta2, omb2, eps;
    int32_t decoupled, zero_grads;
} mx_adamw_mix_bf16_call;
int mx_adamw_mix_bf16_tile(int n_slots);
int mx_adamw_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_adamw_mix_bf16_set(const char* key, int value);
int mx_adamw_mix_bf16_get(const char* key);
int mx_adamw_mix_bf16(const mx_adamw_mix_bf16_call* call, int64_t iter, int64_t step, float lr, const float* lr_dev,
                      void* stream);
int mx_adamw_mix_bf16_at(const mx_adamw_mix_bf16_call* call, const int64_t* iter_dev, int64_t n_iters,
                         const int64_t* step_dev, float lr, const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- global-norm gradient clipping
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) -- 2-norm, error_if_nonfinite=False -- PER
 * WORKER, for the four fused launches above (csrc/grad_norm.hip).  Every row of the gradient tables is one
 * model's gradient and gets its own norm and its own factor:
 *   S_r      = sum over every segment of row r of f64(g)^2     every square formed and summed in fp64; bfloat16
 *                                                              is widened exactly (bits << 16)
 *   norm[r]  = f32(sqrt(S_r))                                  fp64 square root, ONE rounding to fp32: the
 *                                                              value clip_grad_norm_ returns, before clipping
 *   c        = fmul(fdiv(1.0f, fadd(norm[r], 1e-6f)), max_norm)   one fp32 rounding each: torch evaluates its
 *                                                              max_norm / (total_norm + 1e-6) on a tensor as
 *                                                              reciprocal() * max_norm (Tensor.__rtruediv__)
 *   scale[r] = c > 1.0f ? 1.0f : c                             torch's clamp(max=1.0); a NaN stays a NaN
 * The summation order is fixed (csrc/grad_norm.hip): norm[r] depends only on row r's values and lengths,
 * and the bits are the same on every launch and under every knob; no floating-point atomics.  For
 * P <= 2^26 elements per row any fp64 order is within P * 2^-53 of the exact sum, so norm[r] is within
 * 1 fp32 ulp of the correctly rounded norm.  A NaN element gives a NaN norm and factor, an Inf element
 * norm Inf and factor 0, a row of zeros norm 0 and factor 1.
 * mx_grad_norm_call, built once and kept alive by the caller:
 *   g_ptrs_dev   [nseg][n_local] device table of row pointers and seg_len_dev int64 [nseg] elements per
 *                tensor: the g_ptrs_dev / seg_len_dev of the fused call records, read only.  Nothing at or
 *                past seg_len of a row is read into the sum.
 *   elem_size    4 (fp32) or 2 (bfloat16 bit patterns)
 *   work_dev     fp64 workspace of mx_grad_norm_layout(seg_len_host, nseg, n_local, &chunks) BYTES (the
 *                return value; negative on bad arguments); `chunks` is what that call stored: one slot
 *                per mx_grad_norm_cols() = 4096 columns of a (segment, row).  Every slot is rewritten by
 *                every call: no zeroing.
 *   norm_dev / scale_dev   float [n_local] outputs, on the device
 * mx_grad_norm(call, stream) enqueues two launches -- per-work-item partials into their own workspace
 * slots, then one workgroup per row adding them in a fixed order -- with no host synchronisation and no
 * host read, so it can be captured in a graph.  16-byte loads where a row pointer is 16-byte aligned
 * and the elements are in range, per-element loads elsewhere; plain (temporal) loads, because the fused
 * launch reads the same gradient right afterwards.
 * MX_ERR_INVALID, nothing launched: a null call record, table, output or workspace; elem_size other than
 * 2 or 4; n_local outside [1, 64]; max_norm not a positive finite number.
 * mx_grad_norm_set / _get: "blocks_per_cu" (persistent workgroups per CU of the partial pass, default
 * 8), "grid" (> 0: exact grid size).  Which workgroup computes a work item, never how: speed only. */
typedef struct mx_grad_norm_call {
    const void* const* g_ptrs_dev;
    const int64_t* seg_len_dev;
    double* work_dev;
    float* norm_dev;
    float* scale_dev;
    int64_t chunks;
    int32_t nseg, n_local, elem_size;
    float max_norm;
} mx_grad_norm_call;
int mx_grad_norm_cols(void);
int64_t mx_grad_norm_layout(const int64_t* seg_len_host, int nseg, int n_local, int64_t* chunks_out);
int mx_grad_norm_set(const char* key, int value);
int mx_grad_norm_get(const char* key);
int mx_grad_norm(const mx_grad_norm_call* call, void* stream);

/* The fused launches with a per-row gradient factor: the call record of the unscaled entry point,
 * unchanged, plus gscale_dev (float [n_local] on the device, read when the kernel runs -- scale_dev of an
 * mx_grad_norm enqueued before it on the same stream).  Before anything else in the update
 *   g' = fmul(gscale[r], g)            fp32;  fmul(gscale[r], f32(g)) for bfloat16 gradients
 * and the L2 term, m, v and the momentum buffer all see g', as they do in torch after clip_grad_norm_.
 * g IN MEMORY is never rewritten scaled -- it is zeroed under zero_grads, otherwise left as backward wrote
 * it -- which differs from torch's in-place clipping: whoever reads the gradients after the step sees them
 * unclipped.  gscale_dev == NULL multiplies nothing: every bit is the unscaled entry point's (which pass
 * NULL themselves).  Row handling, launch-side no-ops (nothing of x / w, g, m, v, p is written) and
 * host-side refusals are the unscaled entry points'. */
int mx_sgd_mix_scaled(const mx_sgd_mix_call* call, const float* gscale_dev, int64_t iter, float lr,
                      const float* lr_dev, void* stream);
int mx_sgd_mix_scaled_at(const mx_sgd_mix_call* call, const float* gscale_dev, const int64_t* iter_dev,
                         int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_bf16_scaled(const mx_sgd_mix_bf16_call* call, const float* gscale_dev, int64_t iter, float lr,
                           const float* lr_dev, void* stream);
int mx_sgd_mix_bf16_scaled_at(const mx_sgd_mix_bf16_call* call, const float* gscale_dev, const int64_t* iter_dev,
                              int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_scaled(const mx_adamw_mix_call* call, const float* gscale_dev, int64_t iter, int64_t step,
                        float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_scaled_at(const mx_adamw_mix_call* call, const float* gscale_dev, const int64_t* iter_dev,
                           int64_t n_iters, const int64_t* step_dev, float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_bf16_scaled(const mx_adamw_mix_bf16_call* call, const float* gscale_dev, int64_t iter,
                             int64_t step, float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_bf16_scaled_at(const mx_adamw_mix_bf16_call* call, const float* gscale_dev,
                                const int64_t* iter_dev, int64_t n_iters, const int64_t* step_dev, float lr,
                                const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- consensus distance
 * How far apart the workers are (csrc/consensus.hip): every worker's distance from the mean of the n =
 * n_local rows, the consensus distance and the norm of the mean row, from ONE read of the rows, on the
 * device.  Per column c, rows fp32 or bfloat16 bit patterns (widened exactly, bits << 16):
 *   s_c      = ((f64(x_0c) + f64(x_1c)) + f64(x_2c)) + ...     fp64 adds in ROW ORDER
 *   m_c      = s_c / f64(n)                                    one IEEE fp64 division (a multiplication by
 *                                                              1/n only where n is a power of two: same bits)
 *   d_rc     = f64(x_rc) - m_c                                 one fp64 subtraction
 *   D_r      = sum_c d_rc^2       M = sum_c m_c^2              fp64 over every segment, in a fixed order
 *   dist[r]  = f32(sqrt(D_r))                                  worker r's ||x_r - mean||
 *   stats[0] = f32(sqrt((D_0 + D_1 + ... in row order) / n))   the consensus distance
 *   stats[1] = f32(sqrt(M))                                    ||mean||, for the relative figure
 * The column arithmetic is pinned because x - m cancels: near consensus another order of the mean changes
 * d by far more than an fp64 rounding.  With it pinned every d_rc is the same in every conforming
 * implementation and the sums of the non-negative squares are within P * 2^-53 of exact in any order, so
 * every output is within 1 fp32 ulp of the specification for P <= 2^26 columns.  Identical rows give
 * exactly 0.0 for every n <= 64 (n = 1 included).  A NaN or Inf anywhere in a column makes its mean
 * non-finite, and with it EVERY dist and both stats.  fp32 denormals count; +-3.4e38 does not overflow.
 * Unlike mx_grad_norm's rows, a row's distance depends on every row (the mean does).  The bits are the
 * same on every launch and under every knob; no floating-point atomics.
 * mx_consensus_call, built once and kept alive by the caller (sizeof == 64):
 *   x_ptrs_dev   [nseg][n_local] device table of row pointers and seg_len_dev int64 [nseg] elements per
 *                segment, read only.  Nothing at or past seg_len of a row is read.
 *   elem_size    4 (fp32) or 2 (bfloat16 bit patterns)
 *   work_dev     fp64 workspace of mx_consensus_layout(seg_len_host, nseg, n_local, &chunks) BYTES (the
 *                return value, 8 * (n_local + 1) * chunks; negative on bad arguments); `chunks` is what
 *                that call stored: one slot per row, and one for the mean, per mx_consensus_cols() = 4096
 *                columns of a segment.  Every slot is rewritten by every call: no zeroing.
 *   dist_dev     float [n_local];  stats_dev  float [2], on the device
 * mx_consensus(call, stream) enqueues two launches -- per-work-item partials of all rows into their own
 * workspace slots, then one workgroup adding them in a fixed order -- with no host synchronisation and no
 * host read, so it can be captured in a graph.  Vector loads (16 bytes a lane up to 16 rows, 8 up to 32, 4
 * up to 64; non-temporal) where a row pointer is 16-byte aligned and the elements are in range, per-element
 * loads elsewhere.
 * MX_ERR_INVALID, nothing launched: a null call record, table, output or workspace; elem_size other than
 * 2 or 4; n_local outside [1, 64]; nseg < 1 or chunks < 0; in mx_consensus_layout a negative length.
 * mx_consensus_set / _get: "blocks_per_cu" (persistent workgroups per CU of the partial pass, default 8),
 * "grid" (> 0: exact grid size), as mx_grad_norm_set: which workgroup computes a work item, never how. */
typedef struct mx_consensus_call {
    const void* const* x_ptrs_dev;
    const int64_t* seg_len_dev;
    double* work_dev;
    float* dist_dev;
    float* stats_dev;
    int64_t chunks;
    int32_t nseg, n_local, elem_size, pad_;
} mx_consensus_call;
int mx_consensus_cols(void);
int64_t mx_consensus_layout(const int64_t* seg_len_host, int nseg, int n_local, int64_t* chunks_out);
int mx_consensus_set(const char* key, int value);
int mx_consensus_get(const char* key);
int mx_consensus(const mx_consensus_call* call, void* stream);

/* ---------------------------------------------------------------- per-parameter-group hyperparameters
 * torch.optim's param_groups with their own weight_decay and their own learning-rate multiplier, for the
 * four fused launches above.  The columns [0, seg_len) of every segment are cut into RUNS, half-open
 * column ranges that share one pair (wd_r, s_r); both are fp32, finite and >= 0.  With lr the launch's
 * learning rate (the argument, or *lr_dev), every element of run r gets the entry point's update with
 *   lr_r = fmul(lr, s_r)               one fp32 rounding; s_r = 1.0f gives lr exactly
 *   wd -> wd_r                         the "wd != 0" tests are made per run
 *   lr -> lr_r                         SGD:   x' = fmaf(-lr_r, d, x)
 *                                      AdamW: decay = fmaf(-lr_r, wd_r, 1), ss = fdiv(lr_r, bc1)
 * and nothing else changes: momentum, betas, eps, the bias table, nesterov, decoupled, zero_grads, the
 * clip factor (gscale_dev: one norm per worker over all its runs), the mix of the x' values, the launch-side
 * no-ops and the host-side refusals are the _scaled entry points'.  s_r = 0 freezes the weights of a run
 * while its optimizer state still advances.  The call record's own wd is ignored.
 * mx_param_runs, built once and kept alive by the caller; the tables are device memory READ WHEN THE
 * KERNEL RUNS (a graph-captured launch stays valid when they are rewritten):
 *   run_off_dev   int32 [nseg + 1]: segment s owns runs [run_off[s], run_off[s + 1])
 *   run_end_dev   int64 [nruns]: exclusive end column of each run within its segment, strictly ascending
 *                 per segment, the last equal to the segment's length
 *   wd_dev, lr_scale_dev   float [nruns]
 *   nruns         run_off[nseg]
 * mx_param_runs_check validates HOST copies of the tables before they are uploaded (no GPU needed):
 * MX_ERR_INVALID with a message for a null argument, nseg < 1, run_off[0] != 0, a segment of positive
 * length without runs (a zero-length segment has none), an empty run, ends that are not ascending, a last
 * end that is not the segment's length, and a negative or non-finite wd or scale.  The launches trust the
 * device tables: they steer arithmetic only, never an address that is written.
 * mx_*_grouped(call, runs, gscale_dev, ...): runs == NULL is the _scaled entry point bit for bit (and
 * gscale_dev may be NULL as there); a non-NULL runs with a null table or nruns < 1 is MX_ERR_INVALID,
 * nothing launched.  A work item (see the kernels) that lies inside one run -- every large tensor -- takes
 * the run's pair as scalars; one that holds a boundary resolves the run per element. */
typedef struct mx_param_runs {
    const int32_t* run_off_dev;
    const int64_t* run_end_dev;
    const float* wd_dev;
    const float* lr_scale_dev;
    int32_t nruns;
} mx_param_runs;
int mx_param_runs_check(const int64_t* seg_len_host, int nseg, const int32_t* run_off_host,
                        const int64_t* run_end_host, const float* wd_host, const float* lr_scale_host);
int mx_sgd_mix_grouped(const mx_sgd_mix_call* call, const mx_param_runs* runs, const float* gscale_dev, int64_t iter,
                       float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_grouped_at(const mx_sgd_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                          const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_bf16_grouped(const mx_sgd_mix_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                            int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_sgd_mix_bf16_grouped_at(const mx_sgd_mix_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                               const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev,
                               void* stream);
int mx_adamw_mix_grouped(const mx_adamw_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                         int64_t iter, int64_t step, float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_grouped_at(const mx_adamw_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                            const int64_t* iter_dev, int64_t n_iters, const int64_t* step_dev, float lr,
                            const float* lr_dev, void* stream);
int mx_adamw_mix_bf16_grouped(const mx_adamw_mix_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                              int64_t iter, int64_t step, float lr, const float* lr_dev, void* stream);
int mx_adamw_mix_bf16_grouped_at(const mx_adamw_mix_bf16_call* call, const mx_param_runs* runs,
                                 const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters,
                                 const int64_t* step_dev, float lr, const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, Lion step fused in
 * mx_sgd_mix with the Lion update (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") in
 * place of SGD's (csrc/lion_mix.hip): fp32 rows, one GPU, every partner local, one launch per training
 * iteration.  Lion steps every weight by +-lr along the sign of an interpolation of gradient and momentum,
 * with decoupled weight decay; it keeps ONE state array and needs no sqrt, no division, no bias table and
 * no step counter.  Per row and column, every line one IEEE fp32 rounding:
 *   decay = fmaf(-lr, wd, 1)                              once per launch
 *   x1 = (wd != 0) ? fmul(x, decay) : x                   decoupled decay only, as AdamW's
 *   dm = fsub(g, m)
 *   c  = fmaf(omb1, dm, m)                                (1 - beta1) g + beta1 m in lerp form
 *   x' = c > 0 ? fsub(x1, lr) : c < 0 ? fadd(x1, lr) : c == 0 ? x1 : NaN
 *   m' = fmaf(omb2, dm, m)                                (1 - beta2) g + beta2 m
 * and then mx_sgd_mix's round on the x' values (same plan record, alpha, selfweight, ascending matchings,
 * self term last; a row the record leaves alone, and every row of an all-zero round, keeps x' as it is --
 * an all-zero round is the Lion step alone, NOT a no-op).  omb1 / omb2 are the fp32 roundings of the fp64
 * values 1 - beta; lr and wd the fp32 roundings of the Python floats.  c == 0 (either zero) leaves x1 BIT
 * FOR BIT, an x1 of -0.0 included; a NaN c gives a NaN of any payload.  The momentum buffer starts as
 * zeros; there is no first-step case.  Traffic: 20 bytes per element (24 with zero_grads), SGD with
 * momentum's.
 * mx_lion_mix_call is mx_sgd_mix_call with omb1 / omb2 in place of mom / nesterov: the three tables
 * (m_ptrs_dev is never NULL), the tile (mx_lion_mix_tile: 1024 / 1024 / 512 / 256 columns, 0 above 64
 * rows), the layout prefix, the alignment rule (16-byte accesses where x, g and m of a (segment, row) are
 * all 16-byte aligned and the 4 elements are in range, 4-byte accesses elsewhere; nothing is written at or
 * past seg_len of a row in any array), the host-side refusals (MX_ERR_INVALID, nothing launched:
 * n_slots != n_local, more than 64 rows, M outside [1, 32], a null table -- m included) and the
 * launch-side no-ops (a peer-reads plan record; for _at a counter outside [0, n_iters): x, g and m are not
 * written, the Lion step included) are mx_sgd_mix's.  _scaled and _grouped are the other families':
 * g' = fmul(gscale[r], g) before anything else; per run lr_r = fmul(lr, s_r), decay = fmaf(-lr_r, wd_r, 1),
 * the step +-lr_r, the "wd != 0" test per run, the record's own wd ignored.
 * mx_lion_mix_set / _get: "nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid", "store_policy", as
 * mx_sgd_mix_set's and independent of them.  Speed only, never bits; none of them changes the tile. */
typedef struct mx_lion_mix_call {
    float* const* x_ptrs_dev;
    float* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, omb1, omb2;
    int32_t zero_grads, pad_;
} mx_lion_mix_call;
int mx_lion_mix_tile(int n_slots);
int mx_lion_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_lion_mix_set(const char* key, int value);
int mx_lion_mix_get(const char* key);
int mx_lion_mix(const mx_lion_mix_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_at(const mx_lion_mix_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                   const float* lr_dev, void* stream);
int mx_lion_mix_scaled(const mx_lion_mix_call* call, const float* gscale_dev, int64_t iter, float lr,
                       const float* lr_dev, void* stream);
int mx_lion_mix_scaled_at(const mx_lion_mix_call* call, const float* gscale_dev, const int64_t* iter_dev,
                          int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_grouped(const mx_lion_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                        int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_grouped_at(const mx_lion_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                           const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, mixed-precision Lion fused in
 * mx_lion_mix for models held in bfloat16 (csrc/lion_mix_bf16.hip): the update runs on fp32 MASTER rows,
 * the master rows are what the round mixes, and the bfloat16 model row is the rounded image of its master,
 * rewritten by every launch.  Per (segment, row) four arrays, every length in elements:
 *   w  float*    fp32 master, read and written in place
 *   g  uint16_t* bfloat16 gradient, read; overwritten with zeros when zero_grads != 0
 *   m  momentum, read and written: float* when m_bf16 == 0, uint16_t* (bfloat16) when m_bf16 != 0
 *   p  uint16_t* bfloat16 model row, WRITE ONLY: the kernel never reads it
 * Arithmetic contract: mx_lion_mix's lines on w with g32 = f32(g) (exact widening, bits << 16) and, for a
 * bfloat16 momentum, m32 = f32(m) (exact) in place of m and bf16_rne(m') stored -- ONE rounding, to nearest
 * even, at the store; then mx_lion_mix's round on the w' values and p = bf16_rne(w) of the value stored to w
 * (NaN stays NaN, payload unspecified, in p and in a bfloat16 m alike).  p is written for every row in
 * every launch that runs.  Nothing is written at or past seg_len of a row in any of the four arrays.
 * Traffic: 20 bytes per element (22 with zero_grads) with fp32 momentum, 16 (18) with bfloat16 momentum.
 * Alignment rule: a lane holds 4 elements; where w of a (segment, row) is 16-byte aligned, m is aligned to
 * its own access (16 bytes fp32, 8 bytes bfloat16), g and p are 8-byte aligned and the 4 elements are in
 * range, the accesses are wide; elsewhere they are per element (4 / 2 bytes), zero-filled past the end.
 * The other fields, the tile, the layout prefix, the host-side refusals (a null table -- m and p included)
 * and the launch-side no-ops are mx_lion_mix's; the knobs are independent of every other family's. */
typedef struct mx_lion_mix_bf16_call {
    float* const* w_ptrs_dev;
    uint16_t* const* g_ptrs_dev;
    void* const* m_ptrs_dev;
    uint16_t* const* p_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, omb1, omb2;
    int32_t zero_grads, m_bf16;
} mx_lion_mix_bf16_call;
int mx_lion_mix_bf16_tile(int n_slots);
int mx_lion_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_lion_mix_bf16_set(const char* key, int value);
int mx_lion_mix_bf16_get(const char* key);
int mx_lion_mix_bf16(const mx_lion_mix_bf16_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_bf16_at(const mx_lion_mix_bf16_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                        const float* lr_dev, void* stream);
int mx_lion_mix_bf16_scaled(const mx_lion_mix_bf16_call* call, const float* gscale_dev, int64_t iter, float lr,
                            const float* lr_dev, void* stream);
int mx_lion_mix_bf16_scaled_at(const mx_lion_mix_bf16_call* call, const float* gscale_dev, const int64_t* iter_dev,
                               int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_bf16_grouped(const mx_lion_mix_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                             int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_lion_mix_bf16_grouped_at(const mx_lion_mix_bf16_call* call, const mx_param_runs* runs,
                                const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                                const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, quasi-global momentum fused in
 * mx_sgd_mix with quasi-global momentum (QG-DSGDm: Lin et al., ICML 2021, "Quasi-Global Momentum:
 * Accelerating Decentralized Deep Learning on Heterogeneous Data") in place of SGD's local momentum
 * (csrc/qgm_mix.hip): fp32 rows, one GPU, every partner local, one launch per training iteration.  The
 * momentum buffer mh is fed by the displacement of the worker's row AFTER the gossip round, (x_t - x_{t+1}) /
 * lr, so it follows the direction the neighbourhood actually moved, at no extra communication.  Per row and
 * column, every line one IEEE fp32 rounding (the library is built with -ffp-contract=off and every fma is
 * explicit); g is widened and clip-scaled as in every fused family (g' = fmul(gscale[r], f32(g))); beta is
 * the fp32 rounding of the Python float, omu the fp32 rounding of the fp64 value 1 - mu; (wd_r, scale_r) are
 * the run's pair, the launch's wd and 1.0 when ungrouped:
 *   lr_r = fmul(lr, scale_r)
 *   d    = (wd_r != 0) ? fmaf(wd_r, x, g) : g
 *   m    = fadd(fmul(beta, mh), d)                       mh: the quasi-global buffer, read only here
 *   s    = nesterov ? fmaf(beta, m, d) : m
 *   x'   = fmaf(-lr_r, s, x)
 *   y    = mx_sgd_mix's round on the x' values           rows the record leaves alone, and every row of an
 *                                                        all-zero round: y = x'
 *   rl   = fdiv(1.0f, lr_r)                              once per launch, or per run when grouped
 *   q    = fmul(fsub(x, y), rl)                          x: the value the row held BEFORE this launch
 *   mh'  = (lr_r != 0) ? fmaf(omu, fsub(q, mh), mh) : mh
 *   x    = y        (mixed precision: w = y, p = bf16_rne(y))
 * mu = beta is the paper's setting.  An all-zero round is the local step plus the buffer update, NOT a
 * no-op.  lr_r == 0 (lr = 0, or a run of scale 0) leaves mh BIT FOR BIT while x is still mixed.  q amplifies
 * the rounding of x by 1 / lr; that is inherent to the algorithm in fp32.  The buffer starts as zeros.
 * Traffic: 20 bytes per element (24 with zero_grads), SGD with momentum's.
 * mx_qgm_mix_call is mx_sgd_mix_call with beta / omu in place of mom: the three tables (m_ptrs_dev, the
 * buffer's, is never NULL), the tile (mx_qgm_mix_tile: 1024 / 1024 / 512 / 256 columns, 0 above 64 rows),
 * the layout prefix, the alignment rule (16-byte accesses where x, g and mh of a (segment, row) are all
 * 16-byte aligned and the 4 elements are in range, 4-byte accesses elsewhere, for the loads and stores
 * before the round and for the reload and stores after it alike; nothing is read or written at or past
 * seg_len of a row in any array), the host-side refusals (MX_ERR_INVALID, nothing launched: n_slots !=
 * n_local, more than 64 rows, M outside [1, 32], a null table -- the buffer's included) and the launch-side
 * no-ops (a peer-reads plan record; for _at a counter outside [0, n_iters): x, g and mh are not written) are
 * mx_sgd_mix's.  _scaled and _grouped are the other families'; the record's own wd is ignored when grouped.
 * mx_qgm_mix_set / _get: "nontemporal", "wgpc", "blocks_per_cu", "flat_small", "grid", "store_policy", as
 * mx_sgd_mix_set's and independent of them, and "stage_plain" (0 / 1, default 1): 1 loads x and mh with
 * plain loads before the round where the launch streams, so that their reload after the round finds more
 * of the lines cached; 0 loads them with the streaming hint, as g.  Speed only, never bits; none of them changes the tile. */
typedef struct mx_qgm_mix_call {
    float* const* x_ptrs_dev;
    float* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, beta, omu;
    int32_t nesterov, zero_grads;
} mx_qgm_mix_call;
int mx_qgm_mix_tile(int n_slots);
int mx_qgm_mix_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_qgm_mix_set(const char* key, int value);
int mx_qgm_mix_get(const char* key);
int mx_qgm_mix(const mx_qgm_mix_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_at(const mx_qgm_mix_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                  const float* lr_dev, void* stream);
int mx_qgm_mix_scaled(const mx_qgm_mix_call* call, const float* gscale_dev, int64_t iter, float lr,
                      const float* lr_dev, void* stream);
int mx_qgm_mix_scaled_at(const mx_qgm_mix_call* call, const float* gscale_dev, const int64_t* iter_dev,
                         int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_grouped(const mx_qgm_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                       int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_grouped_at(const mx_qgm_mix_call* call, const mx_param_runs* runs, const float* gscale_dev,
                          const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, mixed-precision QG momentum fused in
 * mx_qgm_mix for models held in bfloat16 (csrc/qgm_mix_bf16.hip): the update runs on fp32 MASTER rows, the
 * master rows are what the round mixes and what the buffer's displacement is taken from, and the bfloat16
 * model row is the rounded image of its master, rewritten by every launch.  Per (segment, row) four arrays:
 *   w  float*    fp32 master, read and written in place
 *   g  uint16_t* bfloat16 gradient, read; overwritten with zeros when zero_grads != 0
 *   m  float*    the fp32 quasi-global buffer mh, read, and written after the round
 *   p  uint16_t* bfloat16 model row, WRITE ONLY: the kernel never reads it
 * Arithmetic contract: mx_qgm_mix's lines on w with g32 = f32(g) (exact widening, bits << 16), then w = y
 * and p = bf16_rne(y) of the value stored to w (ONE rounding, to nearest even; NaN stays NaN, payload
 * unspecified).  p is written for every row in every launch that runs.  Traffic: 20 bytes per element (22
 * with zero_grads), mixed-precision SGD with momentum's.  Alignment rule: a lane holds 4 elements; where w
 * and mh of a (segment, row) are 16-byte aligned, g and p are 8-byte aligned and the 4 elements are in
 * range, the accesses are wide; elsewhere they are per element (4 / 2 bytes), zero-filled past the end --
 * before and after the round alike.  The other fields, the tile, the layout prefix, the host-side refusals
 * (a null table -- the buffer's and p included) and the launch-side no-ops are mx_qgm_mix's; the knobs are
 * its own, independent of every other family's. */
typedef struct mx_qgm_mix_bf16_call {
    float* const* w_ptrs_dev;
    uint16_t* const* g_ptrs_dev;
    float* const* m_ptrs_dev;
    uint16_t* const* p_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, beta, omu;
    int32_t nesterov, zero_grads;
} mx_qgm_mix_bf16_call;
int mx_qgm_mix_bf16_tile(int n_slots);
int mx_qgm_mix_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_qgm_mix_bf16_set(const char* key, int value);
int mx_qgm_mix_bf16_get(const char* key);
int mx_qgm_mix_bf16(const mx_qgm_mix_bf16_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_bf16_at(const mx_qgm_mix_bf16_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                       const float* lr_dev, void* stream);
int mx_qgm_mix_bf16_scaled(const mx_qgm_mix_bf16_call* call, const float* gscale_dev, int64_t iter, float lr,
                           const float* lr_dev, void* stream);
int mx_qgm_mix_bf16_scaled_at(const mx_qgm_mix_bf16_call* call, const float* gscale_dev, const int64_t* iter_dev,
                              int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_bf16_grouped(const mx_qgm_mix_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                            int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_qgm_mix_bf16_grouped_at(const mx_qgm_mix_bf16_call* call, const mx_param_runs* runs,
                               const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                               const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- the hot path, gradient tracking (GT-DSGD)
 * Gradient tracking (DIGing / DSGT / GT-DSGD: Di Lorenzo & Scutari 2016; Nedic, Olshevsky & Shi 2017; Pu &
 * Nedic 2021) removes the stationary error that heterogeneous shards leave in D-PSGD at a constant learning
 * rate.  Every worker keeps a tracker y of the network's mean gradient and steps along it instead of along its
 * own gradient; the trackers are gossiped with the round's own doubly stochastic matrix, so mean_i y_i =
 * mean_i gs_i after every round of a time-varying schedule.  One iteration is TWO launches on the same plan
 * record (the same round), after the backward passes: the TRACK launch, then the STEP launch.
 *
 * Track launch (csrc/gt_track.hip; csrc/gt_track_bf16.hip for bfloat16 gradients).  Per (segment, row) three
 * arrays -- y, the fp32 tracker (the record's x table: the row the round mixes); g, the gradient (float, or
 * uint16_t bfloat16); gp, the fp32 previous gradient -- and per element, every line one IEEE fp32 rounding:
 *   gs = f32(g)                 fp32 g as it is, bf16 g widened exactly (bits << 16); multiplied by the row's
 *                               clip factor where there is one (_scaled: g' = fmul(gscale[r], f32(g)))
 *   t  = fsub(gs, gp)
 *   y' = fadd(y, t)
 *   gp = gs                     always fp32, clip factor included: the differences telescope exactly as the
 *                               tracker saw them
 *   g  = 0                      when zero_grads != 0
 *   y  = mx_sgd_mix's round on the y' values (same plan record, alpha, selfweight, ascending matchings, self
 *        term last, one fma per step; a row the record leaves alone, and every row of an all-zero round,
 *        keeps y' as it is)
 * y and gp start as zeros and there is no first-step case: y' = g falls out.  The launch has no learning rate
 * and no weight decay -- weight decay is local and sits in the step launch, so the track launch never reads the
 * weights.  The family signature is the other families': lr, lr_dev and (for _grouped) the parameter runs are
 * accepted and UNUSED (a non-NULL runs record is still checked for null tables).  Traffic: 20 bytes per element
 * (24 with zero_grads); 18 / 20 with bfloat16 gradients.  Alignment rule: wide accesses (16 bytes on y, gp and
 * fp32 g, 8 bytes on bf16 g) where the three pointers of a (segment, row) are so aligned and the 4 elements are
 * in range, per element elsewhere.  Nothing is written at or past seg_len of a row in any array.  The other
 * record fields, the tile (1024 / 1024 / 512 / 256 columns, 0 above 64 rows), the layout prefix, the host-side
 * refusals (MX_ERR_INVALID, nothing launched: n_slots != n_local, more than 64 rows, M outside [1, 32], a null
 * table, iter < 0) and the launch-side no-ops (a peer-reads plan record; for _at a counter outside
 * [0, n_iters): y, g and gp are not written) are mx_sgd_mix's.  The knobs are mx_sgd_mix_set's, each family's
 * own.  Speed only, never bits.
 *
 * Step launch: torch.optim.SGD's update with the tracker in the gradient's place,
 *   d  = (wd_r != 0) ? fmaf(wd_r, x, y) : y
 *   m  = fadd(fmul(mom, m), d);  d = nesterov ? fmaf(mom, m, d) : m      [mom != 0]
 *   x' = fmaf(-lr_r, d, x)
 *   x  = the round on the x' values;  p = bf16_rne(x) in the mixed-precision form
 * For fp32 rows it IS mx_sgd_mix (and _grouped, _at), called with a second mx_sgd_mix_call whose g_ptrs_dev is
 * the tracker's table and whose zero_grads is 0.  For bfloat16 rows over fp32 masters it is mx_gt_step_bf16
 * (csrc/gt_step_bf16.hip): mx_sgd_mix_bf16 with a float g table (the tracker, 16-byte accesses).  Its record is
 * mx_sgd_mix_bf16_call with that one type changed; zero_grads != 0 is refused (the launch never writes y), and
 * so is a non-NULL gscale_dev (the clip factor entered the tracker in the track launch).  Traffic: 22 bytes per
 * element with momentum, 14 without (fp32: mx_sgd_mix's 20 / 12). */
typedef struct mx_gt_track_call {
    float* const* x_ptrs_dev;              /* the tracker y */
    float* const* g_ptrs_dev;
    float* const* gp_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha;
    int32_t zero_grads;
} mx_gt_track_call;
int mx_gt_track_tile(int n_slots);
int mx_gt_track_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_gt_track_set(const char* key, int value);
int mx_gt_track_get(const char* key);
int mx_gt_track(const mx_gt_track_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_track_at(const mx_gt_track_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                   const float* lr_dev, void* stream);
int mx_gt_track_scaled(const mx_gt_track_call* call, const float* gscale_dev, int64_t iter, float lr,
                       const float* lr_dev, void* stream);
int mx_gt_track_scaled_at(const mx_gt_track_call* call, const float* gscale_dev, const int64_t* iter_dev,
                          int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_gt_track_grouped(const mx_gt_track_call* call, const mx_param_runs* runs, const float* gscale_dev,
                        int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_track_grouped_at(const mx_gt_track_call* call, const mx_param_runs* runs, const float* gscale_dev,
                           const int64_t* iter_dev, int64_t n_iters, float lr, const float* lr_dev, void* stream);

typedef struct mx_gt_track_bf16_call {
    float* const* x_ptrs_dev;              /* the tracker y */
    uint16_t* const* g_ptrs_dev;
    float* const* gp_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha;
    int32_t zero_grads;
} mx_gt_track_bf16_call;
int mx_gt_track_bf16_tile(int n_slots);
int mx_gt_track_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_gt_track_bf16_set(const char* key, int value);
int mx_gt_track_bf16_get(const char* key);
int mx_gt_track_bf16(const mx_gt_track_bf16_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_track_bf16_at(const mx_gt_track_bf16_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                        const float* lr_dev, void* stream);
int mx_gt_track_bf16_scaled(const mx_gt_track_bf16_call* call, const float* gscale_dev, int64_t iter, float lr,
                            const float* lr_dev, void* stream);
int mx_gt_track_bf16_scaled_at(const mx_gt_track_bf16_call* call, const float* gscale_dev, const int64_t* iter_dev,
                               int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_gt_track_bf16_grouped(const mx_gt_track_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                             int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_track_bf16_grouped_at(const mx_gt_track_bf16_call* call, const mx_param_runs* runs,
                                const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                                const float* lr_dev, void* stream);

typedef struct mx_gt_step_bf16_call {
    float* const* w_ptrs_dev;
    float* const* g_ptrs_dev;              /* the tracker y: read only */
    float* const* m_ptrs_dev;
    uint16_t* const* p_ptrs_dev;
    const int64_t* seg_len_dev;
    const int64_t* tile_off_dev;
    const int32_t* plan_dev;
    int64_t total_tiles;
    int32_t nseg, n_slots, n_local, M;
    float alpha, wd, mom;
    int32_t nesterov, zero_grads, pad_;    /* zero_grads must be 0 */
} mx_gt_step_bf16_call;
int mx_gt_step_bf16_tile(int n_slots);
int mx_gt_step_bf16_layout(const int64_t* seg_len_host, int nseg, int n_slots, int64_t* tile_off_host);
int mx_gt_step_bf16_set(const char* key, int value);
int mx_gt_step_bf16_get(const char* key);
int mx_gt_step_bf16(const mx_gt_step_bf16_call* call, int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_step_bf16_at(const mx_gt_step_bf16_call* call, const int64_t* iter_dev, int64_t n_iters, float lr,
                       const float* lr_dev, void* stream);
int mx_gt_step_bf16_scaled(const mx_gt_step_bf16_call* call, const float* gscale_dev, int64_t iter, float lr,
                           const float* lr_dev, void* stream);
int mx_gt_step_bf16_scaled_at(const mx_gt_step_bf16_call* call, const float* gscale_dev, const int64_t* iter_dev,
                              int64_t n_iters, float lr, const float* lr_dev, void* stream);
int mx_gt_step_bf16_grouped(const mx_gt_step_bf16_call* call, const mx_param_runs* runs, const float* gscale_dev,
                            int64_t iter, float lr, const float* lr_dev, void* stream);
int mx_gt_step_bf16_grouped_at(const mx_gt_step_bf16_call* call, const mx_param_runs* runs,
                               const float* gscale_dev, const int64_t* iter_dev, int64_t n_iters, float lr,
                               const float* lr_dev, void* stream);

/* ---------------------------------------------------------------- flatten / unflatten
 * mx_gather replaces flatten_tensors (comm_helpers.py:12-30): flat[off[s] + i] = src[s][i].
 * mx_scatter is the copy_ loop of reset_model over unflatten_tensors views
 * (communicator.py:124-131, comm_helpers.py:33-56): dst[s][i] = flat[off[s] + i].
 *   ptrs_dev  float* [nseg] device;  off_dev int64 [nseg+1] device (off[nseg] = total)
 */
int mx_gather(const float* const* ptrs_dev, const int64_t* off_dev, int nseg, int64_t total,
              float* flat, void* stream);
int mx_scatter(float* const* ptrs_dev, const int64_t* off_dev, int nseg, int64_t total,
               const float* flat, void* stream);

/* ---------------------------------------------------------------- ChocoSGD (compressors.py)
 * mx_topk_abs_diff: q = topk(|x - x_hat|, k) of compressors.get_top_k (compressors.py:3-19)
 * applied to the send buffer of ChocoCommunicator.prepare_comm_buffer (communicator.py:188-190).
 * Writes vals[k] = (x - x_hat)[idx] and idx[k] (int64) sorted by index.  Among equal
 * magnitudes at the k-th threshold the lowest indices are taken (torch.topk(sorted=False)
 * leaves that unspecified).  x_hat may be NULL (treated as zeros: get_top_k on x itself).
 * `work` is a 256-byte aligned device scratch of mx_topk_work_bytes(P) bytes, ZERO-FILLED before
 * its first use (hipMemset); every call leaves its histograms and counters zero again, so no
 * zeroing launch runs per call.  One scratch may serve calls of any P.
 * One full pass over x / x_hat: a sampled top-digit histogram picks a candidate floor, one
 * streaming pass keeps the keys above it, and the exact radix select runs on those only (a
 * too-high floor is detected on the device and the pass re-run keeping every key: the result
 * is exact in every case).
 */
size_t mx_topk_work_bytes(int64_t P);
/* Top-k knobs: "sample_stride" = sample every S-th 1024-element chunk for the candidate floor
 * (0 = auto, about 2^18 sampled elements per row; 1 = exact full histogram, no sampling);
 * "compact_blocks" = persistent workgroups of the full pass, over all rows (0 = auto: 640 for
 * one row, 2560 for several);
 * "sample_pieces" = sampled 1024-element pieces per wave of the sampling pass (default 1);
 * "cand_chunks" = candidate regions per wave of the candidate-histogram / mark passes (0 = auto:
 * 4 for one row, 8 for several);
 * "compact_store" = 1 (default): candidate stores looped over each lane's kept elements, 0: one
 * masked store pair per element;
 * "apply_nt" = mx_choco_apply's access hints: -1 (default) non-temporal with several rows only,
 * 0 / 1 forced;
 * "apply_pf" = 1 (default): mx_choco_apply prefetches every message's tile bounds and first entries
 * under the tile stream, 0: the plain kernel (bounds and entries loaded per message);
 * "apply_persist" = -1 (default): the slot-table apply (mx_choco_apply_slots) of ONE row runs
 * persistent workgroups that acquire and load the message addresses once each, every other apply
 * a workgroup per tile; 0 / 1: one form for all;
 * "select" = 0 (default): the selection after the compaction as four passes (candidate histograms
 * of the 10 and 9 low digits, threshold mark, placement), 1: as ONE launch (select_kernel: B
 * workgroups of 1024 threads per row meeting at two row barriers; measured slower);
 * "fine_floor" = 1 (default): the sampled floor refined to 1/64 of a top digit (key bits 13..18)
 * when it falls in a 4-digit window around the previous call's floor digit on the same scratch (the
 * sampling pass histograms that window's sub-bins too): ~1.35 k candidates instead of 1.5-4 k;
 * 0: the floor is a whole top digit;
 * "floor_hint" = -1 (default): the compaction's candidate floor from a sampled histogram (one
 * sampling launch per call); m >= 0: from the PREVIOUS call's exact k-th key on the same scratch,
 * lowered by an adaptive per-row margin starting at m 12-bit bins (1 bin = 1/16 octave), and no
 * sampling launch -- the first call on a scratch keeps every key; a floor too high re-runs the
 * compaction keeping every key (the fallback), so results never change;
 * "select_blocks" = select_kernel workgroups per row (0 = auto: the fewest whose LDS caches every
 * candidate region, at most 32); "select_trace" = 1: select_kernel stores stage clocks in the
 * scratch (diagnostic, tools/select_trace.py).
 * Knobs tune speed only, never results -- except the test knob "spin_ticks": the bounded row-barrier
 * waits' deadline in 100 MHz ticks (default 2^28, ~2.7 s); 0 makes every wait that has to wait
 * expire, so tests can drive the error path below on purpose.  "spin_ticks" and "compact_trace"
 * live on the device: they apply to the CURRENT device only (set them per device in a process
 * driving several), and mx_topk_get reports the current device's value; every other knob is host-side.
 * mx_topk_get also reads "hist_grid" (the last call's first-candidate-pass grid per row) and
 * "hist_capacity" (the co-resident block cap that grid was held to with sampling on, 0 without). */
int mx_topk_set(const char* key, int64_t value);
int64_t mx_topk_get(const char* key);
/* The rows' sticky error words: a row barrier (the sampled-floor fallback of the first candidate
 * pass, or select_kernel) whose BOUNDED wait expired -- its blocks were not all resident -- leaves
 * that call's output undefined instead of hanging the GPU.  Synchronises `stream`, reads and clears
 * the words; MX_ERR_HIP if any was set.  (work, work_ld_bytes, nrows, P) as in the call checked. */
int mx_topk_check(void* work, int64_t work_ld_bytes, int nrows, int64_t P, void* stream);
/* The same scan, stream-ordered and NON-blocking: the words are read and cleared on `stream` behind
 * the call they belong to, and an expired one sets *flag_dev = first row + 1 with a system-scope
 * release (flag_dev: mx_host_words -- the host polls it without synchronising).  compressors.get_top_k
 * on GPU tensors enqueues it after every call and raises at the next call, or at check_top_k(). */
int mx_topk_err_forward(void* work, int64_t work_ld_bytes, int nrows, int64_t P, int32_t* flag_dev, void* stream);
/* Diagnostics of the candidate floor, per row r: out[5r] = calls made on this scratch, out[5r+1] =
 * how many of them ran the fallback compaction (floor above the k-th key), out[5r+2] = the row's
 * current floor_hint margin (bins), out[5r+3] = the last call's threshold key (bits of |k-th value|),
 * out[5r+4] = its candidate count.  Synchronises `stream`. */
int mx_topk_stats(const void* work, int64_t work_ld_bytes, int nrows, int64_t P, int64_t* out, void* stream);
/* Diagnostic: with mx_topk_set("compact_trace", 1), every workgroup of row 0's candidate compaction
 * stamps the 100 MHz constant clock at its start, once its floor is resolved, and at its end;
 * out[3b .. 3b+2] = workgroup b's stamps of the last launch (nblocks <= 8192).  Synchronises the
 * device.  tools/compact_trace.py reads it (ramp vs tail of the one-row compaction). */
int mx_topk_trace(uint64_t* out, int64_t nblocks);
int mx_topk_abs_diff(const float* x, const float* x_hat, int64_t P, int64_t k, float* vals,
                     int64_t* idx, void* work, void* stream);
/* Batched form (one set of launches for every local worker): row r reads x + r*ld (and
 * x_hat + r*ld), writes its values at out + r*out_ld_bytes and its int64 indices at
 * out + r*out_ld_bytes + idx_off_bytes, and uses work + r*work_ld_bytes
 * (work_ld_bytes >= mx_topk_work_bytes(P)).  bnd_off_bytes >= 0: also writes the message's
 * int32 tile bounds there (bnd[t] = first output entry with index >= 4096 t, t = 0..ceil(P/4096);
 * the layout mx_choco_apply reads); < 0: not written. */
int mx_topk_abs_diff_rows(const float* x, const float* x_hat, int64_t ld, int nrows, int64_t P,
                          int64_t k, void* out, int64_t out_ld_bytes, int64_t idx_off_bytes,
                          int64_t bnd_off_bytes, void* work, int64_t work_ld_bytes, void* stream);

/* ChocoCommunicator.averaging (communicator.py:200-230) for one round of n_local workers,
 * in place on the state rows (a round whose flags are all zero must not be applied):
 *   for each partner j of row r (ascending matching): s_r[idx_j] = s_r[idx_j] + f32(alpha)*v_j
 *   s_r[idx_r] += f32(1-d*alpha) * v_r ; x_hat_r[idx_r] += v_r
 *   x_r = fma(gamma, s_r, x_r) ; x_r = fma(-gamma, x_hat_r, x_r)
 *   x/xhat/s  float [n_local][P] rows with stride ld (floats)
 *   msgs      compressed messages, one per plan slot, msg_ld_bytes apart: a slot holds
 *             vals float[k] at +0, idx int64[k] at +4*round_up(k, 2) and the tile bounds int32
 *             [ceil(P/4096) + 1] right after the indices (mx_choco_msg_bytes(P, k) bytes, written
 *             by mx_topk_abs_diff_rows with bnd_off_bytes = 4*round_up(k, 2) + 8*k); slots
 *             [0, n_local) are the local rows' own messages, the rest received ones
 *   work      unused (the tile bounds travel in the messages); may be NULL
 * One fused pass: per 4096-element tile of a row, s and x_hat are staged in LDS, every message
 * entry in the tile is applied there in the order above, x is updated, and only the touched
 * 64-byte granules of s / x_hat are written back.
 */
int64_t mx_choco_msg_bytes(int64_t P, int64_t k);
/* Scratch of mx_choco_apply: 0 bytes (kept for ABI stability). */
size_t mx_choco_apply_work_bytes(int64_t P, int n_slots);
int mx_choco_apply(float* x, float* xhat, float* s, int64_t ld, int64_t P, int64_t k,
                   const void* msgs, int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev,
                   int64_t iter, int n_local, int M, float alpha, float gamma, void* work,
                   void* stream);
/* Graph-replayable form (as mx_gossip_mix_at): the round is *iter_dev, read on the device; a
 * round outside [0, n_iters) or with no active matching leaves x, x_hat and s untouched. */
int mx_choco_apply_at(float* x, float* x_hat, float* s, int64_t ld, int64_t P, int64_t k, const void* msgs,
                      int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, const int64_t* iter_dev,
                      int64_t n_iters, int n_local, int M, float alpha, float gamma, void* work, void* stream);
/* The pull transport's form (ChocoWorkerGroup under PullTransport; replaces the sendrecv of the
 * compressed messages, communicator.py:214, with loads from the owners' HBM): message `slot` is
 * read at the device address slot_ptrs_dev[slot] (int64 [n_slots]) -- the local rows' messages in
 * this GPU's buffer, the partners' in their owners' IPC-mapped snapshot buffers (mx_snapshot_publish
 * of the message slots, then mx_pull_gate with ld_bytes = the message stride points the remote
 * slots there).  A plan record with the peer-reads bit (mx_plan_set_peer_reads) makes every
 * workgroup acquire at system scope before its first message load.  Same bits as mx_choco_apply. */
int mx_choco_apply_slots(float* x, float* xhat, float* s, int64_t ld, int64_t P, int64_t k,
                         const int64_t* slot_ptrs_dev, int n_slots, const int32_t* plan_dev, int64_t iter,
                         int n_local, int M, float alpha, float gamma, void* stream);

/* ---------------------------------------------------------------- ChocoSGD, scaled-sign compressor
 * The 1-bit quantizer Q(v) = (|v|_1 / P) sign(v) in place of compressors.get_top_k in
 * ChocoCommunicator.prepare_comm_buffer (communicator.py:175-196) and averaging (communicator.py:200-230).
 * For a row with d = x - x_hat (one fp32 subtraction; x_hat NULL: d = x):
 *   L = sum_c f64(|d[c]|) (fp64, any order);  scale = f32(L / f64(P));  bit c = d[c] < 0 (false for +0, -0
 *   and NaN: a zero difference travels as +scale);  q[c] = bit c ? -scale : +scale.
 * A message slot holds mx_choco_sign_msg_bytes(P) = 64 + 8 ceil(P/64) bytes (communicator.py:175-230: the
 * send buffer): float32 scale at 0, float64 L at 8 (diagnostic), int64 P at 16, zeros up to 64, then the
 * bits -- column c is bit c & 7 of byte c >> 3, padding bits past P zero.  -1 for P < 1. */
int64_t mx_choco_sign_msg_bytes(int64_t P);
/* Scratch of mx_choco_sign_compress (communicator.py:175-230; one fp64 partial per 4096 columns of a row);
 * 0 with mx_last_error for P < 1 or nrows < 1.  It needs no zero-fill. */
size_t mx_choco_sign_work_bytes(int64_t P, int nrows);
/* prepare_comm_buffer (communicator.py:175-230) of `nrows` rows: row r reads x + r*ld (and x_hat + r*ld;
 * x_hat may be NULL), writes its message at msgs + r*msg_ld_bytes (8-byte aligned, msg_ld_bytes a multiple of
 * 8 and >= mx_choco_sign_msg_bytes(P); ignored for one row).  Two launches, no atomics: scale depends on the
 * row's values and P alone -- the same bits for any row count, grid or knob -- and is within 1 fp32 ulp of the
 * correctly rounded value for P <= 2^26. */
int mx_choco_sign_compress(const float* x, const float* x_hat, int64_t ld, int nrows, int64_t P, void* msgs,
                           int64_t msg_ld_bytes, void* work, void* stream);
/* averaging (communicator.py:175-230) for one round of n_local workers on scaled-sign messages, in place:
 *   for each partner j of row r (ascending matching): s_r = s_r + f32(alpha) * q_j
 *   s_r += (self weight of the plan record) * q_r ; x_hat_r += q_r
 *   x_r = fma(gamma, s_r, x_r) ; x_r = fma(-gamma, x_hat_r, x_r)
 * msgs: one slot per plan slot, msg_ld_bytes apart; slots [0, n_local) are the local rows' own messages.
 * One elementwise launch; of a message's header only `scale` is read. */
int mx_choco_sign_apply(float* x, float* xhat, float* s, int64_t ld, int64_t P, const void* msgs,
                        int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, int64_t iter, int n_local,
                        int M, float alpha, float gamma, void* stream);
/* Graph-replayable form (communicator.py:175-230; the no-op rules of mx_choco_apply_at): the round is
 * *iter_dev; one outside [0, n_iters) or with no active matching leaves x, x_hat and s untouched. */
int mx_choco_sign_apply_at(float* x, float* xhat, float* s, int64_t ld, int64_t P, const void* msgs,
                           int64_t msg_ld_bytes, int n_slots, const int32_t* plan_dev, const int64_t* iter_dev,
                           int64_t n_iters, int n_local, int M, float alpha, float gamma, void* stream);
/* Knobs of the scaled-sign passes (communicator.py:175-230 has none; speed only, never results):
 * "apply_nt" = mx_choco_sign_apply's access hints: -1 (default) non-temporal with several rows only, 0 / 1
 * forced; "blocks_per_cu" = workgroups per CU of the compress pass's persistent grid (default 8, 1..64);
 * "grid" = its exact grid size (0 = from blocks_per_cu; up to 65536). */
int mx_choco_sign_set(const char* key, int value);
int mx_choco_sign_get(const char* key);

/* ---------------------------------------------------------------- cross-GPU exchange (RCCL)
 * One process per GPU; workers partitioned by owner[].  mx_exchange_round posts, inside one
 * ncclGroupStart/End, an ncclSend of every local row whose active partner lives on another
 * rank (once per destination rank) and an ncclRecv of every distinct remote partner row into
 * the receive slab -- the pairwise comm.sendrecv of decenCommunicator.averaging
 * (communicator.py:110) over xGMI, with each row crossing a link at most once per round.
 * Order: first appearance over (matching ascending, sender worker id ascending); slab slot k
 * is the k-th distinct remote worker in that order (matches mx_plan_build).
 *   flags_row  uint8 [M] host;  partner int32 [M][n_global] host;  owner int32 [n_global] host
 *   rows       device float* [n_local] (host array of device pointers), P floats each
 *   slab       device base; slot k at slab + k * slab_ld
 *   elem_bytes 4 for fp32 rows; also used with 12-byte Choco messages (values + int64 idx)
 */
int mx_rccl_unique_id(void* id_out /* 128 bytes */);
int mx_rccl_init(const void* id /* 128 bytes */, int nranks, int rank, void** comm_out);
/* The communicator is NON-blocking (ncclConfig_t.blocking = 0) and every RCCL call the library
 * makes on it waits for its enqueue against a deadline: a peer rank that never joins (dead, or
 * skipped the call) turns into MX_ERR_RCCL "timed out" instead of a hang.  mx_rccl_init uses
 * $MX_RCCL_TIMEOUT_S (default 300 s); mx_rccl_init_timeout takes it explicitly (the deadline then
 * applies to the init and to every later operation of the process).  An init that times out is
 * aborted before returning; *nonblocking_out (optional) = 1.  Replaces the mpi4py COMM_WORLD set
 * up at train_mpi.py:237-239. */
int mx_rccl_init_timeout(const void* id, int nranks, int rank, int64_t timeout_ms, void** comm_out,
                         int* nonblocking_out);
/* ncclCommAbort: release a communicator whose peers are gone (after a timed-out operation). */
int mx_rccl_abort(void* comm);
/* ncclCommFinalize (waited for with the deadline; aborted on expiry) + ncclCommDestroy. */
int mx_rccl_destroy(void* comm);
/* ncclCommCount: the ranks the communicator holds (the bench line's rccl_ranks). */
int mx_rccl_count(void* comm, int* nranks_out);
/* The deadlines above bound getting an operation enqueued (init, a group's connection setup).
 * A peer that dies or skips an exchange after the connections exist leaves the RCCL kernel
 * waiting on the GPU; mx_rccl_wait is the stream synchronisation with a deadline: an event behind
 * everything enqueued on `stream`, polled until it completes or timeout_ms (<= 0: the init's
 * deadline) passes -- then the communicator is ABORTED (its kernels exit, the stream drains; do not
 * use it again) and MX_ERR_RCCL "timed out" is returned.  Replaces the blocking barriers that
 * bracket averaging (communicator.py:94,119). */
int mx_rccl_wait(void* comm, void* stream, int64_t timeout_ms);
/* The ordered operations mx_exchange_round posts for this rank, host only (no GPU, no RCCL):
 * ops[4i..4i+3] = {kind (0 send / 1 recv), peer rank, local row (send) or slab slot (recv),
 * global id of the worker whose row travels}.  ops == NULL: count only. */
int mx_exchange_plan(const uint8_t* flags_row, int M, const int32_t* partner, int n_global,
                     const int32_t* owner, int my_rank, int row_base, int n_local, int32_t* ops,
                     int cap, int* n_ops);
/* Posts an explicit operation list (mx_exchange_plan's layout) inside one ncclGroupStart/End:
 * kind 0 = ncclSend of rows[op[2]] to op[1], kind 1 = ncclRecv from op[1] into slab slot op[2];
 * row_bytes per operation.  Sends to / receives from one peer pair up in list order.  Every op is
 * validated before anything is posted.  mx_exchange_round = mx_exchange_plan + this. */
int mx_exchange_post(void* comm, const int32_t* ops, int n_ops, void* const* rows, int n_rows, void* slab,
                     int64_t slab_ld_bytes, int64_t row_bytes, void* stream);
int mx_exchange_round(void* comm, const uint8_t* flags_row, int M, const int32_t* partner,
                      int n_global, const int32_t* owner, int my_rank, int row_base, int n_local,
                      void* const* rows, void* slab, int64_t slab_ld_bytes, int64_t row_bytes,
                      int* n_remote_out, void* stream);
/* Pull transport (one process per GPU of a node): device buffers shared through IPC handles
 * (64 bytes, mx_ipc_handle_bytes).  A rank publishes snapshots of its rows in an mx_ipc_alloc
 * buffer and sends the handle to its peers (any host channel); a peer mx_ipc_open's it and the
 * mixing kernel reads the partner rows straight from the owner's HBM over xGMI, in place of
 * comm.sendrecv (communicator.py:110).  mx_ipc_close unmaps a peer buffer, mx_ipc_free releases
 * one's own. */
/* Snapshot of this GPU's rows for its peers: dst[i] = src[i] (n floats, n % 4 == 0, 16-byte
 * aligned), and every workgroup ends with a system-scope release (its stores written back past
 * this GPU's L2 to HBM), so a peer's load over xGMI after the round's barrier sees them. */
int mx_snapshot_publish(const float* src, float* dst, int64_t n, void* stream);
/* The same copy for only the rows a peer reads this round: local row r
 * (0 <= r < n_local, worker row_base + r) is copied -- src + r * src_ld -> dst + r * dst_ld, n floats
 * (multiple of 4, all 16-byte aligned), then the system-scope release -- iff some matching g with
 * flags_row_dev[g] != 0 pairs it with a worker outside [row_base, row_base + n_local) (partner_dev
 * int32 [M][n_global]: the set mx_pull_gate's peers point their slots at); other rows are not
 * touched.  One launch, n_local rows of workgroups; the row test runs on the device. */
int mx_snapshot_publish_rows(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int64_t n, int n_local,
                             const uint8_t* flags_row_dev, int M, const int32_t* partner_dev, int n_global,
                             int row_base, void* stream);
/* Plan word [2] bit 1: the receive slots of these records point at peer GPUs' IPC-mapped memory;
 * the mixing kernels then start with a system-scope acquire per workgroup (buffer_inv sc0 sc1: no
 * line of a peer's buffer cached on this GPU from an earlier round is served).  on = 1 / 0. */
int mx_plan_set_peer_reads(int32_t* plan_dev, int64_t T, int n_local, int M, int on, void* stream);
/* A rank's snapshot buffer (mx_ipc_alloc, zero-filled): MX_PULL_HEADER_BYTES of header -- its
 * uint64 epoch at offset 0 -- then snapshot 0 and snapshot 1, each n_local rows of ld_bytes. */
#define MX_PULL_HEADER_BYTES 256
typedef struct mx_pull_rank {
    int64_t base;      /* the rank's snapshot buffer as mapped in THIS process (own: the allocation) */
    int32_t row_base;  /* its block of workers [row_base, row_base + n_local) */
    int32_t n_local;
} mx_pull_rank;
/* The pull round's handshake, one single-wave kernel on `stream` between mx_snapshot_publish (into
 * snapshot `parity`) and the mixing launch -- replaces the host synchronize + barrier + pointer-table
 * copy per round (and the reference's sendrecv pairing, communicator.py:99-112):
 *   1. epoch[my_rank] = epoch (system-scope release; the snapshot is complete by stream order);
 *   2. bounded wait for epoch[r] >= epoch of every rank r owning an active remote partner of a
 *      local worker under flags_row_dev (this round) or prev_row_dev (the previous pull round);
 *   3. slot_ptrs_dev[n_local + j] = the j-th distinct remote partner's row in its owner's snapshot
 *      `parity` (plan_kernel's slot numbering); prev_row_dev = flags_row_dev afterwards.
 * ranks_dev: mx_pull_rank[nranks] (device).  On expiry after timeout_s: err_dev[0] = 1, [1] = the
 * rank that did not publish, [2] = the epoch awaited, [3] = the last one seen (err_dev: mx_host_words,
 * read by the host once the stream has passed the gate); err_dev[0] = 2: more remote partners than
 * slots.  1 <= n_global <= 4096, nranks <= 64, epochs start at 1 and rise by one per pull round. */
int mx_pull_gate(const uint8_t* flags_row_dev, uint8_t* prev_row_dev, int M, const int32_t* partner_dev,
                 int n_global, const int32_t* owner_dev, const mx_pull_rank* ranks_dev, int nranks, int my_rank,
                 int row_base, int n_local, int64_t ld_bytes, int parity, uint64_t epoch, int64_t* slot_ptrs_dev,
                 int n_slots, double timeout_s, int32_t* err_dev, void* stream);
/* The pull round's fetch of small payloads (ChocoWorkerGroup: the partners' compressed messages,
 * in place of the sendrecv of communicator.py:214), on `stream` after mx_pull_gate: for every remote
 * slot j below the round's remote count (word [1] of plan_rec_dev, the round's plan record), the
 * first nbytes (rounded up to 16) at slot_ptrs_dev[n_local + j] -- a peer's snapshot row -- are
 * copied to dst + j * dst_ld (dst_ld >= that, 16-byte aligned).  Every workgroup acquires at system
 * scope first.  Grid: up to 64 workgroups per slot times max_remote slots. */
int mx_pull_fetch(const int64_t* slot_ptrs_dev, int n_local, int max_remote, const int32_t* plan_rec_dev, void* dst,
                  int64_t dst_ld, int64_t nbytes, void* stream);
/* n zeroed int32 words of coherent mapped host memory: *host_out for the host, *dev_out for kernels. */
int mx_host_words(int n, int32_t** host_out, int32_t** dev_out);
int mx_host_words_free(int32_t* host);
int mx_ipc_handle_bytes(void);
/* A zero-filled device buffer of at least `bytes` whose IPC handle is exported: the size is rounded up
 * to the export granule (default 2 MiB).  hipIpcGetMemHandle refuses ("invalid argument") a block
 * that lands on the address range of an IPC import this process has just closed
 * (tools/ipc_reuse_probe.py); such a block is kept while a second one -- necessarily elsewhere -- is
 * allocated and exported, then freed (knob "hold", default 1; counted as "recovered").  A block that
 * still cannot be exported is logged to stderr, counted (mx_ipc_stats) and returned as MX_ERR_HIP. */
int mx_ipc_alloc(int64_t bytes, void** ptr_out, void* handle_out);
/* Export accounting, process-wide since load: hipIpcGetMemHandle calls, and mx_ipc_alloc calls that
 * returned no exported block (engine.PullTransport reads them: the bench line's ipc_refused, the
 * multi-process tests' zero checks). */
int mx_ipc_stats(int* exports, int* refused);
/* mx_ipc_alloc's knobs: "granule" (bytes, 1 = unrounded .. 1 GiB), "hold" (1 / 0: recover a refused
 * block with a second one); mx_ipc_get returns them, and "recovered" (refused first blocks whose
 * second block exported); -1 for an unknown key.  Test hooks of tests/test_gpu_round6.py and the
 * refusal probe. */
int mx_ipc_set(const char* key, int64_t value);
int64_t mx_ipc_get(const char* key);
int mx_ipc_open(const void* handle, void** ptr_out);
int mx_ipc_close(void* ptr);
int mx_ipc_free(void* ptr);

/* centralizedCommunicator.averaging (communicator.py:56-67): buf = allreduce_sum(buf) / size.
 * mx_allreduce_mean: RCCL's all-reduce (ring / tree order of RCCL's choosing), then the division;
 *   equal to the reference within fp32 reassociation (1e-6 relative for well-conditioned sums).
 * mx_allreduce_mean_ordered: bit-identical to the reference -- every rank's buffer is
 *   all-gathered into `gather` (float[nranks][count], device) and each rank sums the rows in the
 *   reference's order (mx_mean_rows) and divides by nranks.  order 0: the binomial tree of
 *   mpi4py's object all-reduce (rc.fast_reduce, its default); 1: rank order (fast_reduce off). */
int mx_allreduce_mean(void* comm, float* buf, int64_t count, int nranks, void* stream);
int mx_allreduce_mean_ordered(void* comm, float* buf, int64_t count, float* gather, int order, void* stream);
/* ncclAllGather of `count` floats per rank into gather[nranks][count] (rank order). */
int mx_allgather(void* comm, const float* send, int64_t count, float* gather, void* stream);
/* out[i] = (rows[0][i] + ... + rows[nrows-1][i] in the given order) / nrows for i < count; rows
 * are nrows x ld floats (device), 1 <= nrows <= 2^24 (the tree order for any count: a binary counter
 * of partial sums); out may be rows[0].  The division step of
 * the centralized communicator (communicator.py:61-62) and of sync_allreduce (train_mpi.py:46-55),
 * callable after any transport's gather.  = mx_mean_rows_to with ndst = 1. */
int mx_mean_rows(const float* rows, int nrows, int64_t ld, int64_t count, int order, float* out, void* stream);
/* The same mean (same order, same rounding) written to ndst rows dst + d * dst_ld (d < ndst) in one
 * pass: centralizedCommunicator's all-reduce (communicator.py:56-67) / sync_allreduce (train_mpi.py:
 * 34-56) for workers held as rows of one arena -- dst == rows (dst_ld == ld) rewrites every worker's
 * row with the mean in place (each column of every row is read before that column is written);
 * after an mx_allgather, dst = this rank's own rows.  16-byte accesses when everything is 16-byte
 * aligned and the order is the <= 8-row tree or rank order; up to 8 rows in 512-column tiles
 * staged in LDS.  A dst that overlaps the rows other than at whole-row offsets (offset and dst_ld
 * multiples of ld) is refused (MX_ERR_INVALID). */
int mx_mean_rows_to(const float* rows, int nrows, int64_t ld, int64_t count, int order, float* dst, int ndst,
                    int64_t dst_ld, void* stream);
/* The kernel that carries the bulk of mx_mean_rows_to with the same arguments (static string, e.g.
 * "mean_tile_kernel<1>"; the same dispatch, alignment included; nothing launched), for reports. */
const char* mx_mean_kernel_name(const float* rows, int nrows, int64_t ld, int64_t count, int order, const float* dst,
                                int ndst, int64_t dst_ld);

/* ---------------------------------------------------------------- SlowMo outer step
 * SlowMo (Wang, Tantia, Ballas, Rabbat, ICLR 2020) for workers held as rows of one arena
 * (csrc/slowmo.hip): every tau iterations of any base optimizer, the exact average of the n = n_local
 * rows, a slow momentum on the averaged displacement and the broadcast of the new common point, in ONE
 * streaming pass over the rows.  State per group: a, the anchor (the common point of the last outer
 * step), and u, the slow momentum (zeros at the start), fp32 [count] each.  Per column, every line one
 * fp32 rounding (no contraction; the fmas are explicit):
 *   s    = the sum of the n rows' values in mx_mean_rows' order (order 0: binomial tree, 1: rank order)
 *   mean = fdiv(s, (float)n)                     the bits mx_mean_rows_to gives for the same rows and order
 *   rl   = fdiv(1, lr);  al = fmul(alpha, lr)    once per launch
 *   q    = fmul(fsub(a, mean), rl)
 *   u'   = fmaf(beta, u, q)
 *   a'   = fmaf(-al, u', a)
 *   every row x_r = a';  a = a';  u = u'
 *   mixed precision (p non-NULL): the rows are the fp32 masters and every p_r = bf16_rne(a') -- p is the
 *   bfloat16 model arena, write only, rounded once to nearest even; NaN stays NaN
 * lr is the argument or, when lr_dev is non-NULL, the float it points to on the device, read when the
 * kernel runs; a learning rate of exactly 0 read there makes the launch a complete no-op (rl would be
 * Inf).  A NaN or Inf in one row's column reaches a', u' and every row of that column and no other.
 * Every lane reads its columns of all n rows, a and u before it writes anything in them: the step is in
 * place.  Nothing is read or written at or past `count` in any array.
 * Known limitation: for n that is not a power of two the pinned-order mean of n identical values can
 * differ from the value in the last place (12-20 % of random fp32 values for n = 3, 5, 6, 7, 12; none
 * for 2, 8, 16 in the tree order; in rank order the partial sums 3 x, 5 x, ... round for every n > 2), so a
 * synced state is not an exact fixed point there.
 * mx_slowmo_call, built once and kept alive by the caller (sizeof == 72):
 *   rows       n_local rows of ld floats (device); count <= ld columns are used
 *   a, u       float [count] (device); they may not overlap the rows, p or each other
 *   p          NULL (an fp32 group) or the bfloat16 arena, n_local rows of p_ld elements
 *   order      0 or 1, as mx_mean_rows
 *   alpha      the slow learning rate, finite and > 0;  beta  the slow momentum factor, in [0, 1)
 * mx_slowmo_step(call, lr, lr_dev, stream) enqueues one launch, with no host synchronisation and no host
 * read, so it can be captured in a graph.  16-byte accesses on rows, a and u and 8-byte stores on p
 * where every pointer is aligned that far, ld % 4 == 0 (and p_ld % 4 == 0) and the chunk is in range,
 * per element for the last count % 4 columns and for unaligned tables.  Up to 8 rows go through
 * 512-column tiles staged in LDS (mx_mean_rows_to's geometry); 9..64 rows are held per lane, 16 bytes
 * a lane up to 16 rows, 8 up to 32, 4 up to 64.  The bits depend on none of this.
 * MX_ERR_INVALID, nothing launched: a null record, rows, a or u; n_local outside [1, 64]; ld < count
 * (p_ld < count); order not 0 or 1; a or u overlapping the rows, p or each other; alpha not finite and
 * positive; beta outside [0, 1); lr not finite and positive when lr_dev is NULL.
 * mx_slowmo_set / _get: "store_policy" (the 16-byte stores: 1 = nt, the default; 3 = sc1 nt, see
 * mx_mix_set), "wgpc" (the tile kernel's workgroups per CU on rounds of more than 64 MB of rows,
 * default 3, 0 = no cap).  mx_slowmo_kernel_name: the kernel mx_slowmo_step launches for the record
 * (static string, "invalid" for a record it refuses; nothing launched), for reports. */
typedef struct mx_slowmo_call {
    float* rows;
    float* a;
    float* u;
    void* p;
    int64_t ld, p_ld, count;
    int32_t n_local, order;
    float alpha, beta;
} mx_slowmo_call;
int mx_slowmo_step(const mx_slowmo_call* call, float lr, const float* lr_dev, void* stream);
int mx_slowmo_set(const char* key, int value);
int mx_slowmo_get(const char* key);
const char* mx_slowmo_kernel_name(const mx_slowmo_call* call);

/* ---------------------------------------------------------------- host: matching decomposition
 * nx.max_weight_matching (graph_manager.py:64, inside GraphProcessor.getSubGraphs 57-83) without
 * networkx: the blossom algorithm networkx 3.4.2 runs, in its visiting orders, so the same maximum
 * matching comes back.  Host memory, no GPU.  Nodes are 0..n-1 in the graph's node order; node v's
 * neighbours are adj[adj_off[v] .. adj_off[v+1]) in its adjacency order (each edge in both lists),
 * adj_w their integer weights (NULL: all 1).  mate_out[v] = partner or -1; order_out[0..*n_order)
 * = nodes in the order they first entered networkx's `mate` dict (its result set is built by
 * iterating that dict). */
int mx_max_weight_matching(int n, const int64_t* adj_off, const int32_t* adj, const int64_t* adj_w,
                           int maxcardinality, int32_t* mate_out, int32_t* order_out, int* n_order);

/* ---------------------------------------------------------------- utilities
 * splitmix64 -> fp32 uniform[-1,1) synthetic inputs, x[i] for counter i+1. */
int mx_synth_fill(float* dst, int64_t n, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MATCHA_GOSSIP_H */
