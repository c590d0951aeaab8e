/*
 * pp2.h -- C ABI of libpp2_hip.so, the MI355X (gfx950) implementation of the
 * path_planning_2d planner's data-parallel core.
 *
 * Drop-in boundary.  The reference has no library API: its ROS node classes
 * call C++-linkage free functions and launch CUDA kernels on global device
 * pointers.  Every entry point below replaces one of those
 * functions / kernel launches; the replaced reference interface is cited as
 * path:line relative to /root/reference/path_planning_2d/.  INTEGRATION.md
 * shows the edits a maintainer makes in the catkin package to bind them.
 *
 * Conventions
 *  - Every function returns a pp2_status; nothing calls exit() (the
 *    reference's checkCudaErrors exits: helper_cuda.h:984-999).
 *    pp2_last_error() returns a message for the last failure on this thread.
 *  - A context is one grid (or one row shard of a grid) on one device; it
 *    owns all device memory.  Host pointers are caller-owned and only read or
 *    written during the call.  A context is not thread-safe.
 *  - All work is enqueued on the context's stream (its own, or one set with
 *    pp2_set_stream); functions that return host data synchronise it.
 *  - Host arrays use the reference's layouts: T[hw][9 u][9 s'],
 *    L[hw][16 z], R/C[hw][9 u], beliefs/values[hw] with idx = y*W + x.
 *  - Action u in 0..8 is the 3x3 raster with 4 = stay; observation z in 0..15
 *    is m3<<3|m2<<2|m1<<1|m0 (src/pomdp/path_planning_2d.cu:205-207).
 */
#ifndef PP2_H
#define PP2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP2_ABI_VERSION 4

typedef enum {
  PP2_OK = 0,
  PP2_EINVAL = 1,   /* bad argument / shape */
  PP2_EHIP = 2,     /* HIP runtime error */
  PP2_EIO = 3,      /* file I/O or parse error (text model/FIB formats) */
  PP2_ENOMEM = 4,   /* device or host allocation failed */
  PP2_ESTATE = 5,   /* call not valid in the current state */
  PP2_ERCCL = 6     /* RCCL error (sharded contexts) */
} pp2_status;

typedef struct pp2_ctx pp2_ctx;

int pp2_abi_version(void);
const char* pp2_status_string(int status);
const char* pp2_last_error(void);
int pp2_device_count(int* count);

/* ---------------------------------------------------------------- lifetime
 * Replaces allocateDeviceMemory(H,W) / freeDeviceMemory()
 * (src/mdp/path_planning_2d_cuda.cu:40-74), allocateDeviceMemoryOfModel /
 * freeDeviceMemoryOfModel (src/pomdp/model_generation_cuda.cu:41-72),
 * allocateDeviceMemoryOfFIB / freeDeviceMemoryOfFIB
 * (src/pomdp/fast_informed_bound_cuda.cu:54-94) and the dev_* / host_*
 * globals they fill.  `map` is the H*W occupancy grid (1 = occupied) that
 * loadMapFromFile() produces (src/pomdp/path_planning_2d.cu:243-257); it is
 * copied.  (goal_x, goal_y) and gamma are the node's goal_x/goal_y/
 * discount_factor parameters. */
int pp2_create(pp2_ctx** out, int device, uint32_t height, uint32_t width,
               const uint8_t* map, int32_t goal_x, int32_t goal_y, float gamma);
/* Row shard [row_begin, row_end) of a global_height x width grid (no
 * reference counterpart: the reference is single-GPU).  `global_map` is the
 * whole grid.  Once pp2_shard_comm_init has been called on every shard,
 * shards exchange halo rows over RCCL: loop steps k rows deep every k steps
 * (PP2_TUNE_HALO_DEPTH, or e rows per resident launch of up to e steps,
 * PP2_TUNE_RESIDENT_HALO), sweeps and belief-only updates one row per step. */
int pp2_create_shard(pp2_ctx** out, int device, uint32_t global_height,
                     uint32_t width, uint32_t row_begin, uint32_t row_end,
                     const uint8_t* global_map, int32_t goal_x, int32_t goal_y,
                     float gamma);
int pp2_destroy(pp2_ctx* ctx);
/* Enqueue on a caller stream (a hipStream_t, e.g. torch's current stream);
 * NULL restores the context's own stream. */
int pp2_set_stream(pp2_ctx* ctx, void* hip_stream);
int pp2_synchronize(pp2_ctx* ctx);
/* rows = owned rows, row_stride = padded cells per row in device planes. */
int pp2_get_geometry(pp2_ctx* ctx, uint32_t* rows, uint32_t* width,
                     uint32_t* row_stride, uint32_t* row_begin);
/* Tuning: cells per lane of the streaming kernels (1, 2 or 4; default 4). */
int pp2_set_cells_per_lane(pp2_ctx* ctx, int cpt);
/* Tuning knobs.  Unless a key says otherwise, values, actions, the raw
 * (unnormalised) belief of an update and the planner's tree shape are
 * bit-identical for every setting; quantities that pass through a belief's
 * mass or another whole-grid sum (normalised beliefs, Q-values of a belief,
 * the default-order planner's bounds and rewards) are equal to rounding where
 * a setting changes the association of that sum.
 *  PP2_TUNE_CELLS_PER_LANE  1, 2 or 4 (default 4).  The workgroup partials of
 *                           the mass cover other cells at each setting, so
 *                           normalised beliefs and the default-order planner's
 *                           sums are equal to rounding; the raw belief,
 *                           values and actions are bit-identical.  The coded
 *                           model (below) is used at 4 only; the planner's
 *                           expansion kernels exist for 4 and 1 and run as 1
 *                           at 2.
 *  PP2_TUNE_NT_STREAMS      1 (default) = non-temporal loads of the
 *                           once-read T/C streams (loop and sweep kernels at
 *                           4 cells per lane, the dense Q kernel): -8 % time
 *                           per loop step measured.  Bit-identical either way.
 *  PP2_TUNE_CODED_MODEL     1 (default) = loop step and MDP sweep read the
 *                           dictionary-coded model (pp2_model_dict_info)
 *                           when one exists, and FIB sweeps skip the T
 *                           entries the dictionary proved zero; 0 = always
 *                           the dense planes and full sums */
#define PP2_TUNE_CELLS_PER_LANE 1
#define PP2_TUNE_NT_STREAMS 2
#define PP2_TUNE_CODED_MODEL 3
/*  PP2_TUNE_HALO_DEPTH      row shards (RCCL or shard group), launch-per-step
 *                           loop: steps per halo exchange = halo rows
 *                           exchanged, 1..8 (default: the most the smallest
 *                           shard allows) */
#define PP2_TUNE_HALO_DEPTH 4
/*  PP2_TUNE_COMM_STREAM     0 (default): RCCL calls are issued on the context's
 *                           stream; 1: on a dedicated stream entered and left
 *                           through events */
#define PP2_TUNE_COMM_STREAM 5
/*  PP2_TUNE_NORM_BLOCK      unsharded pp2_loop_step: 1 = divide by the exact
 *                           mass every step (bit-exact with per-step host
 *                           normalisation); k = 2..8 (default 8) = divide by
 *                           the exact mass times 2^96 at the first step of
 *                           every k and by 1 in between (beliefs equal to
 *                           rounding; values and actions unchanged) */
#define PP2_TUNE_NORM_BLOCK 6
/*  PP2_TUNE_STEP_PAIRS      1 (default): pp2_loop_run (and
 *                           pp2_shard_group_loop_run) on a context with a
 *                           sparse coded model runs two steps of a
 *                           normalisation / halo block per launch (the first
 *                           over the tile plus a one-row halo, kept in LDS)
 *                           where the grid has a 4096-cell tile per CU;
 *                           2 = pairs on any fitting grid (tests);
 *                           0 = one launch per step.  Results are
 *                           bit-identical either way. */
#define PP2_TUNE_STEP_PAIRS 7
/*  PP2_TUNE_RESIDENT        1 (default): pp2_loop_run on an unsharded context
 *                           with a sparse coded model whose grid fits one
 *                           tile of whole rows per CU (width padded to a
 *                           multiple of 256, rows * width <= 4096 * CUs, the
 *                           dictionary in LDS) runs the whole trajectory in
 *                           one launch (the tile-resident loop, up to 2048
 *                           steps per launch); 0 = step pairs / single steps.
 *                           pp2_mdp_solve and pp2_mdp_sweep(n >= 2) run as
 *                           resident sweeps under the same conditions.
 *                           Results are bit-identical either way.  A plan
 *                           whose tiles cannot all be resident at once is
 *                           never launched.  Resident launches of this
 *                           process run one at a time per device.  A launch
 *                           that still cannot get every tile onto the GPU
 *                           within 0.25 s (another process holding CUs) ends
 *                           early, leaves its inputs intact, and the next
 *                           call on the context re-runs it on per-step
 *                           launches before reading anything (same bits; the
 *                           context then stays on them: pp2_resident_status).
 *                           Consequence: a call after a resident launch
 *                           first waits for that launch to finish -- except
 *                           pp2_loop_run and pp2_mdp_sweep(n >= 2) taking
 *                           the resident path again, which queue behind up
 *                           to 16 unverified launches without a host sync
 *                           (a launch queued behind one that timed out does
 *                           nothing, and all of them are re-run). */
#define PP2_TUNE_RESIDENT 8
/*  PP2_TUNE_RESIDENT_HALO   row shards: the loop runs on the resident kernel
 *                           when a view of the owned rows plus e halo rows
 *                           per side fits one tile per CU; a run of n steps
 *                           is ceil(n / e) launches of up to e steps, each
 *                           after one exchange of e halo rows and one
 *                           {mass, shift} all-reduce.  Value
 *                           = the largest e to use (0, default: the most the
 *                           halo allocation of 128 rows, the smallest shard
 *                           and the CUs allow).  Values and actions are
 *                           bit-identical to the unsharded grid either way. */
#define PP2_TUNE_RESIDENT_HALO 9
/*  PP2_TUNE_RESIDENT_TILE_COLS  tiles of the resident loop: 0 (default) =
 *                           whole rows, or two tile columns (2-D tiles whose
 *                           first and last columns cross CUs as well) when
 *                           whole-row tiles would hold fewer than 4 rows and
 *                           2-D tiles hold 4 or more (a 256 x 2048 rank share
 *                           of the 2048^2 grid on its 512-row view); 1 = whole
 *                           rows always; 2 = two tile columns wherever they
 *                           fit; 3 = transposed tiles on a row shard's view
 *                           whose row count is a multiple of 256 (e and the
 *                           owned rows multiples of 4): a tile is a strip of
 *                           grid columns spanning the whole view, so only its
 *                           two side columns cross CUs (HBM keeps the row-major
 *                           layout; the launch reads and writes it
 *                           transposed).  Values and actions are bit-identical
 *                           either way, beliefs equal to rounding. */
#define PP2_TUNE_RESIDENT_TILE_COLS 12
/*  PP2_TUNE_SHARD_LAG       row shards' resident launches: 0 (default) = a
 *                           normalisation block start inside a launch scales
 *                           the view by the power of two chosen from the
 *                           previous step's mass, after every tile of the view
 *                           has arrived; 1 = from its mass one block earlier
 *                           (staged in LDS ahead of time: no grid-wide wait,
 *                           no barrier).  Measured on the 2-D tiles of the
 *                           config-4 rank share the waited block start costs
 *                           nothing visible and the lagged one's extra state
 *                           ~0.2 us per step, so it is off by default; on
 *                           transposed tiles it is the faster one.  Beliefs
 *                           equal each other to rounding (power-of-two scales
 *                           are exact); values and actions are bit-identical. */
#define PP2_TUNE_SHARD_LAG 13
/*  PP2_TUNE_RESIDENT_MASKED 1 (default): whole-row tiles of the tile-resident
 *                           loop run its masked-support form on a model that
 *                           is admitted to it (pp2_resident_masked; every
 *                           generated model whose goal is a free cell): blocked
 *                           cells are kept as +0 in the tile and the base
 *                           kernel's weights are constants, instead of a table
 *                           read per cell and action.  0 = never.  Results are
 *                           bit-identical either way. */
#define PP2_TUNE_RESIDENT_MASKED 15
/*  Diagnostics (tests):
 *  PP2_TUNE_RESIDENT_CUS    plan resident launches for at most this many CUs
 *                           (0: all); a grid whose tiles do not fit falls
 *                           back before launching
 *  PP2_TUNE_RESIDENT_STALL  tile index that returns at once (-1: none): the
 *                           other tiles' waits time out, exercising the
 *                           re-run of a failed resident launch */
#define PP2_TUNE_RESIDENT_CUS 10
#define PP2_TUNE_RESIDENT_STALL 11
/*  PP2_TUNE_COMM_TIMING     1 = bracket every RCCL round of the context (halo
 *                           exchanges, record groups, all-reduces) with timing
 *                           events on the stream it runs on; read with
 *                           pp2_comm_rounds.  0 (default) = no events. */
#define PP2_TUNE_COMM_TIMING 14
/*  PP2_TUNE_MAP_INCREMENTAL 1 (default): pp2_map_update / pp2_goal_set
 *                           regenerate and re-code only the cells that changed.
 *                           0 = every update regenerates the whole model and
 *                           rebuilds the dictionary.  Results are identical
 *                           either way. */
#define PP2_TUNE_MAP_INCREMENTAL 16
int pp2_set_tuning(pp2_ctx* ctx, int key, int value);
/* Measurement, no reference counterpart (the reference is single-GPU): the
 * RCCL rounds timed since PP2_TUNE_COMM_TIMING was set or the last call --
 * `rounds` timed rounds (at most 256 between calls; later ones are counted in
 * `untimed`, which may be NULL), the first max_rounds of their durations in
 * microseconds (begin event to end event on the issuing stream: the group's
 * own time plus any wait for the peers).  Synchronises; clears the record. */
int pp2_comm_rounds(pp2_ctx* ctx, int* rounds, long long* untimed, float* round_us,
                    int max_rounds);

/* ---------------------------------------------------------------- model
 * generateModelData (src/pomdp/model_generation_cuda.cu:349-368) and the MDP
 * cudaGenerateModelData launch (src/mdp/path_planning_2d.cu:93-106): builds
 * T, L, R (POMDP stage reward) and C (MDP stage cost) on the device. */
int pp2_model_generate(pp2_ctx* ctx);
/* Download in the reference layouts (any pointer may be NULL); replaces the
 * D2H copies into host_trans_prob/host_meas_prob/host_stage_reward
 * (model_generation_cuda.cu:370-375). */
int pp2_model_download(pp2_ctx* ctx, float* T, float* L, float* R, float* C);
/* Upload reference-layout tensors (any may be NULL = keep); the device half
 * of loadModelDataFromFile (model_generation_cuda.cu:150-156). */
int pp2_model_upload(pp2_ctx* ctx, const float* T, const float* L,
                     const float* R, const float* C);
/* Text formats of saveModelDataToFile / loadModelDataFromFile
 * (model_generation_cuda.cu:74-159): files model_data_trans_prob,
 * model_data_meas_prob, model_data_stage_reward in `dir` ("%15.8f"). */
int pp2_model_save(pp2_ctx* ctx, const char* dir);
int pp2_model_load(pp2_ctx* ctx, const char* dir);
/* Dictionary-coded model (no reference counterpart; a lossless re-encoding of
 * the arrays above).  Every call that sets the model (generate / upload /
 * load) rebuilds it: one uint16 code per cell plus one dictionary row per
 * distinct per-cell (T, C, L) tuple, checked bitwise against every cell.
 * entries = dictionary rows (0: more than the LDS budget allows, dense path
 * only); active = 1 when pp2_loop_step / pp2_mdp_sweep use it.  Results are
 * bit-identical either way. */
int pp2_model_dict_info(pp2_ctx* ctx, int* entries, int* active);

/* ---------------------------------------------------------------- live updates
 * No reference counterpart (the reference fixes map and goal at start-up).
 * Unsharded contexts only: a row shard, an RCCL rank or a shard-group member
 * returns PP2_ESTATE.
 *
 * pp2_map_update: rows [y0, y0 + h) x columns [x0, x0 + w) of the stored map
 * take `patch` (h * w bytes, row-major, pp2_create's meaning: 1 = occupied,
 * anything else free).  PP2_EINVAL for an empty rectangle, one that leaves the
 * grid, or a null patch.  Stream ordered like pp2_model_generate.
 * pp2_goal_set: the goal becomes (gx, gy) -- any integers, as for pp2_create;
 * off the grid means no goal cell.
 *
 * Before a model exists both only rewrite the stored map / goal.  With a
 * generated model in force (made by pp2_model_generate and kept so by these
 * calls) they leave the context exactly as a freshly created context with the
 * new map and goal would be after pp2_model_generate:
 *   - T, L, R and C have the fresh context's bits;
 *   - the coded model is active under the same conditions;
 *   - the masked-support admission (pp2_resident_masked) is the one a fresh
 *     build decides;
 *   - the dictionary's entry numbering may differ from a fresh build and rows
 *     that no cell uses any more may remain (pp2_model_dict_info's entry count
 *     may be larger); no result depends on either.
 * A cell's model is a function of its 3x3 occupancy and of being the goal, so
 * a w x h rectangle regenerates at most (w + 2) x (h + 2) cells and a goal move
 * two; each is re-coded against the dictionary in force, new tuples append
 * rows.  Anything the patch path cannot settle (a hash collision, more than
 * the dictionary's row limit) runs the full build instead: correctness never
 * rests on the fast path (PP2_TUNE_MAP_INCREMENTAL 0 always takes the full one).
 * With an uploaded or loaded model in force they return PP2_ESTATE:
 * regenerating part of a foreign model would mix two models.
 *
 * The belief, J / A, the FIB alphas, the PBVI beliefs and alphas and every
 * tuning setting are state: kept untouched -- the caller re-solves
 * (pp2_mdp_resolve, pp2_fib_solve, ...).  A generated model is clean, so the
 * state flags of the sparse paths are neither cleared nor set.  Objects that
 * cached model data at creation refuse to run afterwards: pp2_planner_step of
 * a planner created before an update that changed the model returns
 * PP2_ESTATE until pp2_planner_refresh brings its caches up to date; rollouts
 * and episode batches read the model on every run and carry on. */
int pp2_map_update(pp2_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                   const uint8_t* patch);
int pp2_goal_set(pp2_ctx* ctx, int32_t gx, int32_t gy);
/* The map (height * width bytes, as given) and goal in force; any pointer may
 * be NULL. */
int pp2_map_get(pp2_ctx* ctx, uint8_t* map, int32_t* gx, int32_t* gy);
/* Diagnostics: update calls that changed the model, those of them served by
 * the patch path, those that ran the full build (PP2_TUNE_MAP_INCREMENTAL 0,
 * or a fall-back), and the dictionary rows the last such call appended.  A
 * call that changes no cell's occupancy (or moves no goal cell) counts
 * nowhere.  Any pointer may be NULL. */
int pp2_map_update_info(pp2_ctx* ctx, long long* updates, long long* incremental,
                        long long* rebuilds, int* entries_added);

/* Loop steps pp2_loop_run fuses into one kernel launch on this context: 2048
 * for the tile-resident loop (PP2_TUNE_RESIDENT) on an unsharded grid, the
 * resident halo depth e on a row shard (PP2_TUNE_RESIDENT_HALO), 2 when it
 * runs the steps of a normalisation / halo block in pairs
 * (PP2_TUNE_STEP_PAIRS with a sparse coded model whose grid has a 4096-cell
 * tile per CU; unsharded, RCCL row shard or shard-group member), else 1.
 * A query: allocates nothing. */
int pp2_loop_steps_per_launch(pp2_ctx* ctx, int* steps);
/* The tiling of the tile-resident loop this context would launch (its grid,
 * or a row shard's view): tiles (one per CU), rows per tile and tile columns
 * (1: whole rows; 2: 2-D tiles, PP2_TUNE_RESIDENT_TILE_COLS; 3: transposed
 * tiles of a shard view, rows per tile = grid columns per tile); all 0 when the
 * loop does not run resident.  A query: allocates nothing. */
int pp2_resident_tiling(pp2_ctx* ctx, int* tiles, int* rows_per_tile, int* tile_cols);
/* Diagnostics: resident launches so far on this context -- tile-resident loop
 * launches (pp2_loop_run) and resident MDP-solve launches (pp2_mdp_solve);
 * either pointer may be NULL.  No reference counterpart. */
int pp2_resident_launches(pp2_ctx* ctx, int* loop_launches, int* solve_launches);
/* Whether the current model is admitted to the masked-support form of the
 * tile-resident loop (re-evaluated whenever the model is set: generate, upload,
 * load), and how many of the loop launches counted by pp2_resident_launches
 * ran it (PP2_TUNE_RESIDENT_MASKED); either pointer may be NULL. */
int pp2_resident_masked(pp2_ctx* ctx, int* admitted, int* launches);
/* Resident launches re-run on per-step launches after a timeout, and whether
 * the resident kernels are still enabled on the context (either may be NULL). */
int pp2_resident_status(pp2_ctx* ctx, int* fallbacks, int* enabled);

/* ---------------------------------------------------------------- belief
 * The belief lives on the device with deferred normalisation: each update
 * applies the previous step's 1/sum and records its own sum on the device,
 * so no host round trip is needed per step.
 *
 * pp2_belief_set: root belief from a Belief message (msg->belief,
 * src/pomdp/path_planning_2d.cu:208), used as given. */
int pp2_belief_set(pp2_ctx* ctx, const float* belief);
/* Normalised belief b/sum (host renormalisation of search_tree_cuda.cu:
 * 608-612). */
int pp2_belief_get(pp2_ctx* ctx, float* belief);
/* cudaBayesBeliefUpdate (point_based_value_iteration_cuda.cu:88-133) +
 * renormalisation (search_tree_cuda.cu:601-612).  Asynchronous. */
int pp2_belief_update(pp2_ctx* ctx, uint8_t u, uint8_t z);
/* The stored (unnormalised) belief and its mass: belief_get == raw / mass.
 * Exposes the kernel output itself, for bit-exact parity checks. */
int pp2_belief_get_raw(pp2_ctx* ctx, float* belief, float* mass);
/* Unnormalised mass of the current belief (= p(z | b, u) after an update
 * from a normalised belief). Synchronises. */
int pp2_belief_mass(pp2_ctx* ctx, float* mass);

/* ---------------------------------------------------------------- MDP
 * J := 0, A := 0 (cudaMemset, src/mdp/path_planning_2d_cuda.cu:55-61). */
int pp2_mdp_reset(pp2_ctx* ctx);
/* n Bellman sweeps, cudaOneStepValueIteration
 * (src/mdp/path_planning_2d_cuda.cu:215-264). Asynchronous. */
int pp2_mdp_sweep(pp2_ctx* ctx, int n);
/* MdpPathPlanning2d::valueIteration (src/mdp/path_planning_2d.cu:207-269)
 * without the OpenCV windows: blocks of 100 sweeps until the inf-norm of the
 * change over a block is <= 1e-3*5/(1-gamma).  max_sweeps <= 0: no cap. */
int pp2_mdp_solve(pp2_ctx* ctx, int max_sweeps, int* sweeps,
                  double* final_norm);
/* pp2_mdp_solve without its pp2_mdp_reset: the same driver, stop rule and
 * resident path, started from the current J (after pp2_map_update /
 * pp2_goal_set: the previous solution).  If a resident launch times out it
 * falls back as pp2_mdp_solve does, which restarts from J = 0. */
int pp2_mdp_resolve(pp2_ctx* ctx, int max_sweeps, int* sweeps,
                    double* final_norm);
/* D2H of dev_optimal_cost1 / dev_optimal_action
 * (src/mdp/path_planning_2d.cu:119-126).  Either may be NULL. */
int pp2_mdp_get(pp2_ctx* ctx, float* J, uint8_t* A);

/* ---------------------------------------------------------------- north star
 * One iteration of the benchmarked loop: one belief update (u, z) and one
 * Bellman sweep in one launch.  The stored belief is renormalised by its
 * exact mass every PP2_TUNE_NORM_BLOCK steps (power-of-two scaled in
 * between); reads always divide by the true mass.  Sharded contexts also
 * exchange halo rows and all-reduce the belief mass at each block start.
 * Asynchronous. */
int pp2_loop_step(pp2_ctx* ctx, uint8_t u, uint8_t z);
int pp2_loop_run(pp2_ctx* ctx, int n, const uint8_t* us, const uint8_t* zs);

/* ---------------------------------------------------------------- control
 * The next control from the device-resident belief, J and A, without moving a
 * plane to the host: each call copies one small record back and synchronises.
 * Unsharded contexts only (a row shard or shard-group member: PP2_ESTATE).
 *
 * pp2_belief_mode: the scan of MdpPathPlanning2d::beliefCallback
 * (src/mdp/path_planning_2d.cu:168-189) over the normalised belief n =
 * pp2_belief_get: cell = the smallest idx = y*W + x with n(idx) > 0 and
 * n(idx) >= n(j) for all j, prob = n(cell); cell 0, prob 0 when no cell is
 * > 0 (NaNs never win).  Either pointer may be NULL. */
int pp2_belief_mode(pp2_ctx* ctx, int32_t* cell, float* prob);
/* Belief-expected Q values of the current J (no reference counterpart):
 * q[u] = (sum_x b(x) Q(x,u)) / mass over the stored belief b and its mass,
 * Q(x,u) = C[x][u] + sum_i gamma*T[x][u][i] * J(x+off_i) with
 * pp2_mdp_sweep's arithmetic, J = 0 outside the grid.  Summed in a fixed
 * order: bit-identical from run to run and between PP2_TUNE_CODED_MODEL 0 and
 * 1.  Needs a model (else PP2_ESTATE). */
int pp2_mdp_qvalues(pp2_ctx* ctx, float q[9]);
/* The control of a policy.  PP2_CONTROL_MODE: cell = pp2_belief_mode's,
 * action = A[cell], value = J[cell] (the planes of pp2_mdp_get).
 * PP2_CONTROL_QMDP: action = the first u attaining min_u q[u] (strict <, the
 * sweep's tie rule), value = q[action], cell = -1.  value and cell may be
 * NULL.  Needs a model (else PP2_ESTATE); an unknown policy is PP2_EINVAL. */
#define PP2_CONTROL_MODE 0   /* reference MDP node: action of the belief's mode */
#define PP2_CONTROL_QMDP 1   /* argmin_u of the belief-expected Q over the current J */
int pp2_mdp_control(pp2_ctx* ctx, int policy, uint8_t* action, float* value, int32_t* cell);

/* ---------------------------------------------------------------- FIB
 * cudaFIBValueIteration sweeps (fast_informed_bound_cuda.cu:97-204) from the
 * current alphas (zero after create). Asynchronous. */
int pp2_fib_reset(pp2_ctx* ctx);
int pp2_fib_sweep(pp2_ctx* ctx, int n);
/* fastInformedBound driver (fast_informed_bound_cuda.cu:206-276): blocks of
 * 10 sweeps until the inf-norm of the change <= 0.01. */
int pp2_fib_solve(pp2_ctx* ctx, int max_sweeps, int* sweeps, float* final_norm);
/* pp2_fib_solve without its pp2_fib_reset: the same blocks of 10 sweeps and
 * the same stop rule, started from the current alphas (after pp2_map_update /
 * pp2_goal_set: the previous solution).  The sweep is a contraction, so a
 * warm start converges to the same fixed point as a cold one, within the stop
 * rule's tolerance.  From alphas of 0 the iterates fall monotonically and each
 * is an upper bound; from an arbitrary start they are not monotone, so after
 * an update that removed an obstacle (values rise) the alphas need not be
 * upper bounds before convergence.  The caller chooses: pp2_fib_resolve where
 * fewer sweeps matter, pp2_fib_solve where every iterate must bound. */
int pp2_fib_resolve(pp2_ctx* ctx, int max_sweeps, int* sweeps, float* final_norm);
/* host_fib_alphas layout [hw][9] (fast_informed_bound_cuda.cu:270-271). */
int pp2_fib_get(pp2_ctx* ctx, float* alphas);
int pp2_fib_set(pp2_ctx* ctx, const float* alphas);
/* saveFibDataToFile / loadFibDataFromFile (fast_informed_bound_cuda.cu:
 * 343-394): dir/fib_alphas (one cell per line, 9 "%15.8f" values) and
 * dir/fib_actions (the 9 actions, "%10u" per line).  dir NULL: ".". */
int pp2_fib_save(pp2_ctx* ctx, const char* dir);
int pp2_fib_load(pp2_ctx* ctx, const char* dir);

/* ---------------------------------------------------------------- PBVI
 * Point-based value iteration lower bound (src/pomdp/
 * point_based_value_iteration_cuda.cu), state kept in the context (unsharded
 * contexts only): the belief set B[S][hw], alpha vectors alphas[S][hw] and
 * their actions[S] (host_pbvi_alphas / host_pbvi_actions, :51-57).  The
 * reference's node uses S = 500 (src/pomdp/path_planning_2d.cu:122,140).
 *
 * generateBeliefSet (:165-295): S beliefs (1..4096) grown from b0 (hw
 * floats, used as given).  Three glibc rand() draws per (belief, action) and round from
 * srand(rand_seed) (the reference never seeds: 1); *rand_calls (may be NULL)
 * gets the number drawn, so a planner can continue the same stream.  Resets
 * the alphas to 0 (pointBasedValueIteration, :652-657). */
int pp2_pbvi_belief_set(pp2_ctx* ctx, const float* b0, uint32_t set_size,
                        uint32_t rand_seed, uint64_t* rand_calls);
/* Any S beliefs [S][hw] as the belief set (alphas reset to 0). */
int pp2_pbvi_set_beliefs(pp2_ctx* ctx, uint32_t set_size, const float* beliefs);
int pp2_pbvi_get_beliefs(pp2_ctx* ctx, float* beliefs);
/* backupAlphaVectors (:319-641): `iterations` synchronous point-based
 * backups from the current alphas; iterations <= 0 runs the reference's
 * ceil(log(1e-3/5) / log(gamma)) (:440-441).  Asynchronous. */
int pp2_pbvi_backup(pp2_ctx* ctx, int iterations);
/* pointBasedValueIteration (:643-676): belief set + zero alphas + backup. */
int pp2_pbvi_solve(pp2_ctx* ctx, const float* b0, uint32_t set_size,
                   uint32_t rand_seed, uint64_t* rand_calls);
/* S (0 before any PBVI call) and whether a belief set is present. */
int pp2_pbvi_info(pp2_ctx* ctx, uint32_t* set_size, int* has_beliefs);
/* alphas [S][hw] and actions [S]; either may be NULL. */
int pp2_pbvi_get(pp2_ctx* ctx, float* alphas, uint8_t* actions);
int pp2_pbvi_set(pp2_ctx* ctx, uint32_t set_size, const float* alphas,
                 const uint8_t* actions);
/* evaluatePbviCpu (:678-699) for n beliefs [n][hw]: values[i] = max over k
 * of inner_product(b_i, alpha_k) (x-ordered, multiply then add), actions[i]
 * = the action of the first maximising alpha.  Either output may be NULL. */
int pp2_pbvi_evaluate(pp2_ctx* ctx, int n, const float* beliefs, float* values,
                      uint8_t* actions);
/* savePbviDataToFile / loadPbviDataFromFile (:737-797): dir/pbvi_alphas (one
 * alpha vector per line, "%15.8f" per cell) and dir/pbvi_actions ("%10u" per
 * line; read back into uint8 storage, which the reference overflows). */
int pp2_pbvi_save(pp2_ctx* ctx, const char* dir);
int pp2_pbvi_load(pp2_ctx* ctx, const char* dir, uint32_t set_size);

/* ---------------------------------------------------------------- QV-tree
 * Online POMDP planner: QNode / VNode / SearchTree
 * (include/path_planning_2d/search_tree.h:31-165, src/pomdp/
 * search_tree_cuda.cu:161-626) driven like PomdpPathPlanning2d::beliefCallback
 * (src/pomdp/path_planning_2d.cu:199-241).  Tree logic runs on the host
 * exactly as the reference; every belief update, renormalisation and leaf
 * bound of one VNode::expand (9 actions x all observations) is one batched
 * device pass over the context's model (T, L, R) and FIB alphas (set them
 * with pp2_fib_solve / pp2_fib_set first).  Beliefs of expanded nodes stay
 * on the device; leaf children are scored without being materialised.
 *
 * Sampling follows the reference bit for bit in algorithm: 50 state samples
 * per QNode from glibc rand() over the fp32 prefix sum of the belief
 * (search_tree_cuda.cu:326-337), next state and observation from the cuRAND
 * XORWOW stream curand_init(1234, idx, 0) that every QNode re-creates
 * (:84-147, :318-323). */
typedef struct pp2_planner pp2_planner;

typedef struct {
  int32_t max_search_tree_depth;  /* launch default 50 */
  int32_t max_online_iteration;   /* launch default 15 */
  int32_t lower_bound_mode;       /* 0: constant -5/(1-gamma), the reference's
                                     commented fallback (search_tree_cuda.cu:382-383);
                                     1: PBVI, evaluatePbviCpu (:379) over the
                                     context's alpha vectors (pp2_pbvi_*) */
  uint32_t rand_seed;             /* glibc srand seed; reference never seeds: 1 */
  uint32_t sample_num;            /* observation samples per QNode (:176): 50 */
  uint64_t curand_seed;           /* curand_init seed (:90): 1234 */
  uint64_t rand_skip;             /* rand() draws already taken from the stream
                                     (the reference's generateBeliefSet runs
                                     first: pp2_pbvi_solve's *rand_calls) */
  int32_t reference_order;        /* 1 (default, the drop-in): every sum the
                                     reference runs on its host -- the QNode
                                     reward inner_product and the child
                                     renormalisation accumulate
                                     (search_tree_cuda.cu:168-173, :225-229),
                                     evaluateFibCpu / evaluatePbviCpu
                                     (fast_informed_bound_cuda.cu:278-297,
                                     point_based_value_iteration_cuda.cu:
                                     678-699) and the sampling cdf (:176-183)
                                     -- gives the result of the reference's
                                     x-ordered fp32 chain (multiply, then add;
                                     IEEE division), so bounds, rewards,
                                     weights and the tree equal the
                                     reference's arithmetic bit for bit.
                                     0 (opt-in fast variant, NOT bit-exact):
                                     grid-wide sums as parallel trees (fp64
                                     where the reference's fp32 chains lose
                                     digits); within rel 1e-4 of the
                                     reference, which can flip a near-tied
                                     expansion choice. */
} pp2_planner_params;

/* Snapshot of the root and its children, for inspection and parity tests. */
typedef struct {
  uint32_t depth;
  float root_upper_bound, root_lower_bound, root_heuristic;
  uint32_t n_root_children;  /* 0 (unexpanded) or 9 */
  float q_upper_bound[9], q_lower_bound[9], q_reward[9], q_heuristic[9];
  uint32_t q_depth[9], q_nchildren[9];
  uint8_t q_obs[9][16];
  float q_weight[9][16], v_upper_bound[9][16], v_lower_bound[9][16];
  uint32_t total_vnodes, total_qnodes, expansions;
} pp2_tree_info;

int pp2_planner_default_params(pp2_planner_params* p);
/* PomdpPathPlanning2d::initialize tail (src/pomdp/path_planning_2d.cu:145-155):
 * binds the planner to a context whose model and FIB alphas are ready. */
int pp2_planner_create(pp2_planner** out, pp2_ctx* ctx,
                       const pp2_planner_params* params);
int pp2_planner_destroy(pp2_planner* p);
/* One plan step = beliefCallback (:199-241): first call (or after reset)
 * builds the tree from `belief` (hw floats, used as given); later calls
 * re-root with (action, observation).  Expands while depth < max depth and
 * fewer than max_online_iteration expansions, then returns the action with
 * the largest Q upper bound. */
int pp2_planner_step(pp2_planner* p, uint8_t action, uint8_t observation,
                     const float* belief, uint8_t* new_action,
                     float* new_value);
/* resetSearchTreeCallback (:275-282). */
int pp2_planner_reset(pp2_planner* p);
int pp2_planner_info(pp2_planner* p, pp2_tree_info* info);
/* Brings a planner's cached model (its host copies of T and L, its dense R
 * and L rows) up to the context's current model after pp2_map_update /
 * pp2_goal_set; until then pp2_planner_step returns PP2_ESTATE.  With the
 * model unchanged since the planner last read it: PP2_OK, nothing is launched,
 * the tree is kept, the call counts nowhere.  Otherwise the caches are patched
 * over the cells the updates regenerated (one kernel launch, one synchronise)
 * when the context still remembers every update since (its journal holds the
 * last 16), those rectangles hold at most 4096 cells together and
 * PP2_TUNE_MAP_INCREMENTAL is 1 at the time of the call; else they are read
 * again in full, as pp2_planner_create reads them.  Correctness never rests on
 * the patch path.  Either way nothing is allocated besides the patch path's
 * staging buffer on its first use.
 *
 * The tree was built under the old model: every node below the root is
 * deleted.  The root's belief stays where it is, the same bits with the same
 * mass, and becomes a fresh unexpanded root (depth 0) whose bounds are those
 * of the current model, the current FIB alphas and, in lower_bound_mode 1, the
 * current PBVI alphas: the caller re-solves them first (pp2_fib_resolve /
 * pp2_fib_solve, ...), refresh uses whatever alphas are current.  The next
 * pp2_planner_step(action, observation, NULL, ...) re-roots from that belief.
 * Without a root (never stepped, or reset) only the caches are refreshed.  The
 * rand() stream continues, the cuRAND uniforms and the parameters stay.  A
 * changed PBVI set size is reported by the next step.
 *
 * pp2_model_upload does not count as an update: it leaves a planner's caches
 * stale without any refusal, and refresh sees nothing to do (existing
 * behaviour; create the planner after the upload). */
int pp2_planner_refresh(pp2_planner* p);
/* Diagnostics: refreshes that found a changed model, those of them served by
 * the patch path, those that read the caches in full, and the cells the last
 * such refresh patched (rectangles of several updates that overlap count a
 * cell once each; 0 after a full one).  Any pointer may be NULL. */
int pp2_planner_refresh_info(pp2_planner* p, long long* refreshes, long long* incremental,
                             long long* full, long long* cells_patched);
/* The root's belief (hw floats) as a new tree would be given it: under
 * reference_order 1 the root's normalised row bit for bit, under
 * reference_order 0 the stored belief divided by its stored mass (IEEE
 * division on the host).  PP2_ESTATE without a root.  Synchronises. */
int pp2_planner_root_belief(pp2_planner* p, float* belief);
/* rand_skip plus every rand() draw the planner has taken: the rand_skip a
 * planner created now needs to continue the same stream. */
int pp2_planner_rand_calls(pp2_planner* p, uint64_t* calls);
/* The 2*n curand_uniform draws the reference's cudaForwardSampling sees:
 * u1[i], u2[i] = first and second draw of curand_init(seed, i, 0). */
int pp2_curand_uniforms(uint64_t seed, int n, float* u1, float* u2);

/* ---------------------------------------------------------------- rollouts
 * Batched QV-tree rollouts (BASELINE configs[4]: 4096 copies x depth 5 at
 * 512x512): C copies of a root belief each follow their own (u_k, z_k),
 * k < depth.  Per copy and step: reward r_k = <b_k, R[:,u_k]> (QNode reward,
 * search_tree_cuda.cu:168-173), observation likelihood p_k = sum of the
 * unnormalised update, b_{k+1} = normalise(L_zk . T_uk^T b_k) (the
 * reference update + renormalisation); leaf: FIB bound max_i <b_depth,
 * alpha_i> (evaluateFibCpu); value = sum_k gamma^k r_k + gamma^depth * leaf.
 * Beliefs are stored as per-copy max-normalised fp16 (2 B per cell-copy),
 * arithmetic is fp32; expect ~1e-3 relative agreement with an fp32 rollout. */
typedef struct pp2_rollout pp2_rollout;
/* copies 1..131072, depth >= 1 */
int pp2_rollout_create(pp2_rollout** out, pp2_ctx* ctx, int copies, int depth);
int pp2_rollout_destroy(pp2_rollout* r);
/* root belief (hw floats): every copy starts from it (one fp16 image that
 * the first step of every run reads for all copies) */
int pp2_rollout_set_root(pp2_rollout* r, const float* belief);
/* us, zs: [depth][copies]; every run starts from the root.  Asynchronous. */
int pp2_rollout_run(pp2_rollout* r, const uint8_t* us, const uint8_t* zs);
/* rewards, obs_prob: [depth][copies]; leaf_upper, value: [copies]; any may be
 * NULL.  Synchronises. */
int pp2_rollout_results(pp2_rollout* r, float* rewards, float* obs_prob,
                        float* leaf_upper, float* value);
/* normalised fp32 belief of one copy after the run, or the root before any
 * run (hw floats) */
int pp2_rollout_get_belief(pp2_rollout* r, int copy, float* belief);

/* ---------------------------------------------------------------- episodes
 * Batched closed-loop policy episodes (what the reference does by running its
 * node against dummy_simulator): E simulated robots, each with its own fp32
 * belief, follow a control policy for up to `horizon` steps in one launch --
 * one workgroup per episode, the belief in LDS.  Needs an unsharded context
 * with a model, current J and A, and an active dictionary-coded model with
 * factored rows (pp2_model_dict_info), whose belief fits the LDS of one
 * workgroup (100x40 and 97x131 do, 256x256 does not: PP2_EINVAL) -- unless
 * the batch was created with another placement of the belief:
 *
 * Placement (pp2_episodes_create_placed).  An episode's two belief planes live
 * in the LDS of its workgroup (PP2_EPISODES_LDS, pp2_episodes_create's) or in
 * device memory (PP2_EPISODES_GLOBAL), which admits any grid the context
 * supports; PP2_EPISODES_AUTO decides per launch: LDS if that launch's LDS
 * layout fits (an alpha run's is larger than a MODE / QMDP run's), else device
 * memory.  The placement changes no result: every step below, every rounding,
 * the pinned Q-dot order, the random numbers, statuses and traces are the
 * same bits from either.  The device-memory planes are one scratch per batch,
 * allocated (and zeroed, once) at the first launch that needs it, never at
 * create -- PP2_ENOMEM if that fails, the batch stays usable -- and freed by
 * pp2_episodes_destroy: per workgroup two fp32 planes [H + 2][stride + 4] + 4
 * (zero halo rows and x pads, rounded up to 256 bytes), then one padded image
 * of b0 and one padded uint16 code plane, both rebuilt by every such run and
 * shared by all workgroups.  Workgroups of such a launch = min(episodes,
 * CUs x 4, what 1 GiB of scratch holds), at least 1.  MODE, QMDP and alpha
 * runs (FIB, and PBVI with any K <= 4096) take either placement, and so does
 * the lookahead through pp2_episodes_run_lookahead_placed (a device-memory
 * lookahead launch has min(episodes, workgroups the scratch holds, CUs x 2)
 * workgroups, what its registers admit); the older entry
 * pp2_episodes_run_lookahead keeps its contract and runs from LDS planes or
 * not at all.
 *
 * Episode e: true cell s = start_cells[e] (y*W + x), stored belief b = b0,
 * cost G = +0, discount d = 1.  If s is the goal: steps 0, status 1, belief
 * b0.  Else each step k = 0 .. horizon-1:
 *  1. control.  PP2_CONTROL_MODE: cell = the smallest y*W + x whose stored
 *     b > 0 and is >= every other cell (cell 0 if none; NaNs never win),
 *     u = A[cell].  The stored values are compared -- the belief is only ever
 *     rescaled by powers of two -- so ties can break differently from
 *     pp2_belief_mode, which compares the quotients b / mass.
 *     PP2_CONTROL_QMDP: S_u = sum_i b[i] Q_u[i] in the pinned order below,
 *     u = the first strict minimum over u = 0..8 from FLT_MAX (no division by
 *     the mass: the argmin does not need it).
 *  2. cost.  G = G + fl(d * C[s][u]), then d = fl(d * gamma): C the MDP cost
 *     of pp2_model_download, separate roundings (no fmaf).
 *  3. motion.  r = U(e, 2k); c = +0, then for i = 0..8 c = c + T[s][u][i]
 *     (fp32): the first i with T[s][u][i] > 0 and r < c, else i = 4; s moves
 *     by (i%3 - 1, i/3 - 1) (a move off the grid, which no generated model
 *     allows, is not taken).
 *  4. observation.  r = U(e, 2k+1); the same scan over L[s'][0..15], else 15.
 *  5. belief.  raw = pp2_belief_update's unnormalised update of the stored b
 *     by (u, z) (the fmaf chain, then * L_z, flush-to-zero); m = max(raw).
 *     If m is not a finite value > 0: status 2 (belief lost), steps k+1, the
 *     stored belief is raw, stop.  Else e2 = clamp(exponent(m), -126, 126) and
 *     the stored belief is raw * 2^-e2 (exact, flush-to-zero): max in [1, 2).
 *  6. goal.  s' = goal: status 1, steps k+1, stop.  Still running after the
 *     last step: status 0, steps = horizon.
 * Random numbers are counter based: mix = splitmix64's finaliser, Gm =
 * 0x9E3779B97F4A7C15, key_e = mix(seed + Gm*(e+1)), x = mix(key_e + Gm*(d+1)),
 * U(e, d) = float(x >> 40) * 2^-24 (mod 2^64).  An episode depends on
 * (seed, e) only: not on E, the workgroup count or earlier runs.
 * Q planes: once per run from the current J, Q_u[x] = pp2_mdp_sweep's cost of
 * action u (C, then nine fmaf(fl(gamma T_i), J_i, .) in i order, J = 0 off
 * the grid), stored as [u][row][row stride] with pad cells +0.
 * Pinned Q-dot order, over the padded index i = y*stride + x, NP = H*stride
 * (pads add +0): 256 lanes; lane t from +0, for j = 0, 1, .. and k = 0..3 with
 * i = 1024j + 4t + k < NP: acc = acc + fl(b[i] * Q_u[i]); each group of 64
 * lanes folded by the xor butterfly 32, 16, 8, 4, 2, 1; then
 * ((w0 + w1) + w2) + w3.
 *
 * Alpha runs (pp2_episodes_run_alpha): the greedy policy of an alpha-vector
 * set, K vectors alpha_k with an action each -- PP2_ALPHA_FIB: the context's
 * current FIB alphas, K = 9, action of vector k = k (never solved: the zeros,
 * valid); PP2_ALPHA_PBVI: the context's PBVI alpha vectors and their actions,
 * K = S <= 4096.  An alpha run is pp2_episodes_run with step 1 replaced; steps
 * 2-6, the random numbers, the results and the statuses are unchanged, and the
 * cost G still accumulates the MDP cost C[s][u], so all four policies are
 * compared on one scale.
 *  1. control.  V_k = sum_i b[i] alpha_k[i] in the pinned Q-dot order above
 *     with alpha_k in place of Q_u (separate roundings, flush-to-zero, over
 *     the padded planes alpha_k[y*stride + x], pads +0); best = 0, then for
 *     k = 1 .. K-1: if (V_best < V_k) best = k; u = action[best].  So the first
 *     maximum wins, a NaN sum never displaces the incumbent and a NaN V_0 is
 *     never displaced.  Non-finite alpha entries are not rejected: the
 *     arithmetic above defines the result.
 * A run reads the alpha set that is current when it is enqueued (stream
 * ordered, as J and A): once per run it is repacked into planes [K][row][row
 * stride], pads +0, allocated at the first alpha run and regrown when K grows
 * (PP2_ENOMEM if that fails).
 *
 * Lookahead runs (pp2_episodes_run_lookahead): the one-step lookahead policy
 * over an alpha-vector set -- the reference POMDP node's QV-tree at depth 1
 * with the exact observation probabilities as weights,
 *   Q(b, u) = <b, R_u> + gamma * sum_z max_k <L_z . T_u^T b, alpha_k>,
 * where the unnormalised update carries p(z | b, u) as its mass, so nothing is
 * divided.  A lookahead run is pp2_episodes_run_alpha with step 1 replaced;
 * steps 2-6, the random numbers, the results, the statuses and the MDP cost
 * scale are unchanged.  b is the stored belief, dot the pinned Q-dot order
 * above (separate roundings, flush-to-zero, padded planes, pads +0), gamma the
 * context's, and the alpha set (K vectors and their actions) is read and
 * repacked once per run exactly as an alpha run does.
 *  1. control.  For u = 0..8:
 *       rew[u] = dot(b, Rp_u), Rp_u[y*stride + x] = R[y*W + x][u], the POMDP
 *         stage reward of pp2_model_download, pads +0 (repacked once per run
 *         from the context's R planes, as the Q planes are);
 *       for z = 0..15: raw_uz = step 5's unnormalised update of b by (u, z)
 *         (the fmaf chain, then * L_z, flush-to-zero; cells x >= W and pads
 *         +0) -- the bits step 5 stores when (u, z) is the pair that happens;
 *         V_uzk = dot(raw_uz, alpha_k) for k = 0..K-1; i_uz = 0, then for
 *         k = 1..K-1: if (V[i_uz] < V[k]) i_uz = k (the alpha run's rule: the
 *         first maximum wins, NaN never displaces the incumbent);
 *         M_uz = V[i_uz];
 *       S_u = +0, then z ascending: S_u = S_u + M_uz;
 *       Q_u = rew[u] + fl(gamma * S_u) (separate roundings, no fmaf).
 *     best = 0, then for u = 1..8: if (Q_best < Q_u) best = u; the control is
 *     best itself.  The vectors' own actions do not enter the choice (they are
 *     still validated <= 8).  Non-finite alpha entries are not rejected: the
 *     arithmetic above is the definition.
 *
 * The world (pp2_episodes_set_world): a second context that holds the true
 * map, while the batch's own context holds the map the robot believes.  While
 * a world is attached, every run and every resumed segment of the batch, of
 * all six policies and both placements, is the episode above with these
 * changes and no other:
 *  - initial goal test and step 6: the goal is the world's goal cell; a world
 *    goal off the grid means there is none;
 *  - step 2: G = G + fl(d * C_w[s][u]), C_w the world's MDP cost;
 *    d = fl(d * gamma) uses the batch context's gamma -- the world's gamma is
 *    never read;
 *  - steps 3 and 4: the scans run over T_w[s][u][0..8] and L_w[s'][0..15], the
 *    world's; uniforms, thresholds and fall-backs are unchanged;
 *  - steps 1 and 5 are unchanged: they use the batch context's model, J, A,
 *    Q planes, alpha sets, R planes, code plane and tables.
 * Nothing is rejected for being inconsistent (a true cell that the believed
 * map holds occupied, say): the arithmetic above defines the result.  The run
 * reads the world as it stands when the run is enqueued: the launch is ordered
 * after the work already enqueued on the world's stream, and later calls on
 * the world context are ordered after the launch (one event in each direction
 * when the two contexts' streams differ, nothing when they are the same);
 * pending resident launches of the world are settled first, as the batch
 * context's are.  The kernel reads the world's code plane and class tables
 * from device memory, so no workgroup's LDS grows and pp2_episodes_info and
 * every admission limit are those of a run without a world.
 *
 * Resumed segments (pp2_episodes_resume).  Per episode the batch keeps steps,
 * status, cost G, the final cell, the stored belief, and the discount d.  The
 * status is the flag for the kind of the stored belief: a status-2 episode's
 * is the last raw update, every other one's the rescaled raw * 2^-e2 (or b0,
 * for an episode that started on the goal), and a resumed segment never
 * rewrites a finished episode, so a raw belief stays the raw one.  A resumed
 * segment of `horizon` steps, for episode e:
 *  - status != 0: nothing of the episode changes;
 *  - else s = the final cell, b = the stored belief read as it is (it holds
 *    raw * 2^-e2 already: no further scale), G, d and k0 = steps carry over;
 *    the local steps j = 0 .. horizon-1 are the steps 1-6 above with global
 *    step k = k0 + j: the uniforms are U(e, 2k) and U(e, 2k+1) with key_e made
 *    from this call's seed; still running: steps = k0 + horizon; goal reached:
 *    status 1, steps = k + 1; belief lost: status 2, steps = k + 1;
 *  - the traces hold the segment only, indexed by j; the initial goal test
 *    does not apply (k0 > 0 whenever the status is 0).
 * So with one seed and nothing changed in between, a run of h1 steps followed
 * by a resumed segment of h2 equals one run of h1 + h2 steps of a batch with
 * that horizon in every result and belief bit, and the segment's trace rows
 * are rows h1.. of the long run's. */
typedef struct pp2_episodes pp2_episodes;
/* episodes 1..131072, horizon 1..4096; record_trace != 0 keeps the per-step
 * trace.  PP2_ESTATE: no model, a row shard or group member, coded model
 * inactive or not factored.  PP2_EINVAL: the grid does not fit LDS. */
int pp2_episodes_create(pp2_episodes** out, pp2_ctx* ctx, int episodes, int horizon,
                        int record_trace);
int pp2_episodes_destroy(pp2_episodes* ep);
#define PP2_EPISODES_LDS    0  /* pp2_episodes_create's behaviour: planes in LDS, PP2_EINVAL if they do not fit */
#define PP2_EPISODES_GLOBAL 1  /* planes in device memory, any grid the context supports */
#define PP2_EPISODES_AUTO   2  /* per launch: LDS if that launch's LDS layout fits, else device memory */
/* pp2_episodes_create with a placement of the belief planes ("Placement"
 * above); pp2_episodes_create is placement PP2_EPISODES_LDS.  Every check of
 * pp2_episodes_create holds, except that PP2_EPISODES_GLOBAL and
 * PP2_EPISODES_AUTO do not refuse a grid for its LDS size.  PP2_EINVAL: an
 * unknown placement. */
int pp2_episodes_create_placed(pp2_episodes** out, pp2_ctx* ctx, int episodes, int horizon,
                               int record_trace, int placement);
/* requested placement, placement of the last launch (-1 before any run),
 * bytes of device scratch held for the global planes (0 until first needed); any may be NULL */
int pp2_episodes_placement(pp2_episodes* ep, int* requested, int* last, long long* scratch_bytes);
/* b0: hw floats, every entry finite and >= +0; start_cells: [episodes] in
 * [0, hw) (else PP2_EINVAL).  Settles pending work of the context first and
 * re-checks its model, then reads the current J and A.  Asynchronous. */
int pp2_episodes_run(pp2_episodes* ep, int policy, uint64_t seed, const float* b0,
                     const int32_t* start_cells);
/* [episodes] each, any may be NULL: steps taken, status (0 horizon reached,
 * 1 goal reached, 2 belief lost), discounted cost G, the last true cell.
 * Synchronises. */
int pp2_episodes_results(pp2_episodes* ep, int32_t* steps, uint8_t* status, float* cost,
                         int32_t* final_cell);
/* The last run's trace, [horizon][episodes] (qsums [horizon][episodes][9]),
 * any may be NULL: action, observation, true cell after the move, the S_u
 * (PP2_CONTROL_QMDP runs only), the mode cell (PP2_CONTROL_MODE runs only).
 * Steps not taken hold 255, 255, -1, 0, -1.  PP2_ESTATE without record_trace. */
int pp2_episodes_trace(pp2_episodes* ep, uint8_t* actions, uint8_t* observations,
                       int32_t* cells, float* qsums, int32_t* mode_cells);
/* the stored belief of one episode after the run (hw floats) */
int pp2_episodes_get_belief(pp2_episodes* ep, int episode, float* belief);
/* the Q planes of the last run as Q[hw][9]; PP2_ESTATE after an alpha run,
 * which builds none */
int pp2_episodes_get_q(pp2_episodes* ep, float* Q);
/* LDS bytes per workgroup, workgroups and threads per workgroup of the last
 * launch (before any run: of a MODE / QMDP launch; an alpha launch adds its
 * scratch for K != 9, a lookahead launch its own; a device-memory launch
 * keeps only the tables, the reduction scratch and that launch's alpha or
 * lookahead scratch in LDS and reports that, and its own workgroups) */
int pp2_episodes_info(pp2_episodes* ep, int* lds_bytes, int* workgroups, int* threads);
#define PP2_ALPHA_FIB  0   /* the context's current FIB alphas: K = 9, action of vector k = k */
#define PP2_ALPHA_PBVI 1   /* the context's PBVI alpha vectors and their actions: K = S */
/* pp2_episodes_run with the alpha-vector policy ("Alpha runs" above); b0 and
 * start_cells as there.  PP2_EINVAL: unknown alpha_set, a PBVI action > 8, or
 * the workgroup's LDS with the alpha scratch does not fit (all before any
 * launch); PP2_ESTATE: PP2_ALPHA_PBVI without alpha vectors.  Afterwards
 * pp2_episodes_trace returns actions, observations and cells as usual, qsums
 * = the nine V_k (FIB runs; 0 for PBVI runs) and mode_cells = -1.
 * Asynchronous. */
int pp2_episodes_run_alpha(pp2_episodes* ep, int alpha_set, uint64_t seed, const float* b0,
                           const int32_t* start_cells);
/* [horizon][episodes], either may be NULL: index of the winning vector and its
 * sum; steps not taken: -1, 0.  PP2_ESTATE unless the last run was an alpha
 * run, or without record_trace. */
int pp2_episodes_trace_alpha(pp2_episodes* ep, int32_t* best_index, float* best_sum);
/* the alpha set the last alpha or lookahead run read: *count = K; alphas
 * [K][hw], actions [K]; any may be NULL.  PP2_ESTATE unless the last run was
 * an alpha or a lookahead run. */
int pp2_episodes_get_alpha(pp2_episodes* ep, int* count, float* alphas, uint8_t* actions);
/* pp2_episodes_run with the one-step lookahead policy over an alpha set
 * ("Lookahead runs" above): arguments, checks, statuses and asynchrony are
 * those of pp2_episodes_run_alpha; PP2_EINVAL before any launch also when the
 * workgroup's LDS with the lookahead scratch does not fit -- also on a
 * PP2_EPISODES_AUTO batch -- and on every PP2_EPISODES_GLOBAL batch: the
 * lookahead runs from LDS planes only.  Afterwards
 * pp2_episodes_trace returns actions, observations and cells as usual, qsums =
 * the nine Q_u and mode_cells = -1; pp2_episodes_get_alpha answers with the
 * set read; pp2_episodes_trace_alpha and pp2_episodes_get_q return PP2_ESTATE;
 * pp2_episodes_info reports the lookahead launch (its scratch added). */
int pp2_episodes_run_lookahead(pp2_episodes* ep, int alpha_set, uint64_t seed, const float* b0,
                               const int32_t* start_cells);
/* pp2_episodes_run_lookahead following the batch's placement ("Placement"
 * above) the way every other run does: the same arithmetic ("Lookahead
 * runs"), arguments, checks, statuses and asynchrony, the same bits.  A
 * PP2_EPISODES_LDS batch runs it from LDS exactly as the call above (PP2_EINVAL
 * if the layout with the lookahead scratch does not fit); a
 * PP2_EPISODES_GLOBAL batch always runs it from device memory; a
 * PP2_EPISODES_AUTO batch from LDS if the lookahead layout fits, else from
 * device memory.  A device-memory launch keeps the tables, the reduction
 * scratch and the lookahead scratch (4096 bytes) in LDS, uses the batch's
 * scratch (allocated at the first launch that needs it: PP2_ENOMEM if that
 * fails, the batch stays usable) and min(episodes, workgroups that scratch
 * holds, CUs x 2) workgroups; pp2_episodes_placement then reports last =
 * PP2_EPISODES_GLOBAL and pp2_episodes_info that launch.  Afterwards
 * pp2_episodes_trace, pp2_episodes_trace_lookahead, pp2_episodes_get_alpha,
 * pp2_episodes_get_belief and pp2_episodes_results behave as after the call
 * above. */
int pp2_episodes_run_lookahead_placed(pp2_episodes* ep, int alpha_set, uint64_t seed,
                                      const float* b0, const int32_t* start_cells);
/* The last lookahead run's trace, any may be NULL: q and rewards
 * [horizon][episodes][9] (Q_u, rew[u]); leaf_max and leaf_index
 * [horizon][episodes][9][16] (M_uz, i_uz).  Steps not taken hold 0, 0, 0, -1.
 * PP2_ESTATE unless the last run was a lookahead run with record_trace.  The
 * two large arrays are allocated at the first lookahead run of a tracing batch
 * (PP2_ENOMEM if that fails), never at create. */
int pp2_episodes_trace_lookahead(pp2_episodes* ep, float* q, float* rewards, float* leaf_max,
                                 int32_t* leaf_index);
/* Attach the world ("The world" above) that every later run and resumed
 * segment of the batch simulates; NULL detaches, which is the behaviour of a
 * fresh batch.  world may be the batch's own context.  PP2_EINVAL: world is a
 * row shard or group member, on another device than the batch's context, or
 * of another height or width.  The batch keeps a plain pointer: detach, or
 * destroy the batch, before destroying world -- the rule that holds for the
 * batch's own context.  At every run, before any launch, world must satisfy
 * what pp2_episodes_create demands of the batch's context except the LDS size
 * -- a model, an active dictionary-coded model with factored rows and
 * non-negative T and L -- else PP2_ESTATE, the message naming the world. */
int pp2_episodes_set_world(pp2_episodes* ep, pp2_ctx* world);
#define PP2_EPISODE_MODE 0
#define PP2_EPISODE_QMDP 1
#define PP2_EPISODE_FIB 2
#define PP2_EPISODE_PBVI 3
#define PP2_EPISODE_FIB_LOOKAHEAD 4
#define PP2_EPISODE_PBVI_LOOKAHEAD 5
/* Continue every episode of the batch for another `horizon` steps from the
 * state the previous run or resumed segment left it in ("Resumed segments"
 * above) under a PP2_EPISODE_* policy.  Follows the placement as
 * pp2_episodes_run_lookahead_placed does and makes all the checks of the
 * corresponding run; PP2_ESTATE before any run of the batch, PP2_EINVAL for an
 * unknown policy.  Reads the J, A, alpha set, models and world that are
 * current when it is enqueued: between two segments the caller may call
 * pp2_map_update, re-solve, or attach another world.  Afterwards the results,
 * beliefs and traces are read as after the corresponding run.  Asynchronous. */
int pp2_episodes_resume(pp2_episodes* ep, int policy, uint64_t seed);

/* ---------------------------------------------------------------- shortest-path field
 * The A* node's baseline (src/astar/path_planning_2d.cpp:109-160 of the
 * reference: the first step of the shortest 8-connected path from the
 * belief's mode to the goal) as a goal-rooted field over the map in force
 * (pp2_map_get's, 1 = occupied) and the context's goal (gx, gy); it needs no
 * model.  DESIGN.md §2.3.
 *
 * Move u in {0..8} \ {4} displaces by (u%3 - 1, u/3 - 1), the action raster of
 * every other call.  Axis moves cost c_u = 1.0f, diagonal moves
 * c_u = 0x1.6a09e6p+0f (fp32 sqrt 2, bits 0x3fb504f3).  A move is allowed iff
 * its target cell is on the grid and free; a diagonal does not look at the two
 * cells it passes between (the generated model's T has the same rule).
 *   D(goal) = +0 if the goal is on the grid and free;
 *   occupied cells hold +inf (an occupied goal too);
 *   every other free cell x holds D(x) = min over allowed u of
 *     fl32(D(x + off_u) + c_u), +inf where no neighbour is finite
 *     (plain fp32 add, round to nearest, no contraction);
 *   A_path(x): scan u = 0,1,2,3,5,6,7,8 from +inf with strict < over
 *     fl32(D(x + off_u) + c_u), the first minimum wins; A_path = 4 at the goal,
 *     at occupied cells and at cells with D = +inf.
 * A goal off the grid or occupied gives all +inf and all 4: a valid, converged
 * field with reached = 0.  fl32(a + c) > a for c >= 1 and a < 2^24, so the
 * equations have one solution (Dijkstra's with the same add) and every
 * relaxation order from +inf ends on the same bits; H * W <= 2^23 keeps
 * D < 2^24 (pp2_path_solve: PP2_EINVAL above).
 *
 * pp2_path_solve: always starts cold; rounds of a tiled relaxation enqueued on
 * the context's stream in batches, one synchronising poll of a pinned word per
 * batch.  max_rounds < 1: PP2_EINVAL.  Not settled within max_rounds: PP2_OK
 * with *converged = 0, and the field stays invalid.  rounds = the rounds up to
 * and including the first that lowered nothing across a tile border (or
 * max_rounds); reached = the cells with finite D (0 unless converged).  The
 * planes are allocated at the first call (PP2_ENOMEM if that fails: the
 * context stays usable) and freed by pp2_destroy.  A row shard, RCCL rank or
 * group member: PP2_ESTATE.  Output pointers may be NULL.
 *
 * The field is valid after a converged solve or resolve until a
 * pp2_map_update changes a cell's occupancy or a pp2_goal_set changes the
 * goal.  pp2_path_get, pp2_path_control and pp2_path_trace return PP2_ESTATE
 * without a valid field.
 *
 * pp2_path_resolve: the field of the map and goal in force, the same bits as
 * pp2_path_solve's, repaired from the converged field the planes still hold.
 * pp2_map_update keeps the bounding box of the cells whose occupancy it
 * changed (16 boxes at most) and pp2_goal_set notes a moved goal.  Relaxation
 * alone cannot follow an added obstacle, because it never raises a value; so
 * the cells of the boxes are compared with the map (seed), every value whose
 * old A_path chain runs through a cell that is occupied now is set to +inf in
 * raise rounds, and the relaxation's rounds repair the hole from the tiles
 * that lost or gained a cell; then A_path and reached over the whole grid.
 * *warm = 1 when that path served the call, 0 when the call did exactly what
 * pp2_path_solve does: no converged field in the planes (never solved, or the
 * last solve or resolve ended unconverged), the goal moved, the goal cell's
 * occupancy is not what it was at field time, or more than 16 boxes pending.
 * With a valid field it returns at once without a launch: rounds = 0,
 * converged = 1, the stored reached, warm = 1.  The first five arguments have
 * pp2_path_solve's contract; max_rounds bounds the raise rounds and the
 * relaxation rounds separately, and rounds is their sum.
 * pp2_path_resolve_info, of the last resolve: warm; raised = the cells that
 * were finite, are still free and were raised (the newly occupied cells
 * themselves are not counted: a function of the old field and the new map
 * alone); the rounds of each phase (raise_rounds = 0 when no finite cell
 * became occupied; a cold fall-back reports its rounds as relax_rounds); the
 * cells the seed pass visited.  Any pointer may be NULL.
 *
 * pp2_path_get: D and A_path as [H*W] arrays, either may be NULL.
 * pp2_path_control: the A* node's beliefCallback: cell = pp2_belief_mode's,
 * action = A_path[cell], dist = D[cell]; dist and cell may be NULL.
 * pp2_path_trace: follows A_path from start_cell (a host copy of the table,
 * cached per solve): cells = start ... goal inclusive, *n their count,
 * *length = D[start].  An occupied or unreachable start: *n = 0, PP2_OK.
 * cap < n: PP2_EINVAL with *n set to the count needed.  cells may be NULL
 * when cap is 0; length may be NULL.
 * pp2_path_info: whether the field is valid; rounds, kernel launches and
 * polls of the last solve or resolve (every kernel of the call counts); the
 * relaxation's tile (compile-time constants).  Any pointer may be NULL. */
int pp2_path_solve(pp2_ctx* ctx, int max_rounds, int* rounds, int* converged, int* reached);
int pp2_path_resolve(pp2_ctx* ctx, int max_rounds, int* rounds, int* converged, int* reached,
                     int* warm);
int pp2_path_resolve_info(pp2_ctx* ctx, int* warm, int* raised, int* raise_rounds,
                          int* relax_rounds, int* seed_cells);
int pp2_path_get(pp2_ctx* ctx, float* D, uint8_t* A);
int pp2_path_control(pp2_ctx* ctx, uint8_t* action, float* dist, int32_t* cell);
int pp2_path_trace(pp2_ctx* ctx, int32_t start_cell, int32_t* cells, int cap, int* n,
                   float* length);
int pp2_path_info(pp2_ctx* ctx, int* valid, int* rounds, int* launches, int* polls,
                  int* tile_rows, int* tile_cols);
/* The action table step 1 of a MODE run or resumed MODE segment reads at the
 * belief's mode: the MDP's A (the default, today's behaviour exactly) or the
 * field's A_path of the batch's context -- in both placements, with or
 * without a world (the table is the believed map's either way).  The setting
 * belongs to the batch, as pp2_episodes_set_world's; every other policy
 * ignores it, and the traces are a MODE run's.  Under PP2_TABLE_PATH a MODE
 * run or resumed MODE segment without a valid field returns PP2_ESTATE before
 * any launch.  An unknown table: PP2_EINVAL. */
#define PP2_TABLE_MDP  0
#define PP2_TABLE_PATH 1
int pp2_episodes_set_action_table(pp2_episodes* ep, int table);

/* ---------------------------------------------------------------- policy evaluation
 * The exact outcome fields of a fixed action table: for a robot that knows
 * its cell, follows table pi and moves in a given world, per start cell the
 * expected discounted cost G, the probability P of reaching the goal within
 * the horizon and the expected number of steps N -- the fully observed
 * counterparts of an episode's cost, status == 1 and steps, on the same cost
 * scale, for every start cell at once and without sampling.  The recurrence is
 * the reference's cudaOneStepPolicyEvaluation (src/mdp/
 * path_planning_2d_cuda.cu:266-306) with an absorbing goal, run for a fixed
 * horizon; P and N ride along on the raw T.
 *
 * Inputs.  ctx holds the believed map and pi.  world holds the model the
 * robot moves in (NULL: ctx itself): unsharded, with a model, on ctx's
 * device and of ctx's geometry (PP2_EINVAL, as pp2_episodes_set_world), its
 * gamma equal to ctx's as fp32 bits (PP2_EINVAL: the world's coded sweep rows
 * hold fl(gamma * T) for its own gamma, so one gamma keeps both routes on the
 * same operands).  T_w and C_w are the world's planes as pp2_model_download
 * returns them; the goal is the world's goal cell, and a goal off the grid
 * means there is none.  pi is
 *   PP2_TABLE_MDP   the context's A as it stands when the call is enqueued
 *                   (all zeros after pp2_mdp_reset, which is valid),
 *   PP2_TABLE_PATH  A_path (PP2_ESTATE without a valid field),
 *   PP2_TABLE_USER  the table last given to pp2_policy_set_table (PP2_ESTATE
 *                   if none was given).
 *
 * Start planes: G_0 = N_0 = +0 everywhere; P_0 = 1.0f at the goal, +0 elsewhere.
 * Step k = 1 .. horizon, for every grid cell x, with u = pi[x] and
 * off_i = (i % 3 - 1, i / 3 - 1); a neighbour off the grid reads +0:
 *   x is the goal:  G_k = +0, P_k = 1.0f, N_k = +0 (absorbing, as episode
 *                   step 6);
 *   otherwise:      g = C_w[x][u];
 *                   for i = 0..8: g = fmaf(fl(gamma * T_w[x][u][i]), G_{k-1}(x + off_i), g)
 *                     (pp2_mdp_sweep's arithmetic for the one action u)
 *                   p = +0;
 *                   for i = 0..8: p = fmaf(T_w[x][u][i], P_{k-1}(x + off_i), p)
 *                   n = 1.0f;
 *                   for i = 0..8: n = fmaf(T_w[x][u][i], N_{k-1}(x + off_i), n)
 * All arithmetic is fp32 and flush-to-zero (subnormal operands read as zero,
 * subnormal results are flushed: a result is rounded to nearest even first and
 * flushed if what the rounding gives is subnormal, so an exact value just
 * below 2^-126 that rounds up to it stays).  Nothing but the goal is special-cased:
 * occupied cells, cells where the table says 4 and a true cell that the
 * believed map holds occupied all follow the arithmetic.  The outputs are
 * G_H, P_H and N_H as [H*W] arrays.
 *
 * Routes.  Each step is a pure function of the previous planes, so tiling,
 * the steps a launch runs and redundant ring computation cannot change a bit:
 * both routes return identical bits.
 *   PP2_POLICY_PLANES  one launch per step from the world's dense T and C
 *                      planes; any model, uploaded ones without a dictionary
 *                      included.  block is ignored.
 *   PP2_POLICY_TILES   the world's dictionary-coded model, a tile of the three
 *                      planes kept in LDS with a ring `block` cells deep,
 *                      `block` steps per launch (0: default_block).
 *                      PP2_ESTATE unless the world's coded model is active with
 *                      factored rows (pp2_model_dict_info) and every T row of
 *                      its dictionary sums to at most 1 + 2^-20 (generated
 *                      models always qualify): the route drops the T == +0
 *                      terms, which is exact while every value is finite.
 *   PP2_POLICY_AUTO    TILES when admissible, else PLANES.
 *
 * pp2_policy_set_table: table is [H*W], every entry <= 8 (else PP2_EINVAL,
 * the earlier table kept); copied before the call returns.  NULL drops it.
 * pp2_policy_evaluate: horizon in 1 .. 65536, block in 0 .. max_block; an
 * unknown table or route or anything out of range is PP2_EINVAL.  A row
 * shard, RCCL rank or group member, as ctx or as world: PP2_ESTATE.
 * Asynchronous on ctx's stream: it first settles pending resident launches
 * of both contexts and re-checks the models (as pp2_episodes_run), and orders
 * itself against the world's stream with one event each way when the streams
 * differ.  Planes and scratch are allocated by the first evaluation
 * (PP2_ENOMEM leaves the context usable) and freed by pp2_destroy.  The
 * result is a snapshot: later map updates, sweeps or solves do not invalidate
 * it, and the next evaluation replaces it.  No belief, value, action table or
 * alpha vector of either context is written.
 * pp2_policy_get: G, P and N as [H*W] arrays, any may be NULL; synchronises.
 * PP2_ESTATE before any evaluation.
 * pp2_policy_info: what the result was computed from (valid, table, horizon,
 * the route taken, steps per launch, kernels launched) and the TILES route's
 * compile-time constants.  Any pointer may be NULL. */
#define PP2_TABLE_USER 2
#define PP2_POLICY_AUTO   0
#define PP2_POLICY_PLANES 1
#define PP2_POLICY_TILES  2
int pp2_policy_set_table(pp2_ctx* ctx, const uint8_t* table);
int pp2_policy_evaluate(pp2_ctx* ctx, pp2_ctx* world, int table, int horizon, int route,
                        int block);
int pp2_policy_get(pp2_ctx* ctx, float* G, float* P, float* N);
int pp2_policy_info(pp2_ctx* ctx, int* valid, int* table, int* horizon, int* route_taken,
                    int* block, int* launches, int* tile_rows, int* tile_cols,
                    int* default_block, int* max_block);

/* ---------------------------------------------------------------- occupancy
 * The forward occupancy of an action table: where a robot that knows its
 * cell, follows table pi and moves in a given world is after k steps from a
 * start distribution b0, which cells it passes through and how often, and how
 * the probability of having arrived grows step by step.  The adjoint of the
 * policy evaluation above: with P_H and N_H of pp2_policy_evaluate for the
 * same table, world and horizon H,
 *   <b0, P_H> = D_H(goal) = curve[H]   and   <b0, N_H> = sum over cells of V_H
 * in exact arithmetic (the fp32 results agree to the roundings of H steps).
 *
 * Inputs.  ctx, world (NULL: ctx itself), the table (PP2_TABLE_MDP / _PATH /
 * _USER) and their conditions are pp2_policy_evaluate's: the same geometry,
 * device and gamma-bits checks (PP2_EINVAL), the same PP2_ESTATE cases and the
 * same shard refusal.  The goal is the world's goal; a goal off the grid
 * means there is none.  off_i = (i % 3 - 1, i / 3 - 1), and T_w is the
 * world's T as pp2_model_download returns it.
 * b0 is [H*W] floats, copied before the call returns.  Every entry must
 * satisfy 0 <= e <= 1.0f and must not be NaN, else PP2_EINVAL, and the
 * earlier result stays untouched; -0 and subnormals are read as +0.  b0 need
 * not sum to 1.
 *
 * Start planes: D_0 = b0 after that canonicalisation, V_0 = +0;
 * curve[0] = D_0(goal), or +0 if there is no goal.
 * Step k = 1 .. horizon: let S(x) = D_{k-1}(x) for x off the goal and
 * S(goal) = +0; a source off the grid reads +0.  For every grid cell y:
 *   V_k(y) = V_{k-1}(y) + S(y)       (one fp32 add: the expected visits
 *                                     before arrival; the goal holds +0)
 *   d = D_{k-1}(y) if y is the goal, else +0;
 *   for i = 0..8, with x = y - off_i:
 *     d = fmaf(T_w[x][pi[x]][i], S(x), d)
 *       (the mass that source x sends to its neighbour i, which is y; the
 *        goal absorbs: it keeps its mass and sends none)
 *   D_k(y) = d
 *   curve[k] = D_k(goal)
 * All arithmetic is fp32 and flush-to-zero, as in the evaluator.  Nothing but
 * the goal is special-cased: occupied cells, mass placed on occupied cells
 * and table entries of 4 all follow the arithmetic.  The outputs are D_H
 * [H*W], V_H [H*W] and curve [horizon + 1].
 *
 * Routes.  Each step is a pure function of the previous planes, so tiling,
 * the steps a launch runs and redundant ring computation cannot change a bit:
 * both routes return identical bits.
 *   PP2_OCC_PLANES  any model, uploaded ones without a dictionary included:
 *                   the nine gather weights of every cell, T_w[x][pi[x]][i]
 *                   with x = y - off_i (+0 for a source off the grid or the
 *                   goal), are materialised once per evaluation into nine
 *                   [H*W] planes; then one launch per step.  block is ignored.
 *   PP2_OCC_TILES   the world's dictionary-coded model, a tile of D kept in
 *                   LDS with a ring `block` cells deep, `block` steps per
 *                   launch (0: default_block), the gather weights and V of a
 *                   thread's cells in registers across a launch's steps.
 *                   PP2_ESTATE unless PP2_POLICY_TILES would be admitted in
 *                   the same world (coded model active with factored rows,
 *                   every dictionary T row summing to at most 1 + 2^-20): the
 *                   route multiplies by +0 where the definition skips a
 *                   source, which is exact while every value is finite --
 *                   D(y) <= sum(b0) * (1 + 2^-20)^horizon.
 *   PP2_OCC_AUTO    TILES when admissible, else PLANES.
 *
 * pp2_occupancy_evaluate: horizon in 1 .. 65536, block in 0 .. max_block; a
 * NULL b0, an unknown table or route or anything out of range is PP2_EINVAL.
 * Asynchronous on ctx's stream, with pp2_policy_evaluate's settling, model
 * re-check and stream ordering (one event each way when the world's stream
 * differs).  Planes and scratch are allocated on first use (PP2_ENOMEM leaves
 * the context usable) and freed by pp2_destroy.  The result is a snapshot
 * that the next occupancy evaluation replaces; its storage is separate from
 * the policy evaluation's, so neither call disturbs the other's *_get.  No
 * belief, value, action table or alpha vector of either context is written.
 * pp2_occupancy_get: D and V as [H*W], curve as [horizon + 1] of the last
 * evaluation, any may be NULL; synchronises.  PP2_ESTATE before any evaluation.
 * pp2_occupancy_info: as pp2_policy_info.  launches counts the kernels of the
 * last evaluation: the start planes, the class bytes (TILES) or the weight
 * planes (PLANES), and ceil(horizon / block) step launches (block = 1 under
 * PLANES).  Any pointer may be NULL. */
#define PP2_OCC_AUTO   0
#define PP2_OCC_PLANES 1
#define PP2_OCC_TILES  2
int pp2_occupancy_evaluate(pp2_ctx* ctx, pp2_ctx* world, int table, const float* b0,
                           int horizon, int route, int block);
int pp2_occupancy_get(pp2_ctx* ctx, float* D, float* V, float* curve);
int pp2_occupancy_info(pp2_ctx* ctx, int* valid, int* table, int* horizon, int* route_taken,
                       int* block, int* launches, int* tile_rows, int* tile_cols,
                       int* default_block, int* max_block);

/* ---------------------------------------------------------------- shards
 * Two transports for row shards (no reference counterpart):
 *  - one process per GPU: RCCL (pp2_rccl_unique_id / pp2_shard_comm_init);
 *    then every per-context call exchanges its halos itself;
 *  - one process driving several shard contexts (one or more devices): a
 *    shard group, whose pp2_shard_group_* calls run each step phase-wise
 *    over all shards, moving halo rows and the belief mass with device
 *    copies.  Grouped contexts reject the per-context stepping calls. */
typedef struct pp2_shard_group pp2_shard_group;
/* ctxs[i] must be the shards of one grid in row order (pp2_create_shard). */
int pp2_shard_group_create(pp2_shard_group** out, pp2_ctx* const* ctxs, int n);
int pp2_shard_group_destroy(pp2_shard_group* g);
int pp2_shard_group_loop_step(pp2_shard_group* g, uint8_t u, uint8_t z);
/* n loop steps (pp2_loop_run's contract): pairs of steps of a halo block per
 * launch on every shard where PP2_TUNE_STEP_PAIRS applies, else single steps. */
int pp2_shard_group_loop_run(pp2_shard_group* g, int n, const uint8_t* us, const uint8_t* zs);
int pp2_shard_group_belief_update(pp2_shard_group* g, uint8_t u, uint8_t z);
int pp2_shard_group_mdp_sweep(pp2_shard_group* g, int n);
int pp2_shard_group_mdp_solve(pp2_shard_group* g, int max_sweeps, int* sweeps,
                              double* final_norm);
int pp2_shard_group_fib_sweep(pp2_shard_group* g, int n);
int pp2_shard_group_synchronize(pp2_shard_group* g);

/* RCCL bootstrap for row shards (no reference counterpart).  Rank 0 calls
 * pp2_rccl_unique_id, the 128 bytes are broadcast out of band, then every
 * rank calls pp2_shard_comm_init with its own shard context. */
#define PP2_RCCL_ID_BYTES 128
int pp2_rccl_unique_id(uint8_t id[PP2_RCCL_ID_BYTES]);
int pp2_shard_comm_init(pp2_ctx* ctx, const uint8_t id[PP2_RCCL_ID_BYTES],
                        int nranks, int rank);

#ifdef __cplusplus
}
#endif
#endif /* PP2_H */
