/* dat.h -- C-ABI of the MI355X batched agent-QP solver (libdat.so).
 *
 * Drop-in boundary for the reference's controller hot path.  In the reference
 * (AkshayThiru/distributed-aerial-transportation) the plug-in point is the cvxpy solver
 * backend: control/rqp_cadmm.py:16-17 (_RQPCDMM_SOLVER = cv.CLARABEL), control/rqp_dd.py:17-18
 * (_RQPDD_SOLVER) and control/rqp_centralized.py:132,440 (cv.CLARABEL literal), called once per
 * agent QP from RQPPrimalSolver.solve (control/rqp_cadmm.py:482-501, control/rqp_dd.py:475-505)
 * and RQPCentralizedController.control (control/rqp_centralized.py:436-448).  This library
 * replaces that per-call path with batched calls over B independent scenarios; the Python
 * controller classes in distributed_aerial_transportation_amd/control.py keep the reference
 * constructor and control(state, acc_des) signatures on top of it.
 *
 * Conventions: fp64 everywhere; caller-owned, C-contiguous host buffers, read/written only
 * during the call; block layouts in distributed_aerial_transportation_amd/csrc/dat_layout.h;
 * return 0 on success, < 0 on error (message via dat_last_error()); no C++ exceptions cross
 * the ABI.  A handle is bound to one HIP device and one stream and is not re-entrant.
 */
#ifndef DAT_H
#define DAT_H

#ifdef __cplusplus
extern "C" {
#endif

#define DAT_MODE_CENTRALIZED 0 /* RQPCentralizedController  control/rqp_centralized.py:27-455 */
#define DAT_MODE_CADMM 1       /* RQPCADMMController         control/rqp_cadmm.py:510-688    */
#define DAT_MODE_DD 2          /* RQPDDController            control/rqp_dd.py:558-764       */

/* low-level SO(3) attitude law of RQPLowLevelController(so3_controller_type, ...)
 * (control/rqp_centralized.py:457-484) */
#define DAT_LL_PD 0 /* "pd": so3_pd_tracking_control  utils/so3_tracking_controllers.py:18-43 */
#define DAT_LL_SM 1 /* "sm": so3_sm_tracking_control  utils/so3_tracking_controllers.py:52-95 */

/* per agent-QP status (maps the cvxpy/Clarabel outcomes the reference branches on) */
#define DAT_QP_OPTIMAL 0    /* accepted                         (prob.status == OPTIMAL)        */
#define DAT_QP_INACCURATE 1 /* previous solution held           (non-OPTIMAL status)            */
#define DAT_QP_INFEASIBLE 2 /* previous solution held           (non-OPTIMAL status)            */
#define DAT_QP_FAILED 3     /* equilibrium forces used          (solver exception, :491-494)    */

typedef struct dat_handle dat_handle;

typedef struct dat_config {
  int device;        /* HIP device ordinal                                               */
  int mode;          /* DAT_MODE_*                                                       */
  int n;             /* quadrotors per payload (3 <= n <= 16)                            */
  int batch;         /* number of independent scenarios B                                */
  double dt;         /* simulation step [s] (example/rqp_example.py:85: 1e-3)            */
  int hl_every;      /* simulation steps per high-level step (rqp_example.py:86: 10)     */
  int max_iter;      /* ADMM/DD max_iter (control/rqp_cadmm.py:563: 100)                 */
  double res_tol;    /* ADMM/DD residual tolerance (control/rqp_cadmm.py:561: 1e-2)      */
  int use_total_res; /* C-ADMM residual kind (control/rqp_cadmm.py:562: 1)               */
  double rho0, tau_incr, rho_max; /* C-ADMM penalty schedule (control/rqp_cadmm.py:565-567) */
  int record_err;    /* keep per-iteration residual sequences (SolverStatistics.err_seq) */
} dat_config;

/* ---- lifecycle ------------------------------------------------------------------------- */
/* dat_create replaces the controller constructors (RQPCADMMController.__init__
 * control/rqp_cadmm.py:513-538, RQPDDController.__init__ control/rqp_dd.py:561-586,
 * RQPCentralizedController.__init__ control/rqp_centralized.py:46-132): it allocates the
 * persistent warm state the reference keeps in Python objects (f, f_mean, lambda
 * control/rqp_cadmm.py:569-580; lambda_F, lambda_M control/rqp_dd.py:618-632; prev_f). */
void dat_default_config(dat_config* cfg);
int dat_create(const dat_config* cfg, dat_handle** out);
int dat_destroy(dat_handle* h);
const char* dat_last_error(void); /* thread-local message of the last failing call */
int dat_device_count(void);

/* ---- problem data ------------------------------------------------------------------------ */
/* params: per_scenario ? B x DAT_PARAM_SIZE(n) : DAT_PARAM_SIZE(n) (broadcast).  The block holds
 * RQPParameters' derived fields (system/rigid_quadrotor_payload.py:48-84), f_eq
 * (_set_system_constants, control/rqp_cadmm.py:142-190) and the controller constants
 * (_set_controller_constants, control/rqp_cadmm.py:192-236, rqp_centralized.py:182-225).
 * Resets the warm state to the constructor's (f = f_eq, lambda = 0). */
int dat_set_params(dat_handle* h, const double* params, int per_scenario);
/* forests: num_forests layouts; tree_offsets[num_forests+1] index rows of tree_pos (T x 3; the handle keeps each forest sorted by x);
 * scenario_forest[B] selects a layout per scenario (NULL: all use layout 0, -1: no env);
 * mountain[num_forests x DAT_MOUNTAIN_SIZE] for the desired-acceleration law.  num_forests = 0
 * removes the environment (env = None in the reference). */
/* Replaces the env object handed to the controllers (Forest, example/env_forest.py:35-85) and the
 * hppfcl queries made through it (centralized_distance / distributed_distance :139-212). */
int dat_set_forests(dat_handle* h, int num_forests, const int* tree_offsets, const double* tree_pos,
                    const int* scenario_forest, const double* mountain);
/* set_force_err_tolerance: control/rqp_cadmm.py:683-685, control/rqp_dd.py:760-761 */
int dat_set_tolerance(dat_handle* h, double res_tol, int use_total_res);
/* Stopping tolerance of every agent / centralized QP's interior-point solve (default 1e-10).  The
 * reference solves with Clarabel's default settings (prob.solve(solver=CLARABEL), control/rqp_cadmm.py:492,
 * control/rqp_dd.py:485, control/rqp_centralized.py:440: tol_gap_abs = tol_gap_rel = tol_feas = 1e-8);
 * 1e-8 here is that tolerance.  tol in [1e-12, 1e-7] (the north_star residual bound), else an error. */
int dat_set_qp_tolerance(dat_handle* h, double tol);
/* set_max_iter: control/rqp_cadmm.py:687-688, control/rqp_dd.py:763-764 */
int dat_set_max_iter(dat_handle* h, int max_iter);
/* _set_warm_start: control/rqp_cadmm.py:577-580, control/rqp_dd.py:628-632 */
int dat_reset_warm_start(dat_handle* h);

/* ---- state ------------------------------------------------------------------------------ */
int dat_set_state(dat_handle* h, const double* state /* B x DAT_STATE_SIZE(n) */, const int* counters /* B or NULL */);
int dat_get_state(dat_handle* h, double* state, int* counters);

/* ---- checkpoints: scenarios with their controllers' warm state ------------------------------------------------
 * dat_set_state / dat_get_state move the rigid-body state and the polar counter; a scenario's next control step
 * also reads what the reference keeps in its controller objects between calls -- C-ADMM f, f_mean, lambda_f
 * (control/rqp_cadmm.py:569-580), DD lambda_F, lambda_M and the agents' previous (f_i, F_i, M_i)
 * (control/rqp_dd.py:618-632), the centralized prev_f -- and, with no reference counterpart, the forces the rollout
 * applies (f_des) and the previous step's pass count and slowest IPM count, from which the kernels take the IPM
 * start regime, the drain order and the tail rule.  A checkpoint record is all of that for one scenario
 * (csrc/dat_layout.h, DAT_CK_*); a blob is a header of DAT_CK_HEADER_BYTES and `count` records.  Parameters,
 * forests, the clock and the tracking records (dat_set_clock, dat_set_tracking: handle settings, like parameters),
 * tolerances, schedule switches, work counters, the log and a step's outputs (qp_status, min_env_dist,
 * collision, err_seq) are not part of it.  A scenario's arithmetic depends on neither its batch, its slot nor the
 * schedule, so a record restored into any slot of any handle of the same mode and n (with the same parameters,
 * forest and settings) continues bitwise as the scenario it was taken from.
 *
 * dat_checkpoint_bytes: the size of a blob of `count` records of this handle.
 * dat_checkpoint_save: record k from scenario scenarios[k], any indices in [0, B), repeats allowed (NULL with
 * count = B: all, in order); `bytes` is the blob's size as dat_checkpoint_bytes gives it.  Waits for every stream of
 * the handle, gathers the records on the device and copies them out in one piece.
 * dat_checkpoint_load: blob record records[k] into scenario scenarios[k], k < count.  records may repeat (one
 * record into many scenarios is a fork; the blob's stretch that holds the records named is uploaded once; NULL:
 * 0..count-1); scenarios must be distinct (NULL: 0..count-1); scenarios not named are untouched.  Needs no
 * parameters, touches neither the log nor its clock, and is legal wherever dat_set_state is.  The blob is checked
 * on the host before anything is launched or copied -- magic, version, mode, n and words per record against the
 * handle, `bytes` against the header's record count, every index, duplicate destinations -- and every failure
 * returns < 0 with a message that names the cause and leaves the handle as it was.  As after dat_set_state, the
 * next dat_closed_loop / dat_control_step computes desired acceleration and env rows from the state; the loaded
 * scenarios' advance stamps are cleared, so they are never taken for the coming step's.  Until that step
 * dat_debug_get_env_class still reports what the handle held before the load. */
int dat_checkpoint_bytes(dat_handle* h, int count, long long* bytes);
int dat_checkpoint_save(dat_handle* h, const int* scenarios, int count, void* blob, long long bytes);
int dat_checkpoint_load(dat_handle* h, const void* blob, long long bytes, const int* records, const int* scenarios,
                        int count);
/* Device time [ms] of the last dat_checkpoint_save / dat_checkpoint_load that copied records (HIP events on the
 * handle's stream): of its gather / scatter kernel, and of its copy between the staging buffer and the blob (a
 * load's includes the index lists).  Either pointer may be NULL. */
int dat_get_checkpoint_ms(dat_handle* h, double* kernel_ms, double* copy_ms);

/* ---- one high-level control step for every scenario ---------------------------------------
 * Replaces controller.control(state, acc_des) -> (f_des, SolverStatistics):
 *   RQPCADMMController.control   control/rqp_cadmm.py:631-675  (agent solves :482-501)
 *   RQPDDController.control      control/rqp_dd.py:695-752     (agent solves :475-505)
 *   RQPCentralizedController.control control/rqp_centralized.py:436-448
 * state: B x DAT_STATE_SIZE(n) or NULL (use the device-resident state);
 * acc_des: B x 6 (dvl_des, dwl_des) or NULL (forest law example/rqp_example.py:33-59 on device).
 * Outputs (any may be NULL): f_des B x 3n (agent-major, the forces the controller returns),
 * iters B (SolverStatistics.iter; -1 for centralized), qp_status B x n (last solve per agent),
 * min_env_dist B, collision B, err_seq B x (max_iter+1) (NaN padded; needs record_err). */
int dat_control_step(dat_handle* h, const double* state, const double* acc_des, double* f_des, int* iters,
                     int* qp_status, double* min_env_dist, unsigned char* collision, double* err_seq);

/* ---- fused control steps (QP-level workloads: C-ADMM / DD handles without a forest): `steps`
 * consecutive control steps of every scenario from the resident states, scenario s's step k using
 * acc_seq[(k B + s) x 6 ..] -- the same arithmetic per scenario as `steps` calls of dat_control_step
 * (warm f, f_mean, lambda / lambda_F, lambda_M carried; control/rqp_cadmm.py:631-675,
 * control/rqp_dd.py:695-752), in ONE persistent drain: a scenario that finishes step k starts step
 * k + 1 in its slot at once instead of waiting for the slowest scenario of step k.  Outputs (optional,
 * NULL to skip) are those of the last step.  record_err must be 0. */
int dat_control_steps(dat_handle* h, int steps, const double* acc_seq, double* f_des, int* iters, int* qp_status);

/* ---- rollout: `steps` simulation steps (SO(3) PD low level + rigid-body dynamics) ---------
 * Replaces RQPLowLevelController.control (control/rqp_centralized.py:518-535) followed by
 * RQPDynamics.integrate (system/rigid_quadrotor_payload.py:271-276) per simulation step.
 * f_des: B x 3n held constant over the steps, or NULL to use the last control step's output. */
int dat_rollout(dat_handle* h, int steps, const double* f_des);
/* Low-level law used by dat_rollout / dat_closed_loop: DAT_LL_PD (default, example/rqp_example.py:113)
 * or DAT_LL_SM -- the so3_controller_type argument of RQPLowLevelController (control/rqp_centralized.py:468-482). */
int dat_set_low_level(dat_handle* h, int kind);
/* RQPLowLevelController.control(state, f_des) -> (f, M) (control/rqp_centralized.py:518-535) at the
 * current states: f_des B x 3n (agent-major) or NULL (the last control step's output); thrust B x n,
 * moment B x n x 3 (agent-major 3-vectors). */
int dat_low_level_control(dat_handle* h, const double* f_des, double* thrust, double* moment);
/* Rigid payload driven by actuator forces (RPDynamics.integrate, system/rigid_payload.py:93-172): `steps`
 * steps of dt on the payload part of the states (xl, vl, Rl, wl; Rl projected every 20 steps), forces
 * f B x 3n (agent-major, ground frame; NULL: the last control step's output) held.  The handle carries
 * the rigid-payload parameter block (rigid_payload.pack_rp_params: mT = ml, JT = Jl, r_com = r), whose
 * centralized QP is RPCentralizedController (control/rp_centralized.py:9-306) via dat_control_step. */
int dat_rp_rollout(dat_handle* h, int steps, const double* f);
/* Point-mass rigid-link system: n point-mass robots carry the rigid payload on rigid links.  `steps` calls of
 * PMRLDynamics.integrate (system/point_mass_rigid_link.py:251-254: forward_dynamics :156-208, then
 * PMRLState.integrate :113-132 with project_q :101-105 at every step and project_R every 20) in one launch, on
 * states in the PMRL layout (dat_layout.h: q at DAT_S_Q, dq at DAT_S_DQ, the payload and the counter where they
 * are) with the PMRL parameter block (pmrl.pack_pmrl_params: ml, Jl, r as the rigid payload's, m, L and
 * chol(Jl^-1) at DAT_P_PM_*).  f: the force schedule nf x B x 3n (agent-major, ground frame), nf >= 1 and
 * steps % nf == 0; step s applies set s / (steps / nf), so nf = steps changes the force at every step and nf = 1
 * holds one set.  The link tensions come from the reduced 6 x 6 system of csrc/dat_pmrl_step.hpp instead of the
 * reference's n x n solve (:176-198).  A bad argument or missing parameters: an error code, the message in
 * dat_last_error, nothing launched. */
int dat_pmrl_rollout(dat_handle* h, int steps, const double* f, int nf);
/* PMRLDynamics.forward_dynamics (system/point_mass_rigid_link.py:156-208) at the current states, which it leaves
 * alone: under the thrusts f (B x 3n, agent-major) the accelerations ddq (B x 3n, agent-major), dvl and dwl
 * (B x 3) and the link tensions T (B x n). */
int dat_pmrl_forward(dat_handle* h, const double* f, double* ddq, double* dvl, double* dwl, double* T);

/* ---- device-resident closed loop (the loop of example/rqp_example.py:120-131 with the desired
 * acceleration of :33-59): hl_steps x (desired acceleration + control step +
 * hl_every rollout steps); inputs already in HBM, nothing copied per step. */
int dat_closed_loop(dat_handle* h, int hl_steps);

/* ---- the trajectory-tracking law, the clock and the plant of the resident loop ------------------------------------
 * The reference has a second desired-acceleration law beside the forest law: the time-dependent tracking law its
 * controllers fly without a forest (test/control/test_rqpcontrollers.py:24-48 _desired_acceleration_noenv,
 * test/control/test_rpcentralized.py:14-38): a circle of radius 1 m at 1 m height, 0.5 rad/s, with feed-forward
 * a_ref, no clamp, and dwl_des = (sin t, cos t, pi / 12).  csrc/dat_track.hpp states it once, for the kernels and the
 * host; a scenario's tracking record (DAT_TRACK_SIZE doubles, csrc/dat_layout.h DAT_T_*) holds centre, radius,
 * height, angular rate, time offset T0, gains KP / KV, the clamp AMAX on |dvl_des| (<= 0: none) and dwl_des's
 * amplitude and z component.
 *
 * dat_set_tracking: rec = NULL restores the forest law; otherwise one record (per_scenario = 0) or B records select
 * the tracking law wherever the device computes a desired acceleration (dat_control_step with acc_des = NULL,
 * dat_closed_loop) and for the log's x_ref / v_ref.  Independent of dat_set_forests: env rows stay active.  A
 * non-finite field, RADIUS < 0, FREQ < 0, KP < 0 or KV < 0 is rejected on the host, nothing copied or launched.
 *
 * The clock: simulation steps since dat_create (dat_set_clock to place it; negative: an error).  dat_closed_loop
 * advances it by hl_steps x hl_every, dat_rollout and dat_rp_rollout by `steps`; dat_control_step evaluates the law
 * at the current clock, t = clock x dt (the reference's t_seq[i] = i dt), and does not advance it.  Clock and records
 * are handle settings, like parameters: checkpoints carry neither.
 *
 * dat_set_plant: what dat_closed_loop rolls out.  DAT_PLANT_RQP (default): the quadrotor-payload system.
 * DAT_PLANT_RP: the rigid payload under the controller's forces (RPDynamics.integrate,
 * system/rigid_payload.py:93-130), centralized handles only: hl_steps x (k_cent, k_rp_advance), the resident form of
 * test/control/test_rpcentralized.py:41-62 (there hl_every = 1, dt = 10 ms).  The recorder does not know the RP
 * plant yet: with a log open DAT_PLANT_RP is an error, and so is dat_log_begin under it. */
#define DAT_PLANT_RQP 0
#define DAT_PLANT_RP 1
int dat_set_tracking(dat_handle* h, const double* rec, int per_scenario);
int dat_set_clock(dat_handle* h, long long clock);
int dat_get_clock(dat_handle* h, long long* clock);
int dat_set_plant(dat_handle* h, int plant);
/* C-ADMM handles: run dat_closed_loop on `count` (1..4) contiguous sub-batches of the scenarios, each on
 * its own stream with no synchronisation between sub-batches or steps, so that one sub-batch's kernels
 * fill the others' drain tails and short kernels.  Per scenario the arithmetic is unchanged (a scenario's
 * results never depend on the grouping).  count = 1 (default) restores the single-stream loop.  With a forest
 * and count = 1 the scenarios wedged in a stall (previous step > TAIL_PREV ADMM passes) run in the tail kernel
 * on a second stream beside the drain; with count > 1 (no further stream: the device's hardware queues are
 * shared by all streams) the drain hands them to the tail kernel before their first pass -- the same passes,
 * the same results. */
int dat_set_sub_batches(dat_handle* h, int count);
/* C-ADMM closed loop on one sub-batch with no log open: the advance overlap (default on).  Once the drain's last
 * queue has been claimed empty, the rollout of the scenarios it has finished, and their next step's desired
 * acceleration and env rows, run on a stream of their own beside the drain's ramp-down ("early"); the others
 * follow after the drain ("late").  A scenario's arithmetic is the same in either pass and every result is
 * bitwise that of the serial schedule (on = 0), which sub-batches, an open log, the other modes and the
 * step-by-step entry points keep. */
int dat_set_advance_overlap(dat_handle* h, int on);
/* Where the advance overlap runs (and record_err = 0): the step pipeline (default on).  Each step's drain is split in
 * two over disjoint scenarios.  The main drain of step k + 1 takes the scenarios the early pass of step k advanced
 * and is enqueued directly behind that pass on its stream, so it starts beside step k's ramp-down; the rest drain
 * of step k + 1 takes the others, on the handle's stream, after both drains of step k and the late pass.  The early
 * passes alternate between two streams; with the tail's the handle then holds four.  A call's first step is one
 * drain over all scenarios, after its last step only rollouts run, and at return every scenario is at the same
 * step and every stream idle.  A scenario's arithmetic does not depend on the drain that runs it: every result is
 * bitwise that of the overlap schedule (on = 0) and of the serial one.  dat_get_kernel_ms sums the main drains'
 * spans, which overlap between consecutive steps; the step marks are taken when the host first finds a step's main
 * drain ended. */
int dat_set_step_pipeline(dat_handle* h, int on);
/* Where the advance overlap or the step pipeline runs: the fused advance (default on).  A pass (early or late) that
 * runs the rollout and the next step's inputs of its scenarios does so in one launch, k_advance, instead of three
 * (rollout, desired acceleration, env rows and keys): one grid, the state written once and read back by the block
 * that wrote it.  The launch calls the device functions the three kernels call, on the same inputs in the same
 * order, so every result is bitwise that of on = 0, which runs the three kernels.  Under the step pipeline the
 * launch also counts the sort keys it makes, and the sorts of the two drains behind it only scatter, on many
 * workgroups (which scenarios share a wavefront is fixed by neither sort).  The passes that run only a part
 * -- a call's first step (inputs up front) and last step (rollouts only) -- and every schedule that does not split
 * the advance (serial, sub-batches, a log, the other modes, the step-by-step entry points) keep the three kernels. */
int dat_set_fused_advance(dat_handle* h, int on);
/* Launches of k_advance and of k_bucket_scatter (the sort behind it under the step pipeline) since the handle was
 * made: what tells the fused advance from its fall-backs, whose results are the same by construction. */
int dat_get_fused_launches(dat_handle* h, long long* advance, long long* scatter);
/* Streams the handle holds at the moment (its own, and the side streams made on first use): never more than four.
 * dat_set_sub_batches gives back the streams its new count does not use. */
int dat_get_stream_count(dat_handle* h);
/* Scenario-steps advanced by the early and by the late pass of the advance overlap since the last counter
 * reset; their sum is batch x HL steps run under the overlap (both 0 where the serial schedule ran). */
int dat_get_advance_counts(dat_handle* h, long long* early, long long* late);
/* Test hook: while a mask (batch bytes) is set, dat_closed_loop starts the early pass only after the drain has
 * ended and lets it take exactly the scenarios with early_mask[sc] != 0: a split between the two passes that
 * does not depend on timing.  Null clears it. */
int dat_debug_advance_split(dat_handle* h, const unsigned char* early_mask);
/* Test hook (C-ADMM): what the most recent step's k_env_class left in the handle, read after a control step with a
 * forest set (dat_control_step, or the last step of dat_closed_loop).  Launches nothing: waits for the handle's
 * streams and copies out the env rows k_cadmm consumed, decoded from their device image (per agent the marked
 * slots compacted in slot order, the rest zero, as dat_env_rows reports its rows), and per scenario the env class
 * of its sort key.  lhs: batch x n x 10 x 3, rhs: batch x n x 10, nrow: batch x n, env_class: batch. */
int dat_debug_get_env_class(dat_handle* h, double* lhs, double* rhs, int* nrow, int* env_class);
/* Host steady-clock marks (ms) of the last dat_closed_loop call: [0] its start (0.0), then the completion
 * of each HL step's control kernel; consecutive differences are per-step times of the back-to-back run.
 * Writes up to max_marks values; returns the number of marks (hl_steps + 1).  With sub-batch streams
 * (dat_set_sub_batches > 1) the steps of different sub-batches overlap: only the start and the end of the
 * run are marked (2 marks), so consecutive differences give one whole-run time, not per-step times. */
int dat_get_step_marks(dat_handle* h, double* marks_ms, int max_marks);

/* ---- the closed loop's log: what the reference's loop keeps in its lists (state_seq, x_err_seq, v_err_seq,
 * f_des_seq, iter_seq, solve_time_seq, min_env_dist_seq, w_seq: example/rqp_example.py:112-138), recorded in HBM
 * by the rollout kernel of dat_closed_loop itself and read after the run; nothing is copied per step.
 *
 * dat_log_begin opens a log on the handle.  scenarios[count]: the scenarios whose full records are kept, strictly
 * increasing indices in [0, B) (NULL with count = 0: none; NULL with count = B: all); a recorded scenario's place
 * in that list is its slot.  log_every >= 1 is the reference's log_freq in simulation steps (it need neither
 * divide hl_every nor be a multiple of it); hl_capacity >= 1 the number of HL steps the buffers hold; summary != 0
 * also keeps the summary tier of all B scenarios.  Allocates every buffer and zeroes the log clock.  Errors (a log
 * already open, bad arguments, an allocation failure) leave no log open.
 *
 * The log clock counts the simulation steps run by dat_closed_loop since dat_log_begin; every dat_closed_loop
 * call starts at an HL instant, so it is a multiple of hl_every between calls.  dat_control_step,
 * dat_control_steps, dat_rollout, dat_rp_rollout, dat_pmrl_rollout and dat_pmrl_forward are NOT recorded and do not
 * advance the clock while a log is open.  A dat_closed_loop call that would pass hl_capacity returns an error before
 * it launches anything: states, warm state and log are untouched (dat_log_read_*, dat_log_clear, then call again).
 *
 * Full tier, per slot:
 *   HL record k, after control step k (example/rqp_example.py:121-129): f_des (3n, agent-major), iters (-1 for
 *     centralized), qp_status (n), min_env_dist, collision, and x_ref (3), v_ref (3) of the desired-acceleration
 *     law at that HL instant (:36-48, :122).
 *   step record at every clock value i with i % log_every == 0 (:132-138): thrust (n) and moment (n x 3,
 *     agent-major) the low-level law applied at step i (:130), the state after step i (DAT_STATE_SIZE(n), the
 *     state layout), x_err = |x_ref - xl| and v_err = |v_ref - vl| against the references of the HL instant
 *     that opened the current HL period (:134-135).
 * Summary tier, per HL step and for all B scenarios: iters, min_env_dist, collision (:126-129 and
 *   stats.collision) -- enough to find which scenarios collide and when without stepping the loop from the host.
 * Host side, per HL step: the device time [ms] of the step's control kernels (stats.solve_time, :128; the
 *   per-step share of dat_get_counters' hl_kernel_ms); NaN with sub-batch streams, where steps overlap. */
int dat_log_begin(dat_handle* h, const int* scenarios, int count, int log_every, int hl_capacity, int summary);
/* Records held (written since dat_log_begin or the last dat_log_clear) and the log clock; any pointer may be NULL. */
int dat_log_counts(dat_handle* h, long long* hl_records, long long* step_records, long long* clock);
/* Copy held records [first, first + count) to the caller, time-major [record][slot][...]; any output pointer may
 * be NULL.  dat_log_read_hl: f_des count x slots x 3n, iters count x slots, qp_status count x slots x n,
 * min_env_dist count x slots, collision count x slots, x_ref and v_ref count x slots x 3, solve_ms count.
 * dat_log_read_steps: step_index count (the clock value i of each record), thrust count x slots x n, moment
 * count x slots x n x 3, state count x slots x DAT_STATE_SIZE(n), x_err and v_err count x slots.
 * dat_log_read_summary (needs summary != 0): iters, min_env_dist, collision count x B, per HL record. */
int dat_log_read_hl(dat_handle* h, int first, int count, double* f_des, int* iters, int* qp_status, double* min_env_dist,
                    unsigned char* collision, double* x_ref, double* v_ref, double* solve_ms);
int dat_log_read_steps(dat_handle* h, int first, int count, long long* step_index, double* thrust, double* moment,
                       double* state, double* x_err, double* v_err);
int dat_log_read_summary(dat_handle* h, int first, int count, int* iters, double* min_env_dist,
                         unsigned char* collision);
/* dat_log_clear empties the buffers and keeps the clock (a long run is read out in chunks of hl_capacity HL
 * steps); dat_log_end frees the buffers and closes the log (dat_destroy does so for an open log). */
int dat_log_clear(dat_handle* h);
int dat_log_end(dat_handle* h);

/* ---- episodes: scenarios that end and respawn inside the resident loop ------------------------------------------------
 * The reference's loop flies a fixed time (example/rqp_example.py:120-131); a Monte Carlo campaign wants a scenario to
 * end -- at its goal, at a collision, in a stall, after a step budget -- to be recorded once with its outcome, and its
 * slot to take the next initial condition, without a host round trip per step.  While episodes are open on a handle,
 * dat_closed_loop does this for every scenario at every HL step, after the scenario's control step and before its
 * rollout: it updates the scenario's accumulators (control steps, sum and maximum of iters, steps at max_iter + 1
 * passes, the current run of such steps, the smallest min_env_dist), evaluates the rule below (csrc/dat_episode.hpp,
 * one function for the kernels and the host) on the pre-rollout state, the step's iters, collision flag and
 * min_env_dist and the accumulators, and where a reason fires it appends an outcome record (csrc/dat_layout.h,
 * DAT_EP_*) and overwrites the scenario with a record of the pool INSTEAD of rolling it out.  The respawned scenario's
 * next control step takes its desired acceleration and env rows from the new state, as after dat_checkpoint_load.
 * The lowest code that fires wins:
 *   1 DAT_EP_DIVERGED    a word of xl or vl is not finite, or max |xl_c| > bound (+inf: only the first)
 *   2 DAT_EP_COLLISION   the step's collision flag is set (on_collision != 0)
 *   3 DAT_EP_GOAL        xl_x >= goal_x (+inf: off)
 *   4 DAT_EP_STALL       the last stall_steps control steps of the episode each ran max_iter + 1 passes (0: off;
 *                        refused on centralized handles, which have no passes)
 *   5 DAT_EP_TIME_LIMIT  the episode has computed max_steps control steps (0: off)
 * The pool is a checkpoint blob of P >= 1 records (dat_checkpoint_save's format), uploaded once.  dat_episode_begin
 * loads record s mod P into every slot s (the slot's episode 0; with a pool that is the handle's own checkpoint,
 * nothing changes); slot s starts its j-th episode, j >= 1, from record (s + j B) mod P, s the scenario's index in
 * the whole batch and B the batch: no cursor is shared, so results do not depend on the schedule.  With wrap = 0 a slot
 * whose next index s + j B would reach P takes record s mod P and goes idle: it keeps running, ends no more and
 * records nothing further (a slot s >= P is idle from the start); idle == B tells the host that every record of the
 * pool has been run once.
 * The outcome table holds `capacity` records, appended through one device counter in no fixed order (sort by end tick
 * and slot).  Beyond the capacity an episode still ends and respawns, the per-reason totals stay exact and `lost`
 * counts the records dropped.
 * Works on every schedule of dat_closed_loop, with the serial schedule's results bit for bit; with no episodes open
 * every launch is the one it was.  Not yet with an open log, DAT_PLANT_RP or tracking records (each an error, in
 * either order), and dat_checkpoint_load is refused while episodes are open (dat_checkpoint_save is not).
 * dat_control_step and dat_rollout do not evaluate episodes.
 * Every argument is checked on the host before anything is copied (csrc/dat_episode_host.hpp): an error leaves no
 * episodes open and the handle as it was. */
typedef struct dat_episode_rules {
  double goal_x;    /* GOAL: xl_x >= goal_x; +inf: off                                          */
  double bound;     /* DIVERGED: max |xl_c| > bound; +inf: only non-finite words                */
  int max_steps;    /* TIME_LIMIT after this many control steps; 0: off                         */
  int stall_steps;  /* STALL after this many consecutive steps at max_iter + 1 passes; 0: off   */
  int on_collision; /* COLLISION on the step's collision flag                                   */
  int wrap;         /* next record index modulo P (1), or idle once the pool is used up (0)     */
} dat_episode_rules;
void dat_episode_default_rules(dat_episode_rules* rules); /* everything off, wrap = 1 */
int dat_episode_begin(dat_handle* h, const dat_episode_rules* rules, const void* pool_blob, long long bytes,
                      int capacity);
/* ended[DAT_EP_NREASON] (6 words, csrc/dat_layout.h; may be NULL): episodes ended per reason since dat_episode_begin
 * ([0] unused, 0); records held in the table; records lost to its capacity since the last dat_episode_clear; idle
 * slots. */
int dat_episode_counts(dat_handle* h, long long* ended, long long* held, long long* lost, long long* idle);
/* Held records [first, first + count), in table order; any output may be NULL.  slot, episode, record, reason, steps,
 * iter_sum, iter_max, full_steps (steps at max_iter + 1 passes), stall_run: count ints each; start_tick, end_tick:
 * count; min_env_dist: count; xl, vl: count x 3. */
int dat_episode_read(dat_handle* h, int first, int count, int* slot, int* episode, int* record, int* reason,
                     long long* start_tick, long long* end_tick, int* steps, int* iter_sum, int* iter_max,
                     int* full_steps, int* stall_run, double* min_env_dist, double* xl, double* vl);
/* Empties the table and zeroes `lost`; totals, idle slots and the running episodes stay. */
int dat_episode_clear(dat_handle* h);
/* Closes the episodes and frees pool and table: dat_closed_loop is the plain loop again. */
int dat_episode_end(dat_handle* h);
/* Per slot (batch ints each, any may be NULL): the pool record its running episode started from, the episodes it has
 * finished, the control steps of the running episode, and whether it is idle. */
int dat_episode_slots(dat_handle* h, int* record, int* episodes, int* steps, int* idle);
/* Respawns since dat_episode_begin by the early pass of the overlapped schedules (0 by construction: the early pass
 * runs beside the drain that finished the scenario, whose warm state may not be written back yet, and leaves an
 * ending scenario to the rest pass) and by every other pass; deferred: ending scenarios the early gate left unmarked. */
int dat_get_episode_respawns(dat_handle* h, long long* early, long long* rest, long long* deferred);

/* ---- counters since the last reset: agent-QP solves, IPM iterations, IPM iterations x active
 * constraint rows (for the flop model of DESIGN.md 3.1), control steps, and the summed device time
 * of the high-level kernels [ms] (HIP events on the handle stream).  Any pointer may be NULL. */
int dat_get_counters(dat_handle* h, long long* qp_solves, long long* ipm_iters, long long* ipm_row_iters,
                     long long* hl_steps, double* hl_kernel_ms);
/* C-ADMM only: the same counters for one env class and the summed device time of k_cadmm [ms]
 * (one persistent launch drains every class).  env_class in [0, 4): scenarios whose agent QPs carry
 * no env CBF row this step (0), or at most 2 (1), 5 (2), 10 (3) env rows per agent QP. */
int dat_get_class_counters(dat_handle* h, int env_class, long long* qp_solves, long long* ipm_iters,
                           long long* ipm_row_iters, double* kernel_ms);
/* C-ADMM only, SIMD occupancy of one env class: slot_ipm_iters = sum over wavefront ADMM passes of
 * (the largest IPM iteration count among the wavefront's lanes) x lanes in use, wave_admm_iters =
 * sum over wavefronts of ADMM passes x scenarios per wavefront.  ipm_iters / slot_ipm_iters is the
 * fraction of lane-iterations doing useful work (the rest idle on divergence). */
int dat_get_class_occupancy(dat_handle* h, int env_class, long long* slot_ipm_iters, long long* wave_admm_iters);
int dat_reset_counters(dat_handle* h);
int dat_synchronize(dat_handle* h);
/* C-ADMM / DD: number of resident k_cadmm / k_dd workgroups that drain the scenario queues (0 = default,
 * 4 x CUs).  A scenario's arithmetic does not depend on it; tests cap it at 1-2 workgroups so that
 * scenario slots are refilled many times within one control step. */
int dat_set_persistent_blocks(dat_handle* h, int blocks);
/* C-ADMM launch geometry, as the launcher computes it (host only, no device work).  dat_cadmm_slots: scenario slots
 * per k_cadmm wavefront for a (sub-)batch of `batch` scenarios of this handle (at most 64 / n; fewer when the
 * resident workgroups would otherwise not all get a wavefront).  dat_cadmm_row_mode: where k_cadmm keeps the IPM
 * row state of env class `env_class` at team size n and `slots` slots -- 0 registers, 1 LDS rows, 2 LDS rows and
 * the class's auxiliary slots -- or -1 on arguments out of range.  Tests use the two to build the smallest batch
 * that reaches every instantiation. */
int dat_cadmm_slots(dat_handle* h, int batch, int* slots);
/* Tests: run k_cadmm / k_cadmm0 with the row modes (m0, m1, m2) of env classes 0, 1, 2 instead of those
 * dat_cadmm_row_mode gives, the LDS carve sized by them; (-1, -1, -1) returns to the rule.  k_cadmm is compiled for
 * the mode triples the rule can give only: any other is refused here, and a control step whose carve by the forced
 * modes would exceed a workgroup's dynamic LDS fails without a launch.  Results do not depend on the modes. */
int dat_debug_row_modes(dat_handle* h, int m0, int m1, int m2);
/* Tests: the tail rule of the following control steps with (tail_prev, tail_pass) instead of the library's pair
 * (tail_prev >= 0, tail_pass >= 2; a negative pair returns to it), so that a small case reaches the hand-over in
 * the pass before the rule's first.  With a forest only: without one the rule stays out of reach. */
int dat_debug_tail_rule(dat_handle* h, int tail_prev, int tail_pass);
int dat_cadmm_row_mode(int n, int slots, int env_class);
/* Summed device time [ms] since the last counter reset of the main solver kernel of each control step:
 * k_cadmm (C-ADMM) or k_dd (DD; the per-scenario quasi-Newton setup k_dd_setup excluded), 0 for
 * centralized.  Both are persistent queue drains; dat_set_persistent_blocks caps their grid.  A closed
 * loop on S sub-batches (dat_set_sub_batches) launches k_cadmm S times per HL step, one per sub-batch:
 * the sum then covers hl_steps x S launches. */
int dat_get_kernel_ms(dat_handle* h, double* ms);
/* Agent QPs since the last counter reset (every kernel) that stalled before the IPM tolerance (1e-10:
 * a numerical breakdown of the structured Newton solve at gaps ~1e-12, or the divergence stop) and
 * were accepted as OPTIMAL through their best iterate inside north_star's band (scaled primal / dual
 * residuals <= 1e-7, gap <= 1e-6); beyond_clarabel_tol counts those whose returned iterate is outside
 * Clarabel's own stopping tolerance (1e-8: a point Clarabel would not yet report as solved).  The
 * reference holds its previous solution on a non-OPTIMAL status (control/rqp_cadmm.py:496-499), so
 * beyond_clarabel_tol bounds the branch-disagreement risk; the C-ADMM / DD parity tests require 0. */
int dat_get_inband_exits(dat_handle* h, long long* inband, long long* beyond_clarabel_tol);
/* IPM iterative-refinement passes run and corrections applied by every kernel since the last counter
 * reset: the executed-work terms of the flop model. */
int dat_get_refinement_counters(dat_handle* h, long long* passes, long long* corrections);
/* C-ADMM control steps of a scenario finished by the tail kernel since the last counter reset: k_cadmm
 * hands a scenario's step to k_cadmm_tail, at the ADMM pass it is in, when one of its agent QPs does not
 * end cleanly (INACCURATE, or accepted in band beyond Clarabel's 1e-8: inside the reference's max_iter
 * stalls next to trees) or, with a forest, when the tail rule holds for its next pass (the previous step took
 * more than 20 ADMM passes, or the pass is the 16th); k_env_class routes a scenario whose previous step took
 * more than 20 passes to the tail before the step.  k_cadmm_tail redoes unclean QPs with the robust solver
 * (stiff rows in augmented form) and finishes the step.  Replaces no reference call (Clarabel's internal KKT
 * regularisation); the per-QP surfaces (dat_solve_agent_qp_batch) redo the QP themselves. */
int dat_get_robust_redos(dat_handle* h, long long* redos);
/* The tail kernel's work since the last counter reset (out[6]): [0] ADMM passes, [1] the sum over its passes of
 * the slowest agent QP's IPM iterations (the critical path of the stalled steps), [2] scenario-steps routed to
 * the tail before the step, [3] agent QPs whose rows were certified infeasible (a Farkas certificate on the dvl
 * rows: the QP is held at its previous solution, as the reference holds it when Clarabel reports infeasible,
 * control/rqp_cadmm.py:496-499), [4] solves ended by the stall exit, [5] warm-started solves.  Replaces no
 * reference call. */
int dat_get_tail_counters(dat_handle* h, long long* out);
/* C-ADMM with a forest: scenario-steps with a collision flag and the smallest minimum env distance over every
 * HL step since the last counter reset, signed (negative once a body is inside a tree: the reference logs
 * min_env_dist per step and flags a collision below its threshold: example/rqp_example.py:129,
 * example/env_forest.py:158-159; +inf without a forest). */
int dat_get_collision_stats(dat_handle* h, long long* collisions, double* min_env_dist);
/* Device time [ms] of the last dat_solve_agent_qp_batch launch (k_agent_qp; HIP events on the handle's
 * stream): the solve_time RQPPrimalSolver.solve returns (Clarabel's solver_stats.solve_time,
 * control/rqp_cadmm.py:500, control/rqp_dd.py:497). */
int dat_get_agent_qp_ms(dat_handle* h, double* ms);

/* ---- raw batched kernels (tests / benchmarking of single pieces) ---------------------------
 * dat_env_rows: _set_collision_avoidance_cbf_parameters (control/rqp_cadmm.py:307-373,
 * control/rqp_centralized.py:280-337) for every (scenario, agent).
 * Env CBF rows for every (scenario, agent) of the current state: lhs B x n x 10 x 3, rhs
 * B x n x 10, nrow B x n, collision B x n, min_dist B x n (agent = -1 row when centralized). */
int dat_env_rows(dat_handle* h, double* lhs, double* rhs, int* nrow, unsigned char* collision, double* min_dist);

/* dat_solve_agent_qp_batch: `count` independent agent QPs -- RQPPrimalSolver.solve
 *   C-ADMM handles: solve(state, acc_des, lambda_f, cadmm_rho, f_mean) -> f   control/rqp_cadmm.py:482-501
 *   DD handles:     solve(state, acc_des, c_fi, c_Fi, c_Mi) -> (f_i, F_i, M_i) control/rqp_dd.py:475-505
 * at the handle's current states (dat_set_state), parameters and forests.  Item k: scenario[k],
 * agent[k], acc_des[6k..] (dvl_des, dwl_des) and
 *   C-ADMM: lam[3n k ..] (lambda_f, agent-major 3-vectors), rho[k] > 0, f_mean[3n k ..];
 *   DD:     c9[9k ..] = (c_fi, c_Fi, c_Mi)  (lam, rho, f_mean unused; NULL allowed).
 * Outputs: x[3n k ..] (C-ADMM: agent i's full copy f, agent-major) or x[9k ..] (DD: f_i, F_i, M_i),
 * status[k] (DAT_QP_*), and, if not NULL, ipm_iters[k], collision[k], min_env_dist[k] of the agent's
 * env query (control/rqp_cadmm.py:307-373).  A non-OPTIMAL item returns the IPM's best iterate; the
 * reference's fallbacks (hold previous / f_eq, :491-499) are the caller's (RQP*PrimalSolver in
 * control.py).  No warm state is read or written. */
int dat_solve_agent_qp_batch(dat_handle* h, int count, const int* scenario, const int* agent, const double* acc_des,
                             const double* lam, const double* rho, const double* f_mean, const double* c9, double* x,
                             int* status, int* ipm_iters, unsigned char* collision, double* min_env_dist);

/* dat_solve_agent_qp_rows_batch: dat_solve_agent_qp_batch with the caller's env CBF rows in place of the forest
 * query (_set_collision_avoidance_cbf_parameters, control/rqp_cadmm.py:307-373, is skipped for these items; the
 * handle's forests are not read).  Item k carries nenv[k] (0..DAT_NENV = 10) rows, compacted to the front of
 * env_lhs[30k ..] (10 x 3) and env_rhs[10k ..]; row j means env_lhs[j] . dvl >= env_rhs[j], the convention of
 * dat_env_rows.  The same kernel and arithmetic as dat_solve_agent_qp_batch from the rows on.  No env query is
 * made, so collision[k] = 0 and min_env_dist[k] = +inf.  certified[k] (may be NULL) is 1 exactly when the Farkas
 * certificate on the dvl rows (dvl_rows_infeasible: env rows and the |vl| base row) decided the item, which then
 * returns DAT_QP_INFEASIBLE with 0 IPM iterations; DAT_QP_INFEASIBLE with certified[k] = 0 comes from a zero row
 * with a positive right-hand side or a vanishing base row.  DD handles take the rows and never set certified
 * (no certificate on that path).  Replaces no reference call: tests of the certificate on chosen row sets. */
int dat_solve_agent_qp_rows_batch(dat_handle* h, int count, const int* scenario, const int* agent,
                                  const double* acc_des, const double* lam, const double* rho, const double* f_mean,
                                  const double* c9, const double* env_lhs, const double* env_rhs, const int* nenv,
                                  double* x, int* status, int* ipm_iters, unsigned char* collision,
                                  double* min_env_dist, unsigned char* certified);

/* ---- metric collectives of a sharded run (K8) ----------------------------------------------
 * Scenarios shard over the GPUs of a node with no collective inside the control step; what crosses GPUs is the
 * per-scenario metrics the reference's loop keeps in its lists (iteration counts, min env distance, collision
 * flag: example/rqp_example.py:112-138) and the run's work counters.  The reference runs one scenario in one
 * process and has no such call; these replace the torch.distributed collectives a PyTorch harness would use,
 * over RCCL (xGMI), with host buffers.  One process per GPU: rank 0 creates the id, the launcher hands it to the
 * others (sharding.py: a file keyed by the launcher's rendezvous), every rank calls dat_comm_create. */
#define DAT_COMM_ID_BYTES 128
#define DAT_COMM_SUM 0
#define DAT_COMM_MAX 1
typedef struct dat_comm dat_comm;
int dat_comm_unique_id(unsigned char* id /* DAT_COMM_ID_BYTES */);
int dat_comm_create(int device, int nranks, int rank, const unsigned char* id, dat_comm** out);
int dat_comm_destroy(dat_comm* c);
/* recv[nranks x count] = every rank's send[count], in rank order */
int dat_comm_allgather(dat_comm* c, const double* send, long long count, double* recv);
/* buf[count] = element-wise sum (DAT_COMM_SUM) or max (DAT_COMM_MAX) over the ranks, in place */
int dat_comm_allreduce(dat_comm* c, double* buf, long long count, int op);
/* every rank's device work done, then a one-value all-reduce */
int dat_comm_barrier(dat_comm* c);
const char* dat_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DAT_H */
