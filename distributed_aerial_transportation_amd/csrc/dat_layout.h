// Memory layout of the per-scenario blocks shared by the host wrapper, the C-ABI and the kernels.
// All arrays are fp64, scenario-major (structure of arrays per scenario, scenarios contiguous).
#pragma once

// ---- parameter block (one per scenario), size DAT_PARAM_SIZE(n) doubles -------------------------
// Derived from RQPParameters (reference system/rigid_quadrotor_payload.py:48-84), the equilibrium
// forces f_eq (control/rqp_cadmm.py:165-174) and the controller constants
// (control/rqp_cadmm.py:192-236, control/rqp_centralized.py:182-225).
#define DAT_P_MT 0            // total mass mT
#define DAT_P_XCOM 1          // x_com (3)
#define DAT_P_JT 4            // JT (3x3, row-major)
#define DAT_P_JTI 13          // JT^-1 (3x3)
#define DAT_P_MINFZ 22        // min_fz = mT g / (10 n)
#define DAT_P_MAXF 23         // max_f = 2 mT g / n
#define DAT_P_SEC 24          // sec(max_f_ang)
#define DAT_P_COSP 25         // cos(max_p_ang)
#define DAT_P_MAXWL2 26       // max_wl^2
#define DAT_P_MAXVL2 27       // max_vl^2
#define DAT_P_DISTEPS 28      // dist_eps
#define DAT_P_VISR 29         // vision radius = collision radius + 5
#define DAT_P_COSCONE 30      // cos(vision cone half angle)
#define DAT_P_MAXDEC 31       // max deceleration (g / 5)
#define DAT_P_COLR 32         // capsule (collision) radius
#define DAT_P_KFD 33          // k_f  distributed (0.1 / n)
#define DAT_P_KMD 34          // k_m  distributed
#define DAT_P_KFC 35          // k_f  centralized (0.1)
#define DAT_P_KMC 36          // k_m  centralized
#define DAT_P_KFEQ 37         // k_feq
#define DAT_P_AENVD 38        // alpha_env distributed (1.5)
#define DAT_P_AENVC 39        // alpha_env centralized (2.0)
#define DAT_P_ML 40           // payload mass (informational)
#define DAT_P_HDR 41
#define DAT_P_R(n) (DAT_P_HDR)                    // r (3n): attachment points, body frame, agent-major
#define DAT_P_RCOM(n) (DAT_P_HDR + 3 * (n))      // r_com (3n)
#define DAT_P_FEQ(n) (DAT_P_HDR + 6 * (n))       // f_eq (3n)
#define DAT_P_J(n) (DAT_P_HDR + 9 * (n))         // quad inertias J_i (9n, row-major 3x3 each)
#define DAT_P_JINV(n) (DAT_P_HDR + 18 * (n))     // J_i^-1 (9n)
#define DAT_PARAM_SIZE(n) (DAT_P_HDR + 27 * (n))
// Point-mass rigid-link system (PMRLParameters, reference system/point_mass_rigid_link.py:37-64): ml, Jl, Jl^-1 in
// MT, JT, JTI and r in R and RCOM, as the rigid payload's block; the system has no actuator inertias, so inside the
// region DAT_P_J(n) (9n >= 2n + 9 words for n >= 3) lie the robot masses, the link lengths and the upper Cholesky
// factor U of Jl^-1 (U'U = Jl^-1, :59), row-major 3x3.
#define DAT_P_PM_M(n) (DAT_P_J(n))                   // m (n)
#define DAT_P_PM_L(n) (DAT_P_J(n) + (n))             // L (n)
#define DAT_P_PM_U(n) (DAT_P_J(n) + 2 * (n))         // chol(Jl^-1), upper (9)
#define DAT_P_PM_END(n) (DAT_P_J(n) + 2 * (n) + 9)   // end of the PMRL words of the region

// ---- state block (one per scenario), size DAT_STATE_SIZE(n) doubles ------------------------------
// RQPState (reference system/rigid_quadrotor_payload.py:87-119): R_i (9n, row-major 3x3), w_i (3n),
// xl (3), vl (3), Rl (9, row-major), wl (3).  A per-scenario int counter (steps since the last
// polar projection) lives in a separate int array.
#define DAT_S_R(n) 0
#define DAT_S_W(n) (9 * (n))
#define DAT_S_XL(n) (12 * (n))
#define DAT_S_VL(n) (12 * (n) + 3)
#define DAT_S_RL(n) (12 * (n) + 6)
#define DAT_S_WL(n) (12 * (n) + 15)
#define DAT_STATE_SIZE(n) (12 * (n) + 18)
// PMRLState (reference system/point_mass_rigid_link.py:67-132) in the same block: the link directions q_i (3n,
// agent-major) at the head of the R region, whose other 6n words are zero, their rates dq_i (3n) in the W region;
// xl, vl, Rl, wl and the int counter where they are.
#define DAT_S_Q(n) 0
#define DAT_S_DQ(n) (DAT_S_W(n))

// ---- forest / mountain record (DAT_MOUNTAIN_SIZE doubles) -----------------------------------------
// example/env_forest.py:22-31,74-77: centre (2), radius, sphere radius, centre depth
#define DAT_M_CX 0
#define DAT_M_CY 1
#define DAT_M_RADIUS 2
#define DAT_M_SPHERE_R 3
#define DAT_M_DEPTH 4
#define DAT_MOUNTAIN_SIZE 5

// ---- tracking record (DAT_TRACK_SIZE doubles; dat_set_tracking, the law: dat_track.hpp) ----------------------
// test/control/test_rqpcontrollers.py:24-48, test/control/test_rpcentralized.py:14-38: the reference flies centre
// (0, 0), radius 1, height 1, 0.5 rad/s, T0 = 0, gains 1 and 1, no clamp, dwl_des = (sin t, cos t, pi / 12)
#define DAT_T_CX 0
#define DAT_T_CY 1
#define DAT_T_RADIUS 2
#define DAT_T_HEIGHT 3
#define DAT_T_FREQ 4         // angular rate, rad/s
#define DAT_T_T0 5           // time offset, s
#define DAT_T_KP 6
#define DAT_T_KV 7
#define DAT_T_AMAX 8         // clamp on |dvl_des|; <= 0: none
#define DAT_T_WAMP 9         // dwl_des = (WAMP sin tau, WAMP cos tau, WZ)
#define DAT_T_WZ 10
#define DAT_T_RESERVED 11    // zero
#define DAT_TRACK_SIZE 12

// ---- records of the closed loop's log (dat_log_*), in 8-byte words, laid out [record][slot][word] --------
// HL record (after control step k): f_des (3n, agent-major), min_env_dist, x_ref (3), v_ref (3), then 32-bit
// ints packed two per word: iters, collision, qp_status (n), padded to a whole word.
#define DAT_LOG_HL_MIND(n) (3 * (n))
#define DAT_LOG_HL_XREF(n) (3 * (n) + 1)
#define DAT_LOG_HL_VREF(n) (3 * (n) + 4)
#define DAT_LOG_HL_INTS(n) (3 * (n) + 7)  // int[0] iters, int[1] collision, int[2 + i] qp_status of agent i
#define DAT_LOG_HL_WORDS(n) (3 * (n) + 7 + ((n) + 3) / 2)
// step record (simulation step i): per agent (thrust, moment (3)) applied at step i (4n), the state after the
// step in the state layout (DAT_STATE_SIZE(n)), x_err, v_err.  A multiple of 4 words: every record and every
// agent's (thrust, moment) start on a 32-byte boundary.
#define DAT_LOG_ST_STATE(n) (4 * (n))
#define DAT_LOG_ST_XERR(n) (4 * (n) + DAT_STATE_SIZE(n))
#define DAT_LOG_ST_WORDS(n) (4 * (n) + DAT_STATE_SIZE(n) + 2)

// ---- checkpoint record (dat_checkpoint_*), in 8-byte words ------------------------------------------------------
// One record: everything of one scenario that a later step's arithmetic reads.  All modes: the state block, f_des
// (3n, agent-major: the forces the rollout applies), then 32-bit ints packed two per word: int[0] the polar counter,
// int[1] iters and int[2] ipmx (the previous step's ADMM / DD pass count and slowest IPM count: k_cadmm's IPM start
// regime, the drain order and the tail rule read them), int[3] zero.  Then the mode's warm state, in the device's
// agent-major layout: C-ADMM f (n x 3n, agent i's copy at 3n i), f_mean (3n), lambda_f (n x 3n); DD lambda_F,
// lambda_M (3n each), prev (9n: per agent f_i, F_i, M_i); centralized prev_f (3n).  A record is padded to an even
// number of words, so every record of a blob starts 16-byte aligned behind the header.
#define DAT_CK_STATE(n) 0
#define DAT_CK_FDES(n) (DAT_STATE_SIZE(n))
#define DAT_CK_INTS(n) (DAT_STATE_SIZE(n) + 3 * (n))  // int[0] counter, int[1] iters, int[2] ipmx, int[3] zero
#define DAT_CK_WARM(n) (DAT_STATE_SIZE(n) + 3 * (n) + 2)
#define DAT_CK_F(n) (DAT_CK_WARM(n))                               // C-ADMM
#define DAT_CK_FMEAN(n) (DAT_CK_WARM(n) + 3 * (n) * (n))
#define DAT_CK_LAMF(n) (DAT_CK_WARM(n) + 3 * (n) * (n) + 3 * (n))
#define DAT_CK_END_CADMM(n) (DAT_CK_WARM(n) + 6 * (n) * (n) + 3 * (n))
#define DAT_CK_LAMF_DD(n) (DAT_CK_WARM(n))                         // DD
#define DAT_CK_LAMM_DD(n) (DAT_CK_WARM(n) + 3 * (n))
#define DAT_CK_PREV_DD(n) (DAT_CK_WARM(n) + 6 * (n))
#define DAT_CK_END_DD(n) (DAT_CK_WARM(n) + 15 * (n))
#define DAT_CK_PREVF(n) (DAT_CK_WARM(n))                           // centralized
#define DAT_CK_END_CENT(n) (DAT_CK_WARM(n) + 3 * (n))
#define DAT_CK_WORDS_CADMM(n) (DAT_CK_END_CADMM(n) + (DAT_CK_END_CADMM(n) & 1))
#define DAT_CK_WORDS_DD(n) (DAT_CK_END_DD(n) + (DAT_CK_END_DD(n) & 1))
#define DAT_CK_WORDS_CENT(n) (DAT_CK_END_CENT(n) + (DAT_CK_END_CENT(n) & 1))
// The blob: a header of DAT_CK_HEADER_BYTES, then the records back to back.  Header fields at byte offsets
// (little-endian): magic (8, "DATCKPT\0"), format version, mode (DAT_MODE_*), n, words per record (4 each), record
// count (8), zeros to the header's end.
#define DAT_CK_HEADER_BYTES 64
#define DAT_CK_MAGIC 0x0054504B43544144
#define DAT_CK_VERSION 1
#define DAT_CK_H_MAGIC 0
#define DAT_CK_H_VERSION 8
#define DAT_CK_H_MODE 12
#define DAT_CK_H_N 16
#define DAT_CK_H_WORDS 20
#define DAT_CK_H_COUNT 24
#define DAT_CK_H_PAD 32

// ---- episodes (dat_episode_*; the rule: dat_episode.hpp) ----------------------------------------------------------
// Reasons an episode ends for; the lowest code that fires wins, 0: the episode goes on.
#define DAT_EP_NONE 0
#define DAT_EP_DIVERGED 1
#define DAT_EP_COLLISION 2
#define DAT_EP_GOAL 3
#define DAT_EP_STALL 4
#define DAT_EP_TIME_LIMIT 5
#define DAT_EP_NREASON 6
// Outcome record, DAT_EP_WORDS 8-byte words; 32-bit ints packed two per word (the first in the low half).
#define DAT_EP_SLOT 0         // ints: slot (the global scenario index), episode number of the slot
#define DAT_EP_RECORD 1       // ints: pool record the episode started from, reason (DAT_EP_*)
#define DAT_EP_START 2        // int64: tick of the episode's first control step, on the handle's clock
#define DAT_EP_END 3          // int64: tick of its last control step
#define DAT_EP_STEPS 4        // ints: control steps, sum of iters
#define DAT_EP_ITMAX 5        // ints: maximum of iters, steps at max_iter + 1 passes
#define DAT_EP_RUN 6          // ints: the stall run at the end, zero
#define DAT_EP_MIND 7         // smallest min_env_dist of the episode's steps
#define DAT_EP_XL 8           // terminal xl (3): the state the last control step saw
#define DAT_EP_VL 11          // terminal vl (3)
#define DAT_EP_WORDS 14

#define DAT_BARK_RADIUS 0.3
#define DAT_BARK_HALF_HEIGHT 2.0
#define DAT_NENV 10            // env CBF rows per QP (control/rqp_cadmm.py:218)
#define DAT_MAXROW 13          // tilt + |wl| + |vl| + 10 env rows
#define DAT_GRAVITY 9.80665    // scipy.constants.g
