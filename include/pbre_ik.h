/* pbre_ik.h -- the batched inverse-kinematics query of libpbre.so: per env, the joint positions that bring a point of a link to a target
 * position (and the link to a target orientation), by the damped-least-squares iteration the engines run inside a step, from the state
 * records they keep on the device.
 *
 * Replaces, for callers that stay on the device, p.calculateInverseKinematics (R/envs/panda_envs/panda_env.py:269-272,
 * R/envs/icub_envs/icub_env.py:307-312): the query downloads nothing, never writes the state and writes nothing a step reads.
 * Conventions as in pbre.h: 0 or a negative PBRE_E_* code, message in pbre_last_error.
 *
 * The iteration (oracle/pbre_oracle.c: orc_ik), from q = q_start, at most max_iters times:
 *   x, R   the point's world position and the link's rotation at q (forward kinematics of the chain from the root to `link`)
 *   e      = [target_pos - x ; rotvec(R_target R^T)]      (the three position rows alone without target_quat)
 *   stop   when |e_pos| < residual (and, with rot_residual > 0, the rotation error angle < rot_residual): tested BEFORE the update
 *   q     += J^T (J J^T + damping^2 I)^-1 e               (Cholesky; J: the columns of the DoFs that move)
 * A DoF moves only if it is on the chain from the root to `link`, its link is not ik_passive in the RobotTable and its dof_mask byte
 * (if a mask is given) is non-zero; every other DoF keeps its start value.  With damping, residual and max_iters negative (the ctx's
 * ik_damping, ik_residual, ik_max_iters), rot_residual <= 0, clamp_limits = 0, link = -1 and the commanded hand pose as the target, `q` is
 * what a step of an engine in IK mode computes before it clamps and commands the motors.
 *
 * nd is the RobotTable's n_dof; q_start NULL: Q[dof] of the state record.
 *
 * PBRE_E_ARG: link outside [-1, n_links of the table), target_pos NULL, a NaN in point, max_iters above 1000.  PBRE_E_TABLE: a ctx
 * without a RobotTable, or links out of order.  PBRE_E_UNSUPPORTED: a table with fixed_base = 0 (none is shipped), more than 128 links or
 * 64 DoF, a chain of more than PBRE_IK_MAX_CHAIN links, or more than PBRE_IK_MAX_MOVING DoFs that move (their working set -- 7 floats per
 * DoF and env -- is kept on chip; no shipped table reaches either limit: the longest chain, root to a fingertip of the iCub with hands, has
 * 14 joints).  A refused query launches nothing.
 */
#ifndef PBRE_IK_H
#define PBRE_IK_H
#include "pbre.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PBRE_IK_MAX_CHAIN 64     /* links on the chain from the root to `link`, fixed joints included */
#define PBRE_IK_MAX_MOVING 24    /* DoFs of the chain that move */

typedef struct {
    /* inputs */
    int32_t link;                 /* the link that is driven; -1: the table's ee_link */
    float   point[3];             /* the point of that link (link frame) that is driven to target_pos */
    const float* target_pos;      /* [N][3] world frame; required */
    const float* target_quat;     /* [N][4] x, y, z, w, normalised by the kernel; NULL: position only (3 error rows, a 3 x 3 system) */
    const float* q_start;         /* [N][nd]; NULL: the joint positions of the state record */
    const uint8_t* dof_mask;      /* host memory, [nd] bytes, copied at the call; NULL: every DoF of the chain that is not ik_passive */
    double  damping, residual;    /* negative: the ctx's ik_damping / ik_residual.  residual = 0 never converges: exactly max_iters updates */
    double  rot_residual;         /* <= 0: the stopping rule looks at the position alone (the step's); > 0: also the rotation error angle (rad) */
    int32_t max_iters;            /* negative: the ctx's ik_max_iters; 0: the errors at the start only; at most 1000 */
    int32_t clamp_limits;         /* 0: the step's behaviour (it clamps later, in apply_action); 1: every moved DoF is clamped to [lower, upper]
                                     of the table after each update: q = min(max(q, lower), upper) */
    /* outputs, env-major; every pointer may be NULL: that output is skipped, its buffer untouched */
    float*   q;                   /* [N][nd] float32: the solution; the DoFs that do not move hold their start value */
    float*   err;                 /* [N][2]  position error norm (m), rotation error angle (rad; 0 in position-only mode), at the returned q */
    int32_t* iters;               /* [N]     updates applied before the convergence test passed; max_iters if it never did */
} pbre_ik_query_t;

/* Device buffers on ctx's GPU (the struct itself and dof_mask are host memory); enqueued on `stream` (as for pbre_step_device: a
 * hipStream_t, PBRE_STREAM_LEGACY, or NULL = the ctx's own stream) behind whatever step was last enqueued there; asynchronous.  The query
 * keeps no work buffer in device memory: queries of one ctx on different streams do not disturb each other.  Only the first query of a
 * ctx, which uploads its table, synchronises. */
int pbre_ik_query_device(pbre_ctx* ctx, const pbre_ik_query_t* q, void* stream);
/* Host buffers (target_pos, target_quat and q_start too); synchronous (waits for every step in flight first). */
int pbre_ik_query(pbre_ctx* ctx, const pbre_ik_query_t* q);

#ifdef __cplusplus
}
#endif
#endif
