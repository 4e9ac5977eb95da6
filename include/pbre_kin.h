/* pbre_kin.h -- the batched kinematics / dynamics query of libpbre.so: per env, the pose and velocity of any link, the Jacobian of a point
 * of a link, the joint-space inertia matrix M(q) and the inverse-dynamics torques, from the state records the engines keep on the device.
 *
 * Replaces, for callers that stay on the device, p.getLinkState(..., computeLinkVelocity=1) (R/envs/panda_envs/panda_env.py,
 * R/envs/icub_envs/icub_env.py and icub_env_with_hands.py: get_observation), p.calculateJacobian, p.calculateMassMatrix and
 * p.calculateInverseDynamics: the query downloads nothing and never writes the state.  Conventions as in pbre.h: 0 or a negative PBRE_E_*
 * code, message in pbre_last_error.
 *
 * nd is the RobotTable's n_dof (26 for the floating-base iCub, whose virtual base joints are ordinary columns); q = Q[dof], qd = V[dof] of
 * the state record (lane width W = (record floats - 16) / 2).  Everything is expressed in the world frame.
 *
 * RIGID-BODY QUANTITIES ONLY.  `mass` and `tau` describe the articulated rigid bodies of the RobotTable under gravity and nothing else:
 * no joint damping, no linear or angular damping of the links, no motors, no joint limits, no contacts.  A caller who wants the joint
 * damping torque adds damping * qd themselves.
 *
 * PBRE_E_ARG: a link index outside [0, n_links of the table), n_links above the table's link count, links NULL with n_links > 0, a NaN in
 * jac_point.  PBRE_E_TABLE: a ctx without a RobotTable, or links out of order (the contact query's check).  PBRE_E_UNSUPPORTED: a table
 * with fixed_base = 0 (none is shipped), more than 128 links or 64 DoF.  A refused query launches nothing.
 */
#ifndef PBRE_KIN_H
#define PBRE_KIN_H
#include "pbre.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    /* inputs */
    const int32_t* links;  int32_t n_links;  /* link indices to report (host memory, copied at the call); NULL/0: none */
    int32_t at_com;                          /* 0: the link frame's origin (URDF frame); 1: the link's centre of mass (getLinkState [0]/[6]) */
    int32_t jac_link;                        /* link of the Jacobian; -1: the table's ee_link */
    float   jac_point[3];                    /* point in that link's frame; ignored with jac_at_com = 1 */
    int32_t jac_at_com;
    const float* qdd;                        /* [N][nd] joint accelerations for tau; NULL: zeros (tau = gravity + Coriolis/centrifugal) */
    /* outputs, env-major, float32; every pointer may be NULL: that output is skipped, its buffer untouched, and it costs nothing */
    float* pose;   /* [N][n_links][7]  position, quaternion x,y,z,w (w >= 0) of the link frame; position of the COM with at_com */
    float* vel;    /* [N][n_links][6]  world linear velocity of that point, world angular velocity */
    float* jac;    /* [N][6][nd]       rows: linear x,y,z then angular x,y,z; column = DoF index of the table; world frame */
    float* mass;   /* [N][nd][nd]      M(q), symmetric, both triangles written */
    float* tau;    /* [N][nd]          RNEA(q, qd, qdd) under phys.gravity_z */
} pbre_kin_query_t;

/* Device buffers on ctx's GPU (the struct itself and `links` are host memory; qdd is a device buffer too); enqueued on `stream` (as for
 * pbre_step_device: a hipStream_t, PBRE_STREAM_LEGACY, or NULL = the ctx's own stream) behind whatever step was last enqueued there;
 * asynchronous.  Queries of one ctx share column buffers of per-link quantities (their own, not the contact query's): enqueue them on one
 * stream, or order them yourself.  The first query of a ctx uploads its table and allocates those buffers (as does a later one that needs
 * larger ones: more envs, or an output with larger buffers): only that call synchronises. */
int pbre_kin_query_device(pbre_ctx* ctx, const pbre_kin_query_t* q, void* stream);
/* Host buffers (qdd too); synchronous (waits for every step in flight first). */
int pbre_kin_query(pbre_ctx* ctx, const pbre_kin_query_t* q);

#ifdef __cplusplus
}
#endif
#endif
