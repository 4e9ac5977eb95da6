/* pbre_contacts.h -- the batched contact query of libpbre.so: per env, is the object touching the table or the robot, is the robot touching
 * the table, and how close is each pair.
 *
 * Replaces the host loop behind WorldEnv.check_contact (R/envs/world_envs/world_env.py:128-134), pandaEnv.check_collision and
 * check_contact_fingertips (R/envs/panda_envs/panda_env.py:312-365) and their iCub counterparts for callers that stay on the device: the
 * query reads the state records the engines keep there, downloads nothing and never writes the state.  Conventions as in pbre.h: 0 or a
 * negative PBRE_E_* code, message in pbre_last_error.
 *
 * Pairs (the detection rule of model/contacts.py: contact_flags -- a pair is in contact when its signed distance is < margin):
 *   robot   the RobotTable's collision spheres, in table order
 *   object  phys.obj_shape: box (half extents obj_h), sphere (radius obj_h[0]), cylinder about local z (radius obj_h[0], half height
 *           obj_h[2]), hull or compound (pbre_set_object_hull; the nearest piece counts)
 *   table   the box phys.table_c +- phys.table_h
 * Object against table uses the shape's candidate points -- the 8 box vertices, the sphere's lowest point, the cylinder's 8 rim slots, every
 * vertex of every hull piece -- and a candidate counts only where it lies over the table top in x and y and above the table's underside;
 * its distance is z - top.  The floor is not queried.
 *
 * margin < 0: phys.contact_margin.  margin >= 0 overrides it for this call ("within 1 cm").  NaN: PBRE_E_ARG.
 *
 * Hull objects.  A piece whose bounding sphere is farther from a collision sphere than margin + the largest bounding radius of the
 * object's pieces contributes that lower bound instead of its distance (the face loop is skipped).  So dist[1] is exact wherever it is
 * below margin + that radius -- in particular wherever it is below margin, which is all the flags, counts and fingertip bits need -- and
 * a lower bound (never below margin) above it; nearest[0] then names the sphere with the smallest bound.
 *
 * Sentinels.  With PBRE_F_NO_OBJECT: flag bits 1 and 2 are 0, dist[0] = dist[1] = PBRE_CQ_FAR, nearest[0] = -1, count[0] = 0, tips = 0.
 * No candidate over the table: dist[0] = PBRE_CQ_FAR.  A robot without spheres: PBRE_CQ_FAR, -1 and 0 for the robot entries.  Equal
 * distances: `nearest` names the lower sphere index.
 */
#ifndef PBRE_CONTACTS_H
#define PBRE_CONTACTS_H
#include "pbre.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PBRE_CQ_OBJECT_TABLE = 1, PBRE_CQ_ROBOT_OBJECT = 2, PBRE_CQ_ROBOT_TABLE = 4 };   /* = model/contacts.py */
#define PBRE_CQ_FAR 3.0e38f

typedef struct {            /* every pointer may be NULL: that output is skipped and its buffer untouched */
    int32_t* flags;         /* [N]     OR of the three bits                                                     */
    float*   dist;          /* [N][3]  smallest signed distance: object-table, robot-object, robot-table (m)    */
    int32_t* nearest;       /* [N][2]  RobotTable collision-sphere index attaining dist[1] / dist[2]; -1: none  */
    int32_t* count;         /* [N][2]  spheres whose distance to the object / the table is < margin             */
    int32_t* tips;          /* [N]     bit s set: a sphere with fingertip slot s is within margin of the object */
} pbre_contact_out;

/* Device buffers on ctx's GPU (the struct itself is host memory); enqueued on `stream` (as for pbre_step_device: a hipStream_t,
 * PBRE_STREAM_LEGACY, or NULL = the ctx's own stream) behind whatever step was last enqueued there; asynchronous.  Queries of one ctx
 * share a buffer of link frames: enqueue them on one stream, or order them yourself.  The first query of a ctx uploads its table and
 * allocates that buffer (as does a later one of more envs): only that call synchronises. */
int pbre_contact_query_device(pbre_ctx* ctx, const pbre_contact_out* d_out, float margin, void* stream);
/* Host buffers; synchronous (waits for every step in flight first). */
int pbre_contact_query(pbre_ctx* ctx, const pbre_contact_out* out, float margin);

#ifdef __cplusplus
}
#endif
#endif
