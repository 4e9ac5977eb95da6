/* pbre_camera.h -- the batched ray-cast camera of libpbre.so: depth, segmentation and colour images of every env of a ctx.
 *
 * Replaces p.getCameraImage in the `render` methods of the reference's task envs (R/envs/panda_envs/panda_push_gym_env.py,
 * panda_reach_gym_env.py, R/envs/icub_envs/icub_push_gym_env.py, icub_reach_gym_env.py).  The scene is the engine's own geometry, read
 * from the device-resident state records; nothing is downloaded and rendering never writes the state.  Conventions as in pbre.h:
 * 0 or a negative PBRE_E_* code, message in pbre_last_error.
 *
 * Scene.  Floor: the half space z <= phys.ground_z.  Table: the box phys.table_c +- phys.table_h.  Object (absent with PBRE_F_NO_OBJECT):
 * pose from the state record, shape by phys.obj_shape -- box (half extents obj_h), sphere (radius obj_h[0]), cylinder about local z (radius
 * obj_h[0], half height obj_h[2]), hull or compound (the face planes of every piece of the hull table).  Robot: a list of visual primitives,
 * each a capsule (a sphere when a == b) in a link's frame.  A record is 12 floats:
 *     link index | a[3] | b[3] | radius | r, g, b in [0, 1] | reserved
 * (the colour is kept with 8 bits per channel: base = floor(255 c + 0.5) / 255).  Without a list the RobotTable's collision spheres are
 * rendered (grey, 0.7).  At most PBRE_CAM_MAX_PRIMS primitives; link indices below 256.
 *
 * Camera.  PyBullet's: view[16] and proj[16], column major (OpenGL).  The eye and the camera axes come from `view`, the tangent half
 * extents and centre offsets from proj[0], proj[5], proj[8], proj[9], near and far from proj[10], proj[14]; proj[11] must be -1 (a
 * perspective projection; orthographic: PBRE_E_UNSUPPORTED).  Pixel (row j, column i) looks through NDC x = 2 (i + .5) / W - 1,
 * y = 1 - 2 (j + .5) / H; row 0 is the top.
 *
 * Outputs, per env (a null pointer skips that output):
 *   depth  float32 [N][H][W]      distance along the view axis in metres; a hit outside [near, far] does not count; no hit: far
 *   seg    int32   [N][H][W]      PyBullet's body + ((link + 1) << 24); background -1; floor, table and object have link -1; a robot
 *                                 primitive carries its RobotTable link index.  Equal depths go to the first of: the robot list in order,
 *                                 object, table, floor
 *   rgba   uint8   [N][H][W][4]   flat Lambert shading, no shadows: channel = floor(255 base (ambient + (1 - ambient) max(0, n.l)) + 0.5), A = 255
 * A ray that starts inside a primitive does not see it (entry points only).
 */
#ifndef PBRE_CAMERA_H
#define PBRE_CAMERA_H
#include "pbre.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PBRE_CAM_MAX_PRIMS = 192, PBRE_CAM_PRIM_FLOATS = 12 };

typedef struct {
    float view[16], proj[16];          /* column major */
    int32_t per_env_view;              /* 0: `view` for every env; 1: views[num_envs][16], one per env (camera randomisation) */
    const float* views;                /* HOST memory in both render calls; read before the call returns (pbre_camera_render_device then
                                          waits for their upload on `stream`) */
    int32_t width, height;
    int32_t robot_id, table_id, object_id, floor_id;     /* body ids of the segmentation: 0, 1, 2, 3 */
    float light[3], ambient;           /* unit vector towards the light: normalize(0.3, -0.4, 0.85); 0.4 */
    float background[3], floor_rgb[3], table_rgb[3], object_rgb[3];
} pbre_camera;

/* The defaults above, and the task envs' camera (target the origin, distance 1.3, yaw 180, pitch -40, fov 60, near 0.1, far 100). */
int pbre_camera_default(pbre_camera* cam, int32_t width, int32_t height);
/* records: host [n][PBRE_CAM_PRIM_FLOATS]; n = 0: back to the collision spheres.  PBRE_E_ARG: n > PBRE_CAM_MAX_PRIMS, a bad link
 * index, a negative or non-finite radius. */
int pbre_camera_set_visuals(pbre_ctx* ctx, const float* records, int32_t n);
/* Device buffers on ctx's GPU; enqueued on `stream` (as for pbre_step_device: a hipStream_t, PBRE_STREAM_LEGACY, or NULL = the ctx's own
 * stream) behind whatever step was last enqueued there; asynchronous. */
int pbre_camera_render_device(pbre_ctx* ctx, const pbre_camera* cam, float* d_depth, int32_t* d_seg, uint8_t* d_rgba, void* stream);
/* Host buffers; synchronous (waits for every step in flight first). */
int pbre_camera_render(pbre_ctx* ctx, const pbre_camera* cam, float* depth, int32_t* seg, uint8_t* rgba);

#ifdef __cplusplus
}
#endif
#endif
