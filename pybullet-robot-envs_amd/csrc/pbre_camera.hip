// pbre_camera.hip -- the batched ray-cast camera (include/pbre_camera.h): depth, segmentation and colour images of every env, from the
// state records the engines keep on the device.  Two kernels on the caller's stream:
//   k_cam_scene  one thread per env: forward kinematics of the RobotTable in fp32 (links in table order: parent before child), then the
//                env's visual primitives in world space as 32-byte records (end point a | radius, end point b | link + colour) and the
//                object's rotation and position, [N][8 n_prims + 16] floats.  The link frames go through a buffer [n_links][12][N] (one
//                column per env: coalesced) instead of per-thread arrays, so the kernel needs no scratch memory.
//   k_cam_rays   one 256-thread workgroup per (env, strip of 256 consecutive pixels): the env's records are copied to LDS once (<= 6208
//                bytes), every thread casts one ray through all of them (a loop over the runtime count, not unrolled), then the object in
//                its own frame, the table and the floor.  All three outputs are stored coalesced.  No atomics, nothing between workgroups.
// The ctx's record (pbre_ctx::readers: the RobotTable copy, CamBufs), the link table and the forward kinematics are pbre_scene.hpp's, shared
// with the contact query; the ctx is reached through pbre_engine.hpp (state_view, fail: pbre_capi.hip).
// Neither kernel writes the state.  The per-ray functions are in pbre_camera.hpp (shared with the host tests).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/pbre_camera.h"
#include "pbre_engine.hpp"
#include "pbre_tables.hpp"
#include "pbre_scene.hpp"
#define PBRE_HD __host__ __device__ __forceinline__
#include "pbre_camera.hpp"

namespace pbre {

constexpr int CAM_TPB = 256, SCENE_TPB = 64;

struct RayParams {
    const float* scene; int sstride, nprims;
    const float* views;                         // per-env views [N][16] on the device, or null: `view`
    float view[16];
    float tx, ty, cx, cy, znear, zfar;
    int W, H, npix, strips;
    int ids[4];                                 // robot, table, object, floor
    float light[3], ambient, bg[3], col_floor[3], col_table[3], col_obj[3];
    float tab_c[3], tab_h[3], ground_z, obj_h[3];
    int obj_shape;                              // PBRE_SHAPE_*, -1: no object
    const float* hull;
    float* depth; int* seg; uchar4* rgba;
};

__global__ __launch_bounds__(SCENE_TPB) void k_cam_scene(const float* __restrict__ tab, const float* __restrict__ state, int stride, int n, int obj_lane,
                                                         float* __restrict__ frames, float* __restrict__ scene, int sstride) {
    const int env = blockIdx.x * SCENE_TPB + threadIdx.x;
    if (env >= n) return;
    const float* st = state + (size_t)env * stride;
    const int nl = (int)tab[0], np = (int)tab[1];
    const size_t N = (size_t)n;
    scene_fk(tab, st, env, N, frames);
    float* sc = scene + (size_t)env * sstride;
#pragma unroll 1
    for (int k = 0; k < np; k++) {
        const float* V = tab + CT_HDR + CT_LINK * nl + PBRE_CAM_PRIM_FLOATS * k;
        const int link = (int)V[0];
        const float* F = frames + (size_t)link * 12 * N + env;
        float R[9], p[3];
        for (int j = 0; j < 9; j++) R[j] = F[j * N];
        for (int j = 0; j < 3; j++) p[j] = F[(9 + j) * N];
        float4 a, b;
        a.x = p[0] + R[0] * V[1] + R[1] * V[2] + R[2] * V[3]; a.y = p[1] + R[3] * V[1] + R[4] * V[2] + R[5] * V[3]; a.z = p[2] + R[6] * V[1] + R[7] * V[2] + R[8] * V[3];
        b.x = p[0] + R[0] * V[4] + R[1] * V[5] + R[2] * V[6]; b.y = p[1] + R[3] * V[4] + R[4] * V[5] + R[5] * V[6]; b.z = p[2] + R[6] * V[4] + R[7] * V[5] + R[8] * V[6];
        a.w = V[7];
        b.w = V[8];                          // (bit pattern: link | r << 8 | g << 16 | b << 24, packed on the host)
        ((float4*)sc)[2 * k] = a; ((float4*)sc)[2 * k + 1] = b;
    }
    {   // the object's rotation (quaternion x, y, z, w as stored, not renormalised) and position
        const float* o = st + obj_lane;
        const float x = o[3], y = o[4], z = o[5], w = o[6];
        float4 q0, q1, q2, q3;
        q0.x = 1.0f - 2.0f * (y * y + z * z); q0.y = 2.0f * (x * y - w * z); q0.z = 2.0f * (x * z + w * y);
        q0.w = 2.0f * (x * y + w * z); q1.x = 1.0f - 2.0f * (x * x + z * z); q1.y = 2.0f * (y * z - w * x);
        q1.z = 2.0f * (x * z - w * y); q1.w = 2.0f * (y * z + w * x); q2.x = 1.0f - 2.0f * (x * x + y * y);
        q2.y = o[0]; q2.z = o[1]; q2.w = o[2];
        q3.x = q3.y = q3.z = q3.w = 0.0f;
        float4* O = (float4*)sc + 2 * np;
        O[0] = q0; O[1] = q1; O[2] = q2; O[3] = q3;
    }
}

__global__ __launch_bounds__(CAM_TPB) void k_cam_rays(const RayParams P) {
    __shared__ float4 s[2 * PBRE_CAM_MAX_PRIMS + 4];
    const int env = blockIdx.x / P.strips, strip = blockIdx.x - env * P.strips;
    {
        const float4* src = (const float4*)(P.scene + (size_t)env * P.sstride);
        const int nq = 2 * P.nprims + 4;
        for (int i = threadIdx.x; i < nq; i += CAM_TPB) s[i] = src[i];
    }
    __syncthreads();
    const int pix = strip * CAM_TPB + threadIdx.x;
    if (pix >= P.npix) return;
    const int row = pix / P.W, col = pix - row * P.W;
    float V[16];
    if (P.views) { for (int k = 0; k < 16; k++) V[k] = P.views[(size_t)env * 16 + k]; }
    else { for (int k = 0; k < 16; k++) V[k] = P.view[k]; }
    // view = [R | t] with rows right, up, -forward: eye = -R^T t
    const float o[3] = {-(V[0] * V[12] + V[1] * V[13] + V[2] * V[14]), -(V[4] * V[12] + V[5] * V[13] + V[6] * V[14]), -(V[8] * V[12] + V[9] * V[13] + V[10] * V[14])};
    const float X = ((2.0f * ((float)col + 0.5f)) / (float)P.W - 1.0f + P.cx) * P.tx;
    const float Y = (1.0f - (2.0f * ((float)row + 0.5f)) / (float)P.H + P.cy) * P.ty;
    const float d[3] = {-V[2] + X * V[0] + Y * V[1], -V[6] + X * V[4] + Y * V[5], -V[10] + X * V[8] + Y * V[9]};
    float best = cam::CAM_BIG;
    int who = -1;                            // >= 0: primitive; -2 object, -3 table, -4 floor
    float n[3] = {0.0f, 0.0f, 1.0f};
#pragma unroll 1
    for (int k = 0; k < P.nprims; k++) {
        const float4 A = s[2 * k], B = s[2 * k + 1];
        const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z};
        const float t = cam::ray_capsule(o, d, a, b, A.w);
        if (t >= P.znear && t <= P.zfar && t < best) { best = t; who = k; }
    }
    if (P.obj_shape >= 0) {
        const float4 q0 = s[2 * P.nprims], q1 = s[2 * P.nprims + 1], q2 = s[2 * P.nprims + 2];
        const float R[9] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x};
        const float e[3] = {o[0] - q2.y, o[1] - q2.z, o[2] - q2.w};
        const float ol[3] = {R[0] * e[0] + R[3] * e[1] + R[6] * e[2], R[1] * e[0] + R[4] * e[1] + R[7] * e[2], R[2] * e[0] + R[5] * e[1] + R[8] * e[2]};
        const float dl[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2], R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};
        float t = cam::CAM_MISS, m[3] = {0.0f, 0.0f, 1.0f};
        if (P.obj_shape == PBRE_SHAPE_BOX) {
            const float z3[3] = {0.0f, 0.0f, 0.0f};
            t = cam::ray_box(ol, dl, z3, P.obj_h, m);
        } else if (P.obj_shape == PBRE_SHAPE_SPHERE) {
            const float z3[3] = {0.0f, 0.0f, 0.0f};
            t = cam::ray_capsule(ol, dl, z3, z3, P.obj_h[0]);
            const float x[3] = {ol[0] + t * dl[0], ol[1] + t * dl[1], ol[2] + t * dl[2]};
            cam::capsule_normal(x, z3, z3, m);
        } else if (P.obj_shape == PBRE_SHAPE_CYLINDER) {
            t = cam::ray_cylinder(ol, dl, P.obj_h[0], P.obj_h[2], m);
        } else {
            const float* H = P.hull;
            const int npc = (int)H[0];
            float tb = cam::CAM_BIG;
#pragma unroll 1
            for (int p = 0; p < npc; p++) {
                const float* D = H + HULL_D0 + HULL_DP * p;
                if (!cam::ray_meets_ball(ol, dl, D + 4, D[7] * 1.0001f)) continue;      // (the directory's radius is a rounded float)
                const float* T = H + HULL_T0 + 12 * (int)D[1];
                float mp[3];
                const float tp = cam::ray_planes(ol, dl, T, T + 9, 12, (int)D[3], mp);
                if (tp >= P.znear && tp <= P.zfar && tp < tb) { tb = tp; m[0] = mp[0]; m[1] = mp[1]; m[2] = mp[2]; }
            }
            if (tb < cam::CAM_BIG) t = tb;
        }
        if (t >= P.znear && t <= P.zfar && t < best) {
            best = t; who = -2;
            n[0] = R[0] * m[0] + R[1] * m[1] + R[2] * m[2]; n[1] = R[3] * m[0] + R[4] * m[1] + R[5] * m[2]; n[2] = R[6] * m[0] + R[7] * m[1] + R[8] * m[2];
        }
    }
    {
        float m[3];
        const float t = cam::ray_box(o, d, P.tab_c, P.tab_h, m);
        if (t >= P.znear && t <= P.zfar && t < best) { best = t; who = -3; n[0] = m[0]; n[1] = m[1]; n[2] = m[2]; }
    }
    {
        const float t = cam::ray_floor(o, d, P.ground_z);
        if (t >= P.znear && t <= P.zfar && t < best) { best = t; who = -4; n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f; }
    }
    float base[3] = {P.bg[0], P.bg[1], P.bg[2]};
    int id = -1;
    if (who >= 0) {
        const float4 A = s[2 * who], B = s[2 * who + 1];
        const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z};
        const float x[3] = {o[0] + best * d[0], o[1] + best * d[1], o[2] + best * d[2]};
        cam::capsule_normal(x, a, b, n);
        const unsigned bits = __float_as_uint(B.w);
        id = P.ids[0] + (int)(((bits & 255u) + 1u) << 24);
        base[0] = (float)((bits >> 8) & 255u) / 255.0f; base[1] = (float)((bits >> 16) & 255u) / 255.0f; base[2] = (float)(bits >> 24) / 255.0f;
    } else if (who == -2) { id = P.ids[2]; base[0] = P.col_obj[0]; base[1] = P.col_obj[1]; base[2] = P.col_obj[2]; }
    else if (who == -3) { id = P.ids[1]; base[0] = P.col_table[0]; base[1] = P.col_table[1]; base[2] = P.col_table[2]; }
    else if (who == -4) { id = P.ids[3]; base[0] = P.col_floor[0]; base[1] = P.col_floor[1]; base[2] = P.col_floor[2]; }
    const size_t at = (size_t)env * P.npix + pix;
    if (P.depth) P.depth[at] = who == -1 ? P.zfar : best;
    if (P.seg) P.seg[at] = id;
    if (P.rgba) {
        // (the background is not lit: n . l = 1 with ambient + (1 - ambient) = 1)
        const float nl = who == -1 ? 1.0f : n[0] * P.light[0] + n[1] * P.light[1] + n[2] * P.light[2];
        uchar4 c;
        c.x = (unsigned char)cam::shade(base[0], nl, P.ambient); c.y = (unsigned char)cam::shade(base[1], nl, P.ambient);
        c.z = (unsigned char)cam::shade(base[2], nl, P.ambient); c.w = 255;
        P.rgba[at] = c;
    }
}

}  // namespace pbre

using namespace pbre;

static unsigned pack_colour(int link, const float* rgb) {
    unsigned w = (unsigned)link & 255u;
    for (int k = 0; k < 3; k++) w |= (unsigned)std::fmin(std::fmax(std::floor(255.0 * rgb[k] + 0.5), 0.0), 255.0) << (8 * (k + 1));
    return w;
}

// the float table of the device (see CT_HDR): links of the RobotTable, then the primitives
static std::vector<float> build_device_table(const Readers& s, int& nprims) {
    const double* t = s.table.data();
    std::vector<float> out = scene_link_table(s);
    auto put = [&](int link, const float* a, const float* b, float rad, const float* rgb) {
        float rec[PBRE_CAM_PRIM_FLOATS] = {(float)link, a[0], a[1], a[2], b[0], b[1], b[2], rad, 0, 0, 0, 0};
        const unsigned w = pack_colour(link, rgb);
        std::memcpy(&rec[8], &w, 4);
        out.insert(out.end(), rec, rec + PBRE_CAM_PRIM_FLOATS);
    };
    nprims = 0;
    if (!s.cam.visuals.empty()) {
        for (size_t k = 0; k * PBRE_CAM_PRIM_FLOATS < s.cam.visuals.size(); k++) {
            const float* v = s.cam.visuals.data() + k * PBRE_CAM_PRIM_FLOATS;
            put((int)v[0], v + 1, v + 4, v[7], v + 8); nprims++;
        }
    } else {
        const float grey[3] = {0.7f, 0.7f, 0.7f};
        for (int k = 0; k < s.ns && k < PBRE_CAM_MAX_PRIMS; k++) {
            const double* r = t + 24 + s.nl * 40 + k * 8;
            const float c[3] = {(float)r[1], (float)r[2], (float)r[3]};
            put((int)r[0], c, c, (float)r[4], grey); nprims++;
        }
    }
    out[1] = (float)nprims;
    return out;
}

static int check_camera(pbre_ctx* ctx, const pbre_camera* cam) {
    if (!ctx) return fail(nullptr, PBRE_E_ARG, "pbre_camera_render: null ctx");
    if (!cam) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: null camera");
    if (cam->width < 1 || cam->height < 1) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: width and height must be at least 1");
    if (cam->proj[11] != -1.0f) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_camera_render: proj[11] != -1 (an orthographic projection) is not supported");
    if (!(cam->proj[0] != 0.0f) || !(cam->proj[5] != 0.0f) || !(cam->proj[10] != 1.0f) || !(cam->proj[10] != -1.0f))
        return fail(ctx, PBRE_E_ARG, "pbre_camera_render: degenerate projection matrix");
    if (cam->per_env_view && !cam->views) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: per_env_view without views");
    return PBRE_OK;
}

// enqueue both kernels on v.stream; the outputs are device pointers (null: skipped)
static int render_on(pbre_ctx* ctx, const StateView& v, const pbre_camera* cam, float* d_depth, int32_t* d_seg, uint8_t* d_rgba) {
    Readers& r = ctx->readers;
    CamBufs& s = r.cam;
    if (r.table.empty()) return fail(ctx, PBRE_E_TABLE, "pbre_camera_render: the ctx has no RobotTable");
    if ((long long)v.n * cam->width * cam->height > 2147483647LL) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: num_envs x height x width exceeds INT32_MAX");
    hipStream_t st = (hipStream_t)v.stream;
    if (s.dirty) {
        int np = 0;
        const std::vector<float> tab = build_device_table(r, np);
        PBRE_CHK_ON(ctx, hipDeviceSynchronize());          // (rare: a render on another stream may still read the old table)
        PBRE_CHK_ON(ctx, grow(s.table, s.cap_table, tab.size(), false));
        PBRE_CHK_ON(ctx, hipMemcpy(s.table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        s.nprims = np; s.dirty = false;
    }
    const int sstride = 8 * s.nprims + 16;
    const size_t f_frames = (size_t)std::max(r.nl, 1) * 12 * v.n, f_scene = (size_t)v.n * sstride, f_views = (size_t)v.n * 16;
    PBRE_CHK_ON(ctx, grow(s.work, s.cap_work, f_frames + f_scene + f_views, true));      // (more primitives: a longer scene)
    float *d_frames = s.work, *d_scene = d_frames + f_frames, *d_views = d_scene + f_scene;
    if (cam->per_env_view) {                     // (the caller's array may be gone when this call returns: wait for its upload)
        PBRE_CHK_ON(ctx, hipMemcpyAsync(d_views, cam->views, f_views * sizeof(float), hipMemcpyHostToDevice, st));
        PBRE_CHK_ON(ctx, hipStreamSynchronize(st));
    }
    RayParams P;
    std::memset(&P, 0, sizeof P);
    P.scene = d_scene; P.sstride = sstride; P.nprims = s.nprims;
    P.views = cam->per_env_view ? d_views : nullptr;
    for (int k = 0; k < 16; k++) P.view[k] = cam->view[k];
    P.tx = 1.0f / cam->proj[0]; P.ty = 1.0f / cam->proj[5]; P.cx = cam->proj[8]; P.cy = cam->proj[9];
    P.znear = cam->proj[14] / (cam->proj[10] - 1.0f); P.zfar = cam->proj[14] / (cam->proj[10] + 1.0f);
    P.W = cam->width; P.H = cam->height; P.npix = cam->width * cam->height; P.strips = (P.npix + CAM_TPB - 1) / CAM_TPB;
    P.ids[0] = cam->robot_id; P.ids[1] = cam->table_id; P.ids[2] = cam->object_id; P.ids[3] = cam->floor_id;
    P.ambient = cam->ambient;
    for (int k = 0; k < 3; k++) {
        P.light[k] = cam->light[k]; P.bg[k] = cam->background[k]; P.col_floor[k] = cam->floor_rgb[k]; P.col_table[k] = cam->table_rgb[k]; P.col_obj[k] = cam->object_rgb[k];
        P.tab_c[k] = (float)v.phys.table_c[k]; P.tab_h[k] = (float)v.phys.table_h[k]; P.obj_h[k] = (float)v.phys.obj_h[k];
    }
    P.ground_z = (float)v.phys.ground_z;
    P.obj_shape = (v.flags & PBRE_F_NO_OBJECT) ? -1 : v.phys.obj_shape;
    P.hull = v.hull;
    if (P.obj_shape == PBRE_SHAPE_HULL && !P.hull) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: a hull object without a hull table");
    P.depth = d_depth; P.seg = d_seg; P.rgba = (uchar4*)d_rgba;
    hipLaunchKernelGGL(k_cam_scene, dim3((v.n + SCENE_TPB - 1) / SCENE_TPB), dim3(SCENE_TPB), 0, st, (const float*)s.table, v.state, v.stride, v.n, v.obj_lane, d_frames, d_scene, sstride);
    PBRE_CHK_ON(ctx, hipGetLastError());
    if (d_depth || d_seg || d_rgba) {
        hipLaunchKernelGGL(k_cam_rays, dim3((unsigned)v.n * (unsigned)P.strips), dim3(CAM_TPB), 0, st, P);
        PBRE_CHK_ON(ctx, hipGetLastError());
    }
    return PBRE_OK;
}

extern "C" {

int pbre_camera_default(pbre_camera* cam, int32_t width, int32_t height) {
    if (!cam || width < 1 || height < 1) return PBRE_E_ARG;
    std::memset(cam, 0, sizeof *cam);
    cam->width = width; cam->height = height;
    cam->robot_id = 0; cam->table_id = 1; cam->object_id = 2; cam->floor_id = 3;
    const double l[3] = {0.3, -0.4, 0.85}, ln = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    for (int k = 0; k < 3; k++) cam->light[k] = (float)(l[k] / ln);
    cam->ambient = 0.4f;
    const float bg[3] = {0.75f, 0.85f, 1.0f}, fl[3] = {0.6f, 0.6f, 0.6f}, tb[3] = {0.55f, 0.4f, 0.25f}, ob[3] = {0.9f, 0.2f, 0.2f};
    for (int k = 0; k < 3; k++) { cam->background[k] = bg[k]; cam->floor_rgb[k] = fl[k]; cam->table_rgb[k] = tb[k]; cam->object_rgb[k] = ob[k]; }
    // the task envs' camera about the origin: yaw 180, pitch -40, roll 0, distance 1.3 -- forward f = (-cos p sin y, cos p cos y, sin p),
    // up = Rz(yaw) Rx(pitch) z, then a look-at
    const double PI = 3.14159265358979323846, yaw = PI, pitch = -40.0 * PI / 180.0, dist = 1.3;
    const double f[3] = {-std::cos(pitch) * std::sin(yaw), std::cos(pitch) * std::cos(yaw), std::sin(pitch)};
    const double up0[3] = {std::sin(yaw) * std::sin(pitch), -std::cos(yaw) * std::sin(pitch), std::cos(pitch)};
    const double eye[3] = {-dist * f[0], -dist * f[1], -dist * f[2]};
    double r[3] = {f[1] * up0[2] - f[2] * up0[1], f[2] * up0[0] - f[0] * up0[2], f[0] * up0[1] - f[1] * up0[0]};
    const double rn = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double& x : r) x /= rn;
    const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
    for (int k = 0; k < 3; k++) { cam->view[4 * k] = (float)r[k]; cam->view[4 * k + 1] = (float)u[k]; cam->view[4 * k + 2] = (float)-f[k]; }
    cam->view[12] = (float)-(r[0] * eye[0] + r[1] * eye[1] + r[2] * eye[2]);
    cam->view[13] = (float)-(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
    cam->view[14] = (float)(f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]);
    cam->view[15] = 1.0f;
    const double fov = 60.0 * PI / 180.0, zn = 0.1, zf = 100.0, ft = 1.0 / std::tan(0.5 * fov);
    cam->proj[0] = (float)(ft / ((double)width / (double)height)); cam->proj[5] = (float)ft;
    cam->proj[10] = (float)(-(zf + zn) / (zf - zn)); cam->proj[11] = -1.0f; cam->proj[14] = (float)(-2.0 * zf * zn / (zf - zn));
    return PBRE_OK;
}

int pbre_camera_set_visuals(pbre_ctx* ctx, const float* records, int32_t n) {
    if (!ctx) return fail(nullptr, PBRE_E_ARG, "pbre_camera_set_visuals: null ctx");
    StateView v;
    const int rc = ctx->state_view(&v, nullptr, false);
    if (rc != PBRE_OK) return rc;
    if (n < 0 || (n > 0 && !records)) return fail(ctx, PBRE_E_ARG, "pbre_camera_set_visuals: bad arguments");
    if (n > PBRE_CAM_MAX_PRIMS) return fail(ctx, PBRE_E_ARG, "pbre_camera_set_visuals: more than 192 primitives");
    for (int k = 0; k < n; k++) {
        const float* r = records + (size_t)k * PBRE_CAM_PRIM_FLOATS;
        bool ok = r[0] >= 0.0f && r[0] < (float)ctx->readers.nl && r[0] < 256.0f && r[0] == std::floor(r[0]) && r[7] >= 0.0f;
        for (int j = 1; j < 11; j++) ok = ok && std::isfinite(r[j]);
        if (!ok) return fail(ctx, PBRE_E_ARG, "pbre_camera_set_visuals: bad record (link index out of range, negative radius or a non-finite value)");
    }
    ctx->readers.cam.visuals.assign(records, records + (size_t)n * PBRE_CAM_PRIM_FLOATS);
    ctx->readers.cam.dirty = true;
    return PBRE_OK;
}

int pbre_camera_render_device(pbre_ctx* ctx, const pbre_camera* cam, float* d_depth, int32_t* d_seg, uint8_t* d_rgba, void* stream) {
    int rc = check_camera(ctx, cam);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, stream, false)) != PBRE_OK) return rc;
    return render_on(ctx, v, cam, d_depth, d_seg, d_rgba);
}

int pbre_camera_render(pbre_ctx* ctx, const pbre_camera* cam, float* depth, int32_t* seg, uint8_t* rgba) {
    int rc = check_camera(ctx, cam);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, nullptr, true)) != PBRE_OK) return rc;
    if ((long long)v.n * cam->width * cam->height > 2147483647LL) return fail(ctx, PBRE_E_ARG, "pbre_camera_render: num_envs x height x width exceeds INT32_MAX");
    const size_t px = (size_t)v.n * cam->width * cam->height;
    hipStream_t st = (hipStream_t)v.stream;
    Stage sg;                                    // depth | seg | rgba, 4 bytes per pixel each
    const int i_depth = sg.add(depth, px * 4), i_seg = sg.add(seg, px * 4), i_rgba = sg.add(rgba, px * 4);
    PBRE_CHK_ON(ctx, sg.begin(ctx->readers.cam.out, ctx->readers.cam.cap_out, st));
    if ((rc = render_on(ctx, v, cam, sg.dev<float>(i_depth), sg.dev<int32_t>(i_seg), sg.dev<uint8_t>(i_rgba))) != PBRE_OK) return rc;
    PBRE_CHK_ON(ctx, sg.finish(st));
    return PBRE_OK;
}

}  // extern "C"
