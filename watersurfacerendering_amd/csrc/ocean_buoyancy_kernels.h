// ocean_buoyancy_kernels.h -- the kernel behind ocean_buoyancy_bodies (include/ocean_consumers.h), compiled into ocean_consumers.hip only:
// net force and torque on floating bodies, a segmented reduction over the surface query.  Calls the query's own query_point
// (ocean_consumer_kernels.h; solve_rest + eval_surface): the water under a hull point is exactly what ocean_query_surface answers there.
// The flow form (ocean_buoyancy_bodies_flow) is the same kernel with the drag taken against the water's own velocity, read from the derivative
// twin tiles of the cascade set (ocean_velocity_kernels.h: water_velocity) at the rest point that gave the height.
#pragma once
#include "ocean_velocity_kernels.h"     // (includes ocean_consumer_kernels.h)

namespace ocean {

// One wave64 per body, four bodies per 256-thread block.  Lane k is slot k of the header's reduction: it walks the body's hull points
// k, k + 64, k + 128, ... in that order and adds each point's seven terms to accumulators that start at +0.0f (the residual: fmaxf).  The trip
// count is the same for every lane of the wave, so all 64 lanes reach the tree: six __shfl_down steps per channel, off = 32, 16, 8, 4, 2, 1,
// slot[k] = slot[k] + slot[k + off].  A lane k < off reads lane k + off < 2 off, which the previous steps have left holding slot[k + off]
// of the definition; what the lanes >= off compute is never read by a lane that counts.  Lane 0 writes the two float4.  No LDS, no
// atomics, and the order of every addition is fixed: the result is bit-reproducible and tests/buoyancy.py repeats it step for step.
// fp32, no contraction.  A wave whose body index is past the end leaves as a whole (there is no block-wide step).
struct BuoyancyArgs {
    QueryArgs q;                       // the surface (q.xz / out_* / points unused)
    const float4* hull;                // [hull_points] local x, y, z, edge e
    const float* bodies;               // [count][16] words of ocean_body (words 13 and 14, first_point and points, are read as uint32_t)
    float4* out_force;                 // [count]  (F.x, F.y, F.z, submerged volume)
    float4* out_torque;                // [count]  (T.x, T.y, T.z, largest residual)
    unsigned hull_points;
    unsigned count;
    float weight;                      // density * gravity, one float product on the host
    float drag;
    TwinMaps tw;                       // FLOW only: the twins of the cascade set (null otherwise, never read)
};

constexpr int BUOYANCY_BODIES_PER_BLOCK = 4;

// FLOW = false is ocean_buoyancy_bodies as it always was (query_point in the middle); FLOW = true solves the same rest point itself, because it
// needs it a second time for the twins' gather: the height and the residual are query_point's expressions, the normal is not formed.
template <bool FLOW>
__global__ void __launch_bounds__(256) k_buoyancy_bodies(const BuoyancyArgs b)
{
#pragma clang fp contract(off)
    const QueryArgs& a = b.q;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned body = blockIdx.x * BUOYANCY_BODIES_PER_BLOCK + (threadIdx.x >> 6);
    if (body >= b.count) return;
    float amp[OCEAN_MAX_CASCADES];
    cascade_amplitudes(a.s.minmax, a.s.count, amp);
    float tamp[OCEAN_MAX_CASCADES];
    if constexpr (FLOW) cascade_amplitudes(b.tw.minmax, a.s.count, tamp);

    const float* w = b.bodies + (size_t)body * 16;
    const float posx = w[0], posy = w[1], posz = w[2];
    const float qx = w[3], qy = w[4], qz = w[5], qw = w[6];
    const float velx = w[7], vely = w[8], velz = w[9];
    const float omx = w[10], omy = w[11], omz = w[12];
    // the body's range of the hull, clamped to it: a body never reads outside the hull buffer, whatever its words say
    const uint32_t* wu = reinterpret_cast<const uint32_t*>(w);
    const unsigned first = min(wu[13], b.hull_points);
    const unsigned points = min(wu[14], b.hull_points - first);

    float fx = 0.0f, fy = 0.0f, fz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f, vol = 0.0f, res = 0.0f;
    const unsigned trips = (points + 63u) >> 6;
    for (unsigned t = 0; t < trips; ++t) {
        const unsigned i = t * 64u + lane;
        if (i >= points) continue;
        const float4 l = b.hull[first + i];
        const float e = l.w;
        // arm: the hull point rotated by the quaternion as given, t = 2 cross(q.xyz, l), a = (l + w t) + cross(q.xyz, t)
        const float t0 = 2.0f * (qy * l.z - qz * l.y), t1 = 2.0f * (qz * l.x - qx * l.z), t2 = 2.0f * (qx * l.y - qy * l.x);
        const float ax = (l.x + qw * t0) + (qy * t2 - qz * t1);
        const float ay = (l.y + qw * t1) + (qz * t0 - qx * t2);
        const float az = (l.z + qw * t2) + (qx * t1 - qy * t0);
        const float px = posx + ax, py = posy + ay, pz = posz + az;
        // the water under the point is the query's own answer there: H = out_pos.y, the residual = out_nrm.w (the normal is not used)
        float height, residual, wvx = 0.0f, wvy = 0.0f, wvz = 0.0f;
        if constexpr (FLOW) {
            float rx, rz;
            solve_rest(a, amp, px, pz, rx, rz);
            const SurfaceEval ev = eval_surface(a, amp, rx, rz);
            const float ex = (rx + ev.dx) - px, ez = (rz + ev.dz) - pz;
            height = 0.0f + ev.dy;
            residual = sqrtf(ex * ex + ez * ez);
            water_velocity(a, b.tw, tamp, rx, rz, wvx, wvy, wvz);
        } else {
            float4 wpos, wnrm;
            query_point(a, amp, px, pz, wpos, wnrm);
            height = wpos.y; residual = wnrm.w;
        }
        const float s = fminf(fmaxf((height - py) / e + 0.5f, 0.0f), 1.0f);
        const float v = s * ((e * e) * e);
        // the point's own velocity, Archimedes straight up, linear drag in proportion to the submerged volume
        float ux = velx + (omy * az - omz * ay), uy = vely + (omz * ax - omx * az), uz = velz + (omx * ay - omy * ax);
        if constexpr (FLOW) { ux = ux - wvx; uy = uy - wvy; uz = uz - wvz; }      // ... relative to the water
        const float dv = b.drag * v;
        const float px_f = -dv * ux, py_f = b.weight * v - dv * uy, pz_f = -dv * uz;
        fx = fx + px_f; fy = fy + py_f; fz = fz + pz_f;
        tx = tx + (ay * pz_f - az * py_f);
        ty = ty + (az * px_f - ax * pz_f);
        tz = tz + (ax * py_f - ay * px_f);
        vol = vol + v;
        res = fmaxf(res, residual);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        fx = fx + __shfl_down(fx, off); fy = fy + __shfl_down(fy, off); fz = fz + __shfl_down(fz, off);
        tx = tx + __shfl_down(tx, off); ty = ty + __shfl_down(ty, off); tz = tz + __shfl_down(tz, off);
        vol = vol + __shfl_down(vol, off);
        res = fmaxf(res, __shfl_down(res, off));
    }
    if (lane != 0) return;
    b.out_force[body] = make_float4(fx, fy, fz, vol);
    b.out_torque[body] = make_float4(tx, ty, tz, res);
}

}  // namespace ocean
