// ocean_velocity_kernels.h -- the kernel behind ocean_query_velocity (include/ocean_consumers.h), compiled into ocean_consumers.hip only, and
// what it shares with the flow form of the buoyancy kernel (ocean_buoyancy_kernels.h): the water's own velocity from derivative twin tiles.
// A twin is a tile whose spectrum Prepare replaced by i w h0 of its source (k_derive_spectrum, ocean_aux_kernels.h); the unchanged frame
// pipeline then writes the time derivative of the source's maps into the twin's.  Builds on the query's solve_rest / eval_surface
// (ocean_consumer_kernels.h), whose argument block and kernels stay as they are: the twin set travels beside QueryArgs, not in it.
#pragma once
#include "ocean_consumer_kernels.h"

namespace ocean {

// The twins of the cascade set of a QueryArgs: consecutive tiles, twin c at + c * tile_texels (keys: + 2 c), in cascade order.
struct TwinMaps {
    const float4* disp;                // displacement map of the FIRST twin: (lambda dDx/dt, (dh/dt) / A', lambda dDz/dt, -)
    const unsigned* minmax;            // height keys of the first twin: A' = the largest magnitude of dh/dt
};

// V at a given (u, v), tamp = the twins' A' (cascade_amplitudes of tw.minmax): the twins' displacement maps at the uv the sources are sampled at, summed in cascade order from 0.0f.
// One bilinear float4 gather per cascade.
__device__ __forceinline__ void water_velocity_uv(const QueryArgs& a, const TwinMaps& tw, const float (&tamp)[OCEAN_MAX_CASCADES], float u, float v,
                                                  float& vx, float& vy, float& vz)
{
#pragma clang fp contract(off)
    vx = 0.0f; vy = 0.0f; vz = 0.0f;
#pragma unroll
    for (int c = 0; c < OCEAN_MAX_CASCADES; ++c) {
        if (c >= a.s.count) break;
        const float4 d = sample_linear_repeat(tw.disp + (size_t)c * a.s.tile_texels, a.s.n, u * a.s.uv_scale[c], v * a.s.uv_scale[c]);
        vx = vx + d.x; vy = vy + d.y * tamp[c]; vz = vz + d.z;
    }
}

// ... at rest point r: the uv eval_surface samples the sources at, outside the Newton loop.
__device__ __forceinline__ void water_velocity(const QueryArgs& a, const TwinMaps& tw, const float (&tamp)[OCEAN_MAX_CASCADES], float rx, float rz,
                                               float& vx, float& vy, float& vz)
{
    water_velocity_uv(a, tw, tamp, rest_uv(a, rx), rest_uv(a, rz), vx, vy, vz);
}

// Velocity query: one thread per point; the K + 1 evaluations of the surface query, then one more gather per cascade from the twins.
// out_pos is query_point's pos, expression for expression; out_vel.w its residual.  tests/velocity.py repeats it step for step.
struct VelocityArgs {
    QueryArgs q;                       // the surface (q.out_nrm unused; q.out_pos = out_pos)
    TwinMaps tw;
    float4* out_vel;                   // [points]  (V.x, V.y, V.z, residual)
};

__global__ void __launch_bounds__(256) k_query_velocity(const VelocityArgs va)
{
#pragma clang fp contract(off)
    const QueryArgs& a = va.q;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.points) return;
    float amp[OCEAN_MAX_CASCADES], tamp[OCEAN_MAX_CASCADES];
    cascade_amplitudes(a.s.minmax, a.s.count, amp);
    cascade_amplitudes(va.tw.minmax, a.s.count, tamp);
    const float2 q = a.xz[i];
    float rx, rz;
    solve_rest(a, amp, q.x, q.y, rx, rz);
    const SurfaceEval e = eval_surface(a, amp, rx, rz);
    const float px = rx + e.dx, pz = rz + e.dz;
    const float ex = px - q.x, ez = pz - q.y;
    float vx, vy, vz;
    water_velocity(a, va.tw, tamp, rx, rz, vx, vy, vz);
    a.out_pos[i] = make_float4(px, 0.0f + e.dy, pz, e.w);
    va.out_vel[i] = make_float4(vx, vy, vz, sqrtf(ex * ex + ez * ez));
}

}  // namespace ocean
