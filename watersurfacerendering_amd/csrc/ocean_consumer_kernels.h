// ocean_consumer_kernels.h -- the kernels behind include/ocean_consumers.h, compiled into ocean_consumers.hip only: the vertex stage and its
// cascades, the mip chain, the surface query and the ray cast -- and what every consumer of the maps shares: CascadeSet,
// height_amplitude, rest_uv, cascade_sum, vertex_normal.  Foam: ocean_foam_kernels.h; LOD: ocean_lod_kernels.h; frames: ocean_kernels.h.
#pragma once
#include "ocean_kernels.h"

namespace ocean {

// ============================================================================
// Vertex-stage consumer: what the reference's vertex shader does with
// the two maps (src/shaders/WaterSurfaceMesh.vert:24-41) for the grid its mesh generator
// builds (WaterSurfaceMesh.cpp:500-533), as a kernel -- displaced positions and normals for a
// consumer that is not the Vulkan renderer.  Sampling is the sampler the reference creates
// (vulkan/Sampler.cpp:60-66): LINEAR filter, REPEAT addressing, unnormalised coordinate
// s = u*W - 0.5, texels floor(s) and floor(s)+1 (mod W), weights from frac(s), evaluated in
// fp32 in the order written below (no contraction), which oracle/consumer.py repeats.
// One thread per vertex; memory-bound (8 texel reads that mostly hit in cache, 2 writes).
// ============================================================================
constexpr int OCEAN_MAX_CASCADES = 8;

// What every consumer reads of a cascade set: the consecutive tiles first .. first + count - 1 of one frame (a single tile: count = 1).
struct CascadeSet {
    const float4* disp;      // [N][N] maps of the FIRST tile of the set (tile c at + c * tile_texels)
    const float4* nrm;
    const unsigned* minmax;  // keys of the first tile's raw height range, 2 per tile (A = max(|min|, |max|) = WSHeightAmp)
    size_t tile_texels;      // N * N
    int n;                   // map size
    int count;               // cascades, 1 .. OCEAN_MAX_CASCADES
    float uv_scale[OCEAN_MAX_CASCADES];    // ubo.scale of every cascade, 0 beyond count
};

// The vertex stage's arguments: the set and the grid it fills.
struct CascadeArgs {
    CascadeSet s;
    float4* positions;       // [(g+1)^2]  xyz = displaced position, w = displacement.w (jacobian slot)
    float4* normals;         // [(g+1)^2]  xyz = unit normal, w = 0
    int grid;                // quads per side (kTileSize of CreateGridVertices)
    float vertex_distance;   // kScale
    float choppy;            // ubo.WSChoppy = GetDisplacementLambda()
};
struct GridArgs : CascadeArgs {};      // k_displace_grid's: a set of one tile

// A_c of cascade c: the largest magnitude of its height keys.
__device__ __forceinline__ float height_amplitude(const unsigned* minmax, int c)
{
    return fmaxf(fabsf(key_float(minmax[2 * c + 0])), fabsf(key_float(minmax[2 * c + 1])));
}

// ... of every cascade of a set, 0 beyond count.
__device__ __forceinline__ void cascade_amplitudes(const unsigned* minmax, int count, float (&amp)[OCEAN_MAX_CASCADES])
{
#pragma unroll
    for (int c = 0; c < OCEAN_MAX_CASCADES; ++c) amp[c] = c < count ? height_amplitude(minmax, c) : 0.0f;
}

// The reference's normal from slopes and displacement derivatives (.vert:34-38), one sample's or the cascades' sums.
__device__ __forceinline__ float3 vertex_normal(float sx, float sz, float ddx, float ddz, float choppy)
{
#pragma clang fp contract(off)
    const float nx = -(sx / (1.0f + choppy * ddx));
    const float nz = -(sz / (1.0f + choppy * ddz));
    const float len = sqrtf(nx * nx + 1.0f + nz * nz);
    return make_float3(nx / len, 1.0f / len, nz / len);
}

// Vertex i of the grid: its rest point (WaterSurfaceMesh.cpp:514-518) and its uv.  False past the last vertex.
__device__ __forceinline__ bool grid_vertex(const CascadeArgs& o, int i, float& px, float& pz, float& u, float& v)
{
#pragma clang fp contract(off)
    const int side = o.grid + 1;
    if (i >= side * side) return false;
    const int half = o.grid / 2;
    const int xi = i % side - half, yi = i / side - half;
    px = (float)xi * o.vertex_distance; pz = (float)yi * o.vertex_distance;
    u = (float)(xi + half) / (float)o.grid; v = (float)(yi + half) / (float)o.grid;
    return true;
}

__device__ __forceinline__ float4 sample_linear_repeat(const float4* __restrict__ tex, int n, float u, float v)
{
#pragma clang fp contract(off)
    const float s = u * (float)n - 0.5f, t = v * (float)n - 0.5f;
    const float fs = floorf(s), ft = floorf(t);
    const float a = s - fs, b = t - ft;
    const int x0 = (int)fs & (n - 1), y0 = (int)ft & (n - 1);
    const int x1 = (x0 + 1) & (n - 1), y1 = (y0 + 1) & (n - 1);
    const float4 t00 = tex[(unsigned)(y0 * n + x0)], t10 = tex[(unsigned)(y0 * n + x1)];
    const float4 t01 = tex[(unsigned)(y1 * n + x0)], t11 = tex[(unsigned)(y1 * n + x1)];
    const float ia = 1.0f - a, ib = 1.0f - b;
    auto mix = [&](float c00, float c10, float c01, float c11) {
        return (c00 * ia + c10 * a) * ib + (c01 * ia + c11 * a) * b;
    };
    return make_float4(mix(t00.x, t10.x, t01.x, t11.x), mix(t00.y, t10.y, t01.y, t11.y),
                       mix(t00.z, t10.z, t01.z, t11.z), mix(t00.w, t10.w, t01.w, t11.w));
}

// LOD (include/ocean_consumers.h: ocean_sample_surface_lod): the level that fits a footprint of rho texels and the blend towards the next one.
// rho <= 1 (and 0, negative, NaN) stays on the map itself; rho >= top = 2^Lmax sits on the last level; in between lev = floor(log2 rho) is
// rho's exponent field and t = rho / 2^lev - 1 its mantissa, both exact -- the blend is linear in rho, so no log2f whose bits the tests'
// numpy restatement (tests/lod.py: np.frexp) could not repeat.
__device__ __forceinline__ void lod_level(float rho, int lmax, float top, int& lev, float& t)
{
    lev = 0; t = 0.0f;
    if (!(rho > 1.0f)) return;
    if (rho >= top) { lev = lmax; return; }
    const unsigned bits = __float_as_uint(rho);                        // positive, normal: 1 < rho < 2^12
    lev = (int)(bits >> 23) - 127;
    t = __uint_as_float((bits & 0x007fffffu) | 0x3f800000u) - 1.0f;    // ldexpf(rho, -lev) - 1
}

// Level l of a tile: the map itself, or its place in the tile's packed chain (l >= 1 starts at texel sum_{k=1}^{l-1} (n >> k)^2).
__device__ __forceinline__ const float4* lod_level_ptr(const float4* __restrict__ map, const float4* __restrict__ chain, int n, int l)
{
    if (l == 0) return map;
    const unsigned n2 = (unsigned)n * (unsigned)n, m = (unsigned)n >> (l - 1);
    return chain + (n2 - m * m) / 3u;
}

// The trilinear sample: sample_linear_repeat on level lev (extent n >> lev; the 1 x 1 level works with the same index masks) and, where
// t != 0, on level lev + 1, blended A * (1 - t) + B * t per channel.  t == 0 never reads the upper level.
__device__ __forceinline__ float4 sample_lod(const float4* __restrict__ map, const float4* __restrict__ chain, int n, int lev, float t, float u, float v)
{
#pragma clang fp contract(off)
    const float4 a = sample_linear_repeat(lod_level_ptr(map, chain, n, lev), n >> lev, u, v);
    if (t == 0.0f) return a;
    const float4 b = sample_linear_repeat(lod_level_ptr(map, chain, n, lev + 1), n >> (lev + 1), u, v);
    const float it = 1.0f - t;
    return make_float4(a.x * it + b.x * t, a.y * it + b.y * t, a.z * it + b.z * t, a.w * it + b.w * t);
}

__global__ void k_displace_grid(const GridArgs g)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float px, pz, u, v;
    if (!grid_vertex(g, i, px, pz, u, v)) return;
    const float amp = height_amplitude(g.s.minmax, 0);
    const float us = u * g.s.uv_scale[0], vs = v * g.s.uv_scale[0];    // .vert:26
    float4 d = sample_linear_repeat(g.s.disp, g.s.n, us, vs);
    d.y = d.y * amp;                                               // .vert:27
    g.positions[i] = make_float4(px + d.x, 0.0f + d.y, pz + d.z, d.w);   // .vert:28-29
    const float4 sl = sample_linear_repeat(g.s.nrm, g.s.n, us, vs);    // .vert:33
    const float3 nv = vertex_normal(sl.x, sl.y, sl.z, sl.w, g.choppy);
    g.normals[i] = make_float4(nv.x, nv.y, nv.z, 0.0f);
}

// Cascades (the reference's own to-do "Endless - solving the tiling artifacts", README.md:37-44): the
// usual cure for the visible repetition of one FFT tile is to add several tiles of different lengths and seeds, each
// sampled at its own rate.  The tiles of a batch already are independent oceans with their own tile length, so the
// consumer only has to sum them: vertex = grid point + sum_c D_c(uv * s_c) (each height times its own amplitude A_c),
// normal from the summed slopes and summed displacement derivatives with the reference's formula (.vert:34-38).
// w carries the smallest Jacobian slot of the cascades (all 1 unless OCEAN_MODE_JACOBIAN).
struct SurfaceEval {
    float dx, dy, dz, w;               // summed displacement (heights times their amplitude), smallest Jacobian slot
    float sx, sz, ddx, ddz;            // summed normal-map samples
    float jx, jz;                      // sum_c gain_c * (nrm_c.z, nrm_c.w): the Newton step's, 0 where JACOBIAN is not asked for
};

// The maps themselves as the sum's sampler; sample_lod at a per-cascade level is the other one (LodSampler, ocean_lod_kernels.h).
struct MapSampler {
    __device__ __forceinline__ void operator()(const CascadeSet& s, int c, float us, float vs, float4& d, float4& sl) const
    {
        d = sample_linear_repeat(s.disp + (size_t)c * s.tile_texels, s.n, us, vs);
        sl = sample_linear_repeat(s.nrm + (size_t)c * s.tile_texels, s.n, us, vs);
    }
};

// THE cascade sum at (u, v): every cascade's two samples, summed in cascade order from 0.0f / FLT_MAX, no contraction.  each(c, d, sl) is
// shown the samples of cascade c before they are added (the spray emitters' per-cascade Jacobian).  UNROLLED = false: a runtime loop that
// reads A_c from the keys (the vertex stages); true: unrolled, amplitudes in `amp` (cascade_amplitudes; the queries).  JACOBIAN adds the
// Newton step's sums from `gain`.  amp / gain are read only where their flag is set.
template <bool UNROLLED, bool JACOBIAN, class Sampler, class Each>
__device__ __forceinline__ SurfaceEval cascade_sum(const CascadeSet& s, const float* amp, const float* gain, float u, float v,
                                                   Sampler&& sample, Each&& each)
{
#pragma clang fp contract(off)
    SurfaceEval e{0.0f, 0.0f, 0.0f, 3.402823466e+38f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma clang loop unroll_count(UNROLLED ? OCEAN_MAX_CASCADES : 1)
    for (int c = 0; c < (UNROLLED ? OCEAN_MAX_CASCADES : s.count); ++c) {
        if (UNROLLED && c >= s.count) break;
        const float us = u * s.uv_scale[c], vs = v * s.uv_scale[c];
        const float a = UNROLLED ? amp[c] : height_amplitude(s.minmax, c);
        float4 d, sl;
        sample(s, c, us, vs, d, sl);
        each(c, d, sl);
        e.dx = e.dx + d.x; e.dy = e.dy + d.y * a; e.dz = e.dz + d.z;
        e.w = fminf(e.w, d.w);
        e.sx = e.sx + sl.x; e.sz = e.sz + sl.y; e.ddx = e.ddx + sl.z; e.ddz = e.ddz + sl.w;
        if constexpr (JACOBIAN) { e.jx = e.jx + sl.z * gain[c]; e.jz = e.jz + sl.w * gain[c]; }
    }
    return e;
}

struct NoEach { __device__ __forceinline__ void operator()(int, const float4&, const float4&) const {} };

// The cascade vertex stage for vertex i, through either sampler.
template <class Sampler>
__device__ __forceinline__ void displace_grid_vertex(const CascadeArgs& a, int i, Sampler&& sample)
{
#pragma clang fp contract(off)
    float px, pz, u, v;
    if (!grid_vertex(a, i, px, pz, u, v)) return;
    const SurfaceEval e = cascade_sum<false, false>(a.s, nullptr, nullptr, u, v, sample, NoEach{});
    a.positions[i] = make_float4(px + e.dx, 0.0f + e.dy, pz + e.dz, e.w);
    const float3 nv = vertex_normal(e.sx, e.sz, e.ddx, e.ddz, a.choppy);
    a.normals[i] = make_float4(nv.x, nv.y, nv.z, 0.0f);
}

__global__ void k_displace_grid_cascades(const CascadeArgs a)
{
    displace_grid_vertex(a, blockIdx.x * blockDim.x + threadIdx.x, MapSampler{});
}

// Mip chain of the maps (the reference's LOD hook: s_kUseMipMapping, WaterSurfaceMesh.h:216; Texture2D::GenerateMipmaps,
// vulkan/Texture2D.cpp:228-330 -- level i = vkCmdBlitImage(VK_FILTER_LINEAR) of level i-1 into half the extent).  An exact 2:1
// linear blit samples the point shared by four source texels: the bilinear formula of sample_linear_repeat with both weights
// 1/2, evaluated in the same order (oracle/consumer.py::mip_chain repeats it).  One launch per level, both maps per launch
// (blockIdx.y); a level is N^2/4^l texels, so everything after the first two is launch latency.
struct MipArgs {
    const float4* src[2];    // level l-1 of the displacement map, of the normal map
    float4* dst[2];          // level l
    int w;                   // extent of level l (source extent 2w)
};
__global__ void k_mip_level(const MipArgs m)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m.w * m.w) return;
    const int x = i % m.w, y = i / m.w, sw = 2 * m.w;
    const float4* __restrict__ s = m.src[blockIdx.y];
    const float4 t00 = s[(unsigned)((2 * y) * sw + 2 * x)], t10 = s[(unsigned)((2 * y) * sw + 2 * x + 1)];
    const float4 t01 = s[(unsigned)((2 * y + 1) * sw + 2 * x)], t11 = s[(unsigned)((2 * y + 1) * sw + 2 * x + 1)];
    auto mix = [](float c00, float c10, float c01, float c11) { return (c00 * 0.5f + c10 * 0.5f) * 0.5f + (c01 * 0.5f + c11 * 0.5f) * 0.5f; };
    m.dst[blockIdx.y][i] = make_float4(mix(t00.x, t10.x, t01.x, t11.x), mix(t00.y, t10.y, t01.y, t11.y),
                                       mix(t00.z, t10.z, t01.z, t11.z), mix(t00.w, t10.w, t01.w, t11.w));
}

// Surface query (include/ocean_consumers.h: ocean_query_surface): the displaced height and normal of the surface the vertex stage draws
// (k_displace_grid_cascades) at arbitrary points q = (x, z).  The water above rest point r sits at P(r).xz = r + D(r).xz, so the rest point
// of q is solved for with a diagonal Newton iteration from r_0 = q:
//   r_{k+1} = r_k - (P(r_k).xz - q) / J(r_k),   J = 1 + sum_c gain_c * (nrm_c.z, nrm_c.w),   |J| clamped to >= 0.1 (sign kept, 0 -> +0.1)
// gain_c = lambda_c * (s_c * L_c / (grid * vertex_distance)) (host-computed): the normal map's z / w hold dDx/dx, dDz/dz in ocean metres,
// one mesh metre is s_c * L_c / (grid * vertex_distance) ocean metres of tile c, and disp.x carries lambda.  P, the normal and
// w = min_c D_c.w are then evaluated at r_K exactly as the cascade vertex stage would for a vertex at r_K; out_nrm.w = |P(r_K).xz - q|.
// One thread per point; K + 1 evaluations of 2 bilinear float4 gathers per cascade, all in fp32 in the order written below (no
// contraction), which tests/surface_query.py repeats step for step.
struct QueryArgs {
    CascadeSet s;
    float gain[OCEAN_MAX_CASCADES];    // the Newton step's unit factor per cascade
    const float2* xz;                  // [points]
    float4* out_pos;                   // [points]  (P.x, P.y, P.z, min_c D_c.w)
    float4* out_nrm;                   // [points]  (n.x, n.y, n.z, residual)
    unsigned points;
    int iterations;                    // K, 1 .. 32
    float grid;                        // grid_size
    float half;                        // grid_size / 2 (integer division, as the vertex stage's centring)
    float vertex_distance;
    float choppy;
};

// The u (or v) of rest coordinate x on the grid a query describes (QueryArgs, or anything else with these three fields).
template <class Args>
__device__ __forceinline__ float rest_uv(const Args& a, float x)
{
#pragma clang fp contract(off)
    return (x / a.vertex_distance + a.half) / a.grid;
}

// The sum on the maps at a given (u, v), amplitudes in registers.  JACOBIAN as cascade_sum's: only the Newton step reads jx / jz.
template <bool JACOBIAN, class Each>
__device__ __forceinline__ SurfaceEval eval_surface_uv(const QueryArgs& a, const float (&amp)[OCEAN_MAX_CASCADES], float u, float v, Each&& each)
{
    return cascade_sum<true, JACOBIAN>(a.s, amp, a.gain, u, v, MapSampler{}, each);
}

// ... at rest point (rx, rz): the (u, v) the query forms from it.
template <bool JACOBIAN = false>
__device__ __forceinline__ SurfaceEval eval_surface(const QueryArgs& a, const float (&amp)[OCEAN_MAX_CASCADES], float rx, float rz)
{
    return eval_surface_uv<JACOBIAN>(a, amp, rest_uv(a, rx), rest_uv(a, rz), NoEach{});
}

__device__ __forceinline__ float clamp_jacobian(float j)
{
    return fabsf(j) < 0.1f ? (j < 0.0f ? -0.1f : 0.1f) : j;
}

// The K Newton steps from r_0 = q: the rest point whose displaced xz is q.
__device__ __forceinline__ void solve_rest(const QueryArgs& a, const float (&amp)[OCEAN_MAX_CASCADES], float qx, float qz, float& rx, float& rz)
{
#pragma clang fp contract(off)
    rx = qx; rz = qz;
    for (int k = 0; k < a.iterations; ++k) {
        const SurfaceEval e = eval_surface<true>(a, amp, rx, rz);
        const float ex = (rx + e.dx) - qx, ez = (rz + e.dz) - qz;
        const float jx = clamp_jacobian(1.0f + e.jx), jz = clamp_jacobian(1.0f + e.jz);
        rx = rx - ex / jx;
        rz = rz - ez / jz;
    }
}

// The whole query at q: out_pos / out_nrm of ocean_query_surface.
__device__ __forceinline__ void query_point(const QueryArgs& a, const float (&amp)[OCEAN_MAX_CASCADES], float qx, float qz, float4& pos, float4& nrm)
{
#pragma clang fp contract(off)
    float rx, rz;
    solve_rest(a, amp, qx, qz, rx, rz);
    const SurfaceEval e = eval_surface(a, amp, rx, rz);
    const float px = rx + e.dx, pz = rz + e.dz;
    const float ex = px - qx, ez = pz - qz;
    pos = make_float4(px, 0.0f + e.dy, pz, e.w);
    const float3 nv = vertex_normal(e.sx, e.sz, e.ddx, e.ddz, a.choppy);
    nrm = make_float4(nv.x, nv.y, nv.z, sqrtf(ex * ex + ez * ez));
}

// H(x, z): only the height of the query at q (out_pos.y), without the normal.
__device__ __forceinline__ float surface_height(const QueryArgs& a, const float (&amp)[OCEAN_MAX_CASCADES], float qx, float qz)
{
#pragma clang fp contract(off)
    float rx, rz;
    solve_rest(a, amp, qx, qz, rx, rz);
    return 0.0f + eval_surface(a, amp, rx, rz).dy;
}

__global__ void __launch_bounds__(256) k_query_surface(const QueryArgs a)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.points) return;
    float amp[OCEAN_MAX_CASCADES];
    cascade_amplitudes(a.s.minmax, a.s.count, amp);
    const float2 q = a.xz[i];
    float4 pos, nrm;
    query_point(a, amp, q.x, q.y, pos, nrm);
    a.out_pos[i] = pos;
    a.out_nrm[i] = nrm;
}

// Ray cast (include/ocean_consumers.h: ocean_raycast_surface): the first point where each ray meets the surface of the query, H(x, z).
// The gap f(t) = p(t).y - H(p(t).xz) is sampled at M + 1 points over the part of the ray inside the height slab |y| <= Hmax; the first sample
// with f <= 0 closes the bracket [a, b], R rounds each split it into 16 equal parts and keep the first part that ends at or under the water,
// and the hit is the secant point of the last bracket, queried once more for its position and normal.  The header states every rule.
//
// A lane group of RAYCAST_LANES = 16 lanes per ray, 4 rays per wave64: one group-wide step evaluates 16 consecutive coarse samples, or the
// 15 inner points s_1 .. s_15 of one refinement round (lane j takes sample j; lane 0 has nothing to do in a round), and a 64-bit ballot
// of (f <= 0) with the group's 16 bits cut out gives the first such sample (its ctz).  -DOCEAN_RAYCAST_LANES=1 builds the same loop with
// one thread per ray (one sample per step; a developer variant for tools/raycast_timing.py, DESIGN.md has the figures).  The first sample with f <= 0 does not depend on
// the order of evaluation, so this is bit for bit the sequential definition (tests/surface_raycast.py), with a dependent chain of
// ceil((i + 1) / 16) + R + 1 evaluations instead of i + 1 + 15 R + 1.  Every lane of the wave reaches every ballot and shuffle: a
// group that is done (or has no ray) keeps looping with its state frozen until the wave-uniform loop ends.  fp32, no contraction.
struct RaycastArgs {
    QueryArgs q;                       // the surface (q.xz / out_* / points unused)
    const float* rays;                 // [count][6] ox, oy, oz, dx, dy, dz
    float4* out_hit;                   // [count]
    float4* out_nrm;                   // [count]
    unsigned count;
    float max_distance;
    int steps;                         // M, 1 .. 4096
    int refine;                        // R, 0 .. 8
};

#ifndef OCEAN_RAYCAST_LANES
#define OCEAN_RAYCAST_LANES 16
#endif
constexpr int RAYCAST_LANES = OCEAN_RAYCAST_LANES;
static_assert(RAYCAST_LANES >= 1 && 16 % RAYCAST_LANES == 0, "a lane group divides 16");
// first j of a round's first step: the steps of a round then end exactly at s_15 (0 for 2..16 lanes, 1 for one lane)
constexpr int RAYCAST_J0 = 16 - RAYCAST_LANES * ((15 + RAYCAST_LANES - 1) / RAYCAST_LANES);

__global__ void __launch_bounds__(256) k_raycast_surface(const RaycastArgs r)
{
#pragma clang fp contract(off)
    enum { MARCH, REFINE, DONE };
    enum { MISS, HIT, UNDER };
    const QueryArgs& a = r.q;
    const int sub = (int)(threadIdx.x % RAYCAST_LANES);
    const unsigned gshift = threadIdx.x & (64u - RAYCAST_LANES);       // the group's first bit in the wave's ballot
    const size_t ray = (size_t)blockIdx.x * (blockDim.x / RAYCAST_LANES) + threadIdx.x / RAYCAST_LANES;
    float amp[OCEAN_MAX_CASCADES];
    cascade_amplitudes(a.s.minmax, a.s.count, amp);
    float hsum = 0.0f;
#pragma unroll
    for (int c = 0; c < OCEAN_MAX_CASCADES; ++c) hsum = hsum + amp[c];
    const float hmax = fmaxf(1.001f * hsum, 1e-3f);                    // a 1 mm floor: a flat sea (A = FLT_MIN) still gets a slab to bracket

    int state = DONE, status = MISS;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f, dx = 0.0f, dy = 0.0f, dz = 0.0f, t0 = 0.0f, t1 = 0.0f;
    if (ray < r.count) {
        const float* o = r.rays + ray * 6;
        ox = o[0]; oy = o[1]; oz = o[2];
        dx = o[3]; dy = o[4]; dz = o[5];
        const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (len > 0.0f && len <= 3.402823466e+38f) {                   // zero, inf and NaN lengths miss
            dx = dx / len; dy = dy / len; dz = dz / len;
            bool empty;
            if (oy <= -hmax) {
                status = UNDER;
                empty = true;
            } else if (dy < 0.0f) {
                t0 = fmaxf(0.0f, (hmax - oy) / dy);
                t1 = fminf(r.max_distance, (-hmax - oy) / dy);
                empty = t1 < t0;
            } else if (dy > 0.0f) {
                t0 = fmaxf(0.0f, (-hmax - oy) / dy);
                t1 = fminf(r.max_distance, (hmax - oy) / dy);
                empty = t1 < t0;
            } else {
                t0 = 0.0f;
                t1 = r.max_distance;
                empty = !(oy < hmax);
            }
            if (!empty) state = MARCH;
        }
    }
    const float h = (t1 - t0) / (float)r.steps;
    int base = 0, round = 0, jb = 0;               // MARCH: index of the group's first sample; REFINE: rounds done, first j of this step
    float ta = 0.0f, fa = 0.0f, tb = 0.0f, fb = 0.0f, ra = 0.0f, w = 0.0f, thit = 0.0f;   // ra, w: a and (b - a) / 16 of this round

    while (__ballot(state != DONE) != 0ull) {
        bool valid = false;
        float x = 0.0f, f = 0.0f;
        if (state == MARCH) {
            const int i = base + sub;
            valid = i <= r.steps;
            x = i == r.steps ? t1 : t0 + (float)i * h;
        } else if (state == REFINE) {
            const int j = jb + sub;
            valid = j >= 1 && j <= 15;
            x = ra + (float)j * w;
        }
        if (valid) f = (oy + x * dy) - surface_height(a, amp, ox + x * dx, oz + x * dz);
        const unsigned bits = (unsigned)(__ballot(valid && f <= 0.0f) >> gshift) & ((1u << RAYCAST_LANES) - 1u);
        const int j = bits ? __builtin_ctz(bits) : RAYCAST_LANES - 1;      // the first sample at or under the water, else the last
        const int jp = j > 0 ? j - 1 : 0;
        const float xj = __shfl(x, j, RAYCAST_LANES), fj = __shfl(f, j, RAYCAST_LANES);
        const float xp = __shfl(x, jp, RAYCAST_LANES), fp = __shfl(f, jp, RAYCAST_LANES);
        bool bracketed = false;
        if (state == MARCH) {
            if (bits && base + j == 0) {                                   // the very first sample is wet
                status = t0 == 0.0f ? UNDER : HIT;
                thit = t0;
                state = DONE;
            } else if (bits) {
                if (j > 0) { ta = xp; fa = fp; }                           // else (ta, fa) = the previous step's last sample
                tb = xj; fb = fj;
                bracketed = true;
            } else {
                ta = xj; fa = fj;                                          // carried into the next step
                base += RAYCAST_LANES;
                if (base > r.steps) state = DONE;                          // no sample at or under the water: a miss
            }
        } else if (state == REFINE) {
            if (bits) {
                if (j > 0 && jb + j >= 2) { ta = xp; fa = fp; }            // else a = s_0 stays, or the previous step's last sample
                tb = xj; fb = fj;
                ++round;
                bracketed = true;
            } else {
                ta = xj; fa = fj;                                          // the last sample so far (s_15 at the end of the round)
                jb += RAYCAST_LANES;
                if (jb > 15) { ++round; bracketed = true; }                // none of s_1 .. s_15 is wet: [s_15, b]
            }
        }
        if (bracketed) {
            if (round < r.refine) {
                state = REFINE;
                ra = ta;
                w = (tb - ta) / 16.0f;
                jb = RAYCAST_J0;
            } else {
                status = HIT;
                thit = ta + (tb - ta) * (fa / (fa - fb));
                state = DONE;
            }
        }
    }

    if (sub != 0 || ray >= r.count) return;
    if (status == MISS) {
        r.out_hit[ray] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        r.out_nrm[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const bool under = status == UNDER;
    const float qx = under ? ox : ox + thit * dx, qz = under ? oz : oz + thit * dz;
    const float py = under ? oy : oy + thit * dy;
    float4 pos, nrm;
    query_point(a, amp, qx, qz, pos, nrm);
    r.out_hit[ray] = make_float4(pos.x, pos.y, pos.z, under ? -2.0f : thit);
    r.out_nrm[ray] = make_float4(nrm.x, nrm.y, nrm.z, py - pos.y);
}

}  // namespace ocean
