// ocean_foam_kernels.h -- persistent foam (include/ocean_consumers.h: ocean_update_foam, ocean_query_foam), compiled into ocean_consumers.hip only.
// A per-tile coverage field F[tiles][N][N] in [0, 1] in the maps' texel layout: generated where the Jacobian of the frame's maps falls under
// a threshold, blended towards its 3 x 3 binomial, decayed, cut off.  The header states the step; tests/foam.py repeats it in numpy.
#pragma once
#include "ocean_consumer_kernels.h"

namespace ocean {

// k_foam_update: one step for the tiles blockIdx.y = 0 .. of the selection.  A bandwidth-bound stencil, accounted at 24 B/texel (16 of the
// map texel whose Jacobian is read -- its lines are fetched whole --, 4 of F in, 4 of F' out).
// Row walk: a thread owns four adjacent columns (one float4 of F, four map texels) and walks down a band of `rows` rows with the horizontal
// sums r() of three rows in registers, so F comes from memory once per band plus two rows of overlap.  The column to the left of its four is
// the .w of the lane before it, the one to the right the .x of the lane after it (one shuffle each); a row of N <= 256 texels lies in one
// group of N/4 lanes and wraps inside it, wider rows take one halo float at each wave edge.  Several bands share a wave where N < 256.
// -DOCEAN_FOAM_LDS builds the other form instead (a developer variant for tools/foam_timing.py; DESIGN.md has both figures): a workgroup
// stages an 18 x 66 patch of F with its wrapped halo in LDS and every thread takes four columns of one row from there.
struct FoamArgs {
    const float4* map;       // first selected tile's displacement map (JACOBIAN frame) or normal map (FULL7 frame)
    const float* src;        // F of the first selected tile
    float* dst;              // F' of the first selected tile
    const float* lambda;     // FULL7: per-tile lambda of the frame (indexed like blockIdx.y), or null: lambda_all
    size_t tile_texels;      // N * N
    float lambda_all;
    float threshold, gain, spread, decay, cutoff;
    int n;                   // map size
    int log2_groups;         // log2(N / 4): column groups per row
    int rows;                // rows per band (a power of two, 4 <= rows <= N)
};

constexpr int FOAM_FROM_NORMALS = 0, FOAM_FROM_JACOBIAN = 1;

template <int JSRC>
__device__ __forceinline__ float foam_jacobian(const float4 t, float lam)
{
#pragma clang fp contract(off)
    if (JSRC == FOAM_FROM_JACOBIAN) return t.w;
    return (1.0f + lam * t.z) * (1.0f + lam * t.w);
}

// F' of one texel from its Jacobian, its own value and the three row sums around it.
__device__ __forceinline__ float foam_texel(const FoamArgs& a, float jac, float f, float ru, float rc, float rd)
{
#pragma clang fp contract(off)
    const float g = fminf(fmaxf((a.threshold - jac) * a.gain, 0.0f), 1.0f);
    const float b = ((ru + 2.0f * rc) + rd) * 0.0625f;
    const float s = f + a.spread * (b - f);
    const float c = s * a.decay;
    const float o = fmaxf(c, g);
    return (o < a.cutoff) ? 0.0f : o;
}

#ifndef OCEAN_FOAM_LDS

template <int JSRC>
__global__ void __launch_bounds__(256) k_foam_update(const FoamArgs a)
{
#pragma clang fp contract(off)
    const int n = a.n, groups = n >> 2;
    const unsigned gx = blockIdx.x * 256u + threadIdx.x;
    if (gx >= (unsigned)(groups * (n / a.rows))) return;          // (whole lane groups leave together: the bound is a multiple of the group)
    const int cg = (int)(gx & (unsigned)(groups - 1)), band = (int)(gx >> a.log2_groups);
    const int col0 = cg * 4, row0 = band * a.rows;
    const size_t tile = blockIdx.y;
    const float* __restrict__ src = a.src + tile * a.tile_texels;
    const float4* __restrict__ map = a.map + tile * a.tile_texels;
    float* __restrict__ dst = a.dst + tile * a.tile_texels;
    const float lam = (JSRC == FOAM_FROM_NORMALS && a.lambda) ? a.lambda[tile] : a.lambda_all;
    // the lane group that holds one row (or 64 column groups of it)
    const int lane = (int)(threadIdx.x & 63u), width = groups < 64 ? groups : 64;
    const int sub = lane & (width - 1), base = lane - sub;
    const int lane_l = base + ((sub - 1) & (width - 1)), lane_r = base + ((sub + 1) & (width - 1));
    const bool halo = groups > 64;
    const int col_l = (col0 - 1) & (n - 1), col_r = (col0 + 4) & (n - 1);

    auto load_row = [&](int row, float4& f, float4& r) {
        const float* __restrict__ p = src + (unsigned)((row & (n - 1)) * n);
        f = *reinterpret_cast<const float4*>(p + col0);
        float left = __shfl(f.w, lane_l), right = __shfl(f.x, lane_r);
        if (halo) {
            if (sub == 0) left = p[col_l];
            if (sub == 63) right = p[col_r];
        }
        r.x = (left + 2.0f * f.x) + f.y;
        r.y = (f.x + 2.0f * f.y) + f.z;
        r.z = (f.y + 2.0f * f.z) + f.w;
        r.w = (f.z + 2.0f * f.w) + right;
    };

    float4 fu, ru, fc, rc, fd, rd;
    load_row(row0 - 1, fu, ru);
    load_row(row0, fc, rc);
    for (int i0 = 0; i0 < a.rows; i0 += 4) {          // (rows is a multiple of 4: four rows' loads are in flight together)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = row0 + i0 + k;
            const float4* __restrict__ m = map + (unsigned)(row * n + col0);
            const float4 t0 = m[0], t1 = m[1], t2 = m[2], t3 = m[3];
            load_row(row + 1, fd, rd);
            float4 o;
            o.x = foam_texel(a, foam_jacobian<JSRC>(t0, lam), fc.x, ru.x, rc.x, rd.x);
            o.y = foam_texel(a, foam_jacobian<JSRC>(t1, lam), fc.y, ru.y, rc.y, rd.y);
            o.z = foam_texel(a, foam_jacobian<JSRC>(t2, lam), fc.z, ru.z, rc.z, rd.z);
            o.w = foam_texel(a, foam_jacobian<JSRC>(t3, lam), fc.w, ru.w, rc.w, rd.w);
            *reinterpret_cast<float4*>(dst + (unsigned)(row * n + col0)) = o;
            ru = rc; rc = rd; fc = fd;
        }
    }
}

// workgroups per tile of a launch with `rows` rows per band
inline unsigned foam_blocks(unsigned n, unsigned rows) { return ((n / 4u) * (n / rows) + 255u) / 256u; }

#else   // OCEAN_FOAM_LDS

constexpr int FOAM_LDS_ROWS = 16, FOAM_LDS_COLS = 64;

template <int JSRC>
__global__ void __launch_bounds__(256) k_foam_update(const FoamArgs a)
{
#pragma clang fp contract(off)
    __shared__ float patch[FOAM_LDS_ROWS + 2][FOAM_LDS_COLS + 4];      // rows -1 .. 16, columns -1 .. 64 of the workgroup's patch (+ 2 of padding)
    const int n = a.n;
    const int rows = n < FOAM_LDS_ROWS ? n : FOAM_LDS_ROWS, cols = n < FOAM_LDS_COLS ? n : FOAM_LDS_COLS;      // a 16^2 or 32^2 tile is one narrower patch
    const int patches_x = n / cols;
    const int row0 = (int)(blockIdx.x / (unsigned)patches_x) * rows, col0 = (int)(blockIdx.x % (unsigned)patches_x) * cols;
    const size_t tile = blockIdx.y;
    const float* __restrict__ src = a.src + tile * a.tile_texels;
    const float4* __restrict__ map = a.map + tile * a.tile_texels;
    float* __restrict__ dst = a.dst + tile * a.tile_texels;
    const float lam = (JSRC == FOAM_FROM_NORMALS && a.lambda) ? a.lambda[tile] : a.lambda_all;
    for (int i = (int)threadIdx.x; i < (rows + 2) * (cols + 2); i += 256) {
        const int pr = i / (cols + 2), pc = i % (cols + 2);
        patch[pr][pc] = src[(unsigned)(((row0 + pr - 1) & (n - 1)) * n + ((col0 + pc - 1) & (n - 1)))];
    }
    __syncthreads();
    const int tr = (int)threadIdx.x / (FOAM_LDS_COLS / 4), tc = ((int)threadIdx.x % (FOAM_LDS_COLS / 4)) * 4;
    if (tr >= rows || tc >= cols) return;
    const float4* __restrict__ m = map + (unsigned)((row0 + tr) * n + col0 + tc);
    const float4 t[4] = {m[0], m[1], m[2], m[3]};
    float r[3][4], f[4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            r[k][j] = (patch[tr + k][tc + j] + 2.0f * patch[tr + k][tc + j + 1]) + patch[tr + k][tc + j + 2];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = patch[tr + 1][tc + j + 1];
    float4 o;
    o.x = foam_texel(a, foam_jacobian<JSRC>(t[0], lam), f[0], r[0][0], r[1][0], r[2][0]);
    o.y = foam_texel(a, foam_jacobian<JSRC>(t[1], lam), f[1], r[0][1], r[1][1], r[2][1]);
    o.z = foam_texel(a, foam_jacobian<JSRC>(t[2], lam), f[2], r[0][2], r[1][2], r[2][2]);
    o.w = foam_texel(a, foam_jacobian<JSRC>(t[3], lam), f[3], r[0][3], r[1][3], r[2][3]);
    *reinterpret_cast<float4*>(dst + (unsigned)((row0 + tr) * n + col0 + tc)) = o;
}

inline unsigned foam_blocks(unsigned n, unsigned)
{
    const unsigned rows = n < (unsigned)FOAM_LDS_ROWS ? n : (unsigned)FOAM_LDS_ROWS, cols = n < (unsigned)FOAM_LDS_COLS ? n : (unsigned)FOAM_LDS_COLS;
    return (n / rows) * (n / cols);
}

#endif  // OCEAN_FOAM_LDS

// k_query_foam: the foam above world points.  The rest point of q is the surface query's (solve_rest on the same QueryArgs); the foam of every
// cascade is sampled there with the scalar form of sample_linear_repeat and the cascades are combined with fmaxf from 0.0f in cascade order.
// out = (foam, r.x, r.z, |P(r).xz - q|).  One thread per point; fp32, no contraction (tests/foam.py repeats it).
struct FoamQueryArgs {
    QueryArgs q;             // the surface (q.out_pos / q.out_nrm unused)
    const float* foam;       // F of the FIRST tile of the cascade set (tile c at + c * q.s.tile_texels)
    float4* out;             // [points]
};

__device__ __forceinline__ float sample_linear_repeat_scalar(const float* __restrict__ tex, int n, float u, float v)
{
#pragma clang fp contract(off)
    const float s = u * (float)n - 0.5f, t = v * (float)n - 0.5f;
    const float fs = floorf(s), ft = floorf(t);
    const float a = s - fs, b = t - ft;
    const int x0 = (int)fs & (n - 1), y0 = (int)ft & (n - 1);
    const int x1 = (x0 + 1) & (n - 1), y1 = (y0 + 1) & (n - 1);
    const float c00 = tex[(unsigned)(y0 * n + x0)], c10 = tex[(unsigned)(y0 * n + x1)];
    const float c01 = tex[(unsigned)(y1 * n + x0)], c11 = tex[(unsigned)(y1 * n + x1)];
    const float ia = 1.0f - a, ib = 1.0f - b;
    return (c00 * ia + c10 * a) * ib + (c01 * ia + c11 * a) * b;
}

__global__ void __launch_bounds__(256) k_query_foam(const FoamQueryArgs fa)
{
#pragma clang fp contract(off)
    const QueryArgs& a = fa.q;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.points) return;
    float amp[OCEAN_MAX_CASCADES];
    cascade_amplitudes(a.s.minmax, a.s.count, amp);
    const float2 q = a.xz[i];
    float rx, rz;
    solve_rest(a, amp, q.x, q.y, rx, rz);
    const SurfaceEval e = eval_surface(a, amp, rx, rz);
    const float ex = (rx + e.dx) - q.x, ez = (rz + e.dz) - q.y;
    const float u = rest_uv(a, rx), v = rest_uv(a, rz);
    float foam = 0.0f;
#pragma unroll
    for (int c = 0; c < OCEAN_MAX_CASCADES; ++c) {
        if (c >= a.s.count) break;
        foam = fmaxf(foam, sample_linear_repeat_scalar(fa.foam + (size_t)c * a.s.tile_texels, a.s.n, u * a.s.uv_scale[c], v * a.s.uv_scale[c]));
    }
    fa.out[i] = make_float4(foam, rx, rz, sqrtf(ex * ex + ez * ez));
}

}  // namespace ocean
