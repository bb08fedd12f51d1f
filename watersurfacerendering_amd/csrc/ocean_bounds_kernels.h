// ocean_bounds_kernels.h -- surface bounds (include/ocean_consumers.h: ocean_build_bounds_tiles, ocean_patch_bounds), compiled into
// ocean_consumers.hip only: the min/max pyramids of the displacement maps of a whole tile range in at most two launches, and the kernel that
// turns rest-space rectangles into world-space boxes over a cascade set and classifies them against a frustum.
#pragma once
#include "ocean_lod_kernels.h"

namespace ocean {

// ============================================================================
// Min/max pyramids of a tile range.  The shape of k_mips_tiles (ocean_lod_kernels.h): blockIdx.z = tile, a 256-thread workgroup takes a
// `be` x `be` block of its source (be = 64, or the whole source where that is smaller) down to ONE node -- the first halving from global
// memory, every thread reading 2 x 2 quads as float4 pairs with the lanes along x, then be/4, be/8 ... 1 from LDS with one barrier per
// level -- and a second launch whose source is level 6 of the chains just written finishes the chains of tiles larger than 64.  Two
// differences.  ONE read of the source feeds BOTH chains: a thread reads its quad once and keeps a fminf and a fmaxf of it (TWO = false; in
// the second launch the `lo` chain continues from the `lo` chain and the `hi` chain from the `hi` chain, TWO = true, on at most 64 x 64
// nodes).  And a level below `first_level` is reduced through LDS like every other but not stored: levels 1 and 2 are 94 % of a chain, so a
// caller whose patches are never narrower than 2^first_level texels pays little more than the read of the map.
// LDS: both chains stay in one workgroup, 2 x (32^2 + 16^2) float4 = 40 KB, so four workgroups (16 waves) share a compute unit where
// k_mips_tiles has eight.  Chosen over 128-thread halves (the halves would have to hand their pieces to each other, or each read the quad:
// the second read of the source this kernel exists to avoid) and over a wave-level reduction of the first steps (eight dwords per lane
// through cross-lane moves per step, and a lane layout that no longer reads whole lines of two source rows).  With half the waves of the
// mip kernel per unit, a thread issues the 16 loads of its four quads before it uses the first (72 VGPRs, no scratch; four waves per SIMD
// allow 128), so a unit keeps as many loads in flight as that kernel's eight workgroups do with four loads each; the loop form of
// k_mips_tiles was not measured for this kernel.  min and max are exact: no order of the reduction changes a bit (but for which zero wins
// where a block holds both).  Plain vector loads and stores; no hand-off between workgroups, no counters, no atomics.
// Measured (tools/bounds_timing.py, profiles/bounds_timing.txt; medians, us per call, against ocean_build_mips_tiles on the same range in the
// same run): at first_level 1 26.5 against 37.3 at 2048^2 x 1, 98.7 against 140.3 at 2048^2 x 4, 12.1 against 14.5 at 512^2 x 4 -- but 10.6
// against 9.5 at 512^2 x 1: LONGER, by about the spread of the rounds (10.0-11.7 against 9.4-10.6).  Suspected cause: that shape is 64
// workgroups on 256 compute units and two launches of a few microseconds each, so neither call is near its bytes; what is left is one
// workgroup's chain of a load, six barriers and the second launch, the same for both, and this kernel's workgroup does twice the LDS
// traffic and register work per level while the single map gives the device half as many workgroups to spread it over.  Not tuned for.
// ============================================================================
struct BoundsTilesArgs {
    const float4* src[2];    // the source level of the range's first tile for the lo and the hi chain (the displacement map: the same twice)
    float4* dst[2];          // the lo and hi chains of the range's first tile
    size_t src_stride;       // texels from one tile's source to the next (N^2 for the maps, chain_texels for a chain level)
    size_t chain_texels;     // ocean_mip_texels(N)
    size_t dst_offset;       // where the first level this launch reduces to starts in a chain
    int sw;                  // extent of the source
    int be;                  // block edge: min(64, sw); blocks per tile = (sw / be)^2
    int level;               // the first level this launch reduces to (1, or 7)
    int store_from;          // levels below it are not stored
};

__device__ __forceinline__ float4 min4(const float4& a, const float4& b)
{
    return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w));
}
__device__ __forceinline__ float4 max4(const float4& a, const float4& b)
{
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

template <bool TWO>
__global__ void __launch_bounds__(256) k_bounds_tiles(const BoundsTilesArgs m)
{
    __shared__ float4 lds_a[2][(MIP_BLOCK / 2) * (MIP_BLOCK / 2)];      // [lo, hi] pieces of extent be/2, be/8, be/32
    __shared__ float4 lds_b[2][(MIP_BLOCK / 4) * (MIP_BLOCK / 4)];      //                           be/4, be/16, be/64
    const int blocks_x = m.sw / m.be;
    const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
    const float4* __restrict__ src_lo = m.src[0] + (size_t)blockIdx.z * m.src_stride;
    const float4* __restrict__ src_hi = m.src[1] + (size_t)blockIdx.z * m.src_stride;
    float4* chain_lo = m.dst[0] + (size_t)blockIdx.z * m.chain_texels;
    float4* chain_hi = m.dst[1] + (size_t)blockIdx.z * m.chain_texels;
    size_t off = m.dst_offset;
    int level = m.level;

    // the first halving: global -> LDS (+ global)
    int p = m.be / 2;                // extent of the block's piece of this level
    int w = m.sw / 2;                // extent of this level
    // (a piece has at most 32^2 nodes, four per thread: all their loads are issued before the first is used)
    constexpr int PER = (MIP_BLOCK / 2) * (MIP_BLOCK / 2) / 256;
    float4 q[PER][4], qh[TWO ? PER : 1][4];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (i < p * p) {
            const int x = i % p, y = i / p;
            const size_t at = (size_t)(by * m.be + 2 * y) * (size_t)m.sw + (size_t)(bx * m.be + 2 * x);
            const float4* r0 = src_lo + at;
            const float4* r1 = r0 + m.sw;
            q[k][0] = r0[0]; q[k][1] = r0[1]; q[k][2] = r1[0]; q[k][3] = r1[1];
            if constexpr (TWO) {
                const float4* h0 = src_hi + at;
                const float4* h1 = h0 + m.sw;
                qh[k][0] = h0[0]; qh[k][1] = h0[1]; qh[k][2] = h1[0]; qh[k][3] = h1[1];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (i >= p * p) break;
        const int x = i % p, y = i / p;
        const float4 lo = min4(min4(q[k][0], q[k][1]), min4(q[k][2], q[k][3]));
        float4 hi;
        if constexpr (TWO) hi = max4(max4(qh[k][0], qh[k][1]), max4(qh[k][2], qh[k][3]));
        else hi = max4(max4(q[k][0], q[k][1]), max4(q[k][2], q[k][3]));
        if (level >= m.store_from) {
            const size_t o = off + (size_t)(by * p + y) * (size_t)w + (size_t)(bx * p + x);
            chain_lo[o] = lo;
            chain_hi[o] = hi;
        }
        lds_a[0][i] = lo;
        lds_a[1][i] = hi;
    }
    // the rest: LDS -> LDS (+ global), the two buffers alternating
    float4* from_lo = lds_a[0];
    float4* from_hi = lds_a[1];
    float4* to_lo = lds_b[0];
    float4* to_hi = lds_b[1];
    while (p > 1) {
        __syncthreads();
        off += (size_t)w * (size_t)w;
        const int sp = p;            // extent of the piece that is read
        p /= 2; w /= 2; ++level;
        const int i = (int)threadIdx.x;
        if (i < p * p) {             // at most 16^2 = 256
            const int x = i % p, y = i / p;
            const int q0 = (2 * y) * sp + 2 * x, q1 = q0 + sp;
            const float4 lo = min4(min4(from_lo[q0], from_lo[q0 + 1]), min4(from_lo[q1], from_lo[q1 + 1]));
            const float4 hi = max4(max4(from_hi[q0], from_hi[q0 + 1]), max4(from_hi[q1], from_hi[q1 + 1]));
            if (level >= m.store_from) {
                const size_t o = off + (size_t)(by * p + y) * (size_t)w + (size_t)(bx * p + x);
                chain_lo[o] = lo;
                chain_hi[o] = hi;
            }
            to_lo[i] = lo;
            to_hi[i] = hi;
        }
        float4* s = from_lo; from_lo = to_lo; to_lo = s;
        s = from_hi; from_hi = to_hi; to_hi = s;
    }
}

// ============================================================================
// Patch bounds (include/ocean_consumers.h: ocean_patch_bounds): one thread per rest-space rectangle.  Per cascade the rectangle's texel index
// range picks a level whose nodes are at least as wide as the range, so at most 2 x 2 nodes cover it (REPEAT through the arithmetic shift of
// negative indices and the mask); their fminf / fmaxf are summed over the cascades as the vertex stage sums its samples, added to the
// rectangle's own corners, and the box is classified against up to six planes.  fp32 throughout, no contraction, in the order the header
// states and tests/bounds.py repeats.  Indices are formed in 64 bits and masked: a rectangle that is not finite or lies beyond 2^31 texels
// reads inside the chains and writes its own row only.
// ============================================================================
struct PatchArgs {
    QueryArgs q;                       // the surface (q.s.disp / nrm, q.xz / iterations / choppy / gain unused; q.s.minmax gives A_c)
    const float4* lo;                  // chains of the FIRST tile of the cascade set (tile c at + c * chain_texels)
    const float4* hi;
    const float* rects;                // [count][4] x0, z0, x1, z1
    size_t chain_texels;               // ocean_mip_texels(N)
    int top;                           // log2 N
    int first_level;                   // of the set: 1 .. log2 N
    int pad;                           // ocean_patch_query.pad_texels
    int planes;                        // 0 .. 6
    float plane[6][4];
};

__global__ void __launch_bounds__(256) k_patch_bounds(const PatchArgs p)
{
#pragma clang fp contract(off)
    const QueryArgs& a = p.q;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.points) return;
    const float* in = p.rects + (size_t)i * 4;
    const float x0 = in[0], z0 = in[1], x1 = in[2], z1 = in[3];
    const bool finite = isfinite(x0) && isfinite(z0) && isfinite(x1) && isfinite(z1);
    const float u0 = rest_uv(a, x0), v0 = rest_uv(a, z0);
    const float u1 = rest_uv(a, x1), v1 = rest_uv(a, z1);
    const float fn = (float)a.s.n;
    float lx = 0.0f, ly = 0.0f, lz = 0.0f, lw = 3.402823466e+38f;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;
    for (int c = 0; c < a.s.count; ++c) {
        const float sc = a.s.uv_scale[c];
        const float amp = height_amplitude(a.s.minmax, c);
        const float tx0 = u0 * sc * fn - 0.5f, tx1 = u1 * sc * fn - 0.5f;
        const float tz0 = v0 * sc * fn - 0.5f, tz1 = v1 * sc * fn - 0.5f;
        const long long i0x = (long long)(int)floorf(fminf(tx0, tx1)) - p.pad, i1x = (long long)(int)floorf(fmaxf(tx0, tx1)) + 1 + p.pad;
        const long long i0z = (long long)(int)floorf(fminf(tz0, tz1)) - p.pad, i1z = (long long)(int)floorf(fmaxf(tz0, tz1)) + 1 + p.pad;
        const long long wx = i1x - i0x, wz = i1z - i0z;
        const long long w = (wx > wz ? wx : wz) + 1;
        int l = p.top;
        if (finite && w < (long long)a.s.n) {
            l = 1;
            while ((1ll << l) < w) ++l;
            if (l < p.first_level) l = p.first_level;
        }
        const int ext = a.s.n >> l;
        const long long mask = ext - 1;
        const int nx0 = (int)((i0x >> l) & mask), nx1 = (int)((i1x >> l) & mask);
        const int nz0 = (int)((i0z >> l) & mask), nz1 = (int)((i1z >> l) & mask);
        const float4* lo = lod_level_ptr(nullptr, p.lo + (size_t)c * p.chain_texels, a.s.n, l);
        const float4* hi = lod_level_ptr(nullptr, p.hi + (size_t)c * p.chain_texels, a.s.n, l);
        const unsigned n00 = (unsigned)(nz0 * ext + nx0), n10 = (unsigned)(nz0 * ext + nx1);
        const unsigned n01 = (unsigned)(nz1 * ext + nx0), n11 = (unsigned)(nz1 * ext + nx1);
        const float4 lo_c = min4(min4(lo[n00], lo[n10]), min4(lo[n01], lo[n11]));
        const float4 hi_c = max4(max4(hi[n00], hi[n10]), max4(hi[n01], hi[n11]));
        lx = lx + lo_c.x; ly = ly + lo_c.y * amp; lz = lz + lo_c.z;
        hx = hx + hi_c.x; hy = hy + hi_c.y * amp; hz = hz + hi_c.z;
        lw = fminf(lw, lo_c.w);
    }
    const float4 lo = make_float4(fminf(x0, x1) + lx, 0.0f + ly, fminf(z0, z1) + lz, lw);
    float4 hi = make_float4(fmaxf(x0, x1) + hx, 0.0f + hy, fmaxf(z0, z1) + hz, 1.0f);
    if (p.planes > 0) {
        float cls = 2.0f;
        for (int k = 0; k < p.planes; ++k) {
            const float pa = p.plane[k][0], pb = p.plane[k][1], pc = p.plane[k][2], pd = p.plane[k][3];
            const float far = ((pa * (pa >= 0.0f ? hi.x : lo.x) + pb * (pb >= 0.0f ? hi.y : lo.y)) + pc * (pc >= 0.0f ? hi.z : lo.z)) + pd;
            const float near = ((pa * (pa >= 0.0f ? lo.x : hi.x) + pb * (pb >= 0.0f ? lo.y : hi.y)) + pc * (pc >= 0.0f ? lo.z : hi.z)) + pd;
            if (far < 0.0f) { cls = 0.0f; break; }
            if (near < 0.0f) cls = 1.0f;
        }
        hi.w = cls;
    }
    a.out_pos[i] = lo;
    a.out_nrm[i] = hi;
}

}  // namespace ocean
