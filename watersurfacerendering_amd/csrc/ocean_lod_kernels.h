// ocean_lod_kernels.h -- LOD sampling (include/ocean_consumers.h: ocean_build_mips_tiles, ocean_sample_surface_lod, ocean_displace_grid_lod),
// compiled into ocean_consumers.hip only: the mip chains of a whole tile range in at most two launches, and the two kernels that run
// the cascade sum (cascade_sum, ocean_consumer_kernels.h) through the footprint-driven sampler (sample_lod, beside sample_linear_repeat there).
#pragma once
#include "ocean_consumer_kernels.h"

namespace ocean {

// ============================================================================
// Mip chains of a tile range.  k_mip_level needs log2 N launches per tile and everything after the first two is launch latency; here one
// launch covers every tile of the range and both maps (blockIdx.y = map, blockIdx.z = tile), and a 256-thread workgroup takes a `be` x `be`
// block of its source (be = 64, or the whole source where that is smaller) down to ONE texel: the first halving from global memory -- every
// thread reads 2 x 2 quads as float4 pairs, lanes along x, so a wave covers whole 128-byte lines of two source rows --, written to the chain
// and kept in LDS, then be/4, be/8 ... 1 from LDS with one barrier per level, each piece written to its place in the packed chain.
// That reaches level log2(be); the levels beyond are a second launch of the same kernel whose source is level 6 of the chains just
// written (extent N / 64 <= 64: one block per map and tile), ordered behind the first by the stream.  No hand-off between workgroups, no
// counters, no atomics.  LDS: 32^2 + 16^2 float4 = 20 KB (two buffers that alternate), so eight workgroups share a CU -- the wave limit.
// Every texel is (t00*0.5 + t10*0.5)*0.5 + (t01*0.5 + t11*0.5)*0.5 of the level above, no contraction: the bits of k_mip_level.
// ============================================================================
struct MipTilesArgs {
    const float4* src[2];    // the source level of the range's first tile: displacement, normal
    float4* dst[2];          // the chains of the range's first tile
    size_t src_stride;       // texels from one tile's source to the next (N^2 for the maps, chain_texels for a chain level)
    size_t chain_texels;     // ocean_mip_texels(N)
    size_t dst_offset;       // where the first level this launch writes starts in a chain
    int sw;                  // extent of the source
    int be;                  // block edge: min(64, sw); blocks per map and tile = (sw / be)^2
};

constexpr int MIP_BLOCK = 64;

__device__ __forceinline__ float4 mip_mix(const float4& t00, const float4& t10, const float4& t01, const float4& t11)
{
#pragma clang fp contract(off)
    auto mix = [](float c00, float c10, float c01, float c11) { return (c00 * 0.5f + c10 * 0.5f) * 0.5f + (c01 * 0.5f + c11 * 0.5f) * 0.5f; };
    return make_float4(mix(t00.x, t10.x, t01.x, t11.x), mix(t00.y, t10.y, t01.y, t11.y),
                       mix(t00.z, t10.z, t01.z, t11.z), mix(t00.w, t10.w, t01.w, t11.w));
}

__global__ void __launch_bounds__(256) k_mips_tiles(const MipTilesArgs m)
{
    __shared__ float4 lds_a[(MIP_BLOCK / 2) * (MIP_BLOCK / 2)];      // pieces of extent be/2, be/8, be/32
    __shared__ float4 lds_b[(MIP_BLOCK / 4) * (MIP_BLOCK / 4)];      //                   be/4, be/16, be/64
    const int map = (int)blockIdx.y;
    const int blocks_x = m.sw / m.be;
    const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
    const float4* __restrict__ src = m.src[map] + (size_t)blockIdx.z * m.src_stride;
    float4* chain = m.dst[map] + (size_t)blockIdx.z * m.chain_texels;
    size_t off = m.dst_offset;

    // the first halving: global -> global + LDS
    int p = m.be / 2;                // extent of the block's piece of this level
    int w = m.sw / 2;                // extent of this level
    for (int i = (int)threadIdx.x; i < p * p; i += 256) {
        const int x = i % p, y = i / p;
        const float4* r0 = src + (size_t)(by * m.be + 2 * y) * (size_t)m.sw + (size_t)(bx * m.be + 2 * x);
        const float4* r1 = r0 + m.sw;
        const float4 o = mip_mix(r0[0], r0[1], r1[0], r1[1]);
        chain[off + (size_t)(by * p + y) * (size_t)w + (size_t)(bx * p + x)] = o;
        lds_a[i] = o;
    }
    // the rest: LDS -> global + LDS, the two buffers alternating
    float4* from = lds_a;
    float4* to = lds_b;
    while (p > 1) {
        __syncthreads();
        off += (size_t)w * (size_t)w;
        const int sp = p;            // extent of the piece that is read
        p /= 2; w /= 2;
        const int i = (int)threadIdx.x;
        if (i < p * p) {             // at most 16^2 = 256
            const int x = i % p, y = i / p;
            const float4* r0 = from + (2 * y) * sp + 2 * x;
            const float4* r1 = r0 + sp;
            const float4 o = mip_mix(r0[0], r0[1], r1[0], r1[1]);
            chain[off + (size_t)(by * p + y) * (size_t)w + (size_t)(bx * p + x)] = o;
            to[i] = o;
        }
        float4* s = from; from = to; to = s;
    }
}

// ============================================================================
// The two consumers of the sampler.  What they share: the set's chains, the texels per mesh metre of every cascade (host-computed) and the
// level rule's constants.
// ============================================================================
struct LodSet {
    const float4* mips_disp;           // chains of the FIRST tile of the cascade set (tile c at + c * chain_texels)
    const float4* mips_nrm;
    size_t chain_texels;               // ocean_mip_texels(N)
    float tpm[OCEAN_MAX_CASCADES];     // |uv_scale_c * N / (grid_size * vertex_distance)|
    float scale;                       // ocean_lod.scale
    float top;                         // 2^lmax
    int lmax;                          // log2 N, or min(log2 N, ocean_lod.max_level)
};

// sample_lod as the cascade sum's sampler: cascade c at the level that fits fs * tpm[c] texels, both maps at the same one.  lambda is the
// coarsest level + blend any cascade has used so far (the point form reports it; the grid form leaves it alone).
struct LodSampler {
    const LodSet& lod;
    float fs;                          // footprint in mesh metres, times lod.scale
    float lambda = 0.0f;
    __device__ __forceinline__ void operator()(const CascadeSet& s, int c, float us, float vs, float4& d, float4& sl)
    {
        int lev; float t;
        lod_level(fs * lod.tpm[c], lod.lmax, lod.top, lev, t);
        d = sample_lod(s.disp + (size_t)c * s.tile_texels, lod.mips_disp + (size_t)c * lod.chain_texels, s.n, lev, t, us, vs);
        sl = sample_lod(s.nrm + (size_t)c * s.tile_texels, lod.mips_nrm + (size_t)c * lod.chain_texels, s.n, lev, t, us, vs);
        lambda = fmaxf(lambda, (float)lev + t);
    }
};

// Forward evaluation at rest point (x, z) with footprint f: out_pos / out_nrm of ocean_sample_surface_lod.  fp32, no contraction, in the
// order include/ocean_consumers.h states and tests/lod.py repeats: the cascade sum (ocean_consumer_kernels.h) through the sampler above.
struct LodPointArgs {
    QueryArgs q;                       // the surface (q.xz / iterations / gain unused)
    LodSet lod;
    const float* xzf;                  // [points][3] x, z, footprint
};

__global__ void __launch_bounds__(256) k_sample_surface_lod(const LodPointArgs p)
{
#pragma clang fp contract(off)
    const QueryArgs& a = p.q;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.points) return;
    const float* in = p.xzf + (size_t)i * 3;
    const float x = in[0], z = in[1], f = in[2];
    LodSampler sample{p.lod, f * p.lod.scale};
    const SurfaceEval e = cascade_sum<false, false>(a.s, nullptr, nullptr, rest_uv(a, x), rest_uv(a, z), sample, NoEach{});
    a.out_pos[i] = make_float4(x + e.dx, 0.0f + e.dy, z + e.dz, e.w);
    const float3 nv = vertex_normal(e.sx, e.sz, e.ddx, e.ddz, a.choppy);
    a.out_nrm[i] = make_float4(nv.x, nv.y, nv.z, sample.lambda);
}

// k_displace_grid_cascades with every sample through the sampler at footprint |vertex_distance|: the level is the same for every vertex of a
// cascade, so it is wave-uniform; where no cascade is undersampled this is that kernel's arithmetic, bit for bit.
struct LodGridArgs {
    CascadeArgs a;
    LodSet lod;
};

__global__ void __launch_bounds__(256) k_displace_grid_lod(const LodGridArgs p)
{
#pragma clang fp contract(off)
    displace_grid_vertex(p.a, blockIdx.x * blockDim.x + threadIdx.x, LodSampler{p.lod, fabsf(p.a.vertex_distance) * p.lod.scale});
}

}  // namespace ocean
