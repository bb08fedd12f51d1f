// ocean_spray_kernels.h -- the kernels behind ocean_emit_spray (include/ocean_consumers.h), compiled into ocean_consumers.hip only: the grid
// vertices of a window where the surface is breaking, compacted into a list in ascending lattice index.  A vertex is evaluated with the query's
// eval_surface_uv (ocean_consumer_kernels.h) at the (u, v) the cascade vertex stage forms for it, its velocity with water_velocity_uv
// (ocean_velocity_kernels.h); what is new here is the predicate and the ordered stream compaction, three launches whatever the window:
//   k_spray_count    one workgroup per chunk of C = SPRAY_CHUNK = 1024 consecutive lattice indices, in SPRAY_ROUNDS = 4 rounds of 256: thread t
//                    of round r takes index chunk * C + r * 256 + t, so a wave's 64 lanes hold 64 consecutive indices and its __ballot mask is
//                    their predicate in index order.  The 16 masks of a chunk and its count go to a scratch array the context owns.
//   k_spray_scan     ONE workgroup, SPRAY_SCAN_WIDTH = 256 chunk counts per step (one per thread: a shuffle scan per wave, the four wave sums
//                    through LDS), looping with a running carry while there are more chunks than that (16384 chunks at most: 64 steps); it
//                    replaces each count by the exclusive sum of the counts before it and writes out_count = (total, min(total, capacity)).
//   k_spray_scatter  the chunks again: rank = the chunk's offset + the earlier rounds' and lower waves' counts (through LDS) + the popcount of
//                    the wave's mask below the lane; a passing lane with rank < capacity evaluates its vertex once more and stores its row.
// No workgroup waits for another inside a launch, no atomics at all: the list is a function of the maps alone, the same bits on every run.
// The scatter takes the predicate from the masks the count pass cached, so it evaluates only the vertices it lists (a few hundred of a
// million on a real sea).  The other form -- every vertex evaluated again and balloted anew, no masks -- was built and measured beside it on
// a 1025^2 window (profiles/spray_timing.txt, us per call, masks / re-evaluation): 22.2 / 25.6 and 88.7 / 140.8 over 1 and 4 cascades of
// 512^2, 37.8 / 52.2 and 244 / 433 of 2048^2, the same list; it lost everywhere and is not kept.  The cascade vertex stage alone takes
// 13.3, 68.9, 27.0 and 203 there, count + scan 1.04 ... 1.14 of that: the call stays under the two evaluations it is made of, nothing
// was tuned.  A chunk whose offset is at or past the capacity ends at once.
// fp32, no contraction; tests/spray.py repeats it step for step.
#pragma once
#include "ocean_velocity_kernels.h"

namespace ocean {

constexpr unsigned SPRAY_CHUNK = 1024;          // C: lattice indices per workgroup
constexpr unsigned SPRAY_ROUNDS = SPRAY_CHUNK / 256;
constexpr unsigned SPRAY_SCAN_WIDTH = 256;      // chunk counts per step of the scan
constexpr unsigned SPRAY_MASKS = SPRAY_CHUNK / 64;     // ballot masks per chunk

struct SprayArgs {
    QueryArgs q;                       // the surface (q.xz / out_* / points / iterations / choppy / gain unused)
    TwinMaps tw;                       // the set's twins where twinned != 0
    int twinned;
    int from_slot;                     // the frame was an OCEAN_MODE_JACOBIAN one: J_c = disp.w; otherwise (FULL7) from the normal map and lam
    float lam[OCEAN_MAX_CASCADES];     // lambda of the frame that wrote tile c's maps
    float threshold, gain, min_rise;
    unsigned thin_mask, salt;          // (1 << thin_log2) - 1
    int ix0, iy0, half;                // the window's first vertex; grid_size / 2
    unsigned nx, points;               // points = nx * ny <= 2^24
    unsigned capacity, chunks;         // chunks = ceil(points / C)
    unsigned long long* masks;         // [chunks][SPRAY_MASKS]  scratch: mask r * 4 + w = round r, wave w of the chunk
    unsigned* counts;                  // [chunks]               scratch: the chunk's count, then (scan) the count of all chunks before it
    float4* out_pos;                   // [capacity]
    float4* out_vel;                   // [capacity]
    unsigned* out_index;               // [capacity]
    unsigned* out_count;               // [2]
};

__device__ __forceinline__ unsigned spray_hash(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// Lattice index i of the window: whether the vertex is listed, and its row (pos, vel).  The thinning comes first because it is the cheapest
// term of a conjunction; a vertex it drops is not evaluated (pos / vel are then not set).  The integer steps wrap in 32 bits.
__device__ __forceinline__ bool spray_vertex(const SprayArgs& s, const float (&amp)[OCEAN_MAX_CASCADES], const float (&tamp)[OCEAN_MAX_CASCADES],
                                             unsigned i, float4& pos, float4& vel)
{
#pragma clang fp contract(off)
    if ((spray_hash(i + s.salt) & s.thin_mask) != 0u) return false;
    const QueryArgs& a = s.q;
    const int xi = (int)((unsigned)s.ix0 + i % s.nx), yi = (int)((unsigned)s.iy0 + i / s.nx);
    const float px = (float)xi * a.vertex_distance, pz = (float)yi * a.vertex_distance;
    const float u = (float)(int)((unsigned)xi + (unsigned)s.half) / a.grid, v = (float)(int)((unsigned)yi + (unsigned)s.half) / a.grid;
    float j = 3.402823466e+38f;
    const SurfaceEval e = eval_surface_uv<false>(a, amp, u, v, [&](int c, const float4& d, const float4& sl) {
#pragma clang fp contract(off)
        const float jc = s.from_slot ? d.w : (1.0f + s.lam[c] * sl.z) * (1.0f + s.lam[c] * sl.w);
        j = fminf(j, jc);
    });
    bool pass = j < s.threshold;
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if (s.twinned) {
        water_velocity_uv(a, s.tw, tamp, u, v, vx, vy, vz);
        pass = pass && vy >= s.min_rise;
    }
    const float strength = fminf(fmaxf((s.threshold - j) * s.gain, 0.0f), 1.0f);
    pos = make_float4(px + e.dx, 0.0f + e.dy, pz + e.dz, strength);
    vel = make_float4(vx, vy, vz, j);
    return pass;
}

__device__ __forceinline__ void spray_amplitudes(const SprayArgs& s, float (&amp)[OCEAN_MAX_CASCADES], float (&tamp)[OCEAN_MAX_CASCADES])
{
    cascade_amplitudes(s.q.s.minmax, s.q.s.count, amp);
    if (s.twinned) {
        cascade_amplitudes(s.tw.minmax, s.q.s.count, tamp);
    } else {
#pragma unroll
        for (int c = 0; c < OCEAN_MAX_CASCADES; ++c) tamp[c] = 0.0f;
    }
}

__global__ void __launch_bounds__(256) k_spray_count(const SprayArgs s)
{
    __shared__ unsigned wave_count[4];
    float amp[OCEAN_MAX_CASCADES], tamp[OCEAN_MAX_CASCADES];
    spray_amplitudes(s, amp, tamp);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned mine = 0;                                  // of this wave, all rounds
    for (unsigned r = 0; r < SPRAY_ROUNDS; ++r) {
        const unsigned i = blockIdx.x * SPRAY_CHUNK + r * 256u + threadIdx.x;
        float4 pos, vel;
        const bool pass = i < s.points && spray_vertex(s, amp, tamp, i, pos, vel);
        const unsigned long long m = __ballot(pass);
        if (lane == 0) s.masks[(size_t)blockIdx.x * SPRAY_MASKS + r * 4u + wave] = m;
        mine += (unsigned)__popcll(m);
    }
    if (lane == 0) wave_count[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) s.counts[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

__global__ void __launch_bounds__(256) k_spray_scan(const SprayArgs s)
{
    __shared__ unsigned wave_sum[4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned carry = 0;                                 // the count of all chunks before this step's (the same in every thread)
    for (unsigned base = 0; base < s.chunks; base += SPRAY_SCAN_WIDTH) {
        const unsigned k = base + threadIdx.x;
        const unsigned own = k < s.chunks ? s.counts[k] : 0u;
        unsigned x = own;                               // inclusive sum within the wave
        for (unsigned off = 1; off < 64u; off <<= 1) {
            const unsigned y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) wave_sum[wave] = x;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (unsigned w = 0; w < 4u; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (k < s.chunks) s.counts[k] = carry + before + (x - own);
        carry += all;
        __syncthreads();                                // wave_sum is written again by the next step
    }
    if (threadIdx.x == 0) {
        s.out_count[0] = carry;
        s.out_count[1] = carry < s.capacity ? carry : s.capacity;
    }
}

__global__ void __launch_bounds__(256) k_spray_scatter(const SprayArgs s)
{
    __shared__ unsigned wave_count[SPRAY_ROUNDS][4];
    unsigned rank0 = s.counts[blockIdx.x];              // rows before this round of this chunk
    if (rank0 >= s.capacity) return;                    // (the whole workgroup: nothing of this chunk is stored)
    float amp[OCEAN_MAX_CASCADES], tamp[OCEAN_MAX_CASCADES];
    spray_amplitudes(s, amp, tamp);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned r = 0; r < SPRAY_ROUNDS; ++r) {
        const unsigned i = blockIdx.x * SPRAY_CHUNK + r * 256u + threadIdx.x;
        const unsigned long long m = s.masks[(size_t)blockIdx.x * SPRAY_MASKS + r * 4u + wave];
        const bool pass = (m >> lane) & 1ull;
        if (lane == 0) wave_count[r][wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = 0, all = 0;
        for (unsigned w = 0; w < 4u; ++w) {
            if (w < wave) before += wave_count[r][w];
            all += wave_count[r][w];
        }
        const unsigned rank = rank0 + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (pass && rank < s.capacity) {
            float4 pos, vel;
            (void)spray_vertex(s, amp, tamp, i, pos, vel);
            s.out_pos[rank] = pos;
            s.out_vel[rank] = vel;
            s.out_index[rank] = i;
        }
        rank0 += all;
        if (rank0 >= s.capacity) return;                // (uniform: the later rounds are past the capacity)
    }
}

}  // namespace ocean
