// ocean_waves_kernels.h -- the kernels behind the Gerstner proxy (include/ocean_consumers.h: ocean_extract_waves, ocean_eval_waves,
// ocean_query_waves), compiled into ocean_consumers.hip only.  A tile's wave set is a list of at most WAVES_MAX spectrum bins (ocean_wave
// rows); the kernels here pick the strongest bins of a prepared spectrum and evaluate such a list analytically at any point and time.
//   Selection   a radix select on 64-bit keys, (bits of the bin's power) << 32 | ~bin: the keys are distinct, so "the K largest" has one
//               answer and the order of the integer atomics cannot show.  k_wave_hist counts one 8-bit digit of the keys that share the
//               digits found so far; the host reads the 256 counts, picks the digit that holds the K-th largest and stops as soon as a digit's
//               whole bucket is taken (with distinct powers: after the power's digits, four passes or fewer; only a tie across rank K goes
//               on into the bin's digits).  k_wave_select then collects (power bits, bin) of every key at or above the threshold -- exactly
//               K of them, in any order --, the host sorts those <= 4096 pairs and k_wave_rows fills the rows in rank order.  No launch
//               waits on another workgroup.
//   Evaluation  k_waves_animate turns the rows of every cascade into 12 floats per wave, once per call: (float)jx, (float)jz and the seven
//               per-channel amplitudes c, ux c, uz c, kx c, kz c, kx ux c, kz uz c with c(t) = the frames' height_re(re, im, cos wt, sin wt).
//               k_waves_eval / k_waves_query walk that table per point with a wave-uniform index -- the table is const __restrict__, so the
//               reads are scalar loads that cost the vector ALU nothing -- and keep seven accumulators: per wave two fract, the reduction of
//               the phase in turns, the two polynomials of sincos_f32 on [-pi/4, pi/4] and seven fused multiply-adds.  VALU-bound.
//               The order of the sum is not part of the contract (the header states a derived error bound instead), so the accumulations
//               may contract.
#pragma once
#include "ocean_consumer_kernels.h"

namespace ocean {

constexpr unsigned WAVES_MAX = 4096;            // rows per wave set
constexpr unsigned WAVES_ANIM_VEC = 3;          // float4 per wave of the animated table

// ---- selection -----------------------------------------------------------------------------------------------------------------------------
// The key of device element d = q * N + p (the spectrum is stored transposed: column q = kx index first): power in fp32 without contraction,
// 0 for a bin that is no candidate (p > 0 fails for 0, negative zero and NaN), above the complement of bin = p * N + q, so that of two equal
// powers the lower bin has the larger key.
__device__ __forceinline__ unsigned long long wave_key(const float2* __restrict__ h0, unsigned d, unsigned n, unsigned log2n)
{
#pragma clang fp contract(off)
    const float2 h = h0[d];
    const float pw = h.x * h.x + h.y * h.y;
    const unsigned pkey = pw > 0.0f ? __float_as_uint(pw) : 0u;
    const unsigned p = d & (n - 1u), q = d >> log2n;
    const unsigned bin = p * n + q;
    return ((unsigned long long)pkey << 32) | (unsigned long long)(0xffffffffu - bin);
}

// hist[0 .. 255] += the digit (key >> shift) & 255 of every key whose digits above it equal prefix's; hist[256] += the candidates (first
// pass only: shift == 56).  Per-workgroup counts in LDS, then one global atomic per non-empty digit.
__global__ void __launch_bounds__(256) k_wave_hist(const float2* __restrict__ h0, unsigned n, unsigned log2n, unsigned long long prefix,
                                                   int shift, unsigned* __restrict__ hist)
{
    __shared__ unsigned lh[257];
    for (unsigned i = threadIdx.x; i < 257u; i += 256u) lh[i] = 0u;
    __syncthreads();
    const unsigned n2 = n * n;
    for (unsigned d = blockIdx.x * 256u + threadIdx.x; d < n2; d += gridDim.x * 256u) {
        const unsigned long long key = wave_key(h0, d, n, log2n);
        if (shift == 56) {
            if (key >> 32) atomicAdd(&lh[256], 1u);
        } else if ((key ^ prefix) >> (shift + 8)) continue;
        atomicAdd(&lh[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < 257u; i += 256u)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// list[slot] = (power bits, bin) of every key >= threshold, slots handed out by one counter; a slot at or past `capacity` is counted but
// not written (the host finds the count wrong and reports it).
__global__ void __launch_bounds__(256) k_wave_select(const float2* __restrict__ h0, unsigned n, unsigned log2n, unsigned long long threshold,
                                                     unsigned capacity, unsigned* __restrict__ counter, uint2* __restrict__ list)
{
    const unsigned n2 = n * n;
    for (unsigned d = blockIdx.x * 256u + threadIdx.x; d < n2; d += gridDim.x * 256u) {
        const unsigned long long key = wave_key(h0, d, n, log2n);
        if (key < threshold) continue;
        const unsigned slot = atomicAdd(counter, 1u);
        if (slot < capacity) list[slot] = make_uint2((unsigned)(key >> 32), 0xffffffffu - (unsigned)key);
    }
}

// Row j of the set from bin bins[j] (include/ocean_consumers.h: ocean_wave); fp32, no contraction.
__global__ void __launch_bounds__(256) k_wave_rows(const float2* __restrict__ h0, const float* __restrict__ omega, const float* __restrict__ k1d,
                                                   unsigned n, const unsigned* __restrict__ bins, unsigned count, ocean_wave* __restrict__ rows)
{
#pragma clang fp contract(off)
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const unsigned bin = bins[j] & (n * n - 1u);
    const unsigned p = bin / n, q = bin % n, d = q * n + p;
    ocean_wave w;
    w.jx = (int)q - (int)(n / 2u); w.jz = (int)p - (int)(n / 2u);
    w.kx = k1d[q]; w.kz = k1d[p];
    const float len = sqrtf(w.kx * w.kx + w.kz * w.kz);
    const float r = 1.0f / len;
    w.ux = len <= 1e-5f ? 0.0f : w.kx * r;
    w.uz = len <= 1e-5f ? 0.0f : w.kz * r;
    w.re = h0[d].x; w.im = h0[d].y;
    w.omega = omega[d];
    w.bin = bin;
    w.reserved[0] = 0.0f; w.reserved[1] = 0.0f;
    rows[j] = w;
}

// ---- evaluation ----------------------------------------------------------------------------------------------------------------------------
struct WaveSetArgs {
    const ocean_wave* rows;                // sets of the FIRST tile of the cascade set (tile c at + c * WAVES_MAX)
    float4* anim;                          // [cascades][WAVES_MAX][WAVES_ANIM_VEC]
    unsigned count[OCEAN_MAX_CASCADES];    // rows of cascade c's set
    float tt[OCEAN_MAX_CASCADES];          // t + the tile's time offset
};

// grid (WAVES_MAX / 256, cascades).  wt is ONE fp32 multiply and the sine, cosine and height_re are the frames' (ocean_kernels.h).
__global__ void __launch_bounds__(256) k_waves_animate(const WaveSetArgs s)
{
#pragma clang fp contract(off)
    const unsigned c = blockIdx.y, j = blockIdx.x * 256u + threadIdx.x;
    if (j >= s.count[c]) return;
    const ocean_wave w = s.rows[c * WAVES_MAX + j];
    const float wt = mul_nocontract(w.omega, s.tt[c]);
    float sn, cs;
    sincos_f32(wt, sn, cs);
    const float a = height_re(w.re, w.im, cs, sn);
    float4* o = s.anim + ((size_t)c * WAVES_MAX + j) * WAVES_ANIM_VEC;
    o[0] = make_float4((float)w.jx, (float)w.jz, a, w.ux * a);
    o[1] = make_float4(w.uz * a, w.kx * a, w.kz * a, (w.kx * w.ux) * a);
    o[2] = make_float4((w.kz * w.uz) * a, 0.0f, 0.0f, 0.0f);
}

struct WaveEvalArgs {
    WaveSetArgs set;
    const float2* xz;                      // [points]
    float4* out_pos;                       // [points]
    float4* out_nrm;                       // [points]
    unsigned points;
    int cascades;
    int iterations;                        // the inverse only
    float fn, inv_n;                       // (float)N, 1.0f / N
    float grid, half, vertex_distance, choppy;
    float uv_scale[OCEAN_MAX_CASCADES];
    float lam[OCEAN_MAX_CASCADES];         // the tile's lambda at the time of the call
    float gain[OCEAN_MAX_CASCADES];        // lam_c * (s_c * L_c / (grid * vertex_distance)): the Newton step's unit factor, as the map query's
};

// sine and cosine of 2 pi ph for ph in [0, 2]: the quarter turn q = rint(4 ph) is taken off exactly (an FMA of exact operands), what is left
// (|r| <= 1/8 turn) becomes an angle with 2 pi split in two floats, and the polynomials are sincos_f32's (Cephes, [-pi/4, pi/4]).
__device__ __forceinline__ void sincos_turns(float ph, float& s, float& c)
{
    const float fq = rintf(ph * 4.0f);
    const float r = __builtin_fmaf(fq, -0.25f, ph);
    const float x = __builtin_fmaf(r, 6.2831855f, r * -1.7484555e-7f);
    const float z = x * x;
    float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
    const float sn = __builtin_fmaf(ps * z, x, x);
    float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
    const float cs = __builtin_fmaf(pc * z, z, __builtin_fmaf(z, -0.5f, 1.0f));
    const int q = (int)fq;
    const float so = (q & 1) ? cs : sn;
    const float co = (q & 1) ? sn : cs;
    s = (q & 2) ? -so : so;
    c = ((q + 1) & 2) ? -co : co;
}

struct WaveEval {
    float px, py, pz, j;                   // P(r) and the smallest diagonal Jacobian of the cascades
    float sx, sz, ddx, ddz;                // S: the summed slopes and displacement derivatives
    float jx, jz;                          // sum_c gain_c * (dxDx_c, dzDz_c)
};

// The wave sets of every cascade at rest point (rx, rz).
__device__ __forceinline__ WaveEval eval_waves(const WaveEvalArgs& a, const float4* __restrict__ anim, float rx, float rz)
{
    const float u = rest_uv(a, rx), v = rest_uv(a, rz);
    WaveEval e{0.0f, 0.0f, 0.0f, 3.402823466e+38f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < a.cascades; ++c) {
        float fx, fz;
        {
#pragma clang fp contract(off)
            const float tx = (u * a.uv_scale[c]) * a.fn - 0.5f, tz = (v * a.uv_scale[c]) * a.fn - 0.5f;
            const float x = tx * a.inv_n, z = tz * a.inv_n;
            fx = x - floorf(x); fz = z - floorf(z);
        }
        float h = 0.0f, dx = 0.0f, dz = 0.0f, sx = 0.0f, sz = 0.0f, xx = 0.0f, zz = 0.0f;
        const float4* __restrict__ w = anim + (size_t)c * WAVES_MAX * WAVES_ANIM_VEC;
        const unsigned count = a.set.count[c];
#pragma unroll 2
        for (unsigned j = 0; j < count; ++j) {
            const float4 w0 = w[j * WAVES_ANIM_VEC + 0], w1 = w[j * WAVES_ANIM_VEC + 1], w2 = w[j * WAVES_ANIM_VEC + 2];
            float pa, pb;
            {
#pragma clang fp contract(off)
                pa = w0.x * fx; pb = w0.y * fz;
                pa = pa - floorf(pa); pb = pb - floorf(pb);
            }
            float st, ct;
            sincos_turns(pa + pb, st, ct);
            h = __builtin_fmaf(w0.z, ct, h);
            dx = __builtin_fmaf(w0.w, st, dx);
            dz = __builtin_fmaf(w1.x, st, dz);
            sx = __builtin_fmaf(-w1.y, st, sx);
            sz = __builtin_fmaf(-w1.z, st, sz);
            xx = __builtin_fmaf(w1.w, ct, xx);
            zz = __builtin_fmaf(w2.x, ct, zz);
        }
        {
#pragma clang fp contract(off)
            const float lam = a.lam[c];
            e.px = e.px + lam * dx; e.py = e.py + h; e.pz = e.pz + lam * dz;
            e.sx = e.sx + sx; e.sz = e.sz + sz; e.ddx = e.ddx + xx; e.ddz = e.ddz + zz;
            e.j = fminf(e.j, (1.0f + lam * xx) * (1.0f + lam * zz));
            e.jx = e.jx + xx * a.gain[c]; e.jz = e.jz + zz * a.gain[c];
        }
    }
    {
#pragma clang fp contract(off)
        e.px = rx + e.px; e.pz = rz + e.pz;
    }
    return e;
}

__device__ __forceinline__ float4 waves_normal(const WaveEvalArgs& a, const WaveEval& e, float w)
{
    const float3 n = vertex_normal(e.sx, e.sz, e.ddx, e.ddz, a.choppy);
    return make_float4(n.x, n.y, n.z, w);
}

// Forward evaluation: what the cascade vertex stage would draw for a vertex at rest point xz[i], from the wave sets alone.
__global__ void __launch_bounds__(256) k_waves_eval(const WaveEvalArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.points) return;
    const float2 r = a.xz[i];
    const WaveEval e = eval_waves(a, a.set.anim, r.x, r.y);
    a.out_pos[i] = make_float4(e.px, e.py, e.pz, e.j);
    a.out_nrm[i] = waves_normal(a, e, 0.0f);
}

// The inverse: ocean_query_surface's diagonal Newton iteration on the analytic evaluation.
__global__ void __launch_bounds__(256) k_waves_query(const WaveEvalArgs a)
{
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.points) return;
    const float2 q = a.xz[i];
    float rx = q.x, rz = q.y;
    for (int k = 0; k < a.iterations; ++k) {
        const WaveEval e = eval_waves(a, a.set.anim, rx, rz);
        const float ex = e.px - q.x, ez = e.pz - q.y;
        const float jx = clamp_jacobian(1.0f + e.jx), jz = clamp_jacobian(1.0f + e.jz);
        rx = rx - ex / jx;
        rz = rz - ez / jz;
    }
    const WaveEval e = eval_waves(a, a.set.anim, rx, rz);
    const float ex = e.px - q.x, ez = e.pz - q.y;
    a.out_pos[i] = make_float4(e.px, e.py, e.pz, e.j);
    a.out_nrm[i] = waves_normal(a, e, sqrtf(ex * ex + ez * ez));
}

}  // namespace ocean
