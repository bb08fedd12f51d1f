// ocean_aux_kernels.h -- the kernels around the frame path, compiled into ocean_api.hip only: Prepare() (wave vectors, gaussian draws, base
// spectrum and quantised dispersion: WSTessendorf.cpp:36-148), the fp16 copy of the spectrum and the bounds of the half2 intermediates, the
// half-precision pack of the gather, the empirical spectra and the spectrum's moments.  The consumers' kernels are in ocean_consumer_kernels.h and ocean_foam_kernels.h (ocean_consumers.hip).
// The frame kernels themselves are in ocean_kernels.h.
#pragma once
#include "../../include/ocean_consumers.h"      // OCEAN_SPECTRUM_*, OCEAN_SPREAD_*
#include "ocean_kernels.h"

namespace ocean {

// ============================================================================
// Prepare(): wave vectors (.cpp:60-85), gaussian draws (.cpp:87-103, RNG
// replaced by a counter-based one), base spectrum + dispersion (.cpp:105-148).
// No FMA contraction here: omega goes through floor() and must match the fp32
// evaluation order of the reference.
// ============================================================================
__device__ inline uint64_t splitmix64(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ inline float2 gauss_pair(uint64_t seed, uint64_t idx)
{
    const uint64_t z = splitmix64(seed, idx);
    const double u1 = ((double)(z >> 40) + 1.0) * (1.0 / 16777216.0);
    const double u2 = (double)((z >> 8) & 0xFFFFFFull) * (1.0 / 16777216.0);
    const double r = sqrt(-2.0 * log(u1));
    const double a = 6.283185307179586476925286766559 * u2;
    double s, c;
    sincos(a, &s, &c);
    return make_float2((float)(r * c), (float)(r * s));
}

__global__ void k_init_k1d(float* __restrict__ k1d, const TileParams* __restrict__ tp, int n)
{
    const int tile = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // M_PI * (2.0f*i - kSize) / kLength : float numerator, double product/quotient (.cpp:76-79)
    const float num = 2.0f * (float)i - (float)n;
    k1d[(size_t)tile * n + i] =
        (float)(3.14159265358979323846 * (double)num / (double)tp[tile].length);
}

__device__ inline float phillips_nc(const TileParams& p, float ux, float uz, float k)
{
#pragma clang fp contract(off)
    // WSTessendorf.h:249-263
    const float k2 = k * k;
    const float k4 = k2 * k2;
    float cf = ux * p.wind_x + uz * p.wind_y;
    cf = cf * cf;
    const float lw = p.wind_speed * p.wind_speed / 9.81f;
    const float l2 = lw * lw;
    return p.phillips_a * expf(-1.0f / (k2 * l2)) / k4 * cf * expf(-k2 * p.damping * p.damping);
}

__global__ void k_init_spectrum(float2* __restrict__ h0, float* __restrict__ omega, uint16_t* __restrict__ omega_q,
                                float* __restrict__ base_freq, unsigned* __restrict__ omega_q_overflow, float2* __restrict__ xi_out,
                                const float2* __restrict__ xi_in, const float* __restrict__ k1d,
                                const TileParams* __restrict__ tp, int n)
{
#pragma clang fp contract(off)
    const int tile = blockIdx.y;
    const size_t n2 = (size_t)n * n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    const TileParams p = tp[tile];
    // the spectrum is stored TRANSPOSED: element i holds wave index (m, q) = (i % n, i / n),
    // so that a spectrum column (fixed kx) is one contiguous run for the first pass.
    // The gaussian draw of texel (m, q) keeps the reference's row-major index m*n + q.
    const int q = (int)(i / n), m = (int)(i % n);
    const size_t ref = (size_t)m * n + q;
    const float kx = k1d[(size_t)tile * n + q], kz = k1d[(size_t)tile * n + m];
    const float d = kx * kx + kz * kz;
    const float k = sqrtf(d);
    const float2 g = xi_in ? xi_in[tile * n2 + ref] : gauss_pair(p.seed, ref);
    if (xi_out) xi_out[tile * n2 + ref] = g;
    float2 a = make_float2(0.f, 0.f);
    float w = 0.f, steps = 0.f;
    if (i == 0) base_freq[tile] = p.base_freq;
    if (k > 0.00001f) {
        const float inv = 1.0f / sqrtf(d);            // glm::normalize (.h:133-136)
        const float ux = kx * inv, uz = kz * inv;
        const float sp = sqrtf(phillips_nc(p, ux, uz, k));
        const float s = 1.0f / sqrtf(2.0f);
        a.x = (s * g.x) * sp;                         // .h:237-243
        a.y = (s * g.y) * sp;
        float disp;                                   // the relation the reference calls, or one of the two it only defines
        if (p.dispersion == 1)        // sqrt(g k tanh(k D)): in double, rounded once (tanhf differs between libms)
            disp = (float)sqrt((double)(9.81f * k) * tanh((double)k * (double)p.dispersion_param));
        else if (p.dispersion == 2)   // sqrt(g k (1 + k^2 L^2))
            disp = sqrtf(9.81f * k * (1.0f + k * k * p.dispersion_param * p.dispersion_param));
        else
            disp = sqrtf(9.81f * k);
        steps = floorf(disp / p.base_freq);
        w = steps * p.base_freq;                         // .h:284-287
    }
    h0[tile * n2 + i] = a;
    omega[tile * n2 + i] = w;
    // omega is an integer multiple of base_freq: the frame kernels read that integer (2 bytes instead of
    // 4 per texel) and rebuild the same float, float(steps) * base_freq, unless some multiple needs more bits
    omega_q[tile * n2 + i] = (uint16_t)(steps < 65536.0f ? (unsigned)steps : 0u);
    if (!(steps < 65536.0f)) atomicOr(omega_q_overflow, 1u);
}

// Empirical spectra and wavenumber bands (include/ocean_consumers.h: ocean_set_spectrum).  One entry per tile, resolved on the host at
// ocean_prepare: the peak, the level and every constant of the tile in double.  active == 0: the default sea (or a twin, whose spectrum
// k_derive_spectrum writes): k_shape_spectrum leaves the tile alone.
struct SpecParams {
    uint32_t active;         // 0: nothing to do for this tile
    uint32_t kind;           // OCEAN_SPECTRUM_*
    uint32_t spreading;      // OCEAN_SPREAD_*
    int dispersion;          // the context's dispersion kind: the continuous omega and d omega / dk
    float k_min, k_max;      // the band, compared with the fp32 k; k_max == 0: no upper limit
    double dispersion_param;
    double alpha, peak_omega, gamma;
    double tma_depth;
    double spread_s;         // COS2S exponent
    double hass_mu;          // Hasselmann's exponent beyond 1.05 omega_p: -2.33 - 1.45 (U omega_p / g - 1.17)
    double swell2;           // swell^2
    double dk2;              // (2 pi / L)^2
    double scale;
};

// sqrt(P) of one bin, in double throughout: the text of include/ocean_consumers.h ("The spectrum") line for line.
__device__ inline double empirical_amplitude(const SpecParams& sp, double k, double c)
{
#pragma clang fp contract(off)
    const double g = 9.81;
    double w, dwdk;
    if (sp.dispersion == 1) {
        const double kd = k * sp.dispersion_param, th = tanh(kd);
        w = sqrt(g * k * th);
        dwdk = g * (th + kd * (1.0 - th * th)) / (2.0 * w);
    } else if (sp.dispersion == 2) {
        const double kl2 = k * k * sp.dispersion_param * sp.dispersion_param;
        w = sqrt(g * k * (1.0 + kl2));
        dwdk = g * (1.0 + 3.0 * kl2) / (2.0 * w);
    } else {
        w = sqrt(g * k);
        dwdk = 0.5 * sqrt(g / k);
    }
    const double wp = sp.peak_omega;
    const double pw = wp / w, pw2 = pw * pw;
    const double sigma = w <= wp ? 0.07 : 0.09;
    const double dw = w - wp;
    const double r = exp(-(dw * dw) / (2.0 * sigma * sigma * wp * wp));
    const double w2 = w * w;
    double S = sp.alpha * g * g / (w2 * w2 * w) * exp(-1.25 * (pw2 * pw2)) * pow(sp.gamma, r);
    if (sp.kind == OCEAN_SPECTRUM_TMA) {
        const double wh = w * sqrt(sp.tma_depth / g);
        if (wh <= 1.0) S *= 0.5 * wh * wh;
        else if (wh < 2.0) S *= 1.0 - 0.5 * (2.0 - wh) * (2.0 - wh);
    }
    double s;
    if (sp.spreading == OCEAN_SPREAD_HASSELMANN) {
        const double x = w / wp;
        s = x <= 1.05 ? 6.97 * pow(x, 4.06) : 9.77 * pow(x, sp.hass_mu);
    } else {
        s = sp.spread_s;
    }
    s += 16.0 * tanh(pw) * sp.swell2;
    const double lnQ = (2.0 * s - 1.0) * 0.69314718055994530942 - 1.1447298858494001741 + 2.0 * lgamma(s + 1.0) - lgamma(2.0 * s + 1.0);
    const double D = exp(lnQ) * pow(0.5 * (1.0 + c), s);
    const double P = S * D * dwdk / k * sp.dk2;
    return sp.scale * sqrt(P);
}

// Runs behind k_init_spectrum and before k_derive_spectrum.  A tile with an empirical kind gets h0 = ((s g.x) sp, (s g.y) sp) from the draws
// in xi (generated or injected: k_init_spectrum has left them there), sp the double amplitude above rounded once; a texel outside the
// tile's band becomes (0, 0) whatever the kind.  k, ux, uz are formed exactly as k_init_spectrum forms them; omega, omega_q, the draws and
// DC are not touched.  Same transposed layout: element i is wave index (m, q) = (i % n, i / n), its draw sits at m * n + q.
__global__ void k_shape_spectrum(float2* __restrict__ h0, const float2* __restrict__ xi, const float* __restrict__ k1d,
                                 const TileParams* __restrict__ tp, const SpecParams* __restrict__ spec, int n)
{
#pragma clang fp contract(off)
    const int tile = blockIdx.y;
    if (!spec[tile].active) return;
    const size_t n2 = (size_t)n * n;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    const SpecParams sp = spec[tile];
    const int q = (int)(i / n), m = (int)(i % n);
    const float kx = k1d[(size_t)tile * n + q], kz = k1d[(size_t)tile * n + m];
    const float d = kx * kx + kz * kz;
    const float k = sqrtf(d);
    if (!(k > 0.00001f)) return;                        // DC stays what k_init_spectrum wrote: (0, 0)
    if (!(sp.k_min <= k && (sp.k_max == 0.0f || k < sp.k_max))) {
        h0[tile * n2 + i] = make_float2(0.f, 0.f);
        return;
    }
    if (sp.kind == OCEAN_SPECTRUM_PHILLIPS) return;     // inside the band a Phillips tile keeps its bits
    const float inv = 1.0f / sqrtf(d);
    const float ux = kx * inv, uz = kz * inv;
    const double dot = (double)ux * (double)tp[tile].wind_x + (double)uz * (double)tp[tile].wind_y;
    const double c = fmin(fmax(dot, -1.0), 1.0);
    const float a = (float)empirical_amplitude(sp, (double)k, c);
    const float2 g = xi[tile * n2 + (size_t)m * n + q];
    const float s = 1.0f / sqrtf(2.0f);
    h0[tile * n2 + i] = make_float2((s * g.x) * a, (s * g.y) * a);
}

// ocean_spectrum_moments: sum |h0|^2, sum k |h0|^2, sum k^2 |h0|^2 of one tile, in double, in a fixed order, without atomics: the same
// spectrum gives the same bits on every run.  k is the fp32 wavenumber of the bin (as k_init_spectrum forms it) promoted to double.
// Stage 1, one workgroup of 256 per spectrum column (contiguous in the transposed layout): lane l adds elements l, l + 256, ... in that
// order, then a tree over the 256 lane sums (off = 128 ... 1: slot[l] += slot[l + off]).  Stage 2, one workgroup: the same over the n
// column sums.
__device__ inline void moments_tree(double (*sh)[256], double v[3], double* __restrict__ out)
{
    for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] = sh[j][threadIdx.x] + sh[j][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int j = 0; j < 3; ++j) out[j] = sh[j][0];
}

__global__ void __launch_bounds__(256) k_moments_columns(const float2* __restrict__ h0, const float* __restrict__ k1d,
                                                         double* __restrict__ colsum, int n)
{
#pragma clang fp contract(off)
    __shared__ double sh[3][256];
    const int col = blockIdx.x;                         // (h0 and k1d point at the tile)
    const float2* __restrict__ c = h0 + (size_t)col * n;
    const float kx = k1d[col];
    double v[3] = {0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < n; e += 256) {
        const float2 a = c[e];
        const float kz = k1d[e];
        const double k = (double)sqrtf(kx * kx + kz * kz);
        const double p = (double)a.x * (double)a.x + (double)a.y * (double)a.y;
        v[0] = v[0] + p;
        v[1] = v[1] + k * p;
        v[2] = v[2] + (k * k) * p;
    }
    moments_tree(sh, v, colsum + 3 * (size_t)col);
}

__global__ void __launch_bounds__(256) k_moments_total(const double* __restrict__ colsum, double* __restrict__ out, int n)
{
#pragma clang fp contract(off)
    __shared__ double sh[3][256];
    double v[3] = {0.0, 0.0, 0.0};
    for (int col = threadIdx.x; col < n; col += 256)
        for (int j = 0; j < 3; ++j) v[j] = v[j] + colsum[3 * (size_t)col + j];
    moments_tree(sh, v, out);
}

// Derivative twin tiles (include/ocean_consumers.h: ocean_set_velocity_twin).  h~(k, t) = 2 Re(h0 e^{i w t}) has the time derivative
// 2 Re(i w h0 e^{i w t}): the same expression for the spectrum i w h0 = (-w h0.im, w h0.re), and everything behind the spectrum is linear in
// it.  Runs behind k_init_spectrum and before anything else reads h0 (fp16 copy, bounds of the half2 intermediates): overwrites every texel of
// the twin's spectrum from its source's -- same transposed element, one fp32 multiply per component, w the fp32 omega (the float the 16-bit
// form reconstructs) -- and copies the source's draws into the twin's slot.  The twin's k, omega and omega_q are its source's already: it
// was initialised with its source's parameters.  One launch per (twin, source).
__global__ void k_derive_spectrum(float2* __restrict__ h0, const float* __restrict__ omega, float2* __restrict__ xi,
                                  uint32_t twin, uint32_t source, size_t n2)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    const float2 s = h0[source * n2 + i];
    const float w = omega[source * n2 + i];
    h0[twin * n2 + i] = make_float2(-(w * s.y), w * s.x);
    xi[twin * n2 + i] = xi[source * n2 + i];
}

// fp16 spectrum variant (BASELINE config 4): h0 stored as half2 scaled per tile so
// that max|component| maps to 2^14 (keeps the small amplitudes normal numbers).
__global__ void k_h0_absmax(const float2* __restrict__ h0, unsigned* __restrict__ maxbits, size_t n2)
{
    const int tile = blockIdx.y;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        const float2 v = h0[tile * n2 + i];
        m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits + tile, __float_as_uint(m));   // non-negative floats order like uints
}

__global__ void k_h0_to_half(const float2* __restrict__ h0, __half2* __restrict__ h0h, const unsigned* __restrict__ maxbits,
                             float* __restrict__ inv_scale, size_t n2)
{
    const int tile = blockIdx.y;
    const float m = __uint_as_float(maxbits[tile]);
    // power-of-two scale: exact to apply and to undo
    int e = 0;
    if (m > 0.0f) (void)frexpf(m, &e);                 // m = f * 2^e, f in [0.5, 1)
    const float scale = ldexpf(1.0f, 14 - e);
    if (blockIdx.x == 0 && threadIdx.x == 0) inv_scale[tile] = ldexpf(1.0f, e - 14);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        const float2 v = h0[tile * n2 + i];
        h0h[tile * n2 + i] = __floats2half2_rn(v.x * scale, v.y * scale);
    }
}

// Bounds for the half2 intermediates (ocean_set_intermediate_precision(16)), per tile, time independent:
//   |h~(k, t)| <= 2 |h0(k)|, so every component of a z-pass output of spectrum column n is at most
//   2 * sum_e |h0(e, n)| + 2 * sum_e |h0(e, -n)|   for the fields weighted by unit vectors (pair 0, height), and the same
//   with |k| |h0| for the fields weighted by k (pairs 1 and 2).  One workgroup per spectrum column (contiguous in the
//   transposed layout) sums |h0| and |k| |h0|; the maxima over the columns go to bounds[tile][0..1] as float bits.
__global__ void k_inter_bounds(const float2* __restrict__ h0, const float* __restrict__ k1d, unsigned* __restrict__ bounds, int n)
{
    const int tile = blockIdx.y, col = blockIdx.x;
    const float2* __restrict__ c = h0 + ((size_t)tile * n + col) * n;
    const float* __restrict__ k1 = k1d + (size_t)tile * n;
    const float kx = k1[col];
    float su = 0.0f, sk = 0.0f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const float2 v = c[e];
        const float m = sqrtf(v.x * v.x + v.y * v.y), kz = k1[e];
        su += m;
        sk += m * sqrtf(kx * kx + kz * kz);
    }
    __shared__ float ru[16], rk[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { su += __shfl_xor(su, o); sk += __shfl_xor(sk, o); }
    if ((threadIdx.x & 63) == 0) { ru[threadIdx.x >> 6] = su; rk[threadIdx.x >> 6] = sk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tu = 0.0f, tk = 0.0f;
        for (unsigned w = 0; w < (blockDim.x + 63) / 64; ++w) { tu += ru[w]; tk += rk[w]; }
        atomicMax(bounds + 2 * tile + 0, __float_as_uint(tu));      // non-negative floats order like uints
        atomicMax(bounds + 2 * tile + 1, __float_as_uint(tk));
    }
}


// Packed-map gather at half the bytes (the gather is xGMI-bound): one RGBA32F texel -> four halves
// (round to nearest even; |values| of both maps are far below the largest half, 65504, for any sea the reference
// parameters can describe -- larger values saturate to +-inf like any float -> half conversion).
__global__ void k_pack_half(const float4* __restrict__ src, uint2* __restrict__ dst, size_t texels)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < texels; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        const __half2 a = __floats2half2_rn(v.x, v.y), b = __floats2half2_rn(v.z, v.w);
        uint2 o;
        __builtin_memcpy(&o.x, &a, 4); __builtin_memcpy(&o.y, &b, 4);
        dst[i] = o;
    }
}

}  // namespace ocean
