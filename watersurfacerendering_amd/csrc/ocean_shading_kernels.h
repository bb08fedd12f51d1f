// ocean_shading_kernels.h -- the kernels behind the fragment stage (include/ocean_consumers.h: ocean_sky_radiance, ocean_eval_seabed,
// ocean_shade_points, ocean_shade_grid), compiled into ocean_consumers.hip only.  The reference's SkyPreetham.frag and
// WaterSurfaceMesh.frag as pure per-point functions: one thread per point, 256-thread workgroups, a grid-stride loop, 16-byte loads and
// stores of the float4 rows, no LDS, no atomics.  Everything uniform over a launch arrives by value in one argument block the host has
// precomputed (the normalised sun, the 21 sky coefficients with ZenithLum / ZeroThetaSun already divided, 0.33 backscatter / absorb, the
// 0.1-scaled attenuation coefficients).
//   Seabed   value noise over a multiplicative hash: adds, multiplies, floorf, one sqrtf and three divisions.  fp32 without contraction in
//            the order the header states: the one part held to bits (tests/shading.py restates it in float32).  Five fbm4 evaluations per
//            point, 20 noise samples, 80 hashes: the bulk of the shading kernel's arithmetic, so the `seabed` switch is a template
//            parameter -- selected once per launch, and the flat form carries none of it.
//   Optics   may contract; held to the derived bound of tests/shading.py, which assumes a few ulps for each of expf, powf, acosf, sinf,
//            cosf, tanf: the device library's full-precision forms, no fast intrinsics.
#pragma once
#include "ocean_consumer_kernels.h"

namespace ocean {

struct SkyDev {                  // what SKY(d) and the sun terms read
    float sun[3];                // normalised
    float A[3], B[3], C[3], D[3], E[3];
    float zn[3];                 // ZenithLum / ZeroThetaSun per channel of Yxy
    float sun_color[3];
    float sun_intensity;
};

struct SkyArgs {
    SkyDev sky;
    const float* dirs;           // [count][3]
    float4* out;
    unsigned count;
};

struct SeabedArgs {
    const float2* xz;
    float4* out;
    unsigned count;
};

struct ShadeArgs {
    SkyDev sky;
    float cam[3];
    float height;
    float absorb01[3], scatter01[3];     // absorb * 0.1, scatter * 0.1
    float df0[3];                        // (0.33 backscatter) / absorb
    float terrain[3];
    float sky_intensity, specular_intensity, highlights;
    float seabed_factor;
    float f0;                            // ((ior - 1) / (ior + 1))^2
    int physical_fresnel, foam_white, tonemap;
    const float4* pos;
    const float4* nrm;
    float4* out_rgba;
    float4* out_aux;                     // may be null
    unsigned count;
};

// ---- seabed: bit-exact, no contraction -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sb_fract(float a)
{
#pragma clang fp contract(off)
    return a - floorf(a);
}

__device__ __forceinline__ float sb_hash1(float ix, float iy)
{
#pragma clang fp contract(off)
    const float jx = 50.0f * sb_fract(ix * 0.31830987f), jy = 50.0f * sb_fract(iy * 0.31830987f);
    return sb_fract((jx * jy) * (jx + jy));
}

__device__ __forceinline__ float sb_noise(float px, float py)
{
#pragma clang fp contract(off)
    const float ix = floorf(px), iy = floorf(py);
    const float fx = px - ix, fy = py - iy;
    const float ux = ((fx * fx) * fx) * (fx * (fx * 6.0f - 15.0f) + 10.0f);
    const float uy = ((fy * fy) * fy) * (fy * (fy * 6.0f - 15.0f) + 10.0f);
    const float a = sb_hash1(ix, iy), b = sb_hash1(ix + 1.0f, iy), c = sb_hash1(ix, iy + 1.0f), d = sb_hash1(ix + 1.0f, iy + 1.0f);
    return -1.0f + 2.0f * (((a + (b - a) * ux) + (c - a) * uy) + ((((a - b) - c) + d) * ux) * uy);
}

__device__ __forceinline__ float sb_fbm4(float px, float py)
{
#pragma clang fp contract(off)
    float v = 0.0f, g = 0.5f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v = v + g * sb_noise(px, py);
        g = g * 0.5f;
        const float qx = 1.6f * px + 1.2f * py, qy = -1.2f * px + 1.6f * py;
        px = qx; py = qy;
    }
    return v;
}

__device__ __forceinline__ float sb_height(float x, float z)
{
#pragma clang fp contract(off)
    return 0.0f - 8.0f * sb_fbm4(z * 0.02f, x * 0.02f);
}

// (n.x, n.y, n.z, colour factor) of the reference's seabed at terrain point (x, z)
__device__ __forceinline__ float4 seabed_eval(float x, float z)
{
#pragma clang fp contract(off)
    const float factor = fminf(fmaxf(sb_fbm4((z * 0.02f) * 2.0f, (x * 0.02f) * 2.0f), 0.6f), 0.9f);
    const float e = 1e-4f;
    const float nx = sb_height(x - e, z) - sb_height(x + e, z);
    const float ny = 10.0f * e;
    const float nz = sb_height(x, z - e) - sb_height(x, z + e);
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    return make_float4(nx / len, ny / len, nz / len, factor);
}

__global__ void __launch_bounds__(256) k_eval_seabed(const SeabedArgs a)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.count; i += gridDim.x * 256u) {
        const float2 p = a.xz[i];
        a.out[i] = seabed_eval(p.x, p.y);
    }
}

// ---- optics ----------------------------------------------------------------------------------------------------------------------------------
struct SkyLum { float r, g, b, disk; };

// SKY(d) of the header for a direction taken as it is (the callers normalise, or pass the reflection as the shader does)
__device__ __forceinline__ SkyLum sky_lum(const SkyDev& s, float dx, float dy, float dz)
{
    const float cy = fminf(fmaxf(dy, 0.0f), 1.0f);
    const float cg = fminf(fmaxf(s.sun[0] * dx + s.sun[1] * dy + s.sun[2] * dz, 0.0f), 1.0f);
    const float theta = acosf(cy), gamma = acosf(cg);
    const float ct = cosf(theta) + 1e-3f, cgm = cosf(gamma);
    float yxy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = (1.0f + s.A[k] * expf(s.B[k] / ct)) * (1.0f + s.C[k] * expf(s.D[k] * gamma) + s.E[k] * cgm * cgm);
        yxy[k] = s.zn[k] * f;
    }
    const float yy = yxy[0] / yxy[2];
    const float X = yxy[1] * yy, Y = yxy[0], Z = (1.0f - yxy[1] - yxy[2]) * yy;
    SkyLum o;
    o.r = 2.3706743f * X - 0.9000405f * Y - 0.4706338f * Z;
    o.g = -0.5138850f * X + 1.4253036f * Y + 0.0885814f * Z;
    o.b = 0.0052982f * X - 0.0146949f * Y + 1.0093968f * Z;
    const float t = fminf(fmaxf((cg - 0.997f) / (1.0f - 0.997f), 0.0f), 1.0f);
    o.disk = t * t * (3.0f - 2.0f * t);
    return o;
}

__global__ void __launch_bounds__(256) k_sky_radiance(const SkyArgs a)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.count; i += gridDim.x * 256u) {
        const float* in = a.dirs + (size_t)i * 3;
        const float x = in[0], y = in[1], z = in[2];
        const float len = sqrtf(x * x + y * y + z * z);
        const SkyLum l = sky_lum(a.sky, x / len, y / len, z / len);
        const float d = l.disk;
        a.out[i] = make_float4(l.r * 0.05f + (a.sky.sun_color[0] * d) * l.r, l.g * 0.05f + (a.sky.sun_color[1] * d) * l.g,
                               l.b * 0.05f + (a.sky.sun_color[2] * d) * l.b, d);
    }
}

constexpr float WATER_IOR = 1.33477f;
constexpr float WATER_ETA = (float)(1.0 / 1.33477);

template <bool REFERENCE_SEABED>
__global__ void __launch_bounds__(256) k_shade_points(const ShadeArgs a)
{
    const SkyDev& s = a.sky;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.count; i += gridDim.x * 256u) {
        const float4 p = a.pos[i], nn = a.nrm[i];
        // the ray to the unraised position, the unit normal, the raised point
        float dx = p.x - a.cam[0], dy = p.y - a.cam[1], dz = p.z - a.cam[2];
        const float dl = sqrtf(dx * dx + dy * dy + dz * dz);
        dx /= dl; dy /= dl; dz /= dl;
        const float nl = sqrtf(nn.x * nn.x + nn.y * nn.y + nn.z * nn.z);
        const float nx = nn.x / nl, ny = nn.y / nl, nz = nn.z / nl;
        const float pwy = p.y + a.height;
        // the reflected sky
        const float dn = nx * dx + ny * dy + nz * dz;
        const float k2 = 2.0f * dn;
        const SkyLum l = sky_lum(s, dx - k2 * nx, dy - k2 * ny, dz - k2 * nz);
        const float S[3] = {l.r * 0.05f + l.disk * l.r, l.g * 0.05f + l.disk * l.g, l.b * 0.05f + l.disk * l.b};
        const float ndl = fmaxf(nx * s.sun[0] + ny * s.sun[1] + nz * s.sun[2], 0.0f);
        const float ka = a.sky_intensity * ndl;
        // Blinn-Phong glint
        float hx = s.sun[0] - dx, hy = s.sun[1] - dy, hz = s.sun[2] - dz;
        const float hl = sqrtf(hx * hx + hy * hy + hz * hz);
        hx /= hl; hy /= hl; hz /= hl;
        const float ndh = fmaxf(nx * hx + ny * hy + nz * hz, 0.0f);
        const float spec = a.specular_intensity * fminf(fmaxf(powf(ndh, a.highlights), 0.0f), 1.0f);
        const float ks = s.sun_intensity * spec;
        // the sun's ray refracted into the water, down to the plane y = 0
        const float c = -(nx * s.sun[0] + ny * s.sun[1] + nz * s.sun[2]);
        const float kk = 1.0f - (WATER_ETA * WATER_ETA) * (1.0f - c * c);
        float rx = 0.0f, ry = 0.0f, rz = 0.0f;
        if (kk >= 0.0f) {
            const float m = WATER_ETA * c + sqrtf(kk);
            rx = -WATER_ETA * s.sun[0] - m * nx; ry = -WATER_ETA * s.sun[1] - m * ny; rz = -WATER_ETA * s.sun[2] - m * nz;
        }
        const float tg = -pwy / ry;
        const float gx = p.x + tg * rx, gy = pwy + tg * ry, gz = p.z + tg * rz;
        float4 sb = make_float4(0.0f, 1.0f, 0.0f, a.seabed_factor);
        if (REFERENCE_SEABED) sb = seabed_eval(gx, gz);
        const float lg = sb.w * -(sb.x * rx + sb.y * ry + sb.z * rz);
        const float depth = fabsf(pwy - gy);
        // Fresnel reflectivity towards the camera
        const float ci = -dn;
        float fr;
        if (a.physical_fresnel) {
            fr = 1.0f;
            if (ci > 0.0f) {
                const float ct = sqrtf(1.0f - (1.0f - ci * ci) / (WATER_IOR * WATER_IOR));
                const float rs = (ci - WATER_IOR * ct) / (ci + WATER_IOR * ct), rp = (WATER_IOR * ci - ct) / (WATER_IOR * ci + ct);
                fr = 0.5f * (rs * rs + rp * rp);
            }
        } else {
            const float tt = -(nx * rx + ny * ry + nz * rz);
            fr = a.f0;
            if (!(ci <= 1e-5f)) {
                const float t1 = sinf(ci - tt) / sinf(ci + tt), t2 = tanf(ci - tt) / tanf(ci + tt);
                fr = 0.5f * (t1 * t1 + t2 * t2);
            }
        }
        float col[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float la = ka * S[k], ls = ks * S[k];
            const float ldf0 = a.df0[k] * ((3.14159265f * la) * 0.318309886f);
            const float att0 = expf(-a.absorb01[k] * tg);
            const float att1 = expf(-a.absorb01[k] * tg - a.scatter01[k] * depth);
            const float lu = att0 * (lg * a.terrain[k]) + (1.0f - att1) * ldf0;
            col[k] = fr * (ls + la) + (1.0f - fr) * lu;
        }
        if (a.foam_white && p.w < 0.0f) col[0] = col[1] = col[2] = 1.0f;
        float4 o = make_float4(col[0], col[1], col[2], 1.0f);
        if (a.tonemap) o = make_float4(1.0f - expf(-2.0f * o.x), 1.0f - expf(-2.0f * o.y), 1.0f - expf(-2.0f * o.z), 1.0f - expf(-2.0f * o.w));
        a.out_rgba[i] = o;
        if (a.out_aux) a.out_aux[i] = make_float4(gx, gz, tg, fr);
    }
}

}  // namespace ocean
