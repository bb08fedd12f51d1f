// ocean_consumers.hip -- host side of include/ocean_consumers.h: what reads the maps of the most recent frame on the device (vertex stage and
// cascades, mip chain, surface query, ray cast, persistent foam, buoyancy, water velocity, LOD sampling, surface bounds, spray emitters) and the device memory those calls own -- and the Gerstner proxy, which reads the prepared spectrum instead.  Their kernels:
// ocean_consumer_kernels.h, ocean_foam_kernels.h, ocean_velocity_kernels.h, ocean_buoyancy_kernels.h, ocean_lod_kernels.h, ocean_bounds_kernels.h, ocean_spray_kernels.h, ocean_waves_kernels.h, ocean_shading_kernels.h (the fragment stage: sky, seabed, water colour, which read no map either).  What it shares with ocean_api.hip is at the end of ocean_ctx.h.  No CPU fallback here either.
#include <algorithm>
#include <cmath>

#include "ocean_ctx.h"
#include "ocean_foam_kernels.h"     // (includes ocean_consumer_kernels.h)
#include "ocean_buoyancy_kernels.h" // (includes ocean_velocity_kernels.h)
#include "ocean_lod_kernels.h"
#include "ocean_bounds_kernels.h"
#include "ocean_spray_kernels.h"
#include "ocean_waves_kernels.h"
#include "ocean_shading_kernels.h"

using namespace ocean;

// ---- the host path every consumer shares ---------------------------------------------------------------------------------------------------
// What a consumer reads: the most recently enqueued frame.  Its maps and height keys from tile `first_tile` on, and the stream it was enqueued
// on -- the consumer's launch goes there, so it is ordered after the frame that wrote these maps.
struct LastFrame {
    const float4* disp;
    const float4* nrm;
    const unsigned* minmax;
    hipStream_t st;
    int set;                // the frame's chain: c->set_lambda / set_length / set_mode[set] describe it
    size_t n2;              // texels per tile
};
static int last_frame(const ocean_ctx* c, uint32_t first_tile, LastFrame& f)
{
    if (!c->prepared || !c->have_frame) return OCEAN_E_NOT_READY;
    f.set = c->last_set;
    f.n2 = (size_t)c->n * c->n;
    f.disp = maps_of(c, f.set).disp + first_tile * f.n2;
    f.nrm = maps_of(c, f.set).nrm + first_tile * f.n2;
    f.minmax = c->minmax[f.set] + 2 * first_tile;
    f.st = stream_of(c, f.set);
    return OCEAN_OK;
}

// Calls that read no frame: the consumers' stream only orders them among the other consumer calls.
static void no_frame(const ocean_ctx* c, LastFrame& f)
{
    f = LastFrame{};
    f.set = c->last_set;
    f.st = stream_of(c, f.set);
}

// The consumer kernels write context-wide output buffers and run on the stream of the frame they read.  At pipeline depth > 1 consecutive
// consumer calls land on different, mutually unordered chain streams: each call first makes its stream wait for the previous consumer launch,
// so that two of them never write those buffers at once.
static int consumer_begin(ocean_ctx* c, hipStream_t st)
{
    // (a frame whose in-launch wait has given up by now is recovered before anything consumes it; one that gives up later is reported
    //  by the next wait / synchronisation: recover_fault)
    OCEAN_TRY(check_fault(c));
    if (c->consumer_pending && c->consumer_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->consumer_ev, 0));
    return OCEAN_OK;
}
static int consumer_end(ocean_ctx* c, hipStream_t st)
{
    if (!c->consumer_ev) HIP_TRY(hipEventCreateWithFlags(&c->consumer_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->consumer_ev, st));
    c->consumer_stream = st;
    c->consumer_pending = true;
    return OCEAN_OK;
}

// Replaces a context-wide buffer (or two that grow together: b may be null) by one of `bytes` each.  Nothing in flight may still use the old
// one, so everything is drained first; the capacity is zero while there is no buffer, and `invalidate` drops whatever "ready" state described
// the old contents at the moment they are freed -- a growth that fails half way leaves nothing that claims to be readable.
template <class T, class Cap, class Invalidate>
static int regrow(ocean_ctx* c, T** a, T** b, size_t bytes, Cap& capacity, Cap want, Invalidate invalidate)
{
    OCEAN_TRY(sync_all(c));
    for (T** p : {a, b})
        if (p && *p) { (void)hipFree(*p); *p = nullptr; }
    capacity = 0;
    invalidate();
    for (T** p : {a, b})
        if (p) HIP_TRY(hipMalloc(p, bytes));
    capacity = want;
    return OCEAN_OK;
}

template <class T>
static void free_and_null(T*& p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

void ocean_consumers_release(ocean_ctx* c, bool everything)
{
    free_and_null(c->staging); c->staging_bytes = 0;
    for (float*& f : c->foam) free_and_null(f);
    free_and_null(c->foam_lambda); c->foam_lambda_host.clear();
    c->foam_cur = 0; c->foam_ready = false;
    // the grid and mip buffers survive a new tile size (the grid's does not depend on it, ocean_build_mips re-allocates for mips_n != n),
    // their contents do not: they were made from maps that are gone
    c->mips_ready = false; c->grid_vertices = 0; c->grid_fresh = false; c->shaded_vertices = 0;
    c->lod.ready = c->bnd.ready = false;    // (the sets of ocean_build_mips_tiles / _bounds_tiles likewise: their capacity is in texels, whatever the tile size)
    std::fill(c->wave_count.begin(), c->wave_count.end(), 0u);      // (the wave sets name bins of a lattice that is gone; their buffers stay)
    if (!everything) return;
    free_and_null(c->grid_pos); free_and_null(c->grid_nrm); c->grid_capacity = 0;
    free_and_null(c->mips_disp); free_and_null(c->mips_nrm); c->mips_n = 0;
    for (TileChains* t : {&c->lod, &c->bnd}) { free_and_null(t->a); free_and_null(t->b); t->capacity = 0; }
    free_and_null(c->hull); c->hull_points = 0;
    free_and_null(c->spray_scratch); c->spray_chunks = 0;
    free_and_null(c->waves); free_and_null(c->wave_anim); free_and_null(c->wave_scratch);
    free_and_null(c->shaded); c->shaded_capacity = 0;
    if (c->consumer_ev) { (void)hipEventDestroy(c->consumer_ev); c->consumer_ev = nullptr; }
    c->consumer_pending = false;
}

// ---- vertex stage and mip chain ------------------------------------------------------------------------------------------------------------
// What the kernels read of the cascade set of `count` tiles that frame f starts at (f = last_frame(c, first_tile)).
static void cascade_set(const ocean_ctx* c, const LastFrame& f, uint32_t count, const float* uv_scales, CascadeSet& s)
{
    s.disp = f.disp; s.nrm = f.nrm; s.minmax = f.minmax;
    s.tile_texels = f.n2; s.n = (int)c->n; s.count = (int)count;
    for (uint32_t i = 0; i < (uint32_t)OCEAN_MAX_CASCADES; ++i) s.uv_scale[i] = i < count ? uv_scales[i] : 0.0f;
}

// The vertex stage's three calls.  Readiness from tile first_tile on, the output buffers for a grid of grid_size quads per side, and the
// kernels' arguments ...
static int grid_args(ocean_ctx* c, uint32_t first_tile, uint32_t count, const float* uv_scales, uint32_t grid_size, float vertex_distance,
                     float choppy, LastFrame& f, CascadeArgs& o, uint32_t& verts)
{
    OCEAN_TRY(last_frame(c, first_tile, f));
    HIP_TRY(hipSetDevice(c->device));
    verts = (grid_size + 1) * (grid_size + 1);
    if (verts > c->grid_capacity)
        OCEAN_TRY(regrow(c, &c->grid_pos, &c->grid_nrm, (size_t)verts * sizeof(float4), c->grid_capacity, verts, [c] { c->grid_vertices = 0; }));
    o.positions = c->grid_pos; o.normals = c->grid_nrm;
    o.grid = (int)grid_size; o.vertex_distance = vertex_distance; o.choppy = choppy;
    cascade_set(c, f, count, uv_scales, o.s);
    return OCEAN_OK;
}

// ... the launch, one thread per vertex ...
template <class Args>
static int launch_grid(ocean_ctx* c, const LastFrame& f, void (*kernel)(Args), const Args& a, uint32_t verts)
{
    OCEAN_TRY(consumer_begin(c, f.st));
    hipLaunchKernelGGL(kernel, dim3((verts + 255) / 256), dim3(256), 0, f.st, a);
    HIP_TRY(hipGetLastError());
    OCEAN_TRY(consumer_end(c, f.st));
    c->grid_vertices = verts; c->grid_fresh = true;
    return OCEAN_OK;
}

// ... and what the two cascade forms check of their arguments.
static bool cascade_grid_valid(const ocean_ctx* c, uint32_t first_tile, uint32_t count, uint32_t grid_size, const float* uv_scales)
{
    return c && uv_scales && count != 0 && count <= (uint32_t)OCEAN_MAX_CASCADES && first_tile < c->tiles && first_tile + count <= c->tiles &&
           grid_size != 0 && grid_size <= 8192;
}

extern "C" {

int ocean_displace_grid(ocean_t* c, uint32_t tile, uint32_t grid_size, float vertex_distance, float uv_scale, float choppy)
{
    if (!c || tile >= c->tiles || grid_size == 0 || grid_size > 8192) return OCEAN_E_INVALID;
    LastFrame f;
    GridArgs g;
    uint32_t verts;
    OCEAN_TRY(grid_args(c, tile, 1, &uv_scale, grid_size, vertex_distance, choppy, f, g, verts));
    return launch_grid(c, f, k_displace_grid, g, verts);
}

int ocean_displace_grid_cascades(ocean_t* c, uint32_t first_tile, uint32_t count, uint32_t grid_size, float vertex_distance,
                                 const float* uv_scales, float choppy)
{
    if (!cascade_grid_valid(c, first_tile, count, grid_size, uv_scales)) return OCEAN_E_INVALID;
    LastFrame f;
    CascadeArgs a;
    uint32_t verts;
    OCEAN_TRY(grid_args(c, first_tile, count, uv_scales, grid_size, vertex_distance, choppy, f, a, verts));
    return launch_grid(c, f, k_displace_grid_cascades, a, verts);
}

int ocean_read_grid(ocean_t* c, float* positions, float* normals)
{
    if (!c) return OCEAN_E_INVALID;
    if (!c->grid_vertices) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    if (positions) HIP_TRY(hipMemcpy(positions, c->grid_pos, (size_t)c->grid_vertices * sizeof(float4), hipMemcpyDeviceToHost));
    if (normals) HIP_TRY(hipMemcpy(normals, c->grid_nrm, (size_t)c->grid_vertices * sizeof(float4), hipMemcpyDeviceToHost));
    return OCEAN_OK;
}

int ocean_device_grid(ocean_t* c, void** d_positions, void** d_normals, uint32_t* vertices)
{
    if (!c) return OCEAN_E_INVALID;
    if (d_positions) *d_positions = c->grid_pos;
    if (d_normals) *d_normals = c->grid_nrm;
    if (vertices) *vertices = c->grid_vertices;
    return OCEAN_OK;
}

size_t ocean_mip_texels(uint32_t n) { return ((size_t)n * n - 1) / 3; }      // sum of (n >> l)^2, l = 1 .. log2 n

int ocean_build_mips(ocean_t* c, uint32_t tile)
{
    if (!c || tile >= c->tiles) return OCEAN_E_INVALID;
    LastFrame f;
    OCEAN_TRY(last_frame(c, tile, f));
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = c->n;
    if (c->mips_n != n)
        OCEAN_TRY(regrow(c, &c->mips_disp, &c->mips_nrm, ocean_mip_texels(n) * sizeof(float4), c->mips_n, n, [c] { c->mips_ready = false; }));
    MipArgs m;
    m.src[0] = f.disp; m.src[1] = f.nrm;
    m.dst[0] = c->mips_disp; m.dst[1] = c->mips_nrm;
    OCEAN_TRY(consumer_begin(c, f.st));
    for (uint32_t w = n / 2; w >= 1; w /= 2) {
        m.w = (int)w;
        hipLaunchKernelGGL(k_mip_level, dim3((w * w + 255) / 256, 2), dim3(256), 0, f.st, m);
        m.src[0] = m.dst[0]; m.src[1] = m.dst[1];
        m.dst[0] += (size_t)w * w; m.dst[1] += (size_t)w * w;
    }
    HIP_TRY(hipGetLastError());
    OCEAN_TRY(consumer_end(c, f.st));
    c->mips_ready = true;
    return OCEAN_OK;
}

int ocean_read_mips(ocean_t* c, float* disp_mips, float* nrm_mips)
{
    if (!c) return OCEAN_E_INVALID;
    if (!c->mips_ready) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    const size_t bytes = ocean_mip_texels(c->mips_n) * sizeof(float4);
    if (disp_mips) HIP_TRY(hipMemcpy(disp_mips, c->mips_disp, bytes, hipMemcpyDeviceToHost));
    if (nrm_mips) HIP_TRY(hipMemcpy(nrm_mips, c->mips_nrm, bytes, hipMemcpyDeviceToHost));
    return OCEAN_OK;
}

int ocean_device_mips(ocean_t* c, void** d_disp_mips, void** d_nrm_mips, uint32_t* levels)
{
    if (!c) return OCEAN_E_INVALID;
    if (d_disp_mips) *d_disp_mips = c->mips_ready ? c->mips_disp : nullptr;
    if (d_nrm_mips) *d_nrm_mips = c->mips_ready ? c->mips_nrm : nullptr;
    if (levels) { uint32_t l = 0; for (uint32_t w = c->mips_n; c->mips_ready && w > 1; w /= 2) ++l; *levels = l; }
    return OCEAN_OK;
}

}  // extern "C"

// ---- query-like calls: surface query, ray cast, foam query ---------------------------------------------------------------------------------
// Each has a host-blocking form (host arrays in and out, through the staging buffer) and a _device twin (device arrays, stream-ordered), and
// each is: an argument builder (validation, then readiness: *_args below), the checks of call_checks, a launch function that binds the device
// arrays of `count` items into the arguments and launches.  out1 is null where a call has one output.
template <class Args>
using LaunchFn = int (*)(Args& a, uint32_t count, const void* d_in, void* d_out0, void* d_out1, hipStream_t st);

// Behind the builder's verdict `rc`, in the order the callers rely on: nothing to do for no items -- before the pointers are looked at --,
// then the pointers.  (A caller returns OCEAN_OK itself when count == 0.)
static int call_checks(ocean_ctx* c, int rc, uint32_t count, bool null_pointer)
{
    if (rc || count == 0) return rc;
    if (null_pointer) return OCEAN_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    return OCEAN_OK;
}

template <class Args>
static int device_call(ocean_ctx* c, int rc, const LastFrame& f, Args& a, LaunchFn<Args> launch, uint32_t count,
                       const void* d_in, void* d_out0, void* d_out1, int outs)
{
    OCEAN_TRY(call_checks(c, rc, count, !d_in || !d_out0 || (outs == 2 && !d_out1)));
    if (count == 0) return OCEAN_OK;
    OCEAN_TRY(consumer_begin(c, f.st));
    OCEAN_TRY(launch(a, count, d_in, d_out0, d_out1, f.st));
    return consumer_end(c, f.st);
}

// The host-blocking form: in_floats floats per item in, `outs` float4 per item out, staged in c->staging and copied on the frame's stream,
// which is synchronised before the call returns (what lets the three calls share that buffer: ocean_ctx.h).
template <class Args>
static int staged_call(ocean_ctx* c, int rc, const LastFrame& f, Args& a, LaunchFn<Args> launch, uint32_t count,
                       const float* in, size_t in_floats, float* out0, float* out1, int outs)
{
    OCEAN_TRY(call_checks(c, rc, count, !in || !out0 || (outs == 2 && !out1)));
    if (count == 0) return OCEAN_OK;
    const size_t out_bytes = (size_t)count * sizeof(float4), in_bytes = (size_t)count * in_floats * sizeof(float);
    const size_t bytes = (size_t)outs * out_bytes + in_bytes;
    if (bytes > c->staging_bytes) OCEAN_TRY(regrow(c, &c->staging, (void**)nullptr, bytes, c->staging_bytes, bytes, [] {}));
    // [outputs | input]: the float4 arrays first, so that every array is 16-byte aligned
    char* d_out0 = static_cast<char*>(c->staging);
    char* d_out1 = outs == 2 ? d_out0 + out_bytes : nullptr;
    char* d_in = d_out0 + (size_t)outs * out_bytes;
    OCEAN_TRY(consumer_begin(c, f.st));
    HIP_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, f.st));
    OCEAN_TRY(launch(a, count, d_in, d_out0, d_out1, f.st));
    HIP_TRY(hipMemcpyAsync(out0, d_out0, out_bytes, hipMemcpyDeviceToHost, f.st));
    if (outs == 2) HIP_TRY(hipMemcpyAsync(out1, d_out1, out_bytes, hipMemcpyDeviceToHost, f.st));
    OCEAN_TRY(consumer_end(c, f.st));
    HIP_TRY(hipStreamSynchronize(f.st));
    return OCEAN_OK;
}

// Checks and launch arguments of the surface every query-like call reads (the device pointers are bound by the launch function).
static int query_args(ocean_ctx* c, const ocean_surface* s, LastFrame& f, QueryArgs& a)
{
    if (!c || !s || s->cascades == 0 || s->cascades > (uint32_t)OCEAN_MAX_CASCADES || s->first_tile >= c->tiles ||
        s->cascades > c->tiles - s->first_tile || s->grid_size == 0 || s->iterations > 32)
        return OCEAN_E_INVALID;
    OCEAN_TRY(last_frame(c, s->first_tile, f));
    cascade_set(c, f, s->cascades, s->uv_scales, a.s);
    a.iterations = s->iterations ? (int)s->iterations : 8;
    a.grid = (float)s->grid_size;
    a.half = (float)(s->grid_size / 2);
    a.vertex_distance = s->vertex_distance;
    a.choppy = s->choppy;
    for (uint32_t i = 0; i < (uint32_t)OCEAN_MAX_CASCADES; ++i) {
        a.gain[i] = 0.0f;
        if (i < s->cascades) {      // lambda_c * (s_c * L_c / (grid * vertex_distance)) of the frame that wrote tile c's maps
            const uint32_t tile = s->first_tile + i;
            a.gain[i] = c->set_lambda[f.set][tile] * (s->uv_scales[i] * c->set_length[f.set][tile] / (a.grid * s->vertex_distance));
        }
    }
    return OCEAN_OK;
}

// ... of the calls that only evaluate forward: the Newton iterations do not matter there.
static int forward_args(ocean_ctx* c, const ocean_surface* s, LastFrame& f, QueryArgs& a)
{
    ocean_surface forward = *s;
    forward.iterations = 0;
    return query_args(c, &forward, f, a);
}

static int launch_query(QueryArgs& a, uint32_t points, const void* d_xz, void* d_out_pos, void* d_out_nrm, hipStream_t st)
{
    a.xz = static_cast<const float2*>(d_xz);
    a.out_pos = static_cast<float4*>(d_out_pos);
    a.out_nrm = static_cast<float4*>(d_out_nrm);
    a.points = points;
    hipLaunchKernelGGL(k_query_surface, dim3((a.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

// ... of the ray cast: the surface of the query, then the ray settings.
static int raycast_args(ocean_ctx* c, const ocean_surface* s, const ocean_raycast* r, LastFrame& f, RaycastArgs& a)
{
    if (!c || !s || !r || !(r->max_distance > 0.0f) || !std::isfinite(r->max_distance) || r->steps > 4096 || r->refine > 8)
        return OCEAN_E_INVALID;
    OCEAN_TRY(query_args(c, s, f, a.q));
    a.max_distance = r->max_distance;
    a.steps = r->steps ? (int)r->steps : 64;
    a.refine = r->refine ? (int)r->refine : 3;
    return OCEAN_OK;
}

static int launch_raycast(RaycastArgs& a, uint32_t count, const void* d_rays, void* d_out_hit, void* d_out_nrm, hipStream_t st)
{
    a.rays = static_cast<const float*>(d_rays);
    a.out_hit = static_cast<float4*>(d_out_hit);
    a.out_nrm = static_cast<float4*>(d_out_nrm);
    a.count = count;
    const unsigned rays_per_block = 256u / RAYCAST_LANES;
    hipLaunchKernelGGL(k_raycast_surface, dim3((unsigned)(((uint64_t)a.count + rays_per_block - 1u) / rays_per_block)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

// ... of the foam query: the surface of the query, then the foam of its first tile.
static int foam_query_args(ocean_ctx* c, const ocean_surface* s, LastFrame& f, FoamQueryArgs& a)
{
    OCEAN_TRY(query_args(c, s, f, a.q));
    if (!c->foam_ready) return OCEAN_E_NOT_READY;
    a.foam = c->foam[c->foam_cur] + s->first_tile * a.q.s.tile_texels;
    a.q.out_pos = nullptr; a.q.out_nrm = nullptr;
    return OCEAN_OK;
}

static int launch_foam_query(FoamQueryArgs& a, uint32_t points, const void* d_xz, void* d_out, void*, hipStream_t st)
{
    a.q.xz = static_cast<const float2*>(d_xz);
    a.out = static_cast<float4*>(d_out);
    a.q.points = points;
    hipLaunchKernelGGL(k_query_foam, dim3((a.q.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

int ocean_query_surface(ocean_t* c, const ocean_surface* s, const float* xz, uint32_t points, float* out_pos, float* out_nrm)
{
    LastFrame f;
    QueryArgs a;
    return staged_call(c, query_args(c, s, f, a), f, a, launch_query, points, xz, 2, out_pos, out_nrm, 2);
}

int ocean_query_surface_device(ocean_t* c, const ocean_surface* s, const void* d_xz, uint32_t points, void* d_out_pos, void* d_out_nrm)
{
    LastFrame f;
    QueryArgs a;
    return device_call(c, query_args(c, s, f, a), f, a, launch_query, points, d_xz, d_out_pos, d_out_nrm, 2);
}

int ocean_raycast_surface(ocean_t* c, const ocean_surface* s, const ocean_raycast* r, const float* rays, uint32_t count,
                          float* out_hit, float* out_nrm)
{
    LastFrame f;
    RaycastArgs a{};
    return staged_call(c, raycast_args(c, s, r, f, a), f, a, launch_raycast, count, rays, 6, out_hit, out_nrm, 2);
}

int ocean_raycast_surface_device(ocean_t* c, const ocean_surface* s, const ocean_raycast* r, const void* d_rays, uint32_t count,
                                 void* d_out_hit, void* d_out_nrm)
{
    LastFrame f;
    RaycastArgs a{};
    return device_call(c, raycast_args(c, s, r, f, a), f, a, launch_raycast, count, d_rays, d_out_hit, d_out_nrm, 2);
}

}  // extern "C"

// ---- LOD sampling (include/ocean_consumers.h): mip chains of a tile range, the footprint-driven sampler's two consumers ----------------------
static uint32_t log2_of(uint32_t n) { uint32_t l = 0; while ((1u << l) < n) ++l; return l; }

// ---- the two sets of chains of a tile range (TileChains, ocean_ctx.h): the mip chains here, the min/max pyramids further down ---------------
// The set covers the tiles [first, first + count) -- and, where a frame is given, was built from exactly that one (the most recent).
static bool chains_cover(const ocean_ctx* c, const TileChains& t, uint32_t first, uint32_t count, const LastFrame* f)
{
    if (!t.ready || first < t.first || first + count > t.first + t.count) return false;
    return !f || (t.frame == c->frame_serial && t.set == f->set);
}

static int chains_read_tile(ocean_ctx* c, const TileChains& t, uint32_t tile, float* a, float* b)
{
    if (tile >= c->tiles) return OCEAN_E_INVALID;
    if (!c->prepared || !c->have_frame || !chains_cover(c, t, tile, 1, nullptr)) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    const size_t chain = ocean_mip_texels(c->n), at = (tile - t.first) * chain;
    if (a) HIP_TRY(hipMemcpy(a, t.a + at, chain * sizeof(float4), hipMemcpyDeviceToHost));
    if (b) HIP_TRY(hipMemcpy(b, t.b + at, chain * sizeof(float4), hipMemcpyDeviceToHost));
    return OCEAN_OK;
}

static int chains_device(const ocean_ctx* c, const TileChains& t, void** d_a, void** d_b, uint32_t* first_tile, uint32_t* count, uint32_t* levels)
{
    if (d_a) *d_a = t.ready ? t.a : nullptr;
    if (d_b) *d_b = t.ready ? t.b : nullptr;
    if (first_tile) *first_tile = t.ready ? t.first : 0;
    if (count) *count = t.ready ? t.count : 0;
    if (levels) *levels = t.ready ? log2_of(c->n) : 0;
    return OCEAN_OK;
}

// Both sets are built alike (ocean_lod_kernels.h, ocean_bounds_kernels.h): behind the most recent frame, one launch that takes blocks of
// the maps src0 / src1 down to one texel each and, where N > MIP_BLOCK, a second for levels 7 .. log2 N from level 6 of the chains just
// written (at texel sum_{k=1}^{5} (N >> k)^2 of a chain), one block per chain and tile.  launch(second, blocks) enqueues m on f.st.
// From the first re-allocation to the end there is no set: a failure in between leaves none.
template <class Args, class Sources, class Launch>
static int build_chains(ocean_ctx* c, TileChains& t, uint32_t first_tile, uint32_t count, Args& m, Sources sources, Launch launch)
{
    if (!c || count == 0 || first_tile >= c->tiles || count > c->tiles - first_tile) return OCEAN_E_INVALID;
    LastFrame f;
    OCEAN_TRY(last_frame(c, first_tile, f));
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = c->n;
    const size_t need = (size_t)count * ocean_mip_texels(n);
    if (need > t.capacity) OCEAN_TRY(regrow(c, &t.a, &t.b, need * sizeof(float4), t.capacity, need, [&t] { t.ready = false; }));
    t.ready = false;
    sources(f, m);
    m.dst[0] = t.a; m.dst[1] = t.b;
    m.src_stride = f.n2; m.chain_texels = ocean_mip_texels(n); m.dst_offset = 0;
    m.sw = (int)n; m.be = n < (uint32_t)MIP_BLOCK ? (int)n : MIP_BLOCK;
    OCEAN_TRY(consumer_begin(c, f.st));
    launch(false, (n / m.be) * (n / m.be), f.st);
    if (n > (uint32_t)MIP_BLOCK) {
        const size_t level6 = ((size_t)n * n - (size_t)(n >> 5) * (n >> 5)) / 3;
        m.src[0] = t.a + level6; m.src[1] = t.b + level6;
        m.src_stride = m.chain_texels;
        m.sw = m.be = (int)(n / MIP_BLOCK);
        m.dst_offset = level6 + (size_t)m.sw * m.sw;
        launch(true, 1u, f.st);
    }
    HIP_TRY(hipGetLastError());
    OCEAN_TRY(consumer_end(c, f.st));
    t.first = first_tile; t.count = count; t.frame = c->frame_serial; t.set = f.set; t.ready = true;
    return OCEAN_OK;
}

// The sampler's share of the launch arguments for the cascade set first_tile .. first_tile + cascades - 1 read from frame f: the set must
// cover the range and have been built from exactly that frame -- whatever the footprints turn out to be.
static int lod_set_args(const ocean_ctx* c, const ocean_lod* l, const LastFrame& f, uint32_t first_tile, uint32_t cascades, const float* uv_scales,
                        uint32_t grid_size, float vertex_distance, LodSet& s)
{
    if (!chains_cover(c, c->lod, first_tile, cascades, &f)) return OCEAN_E_NOT_READY;
    s.chain_texels = ocean_mip_texels(c->n);
    s.mips_disp = c->lod.a + (first_tile - c->lod.first) * s.chain_texels;
    s.mips_nrm = c->lod.b + (first_tile - c->lod.first) * s.chain_texels;
    for (uint32_t i = 0; i < (uint32_t)OCEAN_MAX_CASCADES; ++i)
        s.tpm[i] = i < cascades ? std::fabs((uv_scales[i] * (float)c->n) / ((float)grid_size * vertex_distance)) : 0.0f;
    s.scale = l->scale;
    const uint32_t top = log2_of(c->n);
    s.lmax = (int)(l->max_level != 0 && l->max_level < top ? l->max_level : top);
    s.top = (float)(1u << s.lmax);
    return OCEAN_OK;
}

static bool lod_valid(const ocean_lod* l) { return l && l->scale > 0.0f && std::isfinite(l->scale); }

// ... of the point form: the LOD settings, the surface of the query (its iterations do not matter here), then the set.
static int lod_point_args(ocean_ctx* c, const ocean_surface* s, const ocean_lod* l, LastFrame& f, LodPointArgs& a)
{
    if (!c || !s || !lod_valid(l)) return OCEAN_E_INVALID;
    OCEAN_TRY(forward_args(c, s, f, a.q));
    return lod_set_args(c, l, f, s->first_tile, s->cascades, s->uv_scales, s->grid_size, s->vertex_distance, a.lod);
}

static int launch_lod_points(LodPointArgs& a, uint32_t points, const void* d_xzf, void* d_out_pos, void* d_out_nrm, hipStream_t st)
{
    a.xzf = static_cast<const float*>(d_xzf);
    a.q.xz = nullptr;
    a.q.out_pos = static_cast<float4*>(d_out_pos);
    a.q.out_nrm = static_cast<float4*>(d_out_nrm);
    a.q.points = points;
    hipLaunchKernelGGL(k_sample_surface_lod, dim3((a.q.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

int ocean_build_mips_tiles(ocean_t* c, uint32_t first_tile, uint32_t count)
{
    MipTilesArgs m;
    return build_chains(c, c->lod, first_tile, count, m, [](const LastFrame& f, MipTilesArgs& a) { a.src[0] = f.disp; a.src[1] = f.nrm; },
                        [&](bool, unsigned blocks, hipStream_t st) { hipLaunchKernelGGL(k_mips_tiles, dim3(blocks, 2, count), dim3(256), 0, st, m); });
}

int ocean_read_mips_tile(ocean_t* c, uint32_t tile, float* disp_mips, float* nrm_mips)
{
    return c ? chains_read_tile(c, c->lod, tile, disp_mips, nrm_mips) : OCEAN_E_INVALID;
}

int ocean_device_mips_tiles(ocean_t* c, void** d_disp_mips, void** d_nrm_mips, uint32_t* first_tile, uint32_t* count, uint32_t* levels)
{
    return c ? chains_device(c, c->lod, d_disp_mips, d_nrm_mips, first_tile, count, levels) : OCEAN_E_INVALID;
}

void ocean_default_lod(ocean_lod* l)
{
    if (!l) return;
    l->scale = 1.0f;
    l->max_level = 0;
}

int ocean_sample_surface_lod(ocean_t* c, const ocean_surface* s, const ocean_lod* l, const float* xzf, uint32_t points,
                             float* out_pos, float* out_nrm)
{
    LastFrame f;
    LodPointArgs a{};
    return staged_call(c, lod_point_args(c, s, l, f, a), f, a, launch_lod_points, points, xzf, 3, out_pos, out_nrm, 2);
}

int ocean_sample_surface_lod_device(ocean_t* c, const ocean_surface* s, const ocean_lod* l, const void* d_xzf, uint32_t points,
                                    void* d_out_pos, void* d_out_nrm)
{
    LastFrame f;
    LodPointArgs a{};
    return device_call(c, lod_point_args(c, s, l, f, a), f, a, launch_lod_points, points, d_xzf, d_out_pos, d_out_nrm, 2);
}

int ocean_displace_grid_lod(ocean_t* c, uint32_t first_tile, uint32_t count, uint32_t grid_size, float vertex_distance,
                            const float* uv_scales, float choppy, const ocean_lod* l)
{
    if (!cascade_grid_valid(c, first_tile, count, grid_size, uv_scales) || !lod_valid(l)) return OCEAN_E_INVALID;
    LastFrame f;
    LodGridArgs a{};
    uint32_t verts;
    // readiness is settled before the grid's buffers may be re-allocated (a refused call leaves the previous grid readable), and once more
    // behind that: a re-allocation drains the context, and a frame it had to run again is a new frame
    OCEAN_TRY(last_frame(c, first_tile, f));
    OCEAN_TRY(lod_set_args(c, l, f, first_tile, count, uv_scales, grid_size, vertex_distance, a.lod));
    OCEAN_TRY(grid_args(c, first_tile, count, uv_scales, grid_size, vertex_distance, choppy, f, a.a, verts));
    OCEAN_TRY(lod_set_args(c, l, f, first_tile, count, uv_scales, grid_size, vertex_distance, a.lod));
    return launch_grid(c, f, k_displace_grid_lod, a, verts);
}

}  // extern "C"

// ---- surface bounds (include/ocean_consumers.h): min/max pyramids of a tile range, patch boxes and their frustum class -----------------------
// ... of the patch query: the settings, the surface of the query (iterations and choppy do not matter here), then the set -- which must cover
// the cascade set and have been built from exactly the frame the call reads.
static int patch_args(ocean_ctx* c, const ocean_surface* s, const ocean_patch_query* q, LastFrame& f, PatchArgs& a)
{
    if (!c || !s || !q || q->planes > 6 || q->pad_texels > 65536) return OCEAN_E_INVALID;
    for (uint32_t k = 0; k < q->planes; ++k)
        for (int j = 0; j < 4; ++j)
            if (!std::isfinite(q->plane[k][j])) return OCEAN_E_INVALID;
    OCEAN_TRY(forward_args(c, s, f, a.q));
    if (!chains_cover(c, c->bnd, s->first_tile, s->cascades, &f)) return OCEAN_E_NOT_READY;
    a.chain_texels = ocean_mip_texels(c->n);
    a.lo = c->bnd.a + (s->first_tile - c->bnd.first) * a.chain_texels;
    a.hi = c->bnd.b + (s->first_tile - c->bnd.first) * a.chain_texels;
    a.top = (int)log2_of(c->n);
    a.first_level = (int)c->bnd_first_level;
    a.pad = (int)q->pad_texels;
    a.planes = (int)q->planes;
    for (int k = 0; k < 6; ++k)
        for (int j = 0; j < 4; ++j) a.plane[k][j] = (uint32_t)k < q->planes ? q->plane[k][j] : 0.0f;
    return OCEAN_OK;
}

static int launch_patch_bounds(PatchArgs& a, uint32_t count, const void* d_rects, void* d_out_lo, void* d_out_hi, hipStream_t st)
{
    a.rects = static_cast<const float*>(d_rects);
    a.q.xz = nullptr;
    a.q.out_pos = static_cast<float4*>(d_out_lo);
    a.q.out_nrm = static_cast<float4*>(d_out_hi);
    a.q.points = count;
    hipLaunchKernelGGL(k_patch_bounds, dim3((a.q.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

int ocean_build_bounds_tiles(ocean_t* c, uint32_t first_tile, uint32_t count, uint32_t first_level)
{
    if (!c || count == 0 || first_tile >= c->tiles || count > c->tiles - first_tile) return OCEAN_E_INVALID;
    const uint32_t n = c->n, top = log2_of(n);
    if (first_level == 0) first_level = 1;
    if (first_level > top) return OCEAN_E_INVALID;
    BoundsTilesArgs m;
    const auto sources = [](const LastFrame& f, BoundsTilesArgs& a) { a.src[0] = a.src[1] = f.disp; };
    // (the second launch reads level 6 whatever first_level says: the first stores from min(first_level, 6) where there is a second)
    const auto launch = [&](bool second, unsigned blocks, hipStream_t st) {
        m.level = second ? 7 : 1;
        m.store_from = (int)(!second && n > (uint32_t)MIP_BLOCK && first_level > 6 ? 6 : first_level);
        if (second) hipLaunchKernelGGL(k_bounds_tiles<true>, dim3(blocks, 1, count), dim3(256), 0, st, m);
        else hipLaunchKernelGGL(k_bounds_tiles<false>, dim3(blocks, 1, count), dim3(256), 0, st, m);
    };
    OCEAN_TRY(build_chains(c, c->bnd, first_tile, count, m, sources, launch));
    c->bnd_first_level = first_level;
    return OCEAN_OK;
}

int ocean_read_bounds_tile(ocean_t* c, uint32_t tile, float* lo_chain, float* hi_chain)
{
    return c ? chains_read_tile(c, c->bnd, tile, lo_chain, hi_chain) : OCEAN_E_INVALID;
}

int ocean_device_bounds_tiles(ocean_t* c, void** d_lo, void** d_hi, uint32_t* first_tile, uint32_t* count, uint32_t* levels, uint32_t* first_level)
{
    if (!c) return OCEAN_E_INVALID;
    if (first_level) *first_level = c->bnd.ready ? c->bnd_first_level : 0;
    return chains_device(c, c->bnd, d_lo, d_hi, first_tile, count, levels);
}

void ocean_default_patch_query(ocean_patch_query* q)
{
    if (!q) return;
    *q = ocean_patch_query{};
}

int ocean_patch_bounds(ocean_t* c, const ocean_surface* s, const ocean_patch_query* q, const float* rects, uint32_t count,
                       float* out_lo, float* out_hi)
{
    LastFrame f;
    PatchArgs a{};
    return staged_call(c, patch_args(c, s, q, f, a), f, a, launch_patch_bounds, count, rects, 4, out_lo, out_hi, 2);
}

int ocean_patch_bounds_device(ocean_t* c, const ocean_surface* s, const ocean_patch_query* q, const void* d_rects, uint32_t count,
                              void* d_out_lo, void* d_out_hi)
{
    LastFrame f;
    PatchArgs a{};
    return device_call(c, patch_args(c, s, q, f, a), f, a, launch_patch_bounds, count, d_rects, d_out_lo, d_out_hi, 2);
}

}  // extern "C"

// ---- water velocity (include/ocean_consumers.h): the twins of a cascade set, the velocity query ---------------------------------------------
// The twins of the set's tiles must be the consecutive tiles v, v + 1, ... in cascade order: their maps and keys of frame f.
static int twin_maps(const ocean_ctx* c, const ocean_surface* s, const LastFrame& f, TwinMaps& tw)
{
    uint32_t twin[OCEAN_MAX_CASCADES], found = 0;
    for (uint32_t k = 0; k < s->cascades; ++k) {
        twin[k] = OCEAN_NO_SOURCE;
        for (uint32_t i = 0; i < c->tiles && twin[k] == OCEAN_NO_SOURCE; ++i)
            if (c->twin_source[i] == s->first_tile + k) twin[k] = i;
        if (twin[k] != OCEAN_NO_SOURCE) ++found;
    }
    if (found == 0) return OCEAN_E_NOT_READY;
    if (found != s->cascades) return OCEAN_E_INVALID;
    for (uint32_t k = 1; k < s->cascades; ++k)
        if (twin[k] != twin[0] + k) return OCEAN_E_INVALID;
    tw.disp = maps_of(c, f.set).disp + twin[0] * f.n2;
    tw.minmax = c->minmax[f.set] + 2 * twin[0];
    return OCEAN_OK;
}

static int velocity_args(ocean_ctx* c, const ocean_surface* s, LastFrame& f, VelocityArgs& a)
{
    OCEAN_TRY(query_args(c, s, f, a.q));
    a.q.out_nrm = nullptr;
    return twin_maps(c, s, f, a.tw);
}

static int launch_velocity(VelocityArgs& a, uint32_t points, const void* d_xz, void* d_out_pos, void* d_out_vel, hipStream_t st)
{
    a.q.xz = static_cast<const float2*>(d_xz);
    a.q.out_pos = static_cast<float4*>(d_out_pos);
    a.out_vel = static_cast<float4*>(d_out_vel);
    a.q.points = points;
    hipLaunchKernelGGL(k_query_velocity, dim3((a.q.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

int ocean_query_velocity(ocean_t* c, const ocean_surface* s, const float* xz, uint32_t points, float* out_pos, float* out_vel)
{
    LastFrame f;
    VelocityArgs a{};
    return staged_call(c, velocity_args(c, s, f, a), f, a, launch_velocity, points, xz, 2, out_pos, out_vel, 2);
}

int ocean_query_velocity_device(ocean_t* c, const ocean_surface* s, const void* d_xz, uint32_t points, void* d_out_pos, void* d_out_vel)
{
    LastFrame f;
    VelocityArgs a{};
    return device_call(c, velocity_args(c, s, f, a), f, a, launch_velocity, points, d_xz, d_out_pos, d_out_vel, 2);
}

}  // extern "C"

// ---- spray emitters (include/ocean_consumers.h): the breaking vertices of a window, compacted in lattice order --------------------------------
// Checks and launch arguments: the settings, the surface of the query (iterations and choppy do not matter here), the Jacobian the frame's
// mode left in the maps (as ocean_update_foam takes it), then the twins -- none at all is a set without velocities, some is an error.
static int spray_args(ocean_ctx* c, const ocean_surface* s, const ocean_spray* p, uint32_t capacity, LastFrame& f, SprayArgs& a)
{
    if (!c || !s || !p || p->nx == 0 || p->ny == 0 || (uint64_t)p->nx * p->ny > ((uint64_t)1 << 24) || p->thin_log2 > 16 ||
        !std::isfinite(p->threshold) || !std::isfinite(p->gain) || !std::isfinite(p->min_rise) || p->gain < 0.0f)
        return OCEAN_E_INVALID;
    OCEAN_TRY(forward_args(c, s, f, a.q));
    const int mode = c->set_mode[f.set];            // of the frame that wrote these maps, not of the next one
    if (mode != OCEAN_MODE_FULL7 && mode != OCEAN_MODE_JACOBIAN) return OCEAN_E_UNSUPPORTED;
    a.from_slot = mode == OCEAN_MODE_JACOBIAN;
    for (uint32_t i = 0; i < (uint32_t)OCEAN_MAX_CASCADES; ++i) a.lam[i] = i < s->cascades ? c->set_lambda[f.set][s->first_tile + i] : 0.0f;
    const int twins = twin_maps(c, s, f, a.tw);
    if (twins != OCEAN_OK && twins != OCEAN_E_NOT_READY) return twins;
    a.twinned = twins == OCEAN_OK;
    a.threshold = p->threshold; a.gain = p->gain; a.min_rise = p->min_rise;
    a.thin_mask = (1u << p->thin_log2) - 1u; a.salt = p->salt;
    a.ix0 = p->ix0; a.iy0 = p->iy0; a.half = (int)(s->grid_size / 2);
    a.nx = p->nx; a.points = p->nx * p->ny;
    a.capacity = capacity;
    a.chunks = (a.points + SPRAY_CHUNK - 1u) / SPRAY_CHUNK;
    return OCEAN_OK;
}

// The three launches behind one another on the frame's stream, on the scratch of the compaction (ocean_ctx::spray_scratch; grown below).
static int launch_spray(ocean_ctx* c, SprayArgs& a, void* d_out_pos, void* d_out_vel, void* d_out_index, void* d_out_count, hipStream_t st)
{
    a.masks = static_cast<unsigned long long*>(c->spray_scratch);
    a.counts = reinterpret_cast<unsigned*>(a.masks + (size_t)c->spray_chunks * SPRAY_MASKS);
    a.out_pos = static_cast<float4*>(d_out_pos);
    a.out_vel = static_cast<float4*>(d_out_vel);
    a.out_index = static_cast<unsigned*>(d_out_index);
    a.out_count = static_cast<unsigned*>(d_out_count);
    hipLaunchKernelGGL(k_spray_count, dim3(a.chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_spray_scan, dim3(1), dim3(256), 0, st, a);
    if (a.capacity) hipLaunchKernelGGL(k_spray_scatter, dim3(a.chunks), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

static int grow_spray_scratch(ocean_ctx* c, const SprayArgs& a)
{
    if (a.chunks <= c->spray_chunks) return OCEAN_OK;
    const size_t bytes = (size_t)a.chunks * (SPRAY_MASKS * sizeof(unsigned long long) + sizeof(unsigned));
    return regrow(c, &c->spray_scratch, (void**)nullptr, bytes, c->spray_chunks, a.chunks, [] {});
}

extern "C" {

void ocean_default_spray(ocean_spray* p)
{
    if (!p) return;
    *p = ocean_spray{};
    p->threshold = 0.3f;
    p->gain = 2.5f;
}

int ocean_emit_spray(ocean_t* c, const ocean_surface* s, const ocean_spray* p, uint32_t capacity,
                     float* out_pos, float* out_vel, uint32_t* out_index, uint32_t out_count[2])
{
    LastFrame f;
    SprayArgs a{};
    OCEAN_TRY(spray_args(c, s, p, capacity, f, a));
    if (!out_count || (capacity && (!out_pos || !out_vel || !out_index))) return OCEAN_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(grow_spray_scratch(c, a));
    // [positions | velocities | indices | the two counts]: the float4 arrays first, so that every array is aligned
    const size_t rows16 = (size_t)capacity * sizeof(float4), rows4 = (size_t)capacity * sizeof(uint32_t);
    const size_t bytes = 2 * rows16 + rows4 + 2 * sizeof(uint32_t);
    if (bytes > c->staging_bytes) OCEAN_TRY(regrow(c, &c->staging, (void**)nullptr, bytes, c->staging_bytes, bytes, [] {}));
    char* d_pos = static_cast<char*>(c->staging);
    char* d_vel = d_pos + rows16;
    char* d_index = d_vel + rows16;
    char* d_count = d_index + rows4;
    OCEAN_TRY(consumer_begin(c, f.st));
    OCEAN_TRY(launch_spray(c, a, d_pos, d_vel, d_index, d_count, f.st));
    HIP_TRY(hipMemcpyAsync(out_count, d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, f.st));
    OCEAN_TRY(consumer_end(c, f.st));
    HIP_TRY(hipStreamSynchronize(f.st));
    const size_t written = out_count[1];            // only the rows that were written travel: the caller's later rows keep what they held
    if (written == 0) return OCEAN_OK;
    HIP_TRY(hipMemcpyAsync(out_pos, d_pos, written * sizeof(float4), hipMemcpyDeviceToHost, f.st));
    HIP_TRY(hipMemcpyAsync(out_vel, d_vel, written * sizeof(float4), hipMemcpyDeviceToHost, f.st));
    HIP_TRY(hipMemcpyAsync(out_index, d_index, written * sizeof(uint32_t), hipMemcpyDeviceToHost, f.st));
    HIP_TRY(hipStreamSynchronize(f.st));
    return OCEAN_OK;
}

int ocean_emit_spray_device(ocean_t* c, const ocean_surface* s, const ocean_spray* p, uint32_t capacity,
                            void* d_out_pos, void* d_out_vel, void* d_out_index, void* d_out_count)
{
    LastFrame f;
    SprayArgs a{};
    OCEAN_TRY(spray_args(c, s, p, capacity, f, a));
    if (!d_out_count || (capacity && (!d_out_pos || !d_out_vel || !d_out_index))) return OCEAN_E_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(grow_spray_scratch(c, a));
    OCEAN_TRY(consumer_begin(c, f.st));
    OCEAN_TRY(launch_spray(c, a, d_out_pos, d_out_vel, d_out_index, d_out_count, f.st));
    return consumer_end(c, f.st);
}

}  // extern "C"

// ---- persistent foam (include/ocean_consumers.h) -----------------------------------------------------------------------------------------
// Both buffers or none (as alloc_jacobian): zero-filled on the stream of the update that asked for them.
static int alloc_foam(ocean_ctx* c, hipStream_t st)
{
    if (c->foam[1]) return OCEAN_OK;               // the second of the two: complete
    const size_t bytes = (size_t)c->tiles * c->n * c->n * sizeof(float);
    for (int k = 0; k < 2; ++k) {
        if (c->foam[k]) { (void)hipFree(c->foam[k]); c->foam[k] = nullptr; }       // leftovers of an earlier failed attempt
        if (hipMalloc(&c->foam[k], bytes) != hipSuccess || hipMemsetAsync(c->foam[k], 0, bytes, st) != hipSuccess) {
            for (int j = 0; j <= k; ++j) if (c->foam[j]) { (void)hipFree(c->foam[j]); c->foam[j] = nullptr; }
            g_last_hip = (int)hipGetLastError();
            return OCEAN_E_NOMEM;
        }
    }
    c->foam_cur = 0; c->foam_ready = false;
    return OCEAN_OK;
}

// Rows per band of k_foam_update's row walk: as long as the launch still has four waves for every compute unit (a band re-reads two rows of F).
static unsigned foam_band_rows(const ocean_ctx* c, uint32_t tiles)
{
    const double waves_per_row = (double)tiles * c->n * c->n / 256.0;
    unsigned rows = 32;
    while (rows > 4 && waves_per_row / rows < 4.0 * (c->cu_count > 0 ? c->cu_count : 256)) rows /= 2;
    return rows < c->n ? rows : c->n;
}

extern "C" {

void ocean_default_foam(ocean_foam* f)
{
    if (!f) return;
    f->threshold = 0.6f;
    f->gain = 2.5f;
    f->lifetime = 4.0f;
    f->spread = 0.25f;
    f->cutoff = 1.0f / 1024.0f;
}

int ocean_update_foam(ocean_t* c, uint32_t tile, const ocean_foam* f, float dt)
{
    if (!c || !f) return OCEAN_E_INVALID;
    if (tile != OCEAN_ALL_TILES && tile >= c->tiles) return OCEAN_E_INVALID;
    if (!std::isfinite(f->threshold) || !std::isfinite(f->gain) || !std::isfinite(f->lifetime) || !std::isfinite(f->spread) || !std::isfinite(f->cutoff) ||
        !std::isfinite(dt))
        return OCEAN_E_INVALID;
    if (!(f->lifetime > 0.0f) || f->spread < 0.0f || f->spread > 1.0f || f->cutoff < 0.0f || f->cutoff > 1.0f || dt < 0.0f) return OCEAN_E_INVALID;
    const uint32_t first = tile == OCEAN_ALL_TILES ? 0u : tile, count = tile == OCEAN_ALL_TILES ? c->tiles : 1u;
    LastFrame fr;
    OCEAN_TRY(last_frame(c, first, fr));
    const int set = fr.set;
    const int mode = c->set_mode[set];              // of the frame that wrote these maps, not of the next one
    if (mode != OCEAN_MODE_FULL7 && mode != OCEAN_MODE_JACOBIAN) return OCEAN_E_UNSUPPORTED;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n2 = fr.n2;
    FoamArgs a;
    a.lambda = nullptr;
    a.lambda_all = c->set_lambda[set][first];
    if (mode == OCEAN_MODE_FULL7) {
        bool uniform = true;
        for (uint32_t i = first + 1; i < first + count && uniform; ++i) uniform = c->set_lambda[set][i] == a.lambda_all;
        if (!uniform) {         // per-tile lambdas: the device copy is replaced only when they change, and then nothing in flight may still read it
            if (c->foam_lambda_host != c->set_lambda[set]) {
                OCEAN_TRY(sync_all(c));
                if (!c->foam_lambda) HIP_TRY(hipMalloc(&c->foam_lambda, c->tiles * sizeof(float)));
                HIP_TRY(hipMemcpy(c->foam_lambda, c->set_lambda[set].data(), c->tiles * sizeof(float), hipMemcpyHostToDevice));
                c->foam_lambda_host = c->set_lambda[set];
            }
            a.lambda = c->foam_lambda + first;
        }
    }
    hipStream_t st = fr.st;
    OCEAN_TRY(consumer_begin(c, st));
    OCEAN_TRY(alloc_foam(c, st));
    const float* src = c->foam[c->foam_cur];
    float* dst = c->foam[c->foam_cur ^ 1];
    a.map = mode == OCEAN_MODE_JACOBIAN ? fr.disp : fr.nrm;
    a.src = src + first * n2;
    a.dst = dst + first * n2;
    a.tile_texels = n2;
    a.threshold = f->threshold; a.gain = f->gain; a.spread = f->spread; a.cutoff = f->cutoff;
    a.decay = (float)std::exp(-(double)dt / (double)f->lifetime);
    a.n = (int)c->n;
    a.log2_groups = 0;
    while ((4u << a.log2_groups) < c->n) ++a.log2_groups;
    a.rows = (int)foam_band_rows(c, count);
    const dim3 grid(foam_blocks(c->n, (unsigned)a.rows), count);
    if (mode == OCEAN_MODE_JACOBIAN) hipLaunchKernelGGL(k_foam_update<FOAM_FROM_JACOBIAN>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_foam_update<FOAM_FROM_NORMALS>, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    // the tiles that were not selected keep their state in the buffer that is current from now on
    if (first > 0) HIP_TRY(hipMemcpyAsync(dst, src, first * n2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (first + count < c->tiles)
        HIP_TRY(hipMemcpyAsync(dst + (first + count) * n2, src + (first + count) * n2, (c->tiles - first - count) * n2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    OCEAN_TRY(consumer_end(c, st));
    c->foam_cur ^= 1;
    c->foam_ready = true;
    return OCEAN_OK;
}

int ocean_reset_foam(ocean_t* c)
{
    if (!c) return OCEAN_E_INVALID;
    if (!c->foam[1]) return OCEAN_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, c->last_set);
    OCEAN_TRY(consumer_begin(c, st));
    HIP_TRY(hipMemsetAsync(c->foam[c->foam_cur], 0, (size_t)c->tiles * c->n * c->n * sizeof(float), st));
    return consumer_end(c, st);
}

int ocean_read_foam(ocean_t* c, uint32_t tile, float* out)
{
    if (!c || !out || tile >= c->tiles) return OCEAN_E_INVALID;
    if (!c->foam_ready) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    const size_t n2 = (size_t)c->n * c->n;
    HIP_TRY(hipMemcpy(out, c->foam[c->foam_cur] + tile * n2, n2 * sizeof(float), hipMemcpyDeviceToHost));
    return OCEAN_OK;
}

int ocean_device_foam(ocean_t* c, void** d_foam)
{
    if (!c || !d_foam) return OCEAN_E_INVALID;
    *d_foam = c->foam_ready ? c->foam[c->foam_cur] : nullptr;
    return OCEAN_OK;
}

int ocean_query_foam(ocean_t* c, const ocean_surface* s, const float* xz, uint32_t points, float* out)
{
    LastFrame f;
    FoamQueryArgs a{};
    return staged_call(c, foam_query_args(c, s, f, a), f, a, launch_foam_query, points, xz, 2, out, nullptr, 1);
}

int ocean_query_foam_device(ocean_t* c, const ocean_surface* s, const void* d_xz, uint32_t points, void* d_out)
{
    LastFrame f;
    FoamQueryArgs a{};
    return device_call(c, foam_query_args(c, s, f, a), f, a, launch_foam_query, points, d_xz, d_out, nullptr, 1);
}

}  // extern "C"

// ---- buoyancy (include/ocean_consumers.h) --------------------------------------------------------------------------------------------------
// ... of the buoyancy call: the parameters, the surface of the query, then the hull.
template <bool FLOW>
static int buoyancy_args(ocean_ctx* c, const ocean_surface* s, const ocean_buoyancy* p, LastFrame& f, BuoyancyArgs& a)
{
    if (!c || !s || !p || !std::isfinite(p->density) || !std::isfinite(p->gravity) || !std::isfinite(p->drag) ||
        p->density < 0.0f || p->gravity < 0.0f || p->drag < 0.0f)
        return OCEAN_E_INVALID;
    OCEAN_TRY(query_args(c, s, f, a.q));
    if (!c->hull) return OCEAN_E_NOT_READY;
    a.hull = c->hull;
    a.hull_points = c->hull_points;
    a.weight = p->density * p->gravity;
    a.drag = p->drag;
    if (FLOW) OCEAN_TRY(twin_maps(c, s, f, a.tw));      // (the flow form: the drag is against the twins' velocity)
    return OCEAN_OK;
}

template <bool FLOW>
static int launch_buoyancy(BuoyancyArgs& a, uint32_t count, const void* d_bodies, void* d_out_force, void* d_out_torque, hipStream_t st)
{
    a.bodies = static_cast<const float*>(d_bodies);
    a.out_force = static_cast<float4*>(d_out_force);
    a.out_torque = static_cast<float4*>(d_out_torque);
    a.count = count;
    const unsigned per_block = BUOYANCY_BODIES_PER_BLOCK;
    hipLaunchKernelGGL(k_buoyancy_bodies<FLOW>, dim3((unsigned)(((uint64_t)a.count + per_block - 1u) / per_block)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

void ocean_default_buoyancy(ocean_buoyancy* b)
{
    if (!b) return;
    b->density = 1025.0f;
    b->gravity = 9.81f;
    b->drag = 1000.0f;
}

int ocean_set_hull(ocean_t* c, const float* points, uint32_t count)
{
    static_assert(sizeof(ocean_body) == 64, "a body is 16 words");
    if (!c || (count && !points)) return OCEAN_E_INVALID;
    for (size_t i = 0; i < (size_t)count; ++i) {
        const float* p = points + 4 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]) || !(p[3] > 0.0f)) return OCEAN_E_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    // the new buffer is complete before the old one goes: a failure leaves the old hull
    float4* fresh = nullptr;
    if (count) {
        const size_t bytes = (size_t)count * sizeof(float4), guard = OCEAN_HULL_GUARD * sizeof(float4);
        HIP_TRY(hipMalloc(&fresh, bytes + guard));
        hipError_t e = hipMemcpy(fresh, points, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(fresh + count, 0xff, guard);        // all bits set: NaN in every word
        if (e != hipSuccess) { (void)hipFree(fresh); HIP_TRY(e); }
    }
    const int rc = c->hull ? sync_all(c) : OCEAN_OK;      // nothing in flight may still read the old one
    if (rc) { if (fresh) (void)hipFree(fresh); return rc; }
    free_and_null(c->hull);
    c->hull = fresh;
    c->hull_points = count;
    return OCEAN_OK;
}

}  // extern "C"

// Both forms of the host call: the bodies' ranges are checked against the hull before anything is launched.
template <bool FLOW>
static int buoyancy_host(ocean_ctx* c, const ocean_surface* s, const ocean_buoyancy* b, const ocean_body* bodies, uint32_t count,
                         float* out_force, float* out_torque)
{
    LastFrame f;
    BuoyancyArgs a{};
    const int rc = buoyancy_args<FLOW>(c, s, b, f, a);
    if (rc == OCEAN_OK && bodies)       // (a NULL array is staged_call's to report)
        for (uint32_t i = 0; i < count; ++i)
            if ((uint64_t)bodies[i].first_point + bodies[i].points > a.hull_points) return OCEAN_E_INVALID;
    return staged_call(c, rc, f, a, launch_buoyancy<FLOW>, count, reinterpret_cast<const float*>(bodies), 16, out_force, out_torque, 2);
}

template <bool FLOW>
static int buoyancy_device(ocean_ctx* c, const ocean_surface* s, const ocean_buoyancy* b, const void* d_bodies, uint32_t count,
                           void* d_out_force, void* d_out_torque)
{
    LastFrame f;
    BuoyancyArgs a{};
    return device_call(c, buoyancy_args<FLOW>(c, s, b, f, a), f, a, launch_buoyancy<FLOW>, count, d_bodies, d_out_force, d_out_torque, 2);
}

extern "C" {

int ocean_buoyancy_bodies(ocean_t* c, const ocean_surface* s, const ocean_buoyancy* b, const ocean_body* bodies, uint32_t count,
                          float* out_force, float* out_torque)
{
    return buoyancy_host<false>(c, s, b, bodies, count, out_force, out_torque);
}

int ocean_buoyancy_bodies_device(ocean_t* c, const ocean_surface* s, const ocean_buoyancy* b, const void* d_bodies, uint32_t count,
                                 void* d_out_force, void* d_out_torque)
{
    return buoyancy_device<false>(c, s, b, d_bodies, count, d_out_force, d_out_torque);
}

int ocean_buoyancy_bodies_flow(ocean_t* c, const ocean_surface* s, const ocean_buoyancy* b, const ocean_body* bodies, uint32_t count,
                               float* out_force, float* out_torque)
{
    return buoyancy_host<true>(c, s, b, bodies, count, out_force, out_torque);
}

int ocean_buoyancy_bodies_flow_device(ocean_t* c, const ocean_surface* s, const ocean_buoyancy* b, const void* d_bodies, uint32_t count,
                                      void* d_out_force, void* d_out_torque)
{
    return buoyancy_device<true>(c, s, b, d_bodies, count, d_out_force, d_out_torque);
}

}  // extern "C"

// ---- Gerstner proxy (include/ocean_consumers.h): a tile's strongest waves as rows, their analytic evaluation and its Newton inverse ---------
// Scratch of the selection, in 32-bit words: the digit counts and the candidates' count, the select counter, then the survivors as
// (power bits, bin) pairs and, behind them, the sorted bins k_wave_rows reads.
constexpr size_t WAVE_HIST = 0, WAVE_COUNTER = 257, WAVE_LIST = 260, WAVE_BINS = WAVE_LIST + 2 * WAVES_MAX, WAVE_SCRATCH_WORDS = WAVE_BINS + WAVES_MAX;

static int alloc_waves(ocean_ctx* c)
{
    if (!c->waves) HIP_TRY(hipMalloc(&c->waves, (size_t)c->tiles * WAVES_MAX * sizeof(ocean_wave)));
    if (!c->wave_anim) HIP_TRY(hipMalloc(&c->wave_anim, (size_t)OCEAN_MAX_CASCADES * WAVES_MAX * WAVES_ANIM_VEC * sizeof(float4)));
    if (!c->wave_scratch) HIP_TRY(hipMalloc(&c->wave_scratch, WAVE_SCRATCH_WORDS * sizeof(unsigned)));
    if (c->wave_count.size() != c->tiles) c->wave_count.assign(c->tiles, 0u);
    if (c->wave_length.size() != c->tiles) c->wave_length.assign(c->tiles, 0.0f);
    return OCEAN_OK;
}

static bool wave_set_exists(const ocean_ctx* c, uint32_t tile) { return tile < c->wave_count.size() && c->wave_count[tile] != 0; }

// Checks and launch arguments of the two evaluations: the surface as the map query checks it, a finite time, Prepare, a set for every cascade.
static int wave_eval_args(ocean_ctx* c, const ocean_surface* s, float t, bool inverse, LastFrame& f, WaveEvalArgs& a)
{
    if (!c || !s || s->cascades == 0 || s->cascades > (uint32_t)OCEAN_MAX_CASCADES || s->first_tile >= c->tiles ||
        s->cascades > c->tiles - s->first_tile || s->grid_size == 0 || s->iterations > 32 || !std::isfinite(t))
        return OCEAN_E_INVALID;
    if (!c->prepared) return OCEAN_E_NOT_READY;
    for (uint32_t i = 0; i < s->cascades; ++i)
        if (!wave_set_exists(c, s->first_tile + i)) return OCEAN_E_NOT_READY;
    no_frame(c, f);
    a.set.rows = c->waves + (size_t)s->first_tile * WAVES_MAX;
    a.set.anim = c->wave_anim;
    a.cascades = (int)s->cascades;
    a.iterations = inverse ? (s->iterations ? (int)s->iterations : 8) : 0;
    a.fn = (float)c->n; a.inv_n = 1.0f / (float)c->n;
    a.grid = (float)s->grid_size;
    a.half = (float)(s->grid_size / 2);
    a.vertex_distance = s->vertex_distance;
    a.choppy = s->choppy;
    for (uint32_t i = 0; i < (uint32_t)OCEAN_MAX_CASCADES; ++i) {
        a.set.count[i] = 0; a.set.tt[i] = 0.0f;
        a.uv_scale[i] = 0.0f; a.lam[i] = 0.0f; a.gain[i] = 0.0f;
        if (i >= s->cascades) continue;
        const uint32_t tile = s->first_tile + i, e = effective_tile(c, tile);
        a.set.count[i] = c->wave_count[tile];
        a.set.tt[i] = t + (c->use_toff ? c->toff_host[e] : 0.0f);       // as the frames: a.t + toff[tile], one fp32 addition
        a.uv_scale[i] = s->uv_scales[i];
        a.lam[i] = c->params[e].lambda;
        a.gain[i] = a.lam[i] * (s->uv_scales[i] * c->wave_length[tile] / (a.grid * s->vertex_distance));
    }
    return OCEAN_OK;
}

template <bool INVERSE>
static int launch_waves(WaveEvalArgs& a, uint32_t points, const void* d_xz, void* d_out_pos, void* d_out_nrm, hipStream_t st)
{
    a.xz = static_cast<const float2*>(d_xz);
    a.out_pos = static_cast<float4*>(d_out_pos);
    a.out_nrm = static_cast<float4*>(d_out_nrm);
    a.points = points;
    hipLaunchKernelGGL(k_waves_animate, dim3(WAVES_MAX / 256u, (unsigned)a.cascades), dim3(256), 0, st, a.set);
    if (INVERSE) hipLaunchKernelGGL(k_waves_query, dim3((a.points + 255u) / 256u), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_waves_eval, dim3((a.points + 255u) / 256u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

int ocean_extract_waves(ocean_t* c, uint32_t tile, uint32_t max_waves, ocean_wave* out, uint32_t* out_count, double* out_energy)
{
    if (!c || !out_count || tile >= c->tiles || max_waves == 0 || max_waves > WAVES_MAX) return OCEAN_E_INVALID;
    if (!c->prepared) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    OCEAN_TRY(alloc_waves(c));
    const unsigned n = c->n, log2n = log2_of(n);
    const size_t n2 = (size_t)n * n;
    const float2* h0 = c->h0 + tile * n2;
    hipStream_t st = stream_of(c, 0);
    const unsigned blocks = (unsigned)std::min<size_t>((n2 + 2047) / 2048, 2048);
    unsigned* hist = c->wave_scratch + WAVE_HIST;
    unsigned* counter = c->wave_scratch + WAVE_COUNTER;
    // the K-th largest key, digit by digit from the top; `remaining` is its rank among the keys that share the digits found so far
    unsigned long long threshold = 0;
    uint32_t count = 0, remaining = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        unsigned h[257];
        HIP_TRY(hipMemsetAsync(hist, 0, 258 * sizeof(unsigned), st));
        hipLaunchKernelGGL(k_wave_hist, dim3(blocks), dim3(256), 0, st, h0, n, log2n, threshold, shift, hist);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (shift == 56) {
            count = std::min<uint32_t>(max_waves, h[256]);
            remaining = count;
            if (count == 0) break;
        }
        unsigned digit = 255, above = 0;
        while (above + h[digit] < remaining) { above += h[digit]; if (digit == 0) return OCEAN_E_HIP; --digit; }
        remaining -= above;
        threshold |= (unsigned long long)digit << shift;
        if (h[digit] == remaining) break;           // the whole bucket is taken: the digits below do not matter
        if (shift == 0) return OCEAN_E_HIP;         // (distinct keys: the last digit's bucket holds one key)
    }
    std::vector<ocean_wave> rows(count);
    if (count) {
        uint2* list = reinterpret_cast<uint2*>(c->wave_scratch + WAVE_LIST);
        unsigned* bins = c->wave_scratch + WAVE_BINS;
        unsigned taken = 0;
        hipLaunchKernelGGL(k_wave_select, dim3(blocks), dim3(256), 0, st, h0, n, log2n, threshold, WAVES_MAX, counter, list);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&taken, counter, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (taken != count) return OCEAN_E_HIP;
        std::vector<uint2> pairs(count);
        HIP_TRY(hipMemcpy(pairs.data(), list, count * sizeof(uint2), hipMemcpyDeviceToHost));
        std::sort(pairs.begin(), pairs.end(), [](const uint2& x, const uint2& y) { return x.x != y.x ? x.x > y.x : x.y < y.y; });   // power descending, bin ascending
        std::vector<unsigned> order(count);
        for (uint32_t j = 0; j < count; ++j) order[j] = pairs[j].y;
        HIP_TRY(hipMemcpyAsync(bins, order.data(), count * sizeof(unsigned), hipMemcpyHostToDevice, st));
        ocean_wave* set = c->waves + (size_t)tile * WAVES_MAX;
        c->wave_count[tile] = 0;                    // from here on the old rows are being overwritten: a failure below leaves no set, not a mixed one
        hipLaunchKernelGGL(k_wave_rows, dim3((count + 255u) / 256u), dim3(256), 0, st, h0, c->omega + tile * n2, c->k1d + (size_t)tile * n, n,
                           bins, count, set);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rows.data(), set, count * sizeof(ocean_wave), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    c->wave_count[tile] = count;                    // (no candidate: no set)
    c->wave_length[tile] = c->prep_length[tile];
    *out_count = count;
    double energy = 0.0;
    for (uint32_t j = 0; j < count; ++j) {
        if (out) out[j] = rows[j];
        energy += (double)rows[j].re * (double)rows[j].re + (double)rows[j].im * (double)rows[j].im;
    }
    if (out_energy) *out_energy = energy;
    return OCEAN_OK;
}

int ocean_set_waves(ocean_t* c, uint32_t tile, const ocean_wave* rows, uint32_t count)
{
    if (!c || tile >= c->tiles || count > WAVES_MAX || (count && !rows)) return OCEAN_E_INVALID;
    if (!c->prepared) return OCEAN_E_NOT_READY;
    const int half = (int)(c->n / 2);
    for (uint32_t j = 0; j < count; ++j) {
        const ocean_wave& w = rows[j];
        for (float v : {w.kx, w.kz, w.ux, w.uz, w.re, w.im, w.omega})
            if (!std::isfinite(v)) return OCEAN_E_INVALID;
        if (w.jx < -half || w.jx >= half || w.jz < -half || w.jz >= half) return OCEAN_E_INVALID;
    }
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));                        // nothing in flight may still read the set that is replaced
    OCEAN_TRY(alloc_waves(c));
    c->wave_count[tile] = 0;                       // (a copy that fails leaves no set, not a mixed one)
    if (count) HIP_TRY(hipMemcpy(c->waves + (size_t)tile * WAVES_MAX, rows, count * sizeof(ocean_wave), hipMemcpyHostToDevice));
    c->wave_count[tile] = count;
    c->wave_length[tile] = c->prep_length[tile];
    return OCEAN_OK;
}

int ocean_get_waves(ocean_t* c, uint32_t tile, ocean_wave* rows, uint32_t* count)
{
    if (!c || !count || tile >= c->tiles) return OCEAN_E_INVALID;
    if (!wave_set_exists(c, tile)) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    if (rows) HIP_TRY(hipMemcpy(rows, c->waves + (size_t)tile * WAVES_MAX, c->wave_count[tile] * sizeof(ocean_wave), hipMemcpyDeviceToHost));
    *count = c->wave_count[tile];
    return OCEAN_OK;
}

int ocean_eval_waves(ocean_t* c, const ocean_surface* s, float t, const float* xz, uint32_t points, float* out_pos, float* out_nrm)
{
    LastFrame f;
    WaveEvalArgs a;
    return staged_call(c, wave_eval_args(c, s, t, false, f, a), f, a, launch_waves<false>, points, xz, 2, out_pos, out_nrm, 2);
}

int ocean_eval_waves_device(ocean_t* c, const ocean_surface* s, float t, const void* d_xz, uint32_t points, void* d_out_pos, void* d_out_nrm)
{
    LastFrame f;
    WaveEvalArgs a;
    return device_call(c, wave_eval_args(c, s, t, false, f, a), f, a, launch_waves<false>, points, d_xz, d_out_pos, d_out_nrm, 2);
}

int ocean_query_waves(ocean_t* c, const ocean_surface* s, float t, const float* xz, uint32_t points, float* out_pos, float* out_nrm)
{
    LastFrame f;
    WaveEvalArgs a;
    return staged_call(c, wave_eval_args(c, s, t, true, f, a), f, a, launch_waves<true>, points, xz, 2, out_pos, out_nrm, 2);
}

int ocean_query_waves_device(ocean_t* c, const ocean_surface* s, float t, const void* d_xz, uint32_t points, void* d_out_pos, void* d_out_nrm)
{
    LastFrame f;
    WaveEvalArgs a;
    return device_call(c, wave_eval_args(c, s, t, true, f, a), f, a, launch_waves<true>, points, d_xz, d_out_pos, d_out_nrm, 2);
}

}  // extern "C"

// ---- fragment stage (include/ocean_consumers.h): Preetham sky, the reference's seabed and water colour ---------------------------------------
static bool all_finite(const float* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// SkyPreetham::Update in double: the normalised sun and A, B, C, D, E, ZenithLum, ZeroThetaSun per channel of Yxy.
static int sky_double(const ocean_sky* s, double sun[3], double co[7][3])
{
    if (!s || !all_finite(s->sun_dir, 3) || !all_finite(s->sun_color, 3) || !std::isfinite(s->turbidity) || !std::isfinite(s->sun_intensity))
        return OCEAN_E_INVALID;
    const double x = s->sun_dir[0], y = s->sun_dir[1], z = s->sun_dir[2], len = std::sqrt(x * x + y * y + z * z);
    if (!(len > 0.0) || !(s->turbidity >= 1.0f && s->turbidity <= 10.0f)) return OCEAN_E_INVALID;
    sun[0] = x / len; sun[1] = y / len; sun[2] = z / len;
    const double t = s->turbidity, th = std::acos(std::max(sun[1], 0.0));
    const double A[3] = {0.1787 * t - 1.4630, -0.0193 * t - 0.2592, -0.0167 * t - 0.2608};
    const double B[3] = {-0.3554 * t + 0.4275, -0.0665 * t + 0.0008, -0.0950 * t + 0.0092};
    const double C[3] = {-0.0227 * t + 5.3251, -0.0004 * t + 0.2125, -0.0079 * t + 0.2102};
    const double D[3] = {0.1206 * t - 2.5771, -0.0641 * t - 0.8989, -0.0441 * t - 1.6537};
    const double E[3] = {-0.0670 * t + 0.3703, -0.0033 * t + 0.0452, -0.0109 * t + 0.0529};
    const double pi = 3.14159265358979323846;
    const double chi = (4.0 / 9.0 - t / 120.0) * (pi - 2.0 * th);
    const double th2 = th * th, th3 = th2 * th, t2 = t * t;
    const double zen[3] = {
        (4.0453 * t - 4.9710) * std::tan(chi) - 0.2155 * t + 2.4192,
        (0.00165 * th3 - 0.00375 * th2 + 0.00209 * th) * t2 + (-0.02903 * th3 + 0.06377 * th2 - 0.03202 * th + 0.00394) * t +
            (0.11693 * th3 - 0.21196 * th2 + 0.06052 * th + 0.25886),
        (0.00275 * th3 - 0.00610 * th2 + 0.00317 * th) * t2 + (-0.04214 * th3 + 0.08970 * th2 - 0.04153 * th + 0.00516) * t +
            (0.15346 * th3 - 0.26756 * th2 + 0.06670 * th + 0.26688)};
    const double cs = std::cos(th);
    for (int k = 0; k < 3; ++k) {
        co[0][k] = A[k]; co[1][k] = B[k]; co[2][k] = C[k]; co[3][k] = D[k]; co[4][k] = E[k];
        co[5][k] = zen[k];
        co[6][k] = (1.0 + A[k] * std::exp(B[k] / 1.0)) * (1.0 + C[k] * std::exp(D[k] * th) + E[k] * cs * cs);
    }
    return OCEAN_OK;
}

// What the kernels read of a sky: the fp32 outputs of ocean_sky_coefficients (what a UBO would carry), with ZenithLum / ZeroThetaSun formed
// from them in double and rounded once.
static int sky_dev(const ocean_sky* s, SkyDev& d)
{
    ocean_sky_coeffs k;
    OCEAN_TRY(ocean_sky_coefficients(s, &k));
    for (int i = 0; i < 3; ++i) {
        d.sun[i] = k.sun_dir[i];
        d.A[i] = k.A[i]; d.B[i] = k.B[i]; d.C[i] = k.C[i]; d.D[i] = k.D[i]; d.E[i] = k.E[i];
        d.zn[i] = (float)((double)k.zenith_lum[i] / (double)k.zero_theta_sun[i]);
        d.sun_color[i] = s->sun_color[i];
    }
    d.sun_intensity = s->sun_intensity;
    return OCEAN_OK;
}

static unsigned point_blocks(uint32_t count)
{
    return std::min<unsigned>((count + 255u) / 256u, 2048u);      // eight workgroups per compute unit; the kernels stride over the rest
}

static int sky_args(ocean_ctx* c, const ocean_sky* s, LastFrame& f, SkyArgs& a)
{
    if (!c) return OCEAN_E_INVALID;
    OCEAN_TRY(sky_dev(s, a.sky));
    no_frame(c, f);
    return OCEAN_OK;
}

static int launch_sky(SkyArgs& a, uint32_t count, const void* d_dirs, void* d_out, void*, hipStream_t st)
{
    a.dirs = static_cast<const float*>(d_dirs);
    a.out = static_cast<float4*>(d_out);
    a.count = count;
    hipLaunchKernelGGL(k_sky_radiance, dim3(point_blocks(count)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

static int seabed_args(ocean_ctx* c, LastFrame& f, SeabedArgs& a)
{
    if (!c) return OCEAN_E_INVALID;
    no_frame(c, f);
    return OCEAN_OK;
}

static int launch_seabed(SeabedArgs& a, uint32_t count, const void* d_xz, void* d_out, void*, hipStream_t st)
{
    a.xz = static_cast<const float2*>(d_xz);
    a.out = static_cast<float4*>(d_out);
    a.count = count;
    hipLaunchKernelGGL(k_eval_seabed, dim3(point_blocks(count)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

// Validation of a sky and a water, and everything of the shading kernel's arguments that is uniform over the launch.
static int shade_args(ocean_ctx* c, const ocean_sky* s, const ocean_water* w, ShadeArgs& a)
{
    if (!c || !w) return OCEAN_E_INVALID;
    OCEAN_TRY(sky_dev(s, a.sky));
    if (!all_finite(w->cam_pos, 3) || !std::isfinite(w->height) || !all_finite(w->absorb, 3) || !all_finite(w->scatter, 3) ||
        !all_finite(w->backscatter, 3) || !all_finite(w->terrain_color, 3) || !std::isfinite(w->sky_intensity) ||
        !std::isfinite(w->specular_intensity) || !std::isfinite(w->specular_highlights) || !std::isfinite(w->seabed_factor))
        return OCEAN_E_INVALID;
    if (!(w->specular_highlights > 0.0f) || w->fresnel > (uint32_t)OCEAN_FRESNEL_PHYSICAL || w->seabed > (uint32_t)OCEAN_SEABED_FLAT) return OCEAN_E_INVALID;
    for (int k = 0; k < 3; ++k) {
        if (!(w->absorb[k] > 0.0f)) return OCEAN_E_INVALID;
        a.cam[k] = w->cam_pos[k];
        a.absorb01[k] = (float)((double)w->absorb[k] * 0.1);
        a.scatter01[k] = (float)((double)w->scatter[k] * 0.1);
        a.df0[k] = (float)((0.33 * (double)w->backscatter[k]) / (double)w->absorb[k]);
        a.terrain[k] = w->terrain_color[k];
    }
    a.height = w->height;
    a.sky_intensity = w->sky_intensity; a.specular_intensity = w->specular_intensity; a.highlights = w->specular_highlights;
    a.seabed_factor = w->seabed_factor;
    const double at0 = (1.33477 - 1.0) / (1.33477 + 1.0);
    a.f0 = (float)(at0 * at0);
    a.physical_fresnel = w->fresnel == (uint32_t)OCEAN_FRESNEL_PHYSICAL;
    a.foam_white = w->foam_white != 0; a.tonemap = w->tonemap != 0;
    return OCEAN_OK;
}

static int launch_shade(ShadeArgs& a, bool reference_seabed, uint32_t count, const void* d_pos, const void* d_nrm,
                        void* d_rgba, void* d_aux, hipStream_t st)
{
    a.pos = static_cast<const float4*>(d_pos);
    a.nrm = static_cast<const float4*>(d_nrm);
    a.out_rgba = static_cast<float4*>(d_rgba);
    a.out_aux = static_cast<float4*>(d_aux);
    a.count = count;
    if (reference_seabed) hipLaunchKernelGGL(k_shade_points<true>, dim3(point_blocks(count)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_shade_points<false>, dim3(point_blocks(count)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return OCEAN_OK;
}

extern "C" {

void ocean_default_sky(ocean_sky* s)
{
    if (!s) return;
    s->sun_dir[0] = 0.0f; s->sun_dir[1] = 0.5f; s->sun_dir[2] = 0.866f;      // WaterSurface.h:119
    s->turbidity = 2.5f;                                                      // SkyPreetham.h:15
    s->sun_color[0] = s->sun_color[1] = s->sun_color[2] = 1.0f;               // SkyModel.h:26-27
    s->sun_intensity = 1.0f;
}

void ocean_default_water(ocean_water* w)
{
    if (!w) return;
    const double absorb[3] = {0.420, 0.063, 0.019}, nm[3] = {680.0, 550.0, 440.0}, terrain[3] = {0.964, 1.0, 0.824};   // WaterSurfaceMesh.h:260-275,303,339,362-383
    w->cam_pos[0] = 0.0f; w->cam_pos[1] = 60.0f; w->cam_pos[2] = 0.0f;
    w->height = 50.0f;
    for (int k = 0; k < 3; ++k) {
        w->absorb[k] = (float)absorb[k];
        w->scatter[k] = (float)(0.037 * ((-0.00113 * nm[k] + 1.62517) / (-0.00113 * 514.0 + 1.62517)));
        w->backscatter[k] = (float)(0.01829 * (double)w->scatter[k] + 0.00006);
        w->terrain_color[k] = (float)terrain[k];
    }
    w->sky_intensity = 1.0f; w->specular_intensity = 1.0f; w->specular_highlights = 32.0f;
    w->fresnel = OCEAN_FRESNEL_REFERENCE; w->seabed = OCEAN_SEABED_REFERENCE;
    w->seabed_factor = 0.75f;
    w->foam_white = 1; w->tonemap = 1;
}

int ocean_sky_coefficients(const ocean_sky* s, ocean_sky_coeffs* out)
{
    if (!out) return OCEAN_E_INVALID;
    double sun[3], co[7][3];
    OCEAN_TRY(sky_double(s, sun, co));
    float* rows[7] = {out->A, out->B, out->C, out->D, out->E, out->zenith_lum, out->zero_theta_sun};
    for (int k = 0; k < 3; ++k) out->sun_dir[k] = (float)sun[k];
    out->turbidity = s->turbidity;
    for (int r = 0; r < 7; ++r) {
        for (int k = 0; k < 3; ++k) rows[r][k] = (float)co[r][k];
        rows[r][3] = 0.0f;
    }
    return OCEAN_OK;
}

int ocean_sky_radiance(ocean_t* c, const ocean_sky* s, const float* dirs, uint32_t count, float* out)
{
    LastFrame f;
    SkyArgs a;
    return staged_call(c, sky_args(c, s, f, a), f, a, launch_sky, count, dirs, 3, out, nullptr, 1);
}

int ocean_sky_radiance_device(ocean_t* c, const ocean_sky* s, const void* d_dirs, uint32_t count, void* d_out)
{
    LastFrame f;
    SkyArgs a;
    return device_call(c, sky_args(c, s, f, a), f, a, launch_sky, count, d_dirs, d_out, nullptr, 1);
}

int ocean_eval_seabed(ocean_t* c, const float* xz, uint32_t count, float* out)
{
    LastFrame f;
    SeabedArgs a;
    return staged_call(c, seabed_args(c, f, a), f, a, launch_seabed, count, xz, 2, out, nullptr, 1);
}

int ocean_eval_seabed_device(ocean_t* c, const void* d_xz, uint32_t count, void* d_out)
{
    LastFrame f;
    SeabedArgs a;
    return device_call(c, seabed_args(c, f, a), f, a, launch_seabed, count, d_xz, d_out, nullptr, 1);
}

int ocean_shade_points_device(ocean_t* c, const ocean_sky* s, const ocean_water* w, const void* d_pos, const void* d_nrm, uint32_t count,
                              void* d_out_rgba, void* d_out_aux)
{
    ShadeArgs a;
    OCEAN_TRY(call_checks(c, shade_args(c, s, w, a), count, !d_pos || !d_nrm || !d_out_rgba));
    if (count == 0) return OCEAN_OK;
    LastFrame f;
    no_frame(c, f);
    OCEAN_TRY(consumer_begin(c, f.st));
    OCEAN_TRY(launch_shade(a, w->seabed == (uint32_t)OCEAN_SEABED_REFERENCE, count, d_pos, d_nrm, d_out_rgba, d_out_aux, f.st));
    return consumer_end(c, f.st);
}

// The host form stages [rgba | aux | pos | nrm], float4 rows all, in the context's buffer (the aux rows also where the caller wants none:
// the layout does not depend on it).
int ocean_shade_points(ocean_t* c, const ocean_sky* s, const ocean_water* w, const float* pos, const float* nrm, uint32_t count,
                       float* out_rgba, float* out_aux)
{
    ShadeArgs a;
    OCEAN_TRY(call_checks(c, shade_args(c, s, w, a), count, !pos || !nrm || !out_rgba));
    if (count == 0) return OCEAN_OK;
    LastFrame f;
    no_frame(c, f);
    const size_t rows = (size_t)count * sizeof(float4), bytes = 4 * rows;
    if (bytes > c->staging_bytes) OCEAN_TRY(regrow(c, &c->staging, (void**)nullptr, bytes, c->staging_bytes, bytes, [] {}));
    char* d_rgba = static_cast<char*>(c->staging);
    char* d_aux = d_rgba + rows;
    char* d_pos = d_aux + rows;
    char* d_nrm = d_pos + rows;
    OCEAN_TRY(consumer_begin(c, f.st));
    HIP_TRY(hipMemcpyAsync(d_pos, pos, rows, hipMemcpyHostToDevice, f.st));
    HIP_TRY(hipMemcpyAsync(d_nrm, nrm, rows, hipMemcpyHostToDevice, f.st));
    OCEAN_TRY(launch_shade(a, w->seabed == (uint32_t)OCEAN_SEABED_REFERENCE, count, d_pos, d_nrm, d_rgba, out_aux ? d_aux : nullptr, f.st));
    HIP_TRY(hipMemcpyAsync(out_rgba, d_rgba, rows, hipMemcpyDeviceToHost, f.st));
    if (out_aux) HIP_TRY(hipMemcpyAsync(out_aux, d_aux, rows, hipMemcpyDeviceToHost, f.st));
    OCEAN_TRY(consumer_end(c, f.st));
    HIP_TRY(hipStreamSynchronize(f.st));
    return OCEAN_OK;
}

int ocean_shade_grid(ocean_t* c, const ocean_sky* s, const ocean_water* w)
{
    ShadeArgs a;
    OCEAN_TRY(shade_args(c, s, w, a));
    if (!c->prepared || !c->grid_fresh || !c->grid_vertices) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t verts = c->grid_vertices;
    if (verts > c->shaded_capacity)
        OCEAN_TRY(regrow(c, &c->shaded, (float4**)nullptr, (size_t)verts * sizeof(float4), c->shaded_capacity, verts, [c] { c->shaded_vertices = 0; }));
    LastFrame f;
    no_frame(c, f);
    OCEAN_TRY(consumer_begin(c, f.st));            // behind the vertex stage that wrote the grid, whichever chain's stream it ran on
    OCEAN_TRY(launch_shade(a, w->seabed == (uint32_t)OCEAN_SEABED_REFERENCE, verts, c->grid_pos, c->grid_nrm, c->shaded, nullptr, f.st));
    OCEAN_TRY(consumer_end(c, f.st));
    c->shaded_vertices = verts;
    return OCEAN_OK;
}

int ocean_read_shaded(ocean_t* c, float* rgba)
{
    if (!c || !rgba) return OCEAN_E_INVALID;
    if (!c->shaded_vertices) return OCEAN_E_NOT_READY;
    HIP_TRY(hipSetDevice(c->device));
    OCEAN_TRY(sync_all(c));
    HIP_TRY(hipMemcpy(rgba, c->shaded, (size_t)c->shaded_vertices * sizeof(float4), hipMemcpyDeviceToHost));
    return OCEAN_OK;
}

int ocean_device_shaded(ocean_t* c, void** d_rgba, uint32_t* vertices)
{
    if (!c) return OCEAN_E_INVALID;
    if (d_rgba) *d_rgba = c->shaded_vertices ? c->shaded : nullptr;
    if (vertices) *vertices = c->shaded_vertices;
    return OCEAN_OK;
}

}  // extern "C"
