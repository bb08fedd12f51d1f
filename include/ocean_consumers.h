/*
 * include/ocean_consumers.h -- SURVEY.md 8f ranks 3-4: what consumes the two maps on the device (vertex stage, cascades, mip chain).
 * Part of the C ABI of libocean_hip.so (include/ocean.h is the drop-in boundary; this header declares more of the same library's exports).
 * Also here: what shapes the sea itself beyond the reference's one Phillips spectrum -- empirical spectra, directional spreading, wavenumber bands.
 */
#ifndef OCEAN_CONSUMERS_H_
#define OCEAN_CONSUMERS_H_

#include "ocean.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- vertex-stage consumer ----------------------------------
 * What the reference's vertex shader does with the two maps
 * (src/shaders/WaterSurfaceMesh.vert:24-41) for the grid its mesh generator builds
 * (WaterSurfaceMesh::CreateGridVertices, WaterSurfaceMesh.cpp:500-533), on the device:
 * vertex (x, y), x, y = -grid_size/2 .. grid_size/2, sits at (x, 0, y) * vertex_distance with
 * uv = (x + half, y + half) / grid_size; both maps are sampled at uv * uv_scale with the
 * reference's sampler (LINEAR, REPEAT: vulkan/Sampler.cpp:60-66);
 *   position = inPos + (D.x, D.y * A, D.z), w = D.w          (A = amplitude of the frame)
 *   normal   = normalize(-s.x / (1 + choppy*s.z), 1, -s.y / (1 + choppy*s.w)), w = 0
 * for the most recent frame of `tile`, ordered on its stream.  choppy is the value the
 * reference feeds (GetDisplacementLambda(), WaterSurfaceMesh.cpp:172).  Results stay in
 * device buffers owned by the context ((grid_size+1)^2 float4 each): ocean_read_grid copies
 * them out (synchronises), ocean_device_grid hands out the pointers.                  */
int ocean_displace_grid(ocean_t* ctx, uint32_t tile, uint32_t grid_size, float vertex_distance,
                        float uv_scale, float choppy);
/* Cascades (the reference's to-do "Endless - solving the tiling artifacts", README.md:37-44): the
 * tiles first_tile .. first_tile+count-1 of the batch (count <= 8) -- independent oceans with their own tile length,
 * wind, seed -- are summed by the consumer, tile c sampled at uv * uv_scales[c]:
 *   position = inPos + sum_c (D_c.x, D_c.y * A_c, D_c.z),  w = min_c D_c.w
 *   normal   = normalize(-S.x / (1 + choppy*S.z), 1, -S.y / (1 + choppy*S.w)),  S = sum_c normal-map sample of tile c
 * With incommensurate scales the surface no longer repeats with the period of one tile.  Same output buffers
 * and read-out as ocean_displace_grid.                                                                          */
int ocean_displace_grid_cascades(ocean_t* ctx, uint32_t first_tile, uint32_t count, uint32_t grid_size,
                                 float vertex_distance, const float* uv_scales /* count */, float choppy);
int ocean_read_grid(ocean_t* ctx, float* positions, float* normals);
int ocean_device_grid(ocean_t* ctx, void** d_positions, void** d_normals, uint32_t* vertices);

/* Mip chain of one tile's maps: the reference's LOD hook.  Its map textures are created and filled with a
 * `mipmapping` flag (s_kUseMipMapping, WaterSurfaceMesh.h:216, passed at WaterSurfaceMesh.cpp:611-618,652-690; off in the
 * shipped build, "LOD. anti-aliasing" on its to-do list, README.md:37-44); when set, Texture2D::GenerateMipmaps
 * (vulkan/Texture2D.cpp:228-330) blits level i-1 into level i at half the extent with VK_FILTER_LINEAR,
 * floor(log2(N)) + 1 levels in all.  ocean_build_mips does the same for both maps of `tile` behind the frame that wrote
 * them: levels 1 .. log2(N) (level 0 is the map itself), each texel the 2 x 2 mean of the level above, tightly packed
 * one after another -- level l starts at texel sum_{k=1}^{l-1} (N >> k)^2, ocean_mip_texels(N) = (N^2 - 1) / 3 texels
 * of RGBA32F per map.  Results stay in device buffers owned by the context: ocean_read_mips copies them out
 * (synchronises), ocean_device_mips hands out the pointers and the number of levels.                                  */
size_t ocean_mip_texels(uint32_t tile_size);
int ocean_build_mips(ocean_t* ctx, uint32_t tile);
int ocean_read_mips(ocean_t* ctx, float* disp_mips, float* nrm_mips);
int ocean_device_mips(ocean_t* ctx, void** d_disp_mips, void** d_nrm_mips, uint32_t* levels);

/* Mip chains of a tile range: what the LOD sampler below reads.  ocean_build_mips_tiles builds the chains of both maps of the tiles
 * first_tile .. first_tile+count-1 (count 1 .. tiles - first_tile) from the most recently enqueued frame, stream-ordered behind it like
 * every other consumer (any pipeline depth, caller-bound or imported output), in at most two kernel launches whatever the count.  Two
 * buffers owned by the context, one per map, hold [count][ocean_mip_texels(N)] float4: tile i of the range keeps the packed layout of
 * ocean_build_mips, so level l of tile i starts at texel i * ocean_mip_texels(N) + sum_{k=1}^{l-1} (N >> k)^2.  Every texel of every
 * level carries exactly the bits of ocean_build_mips' chain: (t00*0.5f + t10*0.5f)*0.5f + (t01*0.5f + t11*0.5f)*0.5f of the level above,
 * no contraction.  The buffers grow on demand (a growth that fails leaves no set), survive a new tile size and go with ocean_destroy.  The
 * context remembers the frame and the range the set was built from; a later call replaces the set, range included.  Memory:
 * 2 * count * (N^2 - 1) / 3 * 16 bytes.  ocean_build_mips and its buffers are independent of all this.
 * ocean_read_mips_tile copies one tile's chains out (synchronises; ocean_mip_texels(N) float4 each; either pointer may be NULL).
 * ocean_device_mips_tiles hands out the pointers (NULL while there is no set), the built range and the number of levels (log2 N).
 * Errors: OCEAN_E_INVALID for a NULL context, count == 0, a range or tile outside the batch; OCEAN_E_NOT_READY without Prepare or frame,
 * and for the read also without a set (none built since the last ocean_prepare or tile size) or for a tile outside the built range.   */
int ocean_build_mips_tiles(ocean_t* ctx, uint32_t first_tile, uint32_t count);
int ocean_read_mips_tile(ocean_t* ctx, uint32_t tile, float* disp_mips, float* nrm_mips);
int ocean_device_mips_tiles(ocean_t* ctx, void** d_disp_mips, void** d_nrm_mips,
                            uint32_t* first_tile, uint32_t* count, uint32_t* levels);

/* ---- surface query: displaced height and normal at arbitrary points --------------------------------------------------
 * What gameplay / physics code asks of an ocean (buoys, boats, cameras kept above the water): how high is the water at
 * world point (x, z), and which way does it face.  The surface is the one ocean_displace_grid_cascades draws (one tile:
 * cascades = 1, the surface of ocean_displace_grid).  A rest point r = (x, z) in mesh coordinates has
 *   u = (x / vertex_distance + grid_size/2) / grid_size,  v = (z / vertex_distance + grid_size/2) / grid_size
 * (grid_size/2 an integer division; at grid vertex (xi, yi) this is the vertex's uv); tile c of the set is sampled at
 * (u, v) * uv_scales[c] (LINEAR, REPEAT) and
 *   P(r) = (r.x + sum_c D_c.x,  sum_c D_c.y * A_c,  r.z + sum_c D_c.z),  w = min_c D_c.w,  n(r) = the vertex stage's normal,
 * exactly what the vertex stage writes for a vertex at rest point r.  The water above rest point r sits at P(r).xz, not at
 * r, so a query point q = (qx, qz) asks for the r with P(r).xz = q.  It is solved for with a diagonal Newton iteration:
 *   r_0 = q;  for k < K:  e = P(r_k).xz - q
 *                         Jx = 1 + sum_c lambda_c * N_c.z * s_c * L_c / (grid_size * vertex_distance)   (N_c: normal-map sample
 *                         Jz = 1 + sum_c lambda_c * N_c.w * s_c * L_c / (grid_size * vertex_distance)    of tile c at r_k)
 *                         J = sign(J) * 0.1 where |J| < 0.1 (J == 0 -> +0.1);  r_{k+1} = r_k - (e.x / Jx, e.z / Jz)
 *   out_pos = (P.x, P.y, P.z, w) at r_K,   out_nrm = (n.x, n.y, n.z, |P(r_K).xz - q|)
 * The normal map's z / w are dDx/dx and dDz/dz in ocean metres and D.x carries lambda, so J is the diagonal of dP.xz/dr.
 * lambda_c and L_c are the displacement lambda and tile length of the frame that wrote tile c's maps (a later
 * ocean_set_lambda does not change the answer).  fp32 throughout, no contraction (the test suite repeats it step for step).
 * out_nrm.w shows convergence: where the surface folds over itself (Jacobian <= 0) the inverse is not unique, and the
 * residual says so.  K = iterations: 1 .. 32, 0 means 8.
 * Supported range: finite points whose texel coordinates stay within |u * s_c * N| < 2^31 (N the tile size) at q and at every
 * r_k.  The out_pos / out_nrm row of a point outside it (NaN, +-inf, beyond 2^31 texels) is unspecified; the texel indices
 * are masked, so such a point reads inside the maps and leaves every other row as it would be without it.
 * Both calls read the most recently enqueued frame (caller-bound or imported output where it is, as ocean_displace_grid)
 * and are stream-ordered behind it like the other consumers, so the rule of ocean.h holds for them unchanged: a query
 * behind a frame whose in-launch wait gave up gets OCEAN_E_HIP once.
 * ocean_query_surface: host arrays xz[2*points], out_pos[4*points], out_nrm[4*points], staged through a device buffer
 * of the context that grows on demand; returns when the results are in out_pos / out_nrm.
 * ocean_query_surface_device: the same arrays in device memory of the context's device; enqueued behind the most recent
 * frame on its stream (ocean_stream), returns at once.
 * Errors: OCEAN_E_NOT_READY without Prepare or frame; OCEAN_E_INVALID for cascades 0 or > 8, a tile range outside the
 * batch, grid_size 0, iterations > 32, a NULL pointer with points > 0.  points == 0 does nothing and returns OCEAN_OK.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                         */
typedef struct ocean_surface {
    uint32_t first_tile, cascades;     /* 1 .. 8 tiles of the batch, as ocean_displace_grid_cascades */
    uint32_t grid_size;                /* as ocean_displace_grid */
    float    vertex_distance, choppy;
    uint32_t iterations;               /* 0 = 8; at most 32 */
    float    uv_scales[8];             /* first `cascades` used */
} ocean_surface;

int ocean_query_surface(ocean_t* ctx, const ocean_surface* s, const float* xz, uint32_t points,
                        float* out_pos, float* out_nrm);
int ocean_query_surface_device(ocean_t* ctx, const ocean_surface* s, const void* d_xz, uint32_t points,
                               void* d_out_pos, void* d_out_nrm);

/* ---- LOD sampling: the surface at the level that fits the caller's mesh (the reference's to-do "LOD. anti-aliasing") -----------
 * A mesh whose vertex spacing exceeds a cascade's texel spacing (uv_scale * N / grid_size > 1: a far-field ring, a coarse grid)
 * aliases when it samples level 0.  These calls read each cascade's maps at the mip level that fits a footprint f, the spacing of the
 * caller's mesh at that vertex in mesh metres -- a clipmap ring's cell size, a projected grid's distance to its neighbours; the
 * library does not dictate the topology.
 * ocean_sample_surface_lod is the FORWARD evaluation: what the cascade vertex stage would write for a vertex at rest point (x, z).
 * It is not the Newton inverse of ocean_query_surface; s->iterations is ignored.  fp32 throughout, no contraction, in this order
 * (tests/lod.py repeats it step for step):
 *   texels per metre (host)   tpm_c = fabsf((uv_scales[c] * (float)N) / ((float)grid_size * vertex_distance))
 *   ratio                     rho = (f * l->scale) * tpm_c
 *   level                     Lmax = log2 N, or min(log2 N, max_level) where max_level != 0
 *                             !(rho > 1.0f)    -> lev = 0, t = 0           (0, negative, NaN)
 *                             rho >= 2^Lmax    -> lev = Lmax, t = 0        (+inf)
 *                             otherwise        -> lev = the unbiased exponent of rho, t = ldexpf(rho, -lev) - 1.0f   (both exact)
 *                             (between two levels the blend is linear in rho, not in log2 rho)
 *   sample                    (u, v) as ocean_query_surface forms them from a rest point; us = u * uv_scales[c], vs likewise;
 *                             A = the LINEAR, REPEAT sample of level lev (extent N >> lev; level 0 is the map, levels >= 1 the set of
 *                             ocean_build_mips_tiles); t == 0 -> A, the upper level is not read; otherwise B = the same sample of
 *                             level lev + 1, it = 1.0f - t, each channel A*it + B*t.  Both maps of a cascade use the same (lev, t).
 *   combine                   as ocean_displace_grid_cascades: sums in cascade order from 0.0f, dy += D.y * A_c, w = fminf from FLT_MAX
 *   out_pos = (x + dx, 0.0f + dy, z + dz, w)
 *   out_nrm = (n.x, n.y, n.z, lambda),  lambda = fmaxf over the cascades, from 0.0f, of (float)lev + t: the coarsest level that went
 *             into the vertex, for the caller's own blending.
 * Readiness: the set of ocean_build_mips_tiles must cover first_tile .. first_tile+cascades-1 and must have been built from the frame
 * the call reads, the most recently enqueued one -- otherwise OCEAN_E_NOT_READY, also when every point would stay on level 0.  A new
 * frame, ocean_prepare or ocean_set_tile_size makes the set stale: rebuild it once per frame, behind the frame.
 * Other errors, supported range, staging, stream order and fault rule as ocean_query_surface / _device; additionally OCEAN_E_INVALID for a
 * NULL l or a scale that is not finite and positive.  points == 0 returns OCEAN_OK before the pointers are looked at.  The host form
 * stages [outputs | 12-byte inputs] in the context's buffer; the device form needs 4-byte-aligned input, 16-byte-aligned outputs.
 * ocean_displace_grid_lod is ocean_displace_grid_cascades with every sample taken through this sampler at f = fabsf(vertex_distance):
 * the same vertices, (u, v), output buffers and read-out (ocean_read_grid, ocean_device_grid), normals.w = 0.0f.  Where no cascade is
 * undersampled (rho <= 1 for all) it equals ocean_displace_grid_cascades in every bit.  Errors: those of that call and those above.
 * (An addition to ABI version 5.)                                                                                                    */
typedef struct ocean_lod {
    float    scale;        /* multiplies every footprint; > 0 and finite          default 1 */
    uint32_t max_level;    /* highest level used; 0 = no limit (log2 N)           default 0 */
} ocean_lod;
void ocean_default_lod(ocean_lod* l);
int ocean_sample_surface_lod(ocean_t* ctx, const ocean_surface* s, const ocean_lod* l,
                             const float* xzf /* 3 * points: x, z, footprint in mesh metres */, uint32_t points,
                             float* out_pos /* 4 * points */, float* out_nrm /* 4 * points */);
int ocean_sample_surface_lod_device(ocean_t* ctx, const ocean_surface* s, const ocean_lod* l,
                                    const void* d_xzf, uint32_t points, void* d_out_pos, void* d_out_nrm);
int ocean_displace_grid_lod(ocean_t* ctx, uint32_t first_tile, uint32_t count, uint32_t grid_size, float vertex_distance,
                            const float* uv_scales /* count */, float choppy, const ocean_lod* l);

/* ---- surface bounds: min/max pyramids per tile, patch boxes, frustum classification ------------------------------------------------
 * A renderer that draws the sea in patches decides every frame which patches to draw at all; for that it needs a box that is guaranteed
 * to contain the DISPLACED patch.  The same box answers "can this patch have folds or foam at all?" (the lower bound of the Jacobian
 * slot) and "can this body touch water?" before a buoyancy call.  Per-frame order: frame -> ocean_build_bounds_tiles ->
 * ocean_patch_bounds(_device) -> draw.
 * The pyramid   ocean_build_bounds_tiles builds, for each of the tiles first_tile .. first_tile+count-1 (count 1 .. tiles - first_tile),
 *          two chains over the DISPLACEMENT map of the most recently enqueued frame, `lo` and `hi`, each in the packed layout of
 *          ocean_build_mips (ocean_mip_texels(N) float4; level l = 1 .. log2 N, extent N >> l, starts at texel sum_{k=1}^{l-1} (N >> k)^2).
 *          Node (y, x) of level l of `lo` holds, per channel (x, y, z, w), the fminf of the map's texels in rows y*2^l .. (y+1)*2^l - 1
 *          and columns x*2^l .. (x+1)*2^l - 1; `hi` holds the fmaxf.  Level 0 is the map itself.  min and max are exact, so every node
 *          has one value whatever the order of the reduction.  The maps are finite: what a NaN texel does to its nodes is unspecified,
 *          and so is the sign of a zero node whose block holds zeros of both signs.
 *          first_level: levels below it are NOT stored -- their place in the chain keeps its offset, its contents are unspecified (all
 *          of it: a build may or may not write there).  0 means 1; 1 .. log2 N are valid, anything else is OCEAN_E_INVALID.  Culling
 *          patches are rarely narrower than 8 texels and levels 1 and 2 are 94 % of a chain: this is what keeps the per-frame cost
 *          near one read of the map.  The patch query never reads below the set's first_level.
 *          Stream-ordered behind the most recently enqueued frame like every consumer (any pipeline depth, caller-bound or imported
 *          output), at most two kernel launches whatever the count.  Two buffers owned by the context, [count][ocean_mip_texels(N)]
 *          float4 each: they grow on demand (a growth that fails leaves no set), survive a new tile size and go with ocean_destroy.
 *          The context remembers the frame, range and first_level the set was built from; a later call replaces the set.  A new
 *          frame, ocean_prepare or ocean_set_tile_size makes it stale.  Memory: 2 * count * (N^2 - 1) / 3 * 16 bytes.
 *          ocean_read_bounds_tile copies one tile's chains out (synchronises; either pointer may be NULL).  ocean_device_bounds_tiles
 *          hands out the pointers (NULL while there is no set), the built range, the number of levels (log2 N) and first_level.
 *          Errors: OCEAN_E_INVALID for a NULL context, count == 0, a range or tile outside the batch, a bad first_level;
 *          OCEAN_E_NOT_READY without Prepare or frame, and for the read also without a set or for a tile outside the built range.
 * The patch query   ocean_patch_bounds turns `count` rest-space rectangles (x0, z0, x1, z1 in mesh metres; the ends in either order)
 *          into world-space boxes of the surface `s` describes (s->iterations and s->choppy are unused).  One thread per rectangle;
 *          fp32 throughout, no contraction, in this order (tests/bounds.py repeats it step for step):
 *   Axis range  for one axis with ends p0, p1 and cascade c:
 *                 t(p) = ((p / vertex_distance + half) / grid_size) * uv_scales[c] * (float)N - 0.5f
 *               exactly as ocean_query_surface forms u and its sampler the texel coordinate; pad = pad_texels;
 *                 i0 = (int)floorf(fminf(t(p0), t(p1))) - pad,   i1 = (int)floorf(fmaxf(t(p0), t(p1))) + 1 + pad     (kept in 64 bits)
 *               Every operation in t is monotone (non-decreasing or non-increasing in p, rounding included), so for any p between
 *               the ends t(p) lies between t(p0) and t(p1), and the two texels floor(t(p)), floor(t(p)) + 1 the bilinear sampler
 *               reads lie in i0 .. i1 -- for either sign of vertex_distance or uv_scales[c].  That is the reason for the rule.
 *   Level       w = max(i1x - i0x, i1z - i0z) + 1 (64-bit: it cannot overflow).  If w >= N, or one of x0, z0, x1, z1 is not finite:
 *               the single node of level log2 N.  Otherwise l = the smallest level with 2^l >= w, raised to the set's first_level.
 *               A range of at most 2^l texels touches at most two nodes per axis, (i0 >> l) & m and (i1 >> l) & m with
 *               m = (N >> l) - 1: the arithmetic shift of negative indices and the mask make this REPEAT.  lo_c / hi_c = the fminf /
 *               fmaxf per channel over those <= 4 nodes of tile c's `lo` / `hi` chain.
 *   Combine     as ocean_displace_grid_cascades, sums from 0.0f in cascade order:
 *                 L.x += lo_c.x,  L.y += lo_c.y * A_c,  L.z += lo_c.z;   H likewise from hi_c;   Lw = fminf over c of lo_c.w from FLT_MAX
 *               (A_c, the amplitude from the frame's height keys as in every consumer, is > 0: the product keeps the order.)
 *   Output      out_lo = (fminf(x0, x1) + L.x,  0.0f + L.y,  fminf(z0, z1) + L.z,  Lw)
 *               out_hi = (fmaxf(x0, x1) + H.x,  0.0f + H.y,  fmaxf(z0, z1) + H.z,  cls)
 *   Class       cls = 1.0f when planes == 0.  Otherwise, for each plane (a, b, c, d) in order (inside is a*x + b*y + c*z + d >= 0):
 *                 far  = ((a * (a >= 0 ? hi.x : lo.x) + b * (b >= 0 ? hi.y : lo.y)) + c * (c >= 0 ? hi.z : lo.z)) + d
 *                 near = the same expression with the opposite corners
 *               far < 0: cls = 0.0f (outside), and the later planes are not looked at;  near < 0 on any plane: cls = 1.0f (straddles);
 *               otherwise cls = 2.0f (inside).
 * Guarantee     For every rest point r inside the rectangle, the position the level-0 forward evaluation writes for r lies in
 *          [out_lo, out_hi] on every axis, up to the rounding of the bilinear blend.  (The level-0 forward evaluation is
 *          ocean_sample_surface_lod at footprint 0; it is the cascade vertex stage wherever that stage's u equals the query's.)  The
 *          blend (c00*ia + c10*a)*ib + (c01*ia + c11*a)*b has 1 - a inexact by at most 2^-25 where a < 0.5, followed by five rounded
 *          operations, so a sample exceeds the largest texel it reads by less than 2^-21 * max|texel|; the sums over the cascades and
 *          the final additions add nothing, because rounding is monotone and both sides add the same terms in the same order.  The
 *          Jacobian slot obeys w >= out_lo.w minus that slack.
 *          Its limits: a caller whose u is formed differently sets pad_texels = 1 (the vertex stage divides integers, and
 *          x / vertex_distance need not return the integer); one who samples at mip level L sets pad_texels = 2^(L+1).  The bound is
 *          conservative, not tight: up to twice the range per axis goes into a box.
 * Readiness: as for the LOD sampler -- OCEAN_E_NOT_READY unless a bounds set covers first_tile .. first_tile+cascades-1 and was built from
 * the frame the call reads.  Other errors are those of ocean_query_surface (iterations are not looked at); additionally OCEAN_E_INVALID
 * for a NULL q, planes > 6, one of the first `planes` planes that is not finite, pad_texels > 65536.  count == 0 returns OCEAN_OK before
 * the pointers are looked at.  The host form stages [outputs | 16-byte inputs] in the context's buffer and returns when the results are
 * there; the device form (rects 4-byte, outputs 16-byte aligned) is enqueued behind the most recent frame on its stream and returns at
 * once.  Supported range as ocean_query_surface: the row of a rectangle outside it (NaN, +-inf, beyond 2^31 texels) is unspecified; the
 * indices are masked, so it reads inside the chains and disturbs no other row.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                                        */
int ocean_build_bounds_tiles(ocean_t* ctx, uint32_t first_tile, uint32_t count, uint32_t first_level /* 0 = 1 */);
int ocean_read_bounds_tile(ocean_t* ctx, uint32_t tile, float* lo_chain, float* hi_chain);   /* either may be NULL */
int ocean_device_bounds_tiles(ocean_t* ctx, void** d_lo, void** d_hi,
                              uint32_t* first_tile, uint32_t* count, uint32_t* levels, uint32_t* first_level);
typedef struct ocean_patch_query {
    uint32_t pad_texels;        /* texels added on every side of each cascade's index range          default 0 */
    uint32_t planes;            /* 0 .. 6 frustum planes; 0 = no classification                      default 0 */
    float    plane[6][4];       /* (a, b, c, d): a point is inside where a*x + b*y + c*z + d >= 0; finite */
} ocean_patch_query;
void ocean_default_patch_query(ocean_patch_query* q);
int ocean_patch_bounds(ocean_t* ctx, const ocean_surface* s, const ocean_patch_query* q,
                       const float* rects /* 4 * count: x0, z0, x1, z1 in mesh metres, rest space */, uint32_t count,
                       float* out_lo /* 4 * count */, float* out_hi /* 4 * count */);
int ocean_patch_bounds_device(ocean_t* ctx, const ocean_surface* s, const ocean_patch_query* q,
                              const void* d_rects, uint32_t count, void* d_out_lo, void* d_out_hi);

/* ---- ray cast: where a ray first meets the water --------------------------------------------------------------------
 * Camera picking, projectiles and splashes, line of sight over the waves, a camera's near plane kept out of a crest, "is the
 * camera under water?".  The surface is exactly the one ocean_query_surface defines for the same ocean_surface (tiles,
 * cascades, grid, vertex distance, choppiness, Newton iterations K): write H(x, z) for the out_pos.y that query returns at
 * (x, z).  fp32 throughout, no contraction, in this order (the test suite repeats it step for step):
 *   Direction   len = sqrtf((dx*dx + dy*dy) + dz*dz); a zero or non-finite len is a miss; d = (dx/len, dy/len, dz/len).
 *   Gap         p(t) = (o.x + t*d.x, o.y + t*d.y, o.z + t*d.z),  f(t) = p(t).y - H(p(t).x, p(t).z): the height above the water.
 *   Slab        Hmax = fmaxf(1.001f * (amp_0 + amp_1 + ...), 1e-3f) (sum from 0.0f in cascade order; amp_c is the largest magnitude
 *               of tile c's height keys, the amplitude the query scales heights with), so every height lies in [-Hmax, Hmax].
 *               The floor of 1 mm is for a flat sea (amp = FLT_MIN): without it the slab has no thickness, every sample of the
 *               march is the one point o.y + t0*d.y, and its rounding decides between hit and miss.
 *               If o.y <= -Hmax the origin is under water (below).  Otherwise [0, max_distance] is clipped to the slab:
 *                 d.y < 0:   t0 = fmaxf(0, (Hmax - o.y) / d.y),   t1 = fminf(max_distance, (-Hmax - o.y) / d.y)
 *                 d.y > 0:   t0 = fmaxf(0, (-Hmax - o.y) / d.y),  t1 = fminf(max_distance, (Hmax - o.y) / d.y)
 *                 d.y == 0:  t0 = 0, t1 = max_distance if o.y < Hmax; otherwise the segment is empty
 *               and the segment is empty where t1 < t0: a miss.
 *   March       M = steps, h = (t1 - t0) / (float)M, samples t_i = t0 + (float)i * h for i = 0 .. M with t_M := t1.  The first i
 *               with f(t_i) <= 0 decides; none is a miss.  i == 0: if t0 == 0 the origin is under water, otherwise the hit is at
 *               t = t0.  Else the bracket is [a, b] = [t_{i-1}, t_i] with f(a) > 0 >= f(b).
 *   Refinement  R = refine rounds; each has s_j = a + (float)j * ((b - a) / 16.0f) for j = 1 .. 15 and s_16 := b, s_0 := a: the
 *               first j with f(s_j) <= 0 gives [a, b] := [s_{j-1}, s_j] (f known at both ends already).
 *   Hit         t = a + (b - a) * (fa / (fa - fb)) (fa = f(a), fb = f(b)), then one query at (p(t).x, p(t).z):
 *                 out_hit = (P.x, P.y, P.z, t),  out_nrm = (query normal, p(t).y - P.y)   (P.y is the water height there;
 *                 out_nrm.w, the signed gap at the hit, is ~ 0)
 *   Under water out_hit = (P.x, P.y, P.z, -2),  out_nrm = (query normal, o.y - P.y)  with P the query at (o.x, o.z): the depth, <= 0
 *   Miss        out_hit = (0, 0, 0, -1),  out_nrm = (0, 0, 0, 0)
 * Not covered: rays that start under water and look for the surface from below get only the depth; where the surface folds
 * (Jacobian <= 0) the height field the query defines is not unique (its residual shows it), and the ray meets that height
 * field, not the folded sheet; a wet interval thinner than one coarse step can be stepped over (raise steps).
 * Both calls read the most recently enqueued frame (caller-bound or imported output where it is) and are stream-ordered
 * behind it like ocean_query_surface.  ocean_raycast_surface: host arrays rays[6*count] (ox, oy, oz, dx, dy, dz),
 * out_hit[4*count], out_nrm[4*count], staged through a device buffer of the context that grows on demand; returns when the
 * results are there.  ocean_raycast_surface_device: the same arrays in device memory of the context's device (rays 4-byte,
 * outputs 16-byte aligned); enqueued behind the most recent frame on its stream (ocean_stream), returns at once.
 * Errors: OCEAN_E_NOT_READY without Prepare or frame; OCEAN_E_INVALID for a NULL s or r, the invalid ocean_surface cases of
 * ocean_query_surface, a max_distance <= 0 or not finite, steps > 4096, refine > 8, a NULL array with count > 0.
 * count == 0 does nothing and returns OCEAN_OK.  (An addition to ABI version 5.)                                         */
typedef struct ocean_raycast {
    float    max_distance;             /* > 0 and finite: rays cover t in [0, max_distance] metres along the unit direction */
    uint32_t steps;                    /* coarse samples across the part of the ray inside the height slab: 0 = 64, at most 4096 */
    uint32_t refine;                   /* refinement rounds, each splitting the bracket into 16 equal parts: 0 = 3, at most 8 */
} ocean_raycast;

int ocean_raycast_surface(ocean_t* ctx, const ocean_surface* s, const ocean_raycast* r,
                          const float* rays, uint32_t count, float* out_hit, float* out_nrm);
int ocean_raycast_surface_device(ocean_t* ctx, const ocean_surface* s, const ocean_raycast* r,
                                 const void* d_rays, uint32_t count, void* d_out_hit, void* d_out_nrm);

/* ---- persistent foam: whitecap coverage accumulated across frames -----------------------------------------------------
 * The reference's to-do "Foam rendering" (README.md:37-44).  Its fragment shader paints the Jacobian slot white where it is
 * negative: an instantaneous, binary mask.  Here the same signal feeds a coverage field with memory, F[tiles][N][N] of float
 * in [0, 1], in the texel layout of the maps (row m = image row), owned by the context: foam appears where the surface
 * compresses, spreads a little and fades over seconds.  It lives in texture (rest) space: drawn through the vertex stage at
 * the vertex's uv it moves with the choppy displacement by construction.  A renderer samples it as a third texture beside
 * the two maps (max over cascades); game code asks for it at world points (ocean_query_foam).
 * One step, for texel (m, n) of a tile, indices wrapped by & (N - 1) (REPEAT, like the sampler); fp32 throughout, no
 * contraction, in exactly this order (the test suite repeats it step for step):
 *   J     Jacobian of the texel, from what the frame that wrote the maps computed (its mode is recorded when it is enqueued):
 *           OCEAN_MODE_JACOBIAN frame:  J = disp.w
 *           OCEAN_MODE_FULL7 frame:     J = (1.0f + lam * nrm.z) * (1.0f + lam * nrm.w), lam the lambda of that tile's frame
 *                                       (the diagonal Jacobian the vertex normal and the surface query use)
 *           CHOPPY5 / HEIGHT1 frame:    OCEAN_E_UNSUPPORTED (the ingredients are not in the maps)
 *   decay = (float)exp(-(double)dt / (double)lifetime), rounded once on the host
 *   g    = fminf(fmaxf((threshold - J) * gain, 0.0f), 1.0f)
 *   r(k) = (F[k][n-1] + 2.0f * F[k][n]) + F[k][n+1]              for k = m-1, m, m+1
 *   b    = ((r(m-1) + 2.0f * r(m)) + r(m+1)) * 0.0625f           (3 x 3 binomial)
 *   s    = F[m][n] + spread * (b - F[m][n])
 *   c    = s * decay
 *   f    = fmaxf(c, g);   F'[m][n] = (f < cutoff) ? 0.0f : f
 * cutoff keeps the field sparse and the spreading tail out of the denormal range; cutoff = 0 disables it.
 * ocean_update_foam applies one step to `tile` (or OCEAN_ALL_TILES: one launch for all of them; the other tiles keep their
 * state) from the most recently enqueued frame (caller-bound or imported output where it is), enqueued behind that frame on
 * its stream and ordered with the other consumers, so updates at pipeline depth > 1 are ordered among themselves.  Calling
 * it twice behind one frame applies two steps.  Two buffers of tiles * N * N floats are allocated on first use
 * (OCEAN_E_NOMEM leaves nothing behind) and alternate: ocean_device_foam hands out the one that holds the state after the
 * most recently enqueued update -- ask again after each update -- and NULL while there is none.  ocean_read_foam copies one
 * tile out (synchronises).  ocean_prepare zeroes the state (not ready until the next update), ocean_set_tile_size frees it,
 * ocean_reset_foam zeroes it stream-ordered (a ready state stays ready; nothing to do before the first update).
 * An update enqueued behind a frame whose in-launch wait gives up has consumed that frame: the call that recovers reports
 * OCEAN_E_HIP once (ocean.h), and the state then contains one step taken from a faulted frame -- reset it or let it fade.
 * ocean_query_foam: for each world point q the K Newton steps of ocean_query_surface on the same ocean_surface give the rest
 * point r = r_K; tile c's foam is sampled at (u, v) * uv_scales[c] (LINEAR, REPEAT; (c00*ia + c10*a)*ib + (c01*ia + c11*a)*b)
 * and the cascades are combined with fmaxf from 0.0f in cascade order (the counterpart of w = min_c D_c.w):
 *   out[i] = (foam, r.x, r.z, |P(r).xz - q|)
 * r is the texture-space coordinate a caller needs for anything else it samples there.  Host / device variants as
 * ocean_query_surface / _device (a staging buffer that grows on demand; or enqueue and return, d_out 16-byte aligned).
 * Errors: OCEAN_E_INVALID for a NULL context, params or destination, a tile outside the batch, lifetime <= 0, spread or
 * cutoff outside [0, 1], a non-finite field or dt, dt < 0, the invalid ocean_surface cases of ocean_query_surface;
 * OCEAN_E_NOT_READY for an update without Prepare or frame, a read or query without an update since Prepare.
 * points == 0 does nothing and returns OCEAN_OK.  (An addition to ABI version 5.)                                      */
typedef struct ocean_foam {
    float threshold;                   /* foam is generated where J < threshold                      default 0.6    */
    float gain;                        /* generation = clamp((threshold - J) * gain, 0, 1)           default 2.5    */
    float lifetime;                    /* e-folding time in seconds, > 0                             default 4.0    */
    float spread;                      /* 0 .. 1, blend towards the 3 x 3 binomial per step          default 0.25   */
    float cutoff;                      /* 0 .. 1, values below it become 0                           default 1/1024 */
} ocean_foam;

void ocean_default_foam(ocean_foam* f);
int ocean_update_foam(ocean_t* ctx, uint32_t tile /* or OCEAN_ALL_TILES */, const ocean_foam* f, float dt);
int ocean_reset_foam(ocean_t* ctx);
int ocean_read_foam(ocean_t* ctx, uint32_t tile, float* out /* N * N */);
int ocean_device_foam(ocean_t* ctx, void** d_foam /* [tiles][N][N] */);
int ocean_query_foam(ocean_t* ctx, const ocean_surface* s, const float* xz, uint32_t points, float* out /* 4 * points */);
int ocean_query_foam_device(ocean_t* ctx, const ocean_surface* s, const void* d_xz, uint32_t points, void* d_out);

/* ---- buoyancy: net force and torque on floating bodies, reduced on the device ------------------------------------------
 * What most callers do with the surface query: push a few hull points per boat through it, read every point back and add up
 * "if (depth > 0) apply_force(...)" on the host.  Here the hull is uploaded once, in body space, and a call takes bodies in and
 * gives one force and one torque per body out.
 * Hull     ocean_set_hull uploads `count` sample points (local x, y, z, edge e) into a device buffer the context owns.  A point is
 *          a cubic cell of edge e centred at the local position: a voxelised hull, or a buoy as one cell.  Checked on the host: every
 *          e > 0 and finite, every position finite, otherwise OCEAN_E_INVALID and the old hull stays.  In-flight work is drained
 *          before the buffer is replaced.  The hull does not depend on the maps: it survives ocean_prepare and ocean_set_tile_size
 *          and is freed by ocean_destroy.  count == 0 drops the hull.
 * Body     ocean_body, 16 words.  Its points are [first_point, first_point + points) of the hull; ranges of different bodies may
 *          overlap or coincide (instancing).  The quaternion (x, y, z, w) is used as given, not normalised.  Torques are about `pos`.
 * The water under a hull point is what ocean_query_surface answers for the same ocean_surface: the same K Newton steps.  For hull
 * point l = (lx, ly, lz), edge e, of a body with quaternion q, in fp32 throughout, no contraction, in exactly this order (the test
 * suite repeats it step for step; cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)):
 *   Arm         t = 2.0f * cross(q.xyz, l) (each component);  a = (l + q.w * t) + cross(q.xyz, t);  p = pos + a
 *   Water       H = out_pos.y and res = out_nrm.w of ocean_query_surface at (p.x, p.z)
 *   Submersion  s = fminf(fmaxf((H - p.y) / e + 0.5f, 0.0f), 1.0f);  v = s * ((e * e) * e)
 *   Force       u = vel + cross(omega, a);  weight = density * gravity (one float product on the host);  dv = drag * v
 *               f = ((-dv) * u.x,  weight * v - dv * u.y,  (-dv) * u.z);   tq = cross(a, f)
 *               Archimedes straight up, and linear drag against the point's own velocity in proportion to its submerged volume.
 *   Reduction   eight channels: f.x, f.y, f.z, tq.x, tq.y, tq.z, v are summed, res is combined with fmaxf from 0.0f.  The order is
 *               fixed: slot k = 0 .. 63 takes the body's points k, k + 64, k + 128, ... in that order, slot = slot + term from +0.0f
 *               (an empty slot stays +0.0f); then for off = 32, 16, 8, 4, 2, 1 in turn slot[k] = slot[k] + slot[k + off] for k < off
 *               (fmaxf(slot[k], slot[k + off]) for res).  The result is slot[0].
 *   Output      out_force[b] = (F.x, F.y, F.z, V), V the submerged volume in m^3;  out_torque[b] = (T.x, T.y, T.z, largest res):
 *               the residual tells when a body sits on a fold, as out_nrm.w does for the query.  A body without points: all +0.0f.
 * Not covered: slamming and added mass; integrating the bodies -- that is the caller's physics engine's job, which is why the call
 * returns forces and not new poses.  (Drag here is against still water; ocean_buoyancy_bodies_flow, below, takes it against the moving water.)
 * Both calls read the most recently enqueued frame (caller-bound or imported output where it is) and are stream-ordered behind it
 * like ocean_query_surface; the fault rule of ocean.h holds unchanged.  ocean_buoyancy_bodies: host arrays bodies[count],
 * out_force[4*count], out_torque[4*count], staged through the context's staging buffer; returns when the results are there.  A body
 * whose [first_point, first_point + points) leaves the hull is rejected (OCEAN_E_INVALID) before anything is launched.
 * ocean_buoyancy_bodies_device: the same arrays in device memory of the context's device (16-byte aligned); enqueued behind the
 * most recent frame on its stream (ocean_stream), returns at once.  The host cannot see those bodies, so the kernel clamps each
 * range to the hull: first = min(first_point, hull points), and the points summed are first .. first + min(points, hull points -
 * first) - 1 (none where first_point is at or past the end).  A body never reads outside the hull buffer.
 * Errors: OCEAN_E_NOT_READY without Prepare or frame, or without a hull; OCEAN_E_INVALID for a NULL context, surface or
 * parameters, the invalid ocean_surface cases of ocean_query_surface, a density, gravity or drag that is negative or not finite,
 * a NULL array with count > 0, a hull point that fails the check above.  count == 0 (bodies) does nothing and returns OCEAN_OK
 * before the pointers are looked at.  (An addition to ABI version 5: nothing of the existing entry points or structures changes.) */
typedef struct ocean_body {            /* 16 words, 64 bytes */
    float    pos[3];                   /* world position of the body origin (torques are about it: put it at the centre of mass) */
    float    quat[4];                  /* x, y, z, w; used as given, not normalised */
    float    vel[3], omega[3];         /* linear / angular velocity, world frame */
    uint32_t first_point, points;      /* this body's range of the uploaded hull; ranges may overlap (instancing) */
    uint32_t reserved;                 /* 0 */
} ocean_body;
typedef struct ocean_buoyancy {
    float density;                     /* of the water, kg/m^3                                       default 1025  */
    float gravity;                     /* m/s^2                                                      default 9.81  */
    float drag;                        /* N per (m/s) per m^3 of submerged volume                    default 1000  */
} ocean_buoyancy;                      /* all finite and >= 0 */

void ocean_default_buoyancy(ocean_buoyancy* b);
int ocean_set_hull(ocean_t* ctx, const float* points /* 4 * count: local x, y, z, edge e */, uint32_t count);
int ocean_buoyancy_bodies(ocean_t* ctx, const ocean_surface* s, const ocean_buoyancy* b, const ocean_body* bodies, uint32_t count,
                          float* out_force /* 4 * count */, float* out_torque /* 4 * count */);
int ocean_buoyancy_bodies_device(ocean_t* ctx, const ocean_surface* s, const ocean_buoyancy* b, const void* d_bodies, uint32_t count,
                                 void* d_out_force, void* d_out_torque);

/* ---- water velocity: derivative twin tiles, a velocity query, drag against the moving water ------------------------------
 * The animated spectrum is real per bin, h~(k, t) = 2 Re(h0(k) e^{i w t}), so its time derivative is 2 Re(i w h0(k) e^{i w t}): the
 * same expression for the spectrum h0' = i w h0 = (-w h0.im, w h0.re).  Everything behind the spectrum is linear in it, so a tile
 * prepared with h0' and run through the unchanged frame pipeline writes maps that are the time derivative of its source tile's
 * maps.  Such a tile is a twin.  It costs one more tile per frame and is opt-in; no frame kernel knows about it.
 * Twin tiles   ocean_set_velocity_twin makes `tile` the twin of `source` (same batch) from the next ocean_prepare on; source =
 *          OCEAN_NO_SOURCE makes it an ordinary tile again.  Host state only, like ocean_set_params, but it drains in-flight work
 *          and leaves the context not prepared: frames and consumers return OCEAN_E_NOT_READY until ocean_prepare.  A source has at
 *          most one twin and twins of twins are rejected: OCEAN_E_INVALID for a tile (or source) outside the batch, tile == source,
 *          a source that is itself a twin, a tile that is some twin's source, a source that already has another twin.  The table
 *          survives ocean_prepare and ocean_set_tile_size.  ocean_velocity_twin reads it (OCEAN_NO_SOURCE for an ordinary tile).
 *          A twin has no parameters of its own: Prepare and the frames read its source's ocean_params (tile length, animation
 *          period, ... and lambda on every frame) and its source's time offset (ocean_set_time_offsets), so k and omega are its
 *          source's.  ocean_set_params / ocean_set_lambda with a twin's explicit index return OCEAN_E_INVALID (OCEAN_ALL_TILES
 *          behaves as always); ocean_get_params(twin) returns the source's.  Prepare then overwrites every texel of the twin's
 *          spectrum: h0[twin] = (-(w * h0[src].y), w * h0[src].x), w = omega[src] (fp32, one multiply per component), and copies
 *          the source's gaussian draws into the twin's slot (injected draws for a twin are ignored).
 *          A twin's maps, in every mode: disp = (lambda dDx/dt, (dh/dt) / A', lambda dDz/dt, the mode's w slot evaluated for the
 *          derivative spectrum), A' = max |dh/dt| from the twin's own height keys (ocean_get_heights(twin); the FLT_MIN floor of a
 *          flat sea as for any tile); nrm = the time derivatives of the four normal-map channels.  A twin's disp.w and its foam
 *          state mean nothing.
 * Velocity query  ocean_query_velocity: the velocity of the water particle that sits at world point q at the frame's time, dP/dt at
 *          a fixed rest point.  The cascade set of `s` is made of source tiles; their twins must be consecutive ascending tiles
 *          v, v+1, ..., v+cascades-1 in cascade order (below or above the sources).  fp32 throughout, no contraction, in this order:
 *            r = the K Newton steps of ocean_query_surface at q;  (u, v) = the uv of r as in that query;  V = (0.0f, 0.0f, 0.0f)
 *            for c in cascade order:  d' = sample of twin c's displacement map at (u, v) * uv_scales[c] (LINEAR, REPEAT)
 *                                     V.x = V.x + d'.x;  V.y = V.y + d'.y * A'_c;  V.z = V.z + d'.z
 *            out_pos = exactly ocean_query_surface's out_pos at q;   out_vel = (V.x, V.y, V.z, |P(r).xz - q|)
 *          Bilinear sampling is linear, so it commutes with the derivative.  Host / device forms, staging, stream order and the
 *          fault rule as ocean_query_surface / _device.  Errors as ocean_query_surface, and: OCEAN_E_NOT_READY for a set of which
 *          no tile has a twin; OCEAN_E_INVALID for a set only partly twinned or with twins that are not consecutive.
 * Flow buoyancy   ocean_buoyancy_bodies_flow / _device: ocean_buoyancy_bodies / _device with the drag taken against the water.  V as
 *          above at the hull point's (p.x, p.z), from the rest point that gave H (no second Newton solve), and
 *            u = ((vel.x + (om.y*a.z - om.z*a.y)) - V.x,  (vel.y + (om.z*a.x - om.x*a.z)) - V.y,  (vel.z + (om.x*a.y - om.y*a.x)) - V.z)
 *          in place of the point's own velocity; everything else -- the reduction order, the outputs, the clamping of body ranges in
 *          the device form, the errors -- is the text above unchanged.  Twin requirements and errors as ocean_query_velocity.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                            */
#define OCEAN_NO_SOURCE 0xffffffffu
int ocean_set_velocity_twin(ocean_t* ctx, uint32_t tile, uint32_t source /* or OCEAN_NO_SOURCE */);
int ocean_velocity_twin(const ocean_t* ctx, uint32_t tile, uint32_t* source);   /* OCEAN_NO_SOURCE for an ordinary tile */
int ocean_query_velocity(ocean_t* ctx, const ocean_surface* s, const float* xz, uint32_t points,
                         float* out_pos /* 4 * points */, float* out_vel /* 4 * points */);
int ocean_query_velocity_device(ocean_t* ctx, const ocean_surface* s, const void* d_xz, uint32_t points,
                                void* d_out_pos, void* d_out_vel);
int ocean_buoyancy_bodies_flow(ocean_t* ctx, const ocean_surface* s, const ocean_buoyancy* b, const ocean_body* bodies, uint32_t count,
                               float* out_force /* 4 * count */, float* out_torque /* 4 * count */);
int ocean_buoyancy_bodies_flow_device(ocean_t* ctx, const ocean_surface* s, const ocean_buoyancy* b, const void* d_bodies, uint32_t count,
                                      void* d_out_force, void* d_out_torque);

/* ---- spray emitters: the breaking vertices of a window, compacted into an ordered list ------------------------------------------------
 * Every call above answers a question about points the caller already knows.  Spray, splash sounds, mist and whitecap decals ask the
 * opposite one: WHERE on the surface is something happening in this frame?  ocean_emit_spray walks a window of the cascade vertex stage's
 * grid on the device, keeps the vertices where the surface is breaking and writes them as a short list -- a few hundred rows instead of the
 * (grid_size+1)^2 float4 a caller would otherwise copy out of ocean_displace_grid_cascades and test on the host.  Per-frame order:
 * frame -> ocean_emit_spray(_device) -> the particle system.  The list is in ascending lattice index and the same bits on every run.
 * A vertex is evaluated in this order; fp32 throughout, no contraction (tests/spray.py repeats it step for step):
 *   Vertex      lattice index i = 0 .. nx*ny - 1 of the window is grid vertex xi = ix0 + i % nx, yi = iy0 + i / nx (int32; the sums wrap).
 *               It is evaluated exactly as ocean_displace_grid_cascades evaluates vertex (xi, yi) for the tiles, grid_size, vertex_distance
 *               and uv_scales of `s`:  px = (float)xi * vertex_distance,  u = (float)(xi + half) / (float)grid_size  (half = grid_size / 2,
 *               an integer division; pz, v likewise from yi), every sample and sum in that call's order.  The window may lie outside
 *               -half .. grid_size - half: REPEAT addressing makes the grid endless.  s->choppy and s->iterations are unused.
 *   J           from the mode recorded for the frame that wrote the maps, as ocean_update_foam takes it; d, sl = the samples of cascade
 *               c's displacement and normal map at (u, v) * uv_scales[c]:
 *                 OCEAN_MODE_JACOBIAN frame:  J_c = d.w
 *                 OCEAN_MODE_FULL7 frame:     J_c = (1.0f + lam_c * sl.z) * (1.0f + lam_c * sl.w), lam_c the lambda of tile c's frame
 *                 CHOPPY5 / HEIGHT1 frame:    OCEAN_E_UNSUPPORTED
 *               J = fminf over the cascades in cascade order, from FLT_MAX: the counterpart of w = min_c D_c.w and of the foam query's max.
 *   V           the twin rule of ocean_query_velocity.  A set of which no tile has a twin: V = (0.0f, 0.0f, 0.0f), and min_rise is not
 *               looked at.  A fully and consecutively twinned set: V = sum_c (d'.x, d'.y * A'_c, d'.z) from 0.0f in cascade order, d' the
 *               sample of twin c's displacement map at the vertex's (u, v) * uv_scales[c].  A partly twinned set: OCEAN_E_INVALID.
 *   Predicate   the vertex is listed where all of these hold:
 *                 J < threshold                                        (a NaN never passes)
 *                 with twins: V.y >= min_rise
 *                 (h & ((1u << thin_log2) - 1u)) == 0,  h = hash(i + salt) in uint32 with wraparound,
 *                 hash(x):  x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16
 *               thin_log2 = k keeps about one breaking vertex in 2^k; a salt that changes per frame moves the kept ones about.
 *   Output      the passing vertices in ascending i; row r of the list is
 *                 out_pos[r]   = (px + dx, 0.0f + dy, pz + dz, strength),  strength = fminf(fmaxf((threshold - J) * gain, 0.0f), 1.0f)
 *                 out_vel[r]   = (V.x, V.y, V.z, J)
 *                 out_index[r] = i
 *               with (dx, dy, dz) the vertex stage's summed displacement.  Only rows 0 .. min(total, capacity) - 1 are written; later rows
 *               keep what they held.  out_count = (total: every passing vertex, not capped;  rows written = min(total, capacity)) is
 *               always written, also with capacity == 0 -- the way to size a list: the outputs are then not looked at and may be NULL.
 * The compaction is three launches whatever the window (count per chunk of 1024 indices, a scan of the chunk counts by one workgroup,
 * scatter); no launch waits on another workgroup and there are no atomics, which is what fixes the order and the bits.  Its scratch (132
 * bytes per chunk) is owned by the context, grows on demand like the staging buffer and goes with ocean_destroy.
 * Both calls read the most recently enqueued frame (caller-bound or imported output where it is) and are stream-ordered behind it like
 * ocean_query_surface; the fault rule of ocean.h holds unchanged.  ocean_emit_spray: host arrays out_pos[4*capacity], out_vel[4*capacity],
 * out_index[capacity], out_count[2], staged through the context's staging buffer; returns when the results are there.
 * ocean_emit_spray_device: the same arrays in device memory of the context's device (out_pos / out_vel 16-byte, out_index / out_count
 * 4-byte aligned); enqueued behind the most recent frame on its stream (ocean_stream), returns at once.
 * Errors: those of ocean_query_surface for the surface (iterations are not looked at); additionally OCEAN_E_INVALID for a NULL p, nx or ny
 * equal to 0 or nx * ny > 2^24, thin_log2 > 16, a threshold, gain or min_rise that is not finite, gain < 0, a NULL output with
 * capacity > 0, a NULL out_count; OCEAN_E_NOT_READY without Prepare or frame.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                                        */
typedef struct ocean_spray {
    float    threshold;                /* a vertex breaks where J < threshold                            default 0.3 */
    float    gain;                     /* strength = clamp((threshold - J) * gain, 0, 1); >= 0           default 2.5 */
    float    min_rise;                 /* with twins: also requires V.y >= min_rise (m/s); finite        default 0   */
    uint32_t thin_log2;                /* 0 .. 16: keep a breaking vertex only where the low thin_log2 bits of hash(i + salt) are 0 */
    uint32_t salt;                     /* changes which vertices the thinning keeps; vary it per frame */
    int32_t  ix0, iy0;                 /* window of grid vertices: xi = ix0 + i % nx, yi = iy0 + i / nx, i = 0 .. nx*ny - 1 */
    uint32_t nx, ny;                   /* 1 <= nx, ny;  nx * ny <= 1 << 24 */
} ocean_spray;

void ocean_default_spray(ocean_spray* p);   /* the defaults above, no thinning; the grid is not known here: nx = ny = 0, the caller sets the window */
int ocean_emit_spray(ocean_t* ctx, const ocean_surface* s, const ocean_spray* p, uint32_t capacity,
                     float* out_pos /* 4 * capacity */, float* out_vel /* 4 * capacity */, uint32_t* out_index /* capacity */,
                     uint32_t out_count[2] /* total breaking (not capped), rows written = min(total, capacity) */);
int ocean_emit_spray_device(ocean_t* ctx, const ocean_surface* s, const ocean_spray* p, uint32_t capacity,
                            void* d_out_pos, void* d_out_vel, void* d_out_index, void* d_out_count);

/* ---- empirical wave spectra: JONSWAP / TMA, directional spreading, wavenumber bands ---------------------------------------
 * ocean_params describes the reference's Phillips sea, whose phillips_const is not a physical scale.  ocean_set_spectrum replaces a
 * tile's spectrum by an empirical one given as a sea state -- wind speed at 10 m (ocean_params.wind_speed, U), fetch F, water depth --
 * with heights in metres, and/or restricts the tile to a wavenumber band, so that the tiles of a cascade set carry disjoint bands
 * instead of counting the wavenumbers they share twice.  After Horvath, "Empirical directional wave spectra for computer graphics"
 * (2015).  Initialisation-time work: the frame kernels and every buffer are unchanged, and a context that never calls this (or sets
 * ocean_default_spectrum) prepares the same bits as before.
 * ocean_set_spectrum  host state only, like ocean_set_params: in effect from the next ocean_prepare, kept across ocean_prepare and
 *          ocean_set_tile_size.  Wind direction and speed come from the tile's ocean_params; the empirical kinds ignore phillips_const
 *          and damping.  With OCEAN_SPECTRUM_PHILLIPS the sea is the one ocean_params describes and only the band applies.  A twin has
 *          no spectrum of its own: its explicit index gives OCEAN_E_INVALID, OCEAN_ALL_TILES skips twins, ocean_get_spectrum(twin)
 *          returns its source's; Prepare derives the twin from its source's new spectrum.
 * The spectrum   For a bin with k > 1e-5f: k, ux, uz and the unit wind vector (wx, wy) are the floats the Phillips path forms (k =
 *          sqrtf(kx*kx + kz*kz), u = k-vector * (1.0f / sqrtf(kx*kx + kz*kz))), promoted to double; everything below is in double, g = 9.81
 *          (the test suite repeats it step for step).
 *   Frequency    w and dw/dk, continuous (not the quantised omega of the frames, which stays what it is), from ocean_set_dispersion:
 *                  deep            w = sqrt(g k)                 dw/dk = 0.5 sqrt(g / k)
 *                  finite depth D  w = sqrt(g k tanh(k D))       dw/dk = g (tanh(k D) + k D (1 - tanh(k D)^2)) / (2 w)
 *                  capillary L     w = sqrt(g k (1 + k^2 L^2))   dw/dk = g (1 + 3 k^2 L^2) / (2 w)
 *   Peak, level  resolved on the host at Prepare unless given (alpha / peak_omega != 0):
 *                  PM              alpha = 0.0081                         wp = 0.855 g / U                   gamma = 1
 *                  JONSWAP, TMA    alpha = 0.076 (U^2 / (F g))^0.22       wp = 22 (g^2 / (U F))^(1/3)        gamma as given
 *   S(w)         alpha g^2 w^-5 exp(-1.25 (wp / w)^4) gamma^r,  r = exp(-(w - wp)^2 / (2 sigma^2 wp^2)),  sigma = 0.07 for w <= wp, else 0.09
 *                TMA multiplies by the Kitaigorodskii factor (Thompson-Vincent), wh = w sqrt(depth / g):
 *                  0.5 wh^2 for wh <= 1;  1 - 0.5 (2 - wh)^2 for 1 < wh < 2;  1 otherwise
 *   Spreading    c = clamp(ux wx + uz wy, -1, 1);  D = Q(s) ((1 + c) / 2)^s,
 *                Q(s) = exp((2 s - 1) ln 2 - ln pi + 2 lgamma(s + 1) - lgamma(2 s + 1))      (the integral of D over direction is 1)
 *                  OCEAN_SPREAD_COS2S        s = spread_s
 *                  OCEAN_SPREAD_HASSELMANN   x = w / wp:  s = 6.97 x^4.06 for x <= 1.05,  else 9.77 x^mu,  mu = -2.33 - 1.45 (U wp / g - 1.17)
 *                then s = s + 16 tanh(wp / w) swell^2
 *   Amplitude    P = S D (dw/dk) / k (2 pi / L)^2,  L the tile length;  sp = (float)(scale * sqrt(P)), rounded once; then in fp32, no
 *                contraction, as the Phillips path:  h0 = ((s * g.x) * sp, (s * g.y) * sp),  s = 1.0f / sqrtf(2.0f),  g the bin's draw
 *   Band         h0 = (0, 0) unless k_min <= k and (k_max == 0 or k < k_max), compared in fp32; for every kind, Phillips included
 *          omega, the draws (generated or injected) and DC are what they are without this call.
 * Normalisation  the frames animate h~ = 2 Re(h0 e^{i w t}) and take the real part of the transform, so the expected height variance
 *          is sum |h0|^2 and E|h0|^2 = P; with dk = 2 pi / L, sum P is a Riemann sum of m0 = integral of S dw.  Heights, and the
 *          amplitude A of a frame, are in metres.
 * ocean_get_spectrum  what was set, with alpha / peak_omega as the most recent ocean_prepare resolved them (as set before the first).
 * ocean_spectrum_moments  synchronises and returns, for whatever the tile's prepared spectrum buffer holds (a twin's: the derivative
 *          spectrum):  out[0] = sum |h0|^2 (m0 in m^2: the significant wave height is Hs = 4 sqrt(out[0])),  out[1] = sum k |h0|^2,
 *          out[2] = sum k^2 |h0|^2 (the expected mean-square slope); k the bin's fp32 wavenumber.  Summed on the device in double in a
 *          fixed order: the same spectrum gives the same bits on every call.
 * Errors: OCEAN_E_INVALID for a NULL argument, a tile outside the batch, an unknown kind or spreading, a non-finite field; fetch,
 * gamma, spread_s or scale <= 0; depth <= 0 with TMA; swell outside [0, 1]; a negative alpha, peak_omega, k_min or k_max; k_max != 0
 * with k_max <= k_min.  ocean_spectrum_moments: OCEAN_E_NOT_READY before Prepare.  (An addition to ABI version 5.)               */
enum { OCEAN_SPECTRUM_PHILLIPS = 0, OCEAN_SPECTRUM_PM = 1, OCEAN_SPECTRUM_JONSWAP = 2, OCEAN_SPECTRUM_TMA = 3 };
enum { OCEAN_SPREAD_COS2S = 0, OCEAN_SPREAD_HASSELMANN = 1 };
typedef struct ocean_spectrum {
    uint32_t kind, spreading;
    float fetch;                       /* m; JONSWAP / TMA                                            default 100e3 */
    float gamma;                       /* peak enhancement; JONSWAP / TMA                             default 3.3   */
    float depth;                       /* m, > 0; TMA only                                            default 20    */
    float spread_s;                    /* exponent s of OCEAN_SPREAD_COS2S, > 0                       default 8     */
    float swell;                       /* 0 .. 1, adds 16 tanh(wp / w) swell^2 to s                   default 0     */
    float alpha;                       /* 0 = derive from wind and fetch */
    float peak_omega;                  /* rad/s, 0 = derive */
    float k_min, k_max;                /* band in rad/m: h0 = 0 unless k_min <= k < k_max; k_max == 0: no upper limit.  EVERY kind */
    float scale;                       /* multiplies the amplitude sqrt(P) of an empirical kind       default 1     */
} ocean_spectrum;

void ocean_default_spectrum(ocean_spectrum* s);     /* Phillips, COS2S, the defaults above, band [0, inf): the sea of ocean_params alone */
int ocean_set_spectrum(ocean_t* ctx, uint32_t tile /* or OCEAN_ALL_TILES */, const ocean_spectrum* s);
int ocean_get_spectrum(const ocean_t* ctx, uint32_t tile, ocean_spectrum* s);
int ocean_spectrum_moments(ocean_t* ctx, uint32_t tile, double out[3]);

/* ---- Gerstner proxy: a tile's strongest waves as rows, evaluated analytically at any point and any time --------------------------------
 * The reference's to-do "Gerstner waves model" (README.md:37-44).  Every call above reads the maps of the most recently enqueued frame; none
 * can answer "how high is the water at (x, z) two seconds from now?" (a helmsman, a projectile's landing point, a netcode rollback) without
 * spending a frame, none evaluates the surface between texels other than bilinearly, and a process without the maps (a game server) cannot
 * reproduce the sea at all.  The sea is a finite sum of standing trochoidal waves, one per spectrum bin, and for a wind sea a few hundred
 * bins carry almost all of the variance: a tile's WAVE SET is the list of its K strongest bins, and these calls evaluate such a list -- the
 * surface the cascade vertex stage draws, truncated to K waves per tile.  Per-Prepare order: ocean_prepare -> ocean_extract_waves per tile.
 * Per frame: nothing; ocean_eval_waves / ocean_query_waves at any t, with or without frames.
 * The row      ocean_wave, 12 words: one bin of the tile's N x N lattice.  A CPU-only process evaluates rows like this, for a tile of N
 *          texels whose position in tile lengths is (X, Z) (X = x / L for a tile that starts at the origin; the calls below form it from
 *          the mesh, see there):
 *            c(t)  = 2 (re cos(omega t) - im sin(omega t))          (the bin's h~, exactly real: the mirror bin is folded in)
 *            theta = 2 pi (jx X + jz Z)                              (the reference's (-1)^(m+n) is the N/2 in jx = q - N/2)
 *            h    += c cos theta
 *            Dx   += ux c sin theta        Dz   += uz c sin theta    (the displacement map's x, z before lambda)
 *            sx   -= kx c sin theta        sz   -= kz c sin theta    (the normal map's x, y)
 *            dxDx += kx ux c cos theta     dzDz += kz uz c cos theta (the normal map's z, w)
 *          At X = n / N, Z = m / N the sum over ALL bins is texel (m, n) of the frame's maps (with disp.y * A the height).
 * Extraction   ocean_extract_waves reads the tile's prepared fp32 spectrum and omega -- what ocean_read_spectrum returns; never the
 *          half-precision copy the frames may read -- and lists the strongest bins: power p = re*re + im*im in fp32 without contraction;
 *          candidates are the bins with p > 0 (a NaN never passes); rank by p descending, ties by bin ascending; rows 0 .. count-1 are the
 *          list in rank order, count = min(max_waves, candidates), 1 <= max_waves <= 4096.  Every field is a function of the spectrum
 *          alone, the same bits on every run (tests/waves.py restates them).  out_energy[0] = the sum over the rows, in list order, of
 *          (double)re*(double)re + (double)im*(double)im: divide by ocean_spectrum_moments' out[0] for the captured share of the variance.
 *          The list stays on the device as the tile's wave set (one per tile; a later call replaces it; no candidate: no set) together
 *          with N and the tile length it was made for.  The call synchronises, as ocean_spectrum_moments does.  On the device: a radix
 *          select over (power bits, ~bin) keys -- at most eight 8-bit histogram passes, four or fewer unless a tie straddles rank K --,
 *          one pass that collects the survivors, the host orders those <= 4096.  A twin tile lists its derivative spectrum: its set is
 *          the velocity proxy (tile length, lambda and time offset are its source's, as for its frames).
 *          ocean_prepare and ocean_set_tile_size drop every set: the sea they belonged to is gone.
 * Hand-made    ocean_set_waves uploads rows as given (artist-made swell, crafted sets): every float finite and jx, jz in -N/2 .. N/2-1,
 *          checked on the host, otherwise OCEAN_E_INVALID and the old set stays; bin and reserved are not looked at; count == 0 drops the
 *          set.  ocean_get_waves copies the set out (synchronises; rows may be NULL to ask for the count).
 * Evaluation   ocean_eval_waves is the FORWARD evaluation at rest points (x, z) (s->iterations unused); it needs Prepare and a set for each
 *          of the tiles first_tile .. first_tile+cascades-1, no frame and no map.  fp32; lam_c is the tile's lambda at the time of the call,
 *          N and L_c the ones the set recorded.  Per rest point and cascade c:
 *            tt = t + the tile's time offset (ocean_set_time_offsets), one addition as in the frames
 *            per wave: wt = omega * tt (ONE fp32 multiply), c = 2 (re cos wt - im sin wt) with the frames' sine and cosine
 *            (u, v) as ocean_query_surface forms them;  tx = (u * uv_scales[c]) * (float)N - 0.5f (the sampler's texel coordinate);
 *            X = tx * (1.0f / N);  fX = X - floorf(X);  Z, fZ likewise from v      -- at a texel centre exactly the texel's lattice point
 *            per wave: a = (float)jx * fX,  b = (float)jz * fZ,  ph = (a - floorf(a)) + (b - floorf(b)) turns,  theta = 2 pi ph
 *            the seven sums above
 *          Over the cascades, in cascade order:
 *            P = (x + sum_c lam_c Dx_c,  sum_c h_c,  z + sum_c lam_c Dz_c),   S = sum_c (sx, sz, dxDx, dzDz),
 *            J = min_c (1 + lam_c dxDx_c)(1 + lam_c dzDz_c), from FLT_MAX
 *            out_pos = (P, J),   out_nrm = (normalize(-S.x / (1 + choppy S.z), 1, -S.y / (1 + choppy S.w)), 0): the vertex stage's formula
 *          Precision: sine and cosine cannot be restated bit for bit and the ORDER OF THE SUM is not part of the contract, so the results
 *          are held to a derived bound, not to bits: each of the seven sums of a cascade is within
 *            2^-21 * sum_j a_j g_j (|jx_j| + |jz_j| + 4 + K/8),   a_j = 2 (|re_j| + |im_j|),  g_j = 1, |ux|, |uz|, |kx|, |kz|, |kx ux|, |kz uz|
 *          of the exact sum of the rows with c_j rounded as above (tests/waves.py has the derivation and what the outputs add to it).
 *          Same rows and arguments give the same bits on every run and in both forms.
 * The inverse  ocean_query_waves is ocean_query_surface's diagonal Newton iteration on that evaluation: r_0 = q; for k < K (= s->iterations,
 *          0 means 8):  e = P(r_k).xz - q,
 *            Jx = 1 + sum_c lam_c dxDx_c * s_c * L_c / (grid_size * vertex_distance),   Jz likewise from dzDz
 *          (dxDx is per ocean metre of tile c and one mesh metre is s_c * L_c / (grid_size * vertex_distance) of them -- the map query's
 *          factor; it is 1 where the mesh spans one tile), |J| clamped to >= 0.1 as there, r_{k+1} = r_k - (e.x / Jx, e.z / Jz);
 *            out_pos = (P(r_K), J),   out_nrm = (n(r_K), |P(r_K).xz - q|)
 *          With t this is the call that answers "where will the water be".
 * Host / device forms as ocean_sample_surface_lod / _device: the host form stages [outputs | 8-byte inputs] in the context's buffer and
 * returns when the results are there; the device form (xz 8-byte, outputs 16-byte aligned) is enqueued on the consumers' stream
 * (ocean_stream), ordered among the other consumer calls, and returns at once.
 * How many waves: K is chosen from the captured share out_energy / m0 -- 0.9 of the variance is 0.95 of the rms height.  Memory:
 * tiles * 4096 * 48 bytes of sets, 1.5 MB for the evaluation's table (8 cascades * 4096 waves * 48 bytes) and 50 KB of selection scratch, allocated on first use, freed by ocean_destroy.
 * Not covered: merging a bin with its point mirror into one row (on the Nyquist row and column the two are not mirror images off the
 * lattice, so rows stay single bins and a caller picks K accordingly); waves off the tile's lattice; a vertex-stage or buoyancy form of the
 * proxy; any accuracy claim for contexts that run the fp16 spectrum (the sets are made from the fp32 one).
 * Errors: OCEAN_E_INVALID for a NULL context, count pointer, surface; a tile outside the batch; max_waves 0 or above 4096; a count above
 * 4096 or a row that fails the check above; the invalid ocean_surface cases of ocean_query_surface; a t that is not finite; a NULL array
 * with points > 0.  OCEAN_E_NOT_READY before Prepare, and for ocean_get_waves and the evaluations without a set (for every tile of the
 * surface).  points == 0 returns OCEAN_OK before the pointers are looked at.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                                            */
typedef struct ocean_wave {            /* 12 words, 48 bytes */
    int32_t  jx, jz;                   /* lattice indices: bin column q = jx + N/2, row p = jz + N/2; -N/2 .. N/2-1 */
    float    kx, kz;                   /* the tile's fp32 wavenumbers k1d[q], k1d[p] */
    float    ux, uz;                   /* kx * r, kz * r, r = 1.0f / sqrtf(kx*kx + kz*kz); (0, 0) where sqrtf(...) <= 1e-5f */
    float    re, im;                   /* h0 of the bin */
    float    omega;                    /* the bin's quantised fp32 omega */
    uint32_t bin;                      /* p * N + q in the layout ocean_read_spectrum returns */
    float    reserved[2];              /* 0 */
} ocean_wave;

int ocean_extract_waves(ocean_t* ctx, uint32_t tile, uint32_t max_waves, ocean_wave* out /* max_waves rows; may be NULL */,
                        uint32_t* out_count, double* out_energy /* may be NULL */);
int ocean_set_waves(ocean_t* ctx, uint32_t tile, const ocean_wave* rows, uint32_t count);
int ocean_get_waves(ocean_t* ctx, uint32_t tile, ocean_wave* rows /* may be NULL */, uint32_t* count);
int ocean_eval_waves(ocean_t* ctx, const ocean_surface* s, float t, const float* xz /* 2 * points */, uint32_t points,
                     float* out_pos /* 4 * points */, float* out_nrm /* 4 * points */);
int ocean_eval_waves_device(ocean_t* ctx, const ocean_surface* s, float t, const void* d_xz, uint32_t points,
                            void* d_out_pos, void* d_out_nrm);
int ocean_query_waves(ocean_t* ctx, const ocean_surface* s, float t, const float* xz /* 2 * points */, uint32_t points,
                      float* out_pos /* 4 * points */, float* out_nrm /* 4 * points */);
int ocean_query_waves_device(ocean_t* ctx, const ocean_surface* s, float t, const void* d_xz, uint32_t points,
                             void* d_out_pos, void* d_out_nrm);

/* ---- fragment stage: Preetham sky and the reference's water colour ---------------------------------------------------------------------
 * Everything above produces what the reference's VERTEX shader produces; these calls are its fragment stage (SkyPreetham::Update,
 * SkyPreetham.frag, WaterSurfaceMesh.frag) as a pure per-point function: no camera model, no march, no image geometry.  They take the
 * (position, normal) rows ocean_displace_grid*, ocean_query_surface, ocean_raycast_surface, ocean_sample_surface_lod and ocean_eval_waves
 * write and return radiance.  Per-frame order: frame -> ocean_displace_grid* -> ocean_shade_grid; or ocean_raycast_surface(_device) ->
 * ocean_shade_points(_device) with foam_white = 0 (a hit's w is t, not the Jacobian): a render in two calls.
 * Sky, host   ocean_sky_coefficients restates SkyPreetham::Update.  A pure host function: no context.  turbidity T and sun_dir are fp32
 *          inputs; everything below is evaluated in double and each output is rounded to fp32 once.
 *            sun = sun_dir / |sun_dir|;   thetaSun = acos(max(sun.y, 0))
 *            A = ( 0.1787 T - 1.4630, -0.0193 T - 0.2592, -0.0167 T - 0.2608)      (per channel of Yxy)
 *            B = (-0.3554 T + 0.4275, -0.0665 T + 0.0008, -0.0950 T + 0.0092)
 *            C = (-0.0227 T + 5.3251, -0.0004 T + 0.2125, -0.0079 T + 0.2102)
 *            D = ( 0.1206 T - 2.5771, -0.0641 T - 0.8989, -0.0441 T - 1.6537)
 *            E = (-0.0670 T + 0.3703, -0.0033 T + 0.0452, -0.0109 T + 0.0529)
 *            chi = (4/9 - T/120) (pi - 2 thetaSun);   Yz = (4.0453 T - 4.9710) tan(chi) - 0.2155 T + 2.4192
 *            xz = ( 0.00165 th^3 - 0.00375 th^2 + 0.00209 th          ) T^2 + (-0.02903 th^3 + 0.06377 th^2 - 0.03202 th + 0.00394) T
 *               + ( 0.11693 th^3 - 0.21196 th^2 + 0.06052 th + 0.25886)                                              (th = thetaSun)
 *            yz = ( 0.00275 th^3 - 0.00610 th^2 + 0.00317 th          ) T^2 + (-0.04214 th^3 + 0.08970 th^2 - 0.04153 th + 0.00516) T
 *               + ( 0.15346 th^3 - 0.26756 th^2 + 0.06670 th + 0.26688)
 *            ZenithLum = (Yz, xz, yz);   ZeroThetaSun = (1 + A exp(B / cos 0)) (1 + C exp(D thetaSun) + E cos^2 thetaSun)
 *          ocean_sky_coeffs has the layout of the uniform block the reference uploads (SkyPreetham::Props: a float3 and the turbidity, then
 *          seven float3 padded to 16 bytes, 128 bytes): a Vulkan host fills its UBO from it.  The padding words are 0.
 * Sky, device  ocean_sky_radiance evaluates SkyPreetham.frag for `count` view directions; fp32, the device's full-precision expf / acosf /
 *          cosf; the optics are held to a derived bound (tests/shading.py), not to bits.  d = dir / |dir|, then SKY(d):
 *            thetaView = acosf(clamp(d.y, 0, 1));   cg = clamp(dot(sun, d), 0, 1);   gamma = acosf(cg)
 *            (the upper clamp is ours: two fp32 unit vectors can have a dot product of 1 + an ulp, and acosf of that is NaN)
 *            F = (1 + A expf(B / (cosf(thetaView) + 1e-3f))) (1 + C expf(D gamma) + E cosf(gamma)^2)        (per channel; kBias = 1e-3f)
 *            (Y, x, y) = ZenithLum (F / ZeroThetaSun)          (the quotient ZenithLum / ZeroThetaSun is formed once, on the host)
 *            X = x (Y / y),  Z = (1 - x - y) (Y / y)
 *            L = ( 2.3706743 X - 0.9000405 Y - 0.4706338 Z,            (CIE-E, the shader's XYZ * M)
 *                 -0.5138850 X + 1.4253036 Y + 0.0885814 Z,
 *                  0.0052982 X - 0.0146949 Y + 1.0093968 Z)
 *            disk = smoothstep(0.997f, 1.0f, cg):  s = clamp((cg - 0.997f) / (1.0f - 0.997f), 0, 1),  disk = s s (3 - 2 s)
 *          out = (L 0.05f + (sun_color disk) L,  disk), not tone-mapped.  Needs a context for the stream and the staging only: neither
 *          Prepare nor a frame.  dirs[3*count] are 4-byte aligned, out[4*count] 16-byte aligned in the device form.
 * Seabed   ocean_eval_seabed evaluates the reference's procedural seabed (WaterSurfaceMesh.frag: TerrainNormal, TerrainColor) at terrain
 *          points p = (x, z): out = (n.x, n.y, n.z, colour factor).  fp32 throughout, NO contraction, fract(a) = a - floorf(a), in exactly
 *          this order (tests/shading.py repeats it step for step in float32 and the device is held to it in every bit):
 *            hash1(ix, iy):  jx = 50.0f * fract(ix * 0.31830987f);  jy = 50.0f * fract(iy * 0.31830987f)       (0.31830987f = (float)(1/pi))
 *                            = fract((jx * jy) * (jx + jy))
 *            noise(px, py):  ix = floorf(px), fx = px - ix;  iy, fy likewise
 *                            ux = ((fx * fx) * fx) * (fx * (fx * 6.0f - 15.0f) + 10.0f);  uy likewise                 (quintic)
 *                            a = hash1(ix, iy), b = hash1(ix + 1.0f, iy), c = hash1(ix, iy + 1.0f), d = hash1(ix + 1.0f, iy + 1.0f)
 *                            = -1.0f + 2.0f * (((a + (b - a) * ux) + (c - a) * uy) + ((((a - b) - c) + d) * ux) * uy)
 *            fbm4(px, py):   v = 0.0f, g = 0.5f; four times:  v = v + g * noise(px, py);  g = g * 0.5f;
 *                            (px, py) = (1.6f * px + 1.2f * py,  -1.2f * px + 1.6f * py)
 *            H(x, z)       = 0.0f - 8.0f * fbm4(z * 0.02f, x * 0.02f)                                        (the shader's p.yx)
 *            factor        = fminf(fmaxf(fbm4((z * 0.02f) * 2.0f, (x * 0.02f) * 2.0f), 0.6f), 0.9f)
 *            e = 1e-4f;  nx = H(x - e, z) - H(x + e, z);  ny = 10.0f * e;  nz = H(x, z - e) - H(x, z + e)
 *            len = sqrtf((nx * nx + ny * ny) + nz * nz);  n = (nx / len, ny / len, nz / len)
 *          It is its own entry point because it is the one part of the fragment stage that CAN be held to bits and the one that cannot be
 *          compared with float64 at all: hash1 resolves 2^-7 at its largest arguments, and a few hundred metres out e is below the ulp of
 *          p, where the finite difference is 0 and the normal (0, 1, 0).  A renderer that draws the seabed takes its colour from here:
 *          factor * terrain_color.  xz[2*count] 8-byte, out 16-byte aligned in the device form.  No Prepare, no frame.
 * Water    ocean_water is the reference's WaterSurfaceUBO without the sky, and four switches.  ocean_shade_points, per point, in the
 *          shader's order; fp32, may contract, held to the derived bound:
 *            d = normalize(pos.xyz - cam_pos)       (the ray goes to the UNRAISED position, as the reference's main does)
 *            n = normalize(nrm.xyz);   p_w = (pos.x, pos.y + height, pos.z);   V = -d
 *            r = d - 2 dot(n, d) n;    S = L 0.05f + disk L  with (L, disk) = SKY(r), r as it is: the water shader's SkyLuminance, whose
 *                                      disk is not multiplied by sun_color
 *            L_a = sky_intensity max(dot(n, sun), 0) S
 *            Hw = normalize(sun + V);  L_s = sun_intensity (specular_intensity clamp(powf(max(dot(n, Hw), 0), specular_highlights), 0, 1)) S
 *            refr = GLSL refract(-sun, n, eta), eta = 1 / 1.33477:  c = dot(n, -sun),  k = 1 - eta^2 (1 - c^2),
 *                                      refr = eta (-sun) - (eta c + sqrtf(k)) n, or 0 where k < 0        (the SUN's ray, not the view's)
 *            t_g = -p_w.y / refr.y  (the plane y = 0);   p_g = p_w + t_g refr
 *            (n_g, factor) = the seabed above at (p_g.x, p_g.z)  (OCEAN_SEABED_REFERENCE)  or  ((0, 1, 0), seabed_factor)  (OCEAN_SEABED_FLAT)
 *            L_g = factor terrain_color dot(n_g, -refr)
 *            L_df0 = ((0.33 backscatter) / absorb) ((pi L_a) (1 / pi))                        (the quotient is formed once, on the host)
 *            Att(dist, depth) = expf(-(absorb 0.1) dist - (scatter 0.1) depth)                (the 0.1-scaled coefficients likewise)
 *            L_u = Att(t_g, 0) L_g + (1 - Att(t_g, |p_w.y - p_g.y|)) L_df0
 *            F_r, OCEAN_FRESNEL_REFERENCE: the shader as shipped.  ti = dot(n, V) and tt = dot(-n, refr) -- two COSINES, the second of the
 *                   sun's refraction angle -- go into a formula written for angles:  ti <= 1e-5f -> ((ior - 1) / (ior + 1))^2 (rounded once
 *                   on the host), otherwise 0.5 (t1^2 + t2^2), t1 = sinf(ti - tt) / sinf(ti + tt), t2 = tanf(ti - tt) / tanf(ti + tt)
 *            F_r, OCEAN_FRESNEL_PHYSICAL:  ci = dot(n, V);  ci <= 0 -> 1;  ct = sqrtf(1 - (1 - ci^2) / ior^2),
 *                   rs = (ci - ior ct) / (ci + ior ct),  rp = (ior ci - ct) / (ior ci + ct),  F_r = 0.5 (rs^2 + rp^2)
 *            colour = F_r (L_s + L_a) + (1 - F_r) L_u;   foam_white and pos.w < 0 -> colour = (1, 1, 1)     (the reference's main)
 *            out_rgba = (colour, 1.0f);   tonemap -> 1 - expf(-2 c) on all four channels
 *            out_aux  = (p_g.x, p_g.z, t_g, F_r): the seabed hit and the reflectance (may be NULL)
 *          Supported range: the row of a point is unspecified where the restated colour is not finite -- a zero normal, pos == cam_pos,
 *          refr.y >= 0, a non-finite input -- and such a point disturbs no other row.
 * The grid ocean_shade_grid shades the context's vertex-stage output -- the buffers ocean_device_grid hands out, from the most recent
 *          ocean_displace_grid, _cascades or _lod -- into a context-owned (grid_size+1)^2 float4 image, stream-ordered behind that vertex
 *          stage, with the kernel of ocean_shade_points: the same grid through ocean_shade_points_device gives the same bits.  The image
 *          grows on demand (a growth that fails leaves nothing behind) and goes with ocean_destroy.  ocean_read_shaded copies it out
 *          (synchronises); ocean_device_shaded hands out the pointer (NULL while there is none) and the vertex count.
 *          OCEAN_E_NOT_READY when no grid has been displaced since ocean_prepare, and for the read without a shaded image.
 * Host / device forms, staging, stream order (ocean_stream) and alignment as ocean_sample_surface_lod / _device: the host forms stage
 * [outputs | inputs] in the context's buffer and return when the results are there; the device forms are enqueued and return at once.
 * Errors: OCEAN_E_INVALID for a NULL context, structure or -- with count > 0 -- array (out_aux excepted); a field that is not finite; a
 * zero sun vector; a turbidity outside [1, 10]; absorb <= 0; specular_highlights <= 0; an unknown fresnel or seabed.  count == 0
 * returns OCEAN_OK before the pointers are looked at.  The reference's three quirks are kept on purpose and named in INTEGRATION.md E12:
 * cosines passed as angles, the sun's refraction angle in Fresnel, the ray to the unraised position.
 * (An addition to ABI version 5: nothing of the existing entry points or structures changes.)                                            */
enum { OCEAN_FRESNEL_REFERENCE = 0, OCEAN_FRESNEL_PHYSICAL = 1 };
enum { OCEAN_SEABED_REFERENCE = 0, OCEAN_SEABED_FLAT = 1 };
typedef struct ocean_sky {
    float sun_dir[3];                  /* towards the sun; normalised by the call                     default (0, 0.5, 0.866) */
    float turbidity;                   /* 1 .. 10                                                     default 2.5 */
    float sun_color[3];                /*                                                             default (1, 1, 1) */
    float sun_intensity;               /*                                                             default 1 */
} ocean_sky;
typedef struct ocean_sky_coeffs {      /* 32 words, 128 bytes: SkyPreetham::Props as uploaded; every fourth word of the float3s is 0 */
    float sun_dir[3];                  /* normalised */
    float turbidity;
    float A[4], B[4], C[4], D[4], E[4];
    float zenith_lum[4];               /* (Y, x, y) of the zenith */
    float zero_theta_sun[4];
} ocean_sky_coeffs;
typedef struct ocean_water {
    float    cam_pos[3];               /*                                                             default (0, 60, 0) */
    float    height;                   /* of the water plane above the seabed's y = 0                 default 50 */
    float    absorb[3];                /* 1/m at 680 / 550 / 440 nm, > 0: Jerlov I                    default (0.420, 0.063, 0.019) */
    float    scatter[3];               /* b(514 nm) = 0.037 through (-0.00113 nm + 1.62517) / (-0.00113 * 514 + 1.62517) */
    float    backscatter[3];           /* 0.01829 scatter + 0.00006 */
    float    terrain_color[3];         /*                                                             default (0.964, 1.0, 0.824) */
    float    sky_intensity, specular_intensity, specular_highlights;      /* highlights > 0           default 1, 1, 32 */
    uint32_t fresnel;                  /* OCEAN_FRESNEL_*                                             default REFERENCE */
    uint32_t seabed;                   /* OCEAN_SEABED_*                                              default REFERENCE */
    float    seabed_factor;            /* colour factor of OCEAN_SEABED_FLAT                          default 0.75 */
    uint32_t foam_white;               /* pos.w < 0 paints (1, 1, 1); 0 for ray-cast hits             default 1 */
    uint32_t tonemap;                  /* 1 - exp(-2 c) on all four channels                          default 1 */
} ocean_water;

void ocean_default_sky(ocean_sky* s);
void ocean_default_water(ocean_water* w);
int ocean_sky_coefficients(const ocean_sky* s, ocean_sky_coeffs* out);
int ocean_sky_radiance(ocean_t* ctx, const ocean_sky* s, const float* dirs /* 3 * count */, uint32_t count, float* out /* 4 * count */);
int ocean_sky_radiance_device(ocean_t* ctx, const ocean_sky* s, const void* d_dirs, uint32_t count, void* d_out);
int ocean_eval_seabed(ocean_t* ctx, const float* xz /* 2 * count */, uint32_t count, float* out /* 4 * count */);
int ocean_eval_seabed_device(ocean_t* ctx, const void* d_xz, uint32_t count, void* d_out);
int ocean_shade_points(ocean_t* ctx, const ocean_sky* s, const ocean_water* w, const float* pos /* 4 * count */,
                       const float* nrm /* 4 * count */, uint32_t count, float* out_rgba /* 4 * count */, float* out_aux /* may be NULL */);
int ocean_shade_points_device(ocean_t* ctx, const ocean_sky* s, const ocean_water* w, const void* d_pos, const void* d_nrm,
                              uint32_t count, void* d_out_rgba, void* d_out_aux /* may be NULL */);
int ocean_shade_grid(ocean_t* ctx, const ocean_sky* s, const ocean_water* w);
int ocean_read_shaded(ocean_t* ctx, float* rgba /* 4 * vertices */);
int ocean_device_shaded(ocean_t* ctx, void** d_rgba, uint32_t* vertices);

#ifdef __cplusplus
}
#endif
#endif /* OCEAN_CONSUMERS_H_ */
