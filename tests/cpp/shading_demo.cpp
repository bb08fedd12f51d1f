// Drives the fragment stage through the C ABI (include/ocean_consumers.h) from a plain C++ host: Prepare, one frame, the vertex stage on a
// grid of the tile's size, then ocean_shade_grid with the reference's default sky and water -- the grid "as rendered" -- and the sky
// coefficients a Vulkan host would upload.  The image is written raw to the file named by the second argument as [vertices][4] float, so that
// the GPU test can compare it with the Python binding bit for bit.  Prints "N vertices checksum zenithY": the checksum is the sum of every
// channel in double.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ocean_consumers.h"

static int fail(const char* what, int rc)
{
    std::fprintf(stderr, "shading_demo: %s: %s\n", what, ocean_strerror(rc));
    return 3;
}

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 64;
    const char* out = argc > 2 ? argv[2] : nullptr;
    const float t = argc > 3 ? (float)std::atof(argv[3]) : 2.0f;
    ocean_sky sky;
    ocean_water water;
    ocean_sky_coeffs ubo;
    ocean_default_sky(&sky);
    ocean_default_water(&water);
    int rc = ocean_sky_coefficients(&sky, &ubo);        // host only: works before (and without) a context
    if (rc) return fail("ocean_sky_coefficients", rc);

    ocean_t* ctx = nullptr;
    if ((rc = ocean_create(&ctx, n, 1, 0))) return fail("ocean_create", rc);
    ocean_params p;
    ocean_default_params(&p);
    float amp = 0.0f;
    if ((rc = ocean_set_params(ctx, 0, &p)) || (rc = ocean_prepare(ctx, 42, nullptr)) || (rc = ocean_compute_waves(ctx, t, &amp)))
        return fail("frame", rc);
    if ((rc = ocean_displace_grid(ctx, 0, n, p.tile_length / (float)n, 1.0f, p.lambda))) return fail("ocean_displace_grid", rc);
    if ((rc = ocean_shade_grid(ctx, &sky, &water))) return fail("ocean_shade_grid", rc);
    uint32_t vertices = 0;
    if ((rc = ocean_device_shaded(ctx, nullptr, &vertices))) return fail("ocean_device_shaded", rc);
    std::vector<float> rgba((size_t)vertices * 4);
    if ((rc = ocean_read_shaded(ctx, rgba.data()))) return fail("ocean_read_shaded", rc);
    double sum = 0.0;
    for (float v : rgba) sum += (double)v;
    std::printf("%u %u %.9g %.9g\n", n, vertices, sum, (double)ubo.zenith_lum[0]);
    if (out) {
        FILE* f = std::fopen(out, "wb");
        if (!f) return 4;
        std::fwrite(rgba.data(), sizeof(float), rgba.size(), f);
        std::fclose(f);
    }
    ocean_destroy(ctx);
    return 0;
}
