// Drives the Gerstner proxy through the C ABI (include/ocean_consumers.h) from a plain C++ host, without a frame: Prepare, extract the K
// strongest waves of the tile, then ask where the water will be at time t at a jittered grid of world points (ocean_query_waves) and what the
// vertex stage would draw at the same points taken as rest points (ocean_eval_waves).  The results are written raw to the file named by the
// third argument as [count] ocean_wave rows, [points][2] float xz, then [points][4] float four times (query pos, query nrm, eval pos, eval
// nrm), so that the GPU test can compare them with the Python binding bit for bit.  Prints "N count share points".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ocean_consumers.h"

static int fail(const char* what, int rc)
{
    std::fprintf(stderr, "waves_demo: %s: %s\n", what, ocean_strerror(rc));
    return 3;
}

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 64;
    const uint32_t k = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 128;
    const char* out = argc > 3 ? argv[3] : nullptr;
    const float t = argc > 4 ? (float)std::atof(argv[4]) : 2.0f;
    ocean_t* ctx = nullptr;
    int rc = ocean_create(&ctx, n, 1, 0);
    if (rc) return fail("ocean_create", rc);
    ocean_params p;
    ocean_default_params(&p);
    p.phillips_const = 5e-11f;
    if ((rc = ocean_set_params(ctx, 0, &p)) || (rc = ocean_prepare(ctx, 42, nullptr))) return fail("prepare", rc);

    std::vector<ocean_wave> rows(k);
    uint32_t count = 0;
    double energy = 0.0, m[3] = {0.0, 0.0, 0.0};
    if ((rc = ocean_extract_waves(ctx, 0, k, rows.data(), &count, &energy)) || (rc = ocean_spectrum_moments(ctx, 0, m))) return fail("extract", rc);
    rows.resize(count);

    ocean_surface s = {};
    s.first_tile = 0; s.cascades = 1; s.grid_size = n;
    s.vertex_distance = p.tile_length / (float)n; s.choppy = p.lambda; s.iterations = 8;
    s.uv_scales[0] = 1.0f;
    const int side = 17;
    std::vector<float> xz;
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const unsigned h = (unsigned)(j * side + i) * 2654435761u;
            xz.push_back(-500.0f + ((float)i + (float)(h & 0xffff) / 65536.0f) * (1000.0f / side));
            xz.push_back(-500.0f + ((float)j + (float)(h >> 16) / 65536.0f) * (1000.0f / side));
        }
    const uint32_t points = (uint32_t)(xz.size() / 2);
    std::vector<float> qpos(4 * points), qnrm(4 * points), epos(4 * points), enrm(4 * points);
    if ((rc = ocean_query_waves(ctx, &s, t, xz.data(), points, qpos.data(), qnrm.data()))) return fail("ocean_query_waves", rc);
    if ((rc = ocean_eval_waves(ctx, &s, t, xz.data(), points, epos.data(), enrm.data()))) return fail("ocean_eval_waves", rc);
    std::printf("%u %u %.6f %u\n", n, count, energy / m[0], points);
    if (out) {
        FILE* f = std::fopen(out, "wb");
        if (!f) return 4;
        std::fwrite(rows.data(), sizeof(ocean_wave), rows.size(), f);
        std::fwrite(xz.data(), sizeof(float), xz.size(), f);
        for (const std::vector<float>* a : {&qpos, &qnrm, &epos, &enrm}) std::fwrite(a->data(), sizeof(float), a->size(), f);
        std::fclose(f);
    }
    ocean_destroy(ctx);
    return 0;
}
