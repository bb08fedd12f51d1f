// Drives WSTessendorf::QuerySurface (include/WSTessendorf.hpp) the way gameplay code would: Prepare, ComputeWaves, then one query
// for a set of world points.  The points are a fixed jittered grid over +-600 m; the results are written raw to the file named by
// the second argument as [points][2] float xz, [points][4] positions, [points][4] normals, so that the GPU test can compare them
// with the Python binding bit for bit.  Prints "N A points max_residual".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "WSTessendorf.hpp"

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : WSTessendorf::s_kDefaultTileSize;
    const char* out = argc > 2 ? argv[2] : nullptr;
    const float t = argc > 3 ? (float)std::atof(argv[3]) : 3.7f;
    try {
        WSTessendorf model(n, WSTessendorf::s_kDefaultTileLength);
        model.SetWindDirection(WSTessendorf::vec2(1.0f, 0.5f));
        model.SetWindSpeed(20.0f);
        model.SetLambda(-1.5f);
        model.Prepare(42);
        const float amp = model.ComputeWaves(t);

        const int side = 64;
        std::vector<WSTessendorf::vec2> xz;
        for (int j = 0; j < side; ++j)
            for (int i = 0; i < side; ++i) {
                const unsigned h = (unsigned)(j * side + i) * 2654435761u;
                const float jx = (float)(h & 0xffff) / 65536.0f, jz = (float)(h >> 16) / 65536.0f;
                xz.push_back(WSTessendorf::vec2(-600.0f + ((float)i + jx) * (1200.0f / side), -600.0f + ((float)j + jz) * (1200.0f / side)));
            }
        std::vector<WSTessendorf::vec4> positions, normals;
        model.QuerySurface(xz, positions, normals);
        float worst = 0.0f;
        for (const auto& q : normals) worst = q.w > worst ? q.w : worst;
        std::printf("%u %.9g %zu %.9g\n", model.GetTileSize(), amp, xz.size(), worst);
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f) return 4;
            std::fwrite(xz.data(), sizeof(xz[0]), xz.size(), f);
            std::fwrite(positions.data(), sizeof(positions[0]), positions.size(), f);
            std::fwrite(normals.data(), sizeof(normals[0]), normals.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "query_demo: %s\n", e.what());
        return 3;
    }
}
