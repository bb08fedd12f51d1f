// Drives WSTessendorf::RaycastSurface (include/WSTessendorf.hpp) the way a camera or a weapon would: Prepare, ComputeWaves, then one ray
// cast for a fan of rays from a camera 25 m above the water looking down at 10-50 degrees.  The results are written raw to the file named
// by the second argument as [rays][3] origins, [rays][3] directions, [rays][4] hits, [rays][4] normals, so that the GPU test can compare
// them with the Python binding bit for bit.  Prints "N A rays hits".
#include <cmath>
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
        std::vector<WSTessendorf::vec3> origins, directions;
        for (int j = 0; j < side; ++j)
            for (int i = 0; i < side; ++i) {
                const float yaw = -1.0f + 2.0f * ((float)i + 0.5f) / side;                      // radians
                const float pitch = 0.17f + 0.7f * ((float)j + 0.5f) / side;                      // below the horizon
                origins.push_back(WSTessendorf::vec3(10.0f, 25.0f, -30.0f));
                directions.push_back(WSTessendorf::vec3(std::cos(pitch) * std::sin(yaw), -std::sin(pitch), std::cos(pitch) * std::cos(yaw)));
            }
        std::vector<WSTessendorf::vec4> hits, normals;
        model.RaycastSurface(origins, directions, 500.0f, hits, normals);
        size_t count = 0;
        for (const auto& h : hits) count += h.w >= 0.0f;
        std::printf("%u %.9g %zu %zu\n", model.GetTileSize(), amp, origins.size(), count);
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f) return 4;
            std::fwrite(origins.data(), sizeof(origins[0]), origins.size(), f);
            std::fwrite(directions.data(), sizeof(directions[0]), directions.size(), f);
            std::fwrite(hits.data(), sizeof(hits[0]), hits.size(), f);
            std::fwrite(normals.data(), sizeof(normals[0]), normals.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "raycast_demo: %s\n", e.what());
        return 3;
    }
}
