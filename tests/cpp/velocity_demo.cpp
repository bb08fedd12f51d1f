// Drives WSTessendorf::QueryVelocity (include/WSTessendorf.hpp) on a model constructed withVelocity: Prepare, ComputeWaves, then the
// velocity of the water at a jittered grid of world points.  The results are written raw to the file named by the second argument as
// [points][2] float xz, [points][4] positions, [points][4] velocities, so that the GPU test can compare them with the Python binding bit
// for bit.  Prints "N A points moving" (moving: points where some component of the velocity exceeds 0.05 m/s).
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
        WSTessendorf model(n, WSTessendorf::s_kDefaultTileLength, 0, true);
        model.SetWindDirection(WSTessendorf::vec2(1.0f, 0.5f));
        model.SetWindSpeed(20.0f);
        model.SetLambda(-1.5f);
        model.Prepare(42);
        const float amp = model.ComputeWaves(t);

        const int side = 17;
        std::vector<WSTessendorf::vec2> xz;
        for (int j = 0; j < side; ++j)
            for (int i = 0; i < side; ++i) {
                const unsigned h = (unsigned)(j * side + i) * 2654435761u;
                const float jx = (float)(h & 0xffff) / 65536.0f, jz = (float)(h >> 16) / 65536.0f;
                xz.push_back(WSTessendorf::vec2(-500.0f + ((float)i + jx) * (1000.0f / side), -500.0f + ((float)j + jz) * (1000.0f / side)));
            }
        std::vector<WSTessendorf::vec4> positions, velocities;
        model.QueryVelocity(xz, positions, velocities);
        size_t moving = 0;
        for (const auto& v : velocities) moving += std::fmax(std::fabs(v.x), std::fmax(std::fabs(v.y), std::fabs(v.z))) > 0.05f;
        std::printf("%u %.9g %zu %zu\n", model.GetTileSize(), amp, xz.size(), moving);
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f) return 4;
            std::fwrite(xz.data(), sizeof(xz[0]), xz.size(), f);
            std::fwrite(positions.data(), sizeof(positions[0]), positions.size(), f);
            std::fwrite(velocities.data(), sizeof(velocities[0]), velocities.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "velocity_demo: %s\n", e.what());
        return 3;
    }
}
