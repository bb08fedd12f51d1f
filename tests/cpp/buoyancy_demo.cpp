// Drives WSTessendorf::SetHull / Buoyancy (include/WSTessendorf.hpp) the way a physics step would: Prepare, ComputeWaves, the hull of
// one boat uploaded once (a 6 x 2 x 3 box of half-metre cells: 36 points), then one call for a fleet of boats that all use it, each with
// its own pose and velocities.  The results are written raw to the file named by the second argument as [points][4] float hull,
// [bodies][16] words of ocean_body, [bodies][4] forces, [bodies][4] torques, so that the GPU test can compare them with the Python
// binding bit for bit.  Prints "N A bodies afloat" (afloat: bodies with some volume under water).
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

        std::vector<WSTessendorf::vec4> hull;
        const float e = 0.5f;
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 6; ++i)
                    hull.push_back(WSTessendorf::vec4(((float)i - 2.5f) * e, ((float)j - 0.5f) * e, ((float)k - 1.0f) * e, e));
        model.SetHull(hull);

        const int side = 15;
        std::vector<ocean_body> bodies;
        for (int j = 0; j < side; ++j)
            for (int i = 0; i < side; ++i) {
                const unsigned h = (unsigned)(j * side + i) * 2654435761u;
                const float jx = (float)(h & 0xffff) / 65536.0f, jz = (float)(h >> 16) / 65536.0f;
                ocean_body b{};
                b.pos[0] = -500.0f + ((float)i + jx) * (1000.0f / side);
                b.pos[1] = (jx - 0.5f) * 2.0f;
                b.pos[2] = -500.0f + ((float)j + jz) * (1000.0f / side);
                const float yaw = 6.2831853f * jz, roll = 0.3f * (jx - 0.5f);       // q = yaw about y, then a small roll about the boat's x
                const float cy = std::cos(0.5f * yaw), sy = std::sin(0.5f * yaw), cr = std::cos(0.5f * roll), sr = std::sin(0.5f * roll);
                b.quat[0] = cy * sr; b.quat[1] = sy * cr; b.quat[2] = -sy * sr; b.quat[3] = cy * cr;
                b.vel[0] = 2.0f * jx; b.vel[1] = jz - 0.5f; b.vel[2] = -jx;
                b.omega[0] = 0.1f * jz; b.omega[1] = 0.2f * jx; b.omega[2] = -0.1f;
                b.first_point = 0; b.points = (uint32_t)hull.size();
                bodies.push_back(b);
            }
        std::vector<WSTessendorf::vec4> forces, torques;
        model.Buoyancy(bodies, forces, torques);
        size_t afloat = 0;
        for (const auto& f : forces) afloat += f.w > 0.0f;
        std::printf("%u %.9g %zu %zu\n", model.GetTileSize(), amp, bodies.size(), afloat);
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f) return 4;
            std::fwrite(hull.data(), sizeof(hull[0]), hull.size(), f);
            std::fwrite(bodies.data(), sizeof(bodies[0]), bodies.size(), f);
            std::fwrite(forces.data(), sizeof(forces[0]), forces.size(), f);
            std::fwrite(torques.data(), sizeof(torques[0]), torques.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "buoyancy_demo: %s\n", e.what());
        return 3;
    }
}
