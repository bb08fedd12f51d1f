// Drives the foam of WSTessendorf (include/WSTessendorf.hpp: UpdateFoam / GetFoam / QueryFoam) the way a game loop would: Prepare, then
// `steps` frames t_j = 0.1 j with one foam step of 0.1 s behind each, then one foam query for a fixed jittered grid of world points over
// +-600 m.  The results are written raw to the file named by the second argument as [N*N] float foam, [points][2] float xz,
// [points][4] query results, so that the GPU test can compare them with the Python binding bit for bit.  Prints "N steps points mean_foam".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "WSTessendorf.hpp"

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : WSTessendorf::s_kDefaultTileSize;
    const char* out = argc > 2 ? argv[2] : nullptr;
    const int steps = argc > 3 ? std::atoi(argv[3]) : 20;
    try {
        WSTessendorf model(n, WSTessendorf::s_kDefaultTileLength);
        model.SetWindDirection(WSTessendorf::vec2(1.0f, 0.5f));
        model.Prepare(42);
        for (int j = 0; j < steps; ++j) {
            model.ComputeWaves(0.1f * (float)j);
            model.UpdateFoam(0.1f);
        }
        const std::vector<float> foam = model.GetFoam();

        const int side = 64;
        std::vector<WSTessendorf::vec2> xz;
        for (int j = 0; j < side; ++j)
            for (int i = 0; i < side; ++i) {
                const unsigned h = (unsigned)(j * side + i) * 2654435761u;
                const float jx = (float)(h & 0xffff) / 65536.0f, jz = (float)(h >> 16) / 65536.0f;
                xz.push_back(WSTessendorf::vec2(-600.0f + ((float)i + jx) * (1200.0f / side), -600.0f + ((float)j + jz) * (1200.0f / side)));
            }
        std::vector<WSTessendorf::vec4> result;
        model.QueryFoam(xz, result);
        double sum = 0.0;
        for (float f : foam) sum += f;
        std::printf("%u %d %zu %.9g\n", model.GetTileSize(), steps, xz.size(), sum / (double)foam.size());
        if (out) {
            FILE* f = std::fopen(out, "wb");
            if (!f) return 4;
            std::fwrite(foam.data(), sizeof(foam[0]), foam.size(), f);
            std::fwrite(xz.data(), sizeof(xz[0]), xz.size(), f);
            std::fwrite(result.data(), sizeof(result[0]), result.size(), f);
            std::fclose(f);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "foam_demo: %s\n", e.what());
        return 3;
    }
}
