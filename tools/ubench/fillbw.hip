// Store-bandwidth ceilings by store flavour (developer tool): a linear 16-B-per-lane fill of a buffer far beyond the
// 256 MiB Infinity Cache, and the same with the 1 KiB-run-per-wave shape of the map stores, for the cache-policy bits
// a gfx950 global store can carry.
//
// `fillbw shapes` prices the pieces a MIRRORED row leaves behind instead (profiles/whole_piece_stores.txt): the same bytes, every
// element written exactly once, but each wave instruction starting one element past a piece boundary, so that the boundary
// 64-byte piece is completed by two waves with two byte-masked requests.
//   map shapes, 16 B per lane, 1 KiB per wave instruction:
//     aligned        lane l of wave w -> element 64 w + l                       (16 whole pieces)
//     shifted        lane l of wave w -> element 64 w + l + 1, cyclic            (15 whole pieces + 48 B + 16 B)
//     mirror whole   the x passes' pair of stores: element i of the lower half ascending, and the upper half DESCENDING over the
//                    lanes, mirrored element n/2 - 1 - i                         (whole pieces: what the rotated hand-off would store)
//     mirror shifted the same pair with mirrored element (n/2 - i) & (n/2 - 1)  (what out() stores today: 1 KiB from 16 B past a boundary)
//   z-pass shapes, 8 B per lane, 512 B per wave instruction (eight 64-byte pieces of eight rows):
//     aligned / shifted by one element: every eighth piece split 56 B + 8 B between two waves (side 1, rows N - p).
// Policies: plain, nt (the maps of pipelined frames), and sc1 (the write-through fp32 intermediates) for the z shapes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
#define FILL_KERNEL(name, bits)                                                                              \
__global__ void name(f4* __restrict__ d, size_t n) {                                                          \
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const size_t s = (size_t)gridDim.x * blockDim.x; \
    const f4 v = {1.f, 2.f, 3.f, 4.f};                                                                        \
    for (; i < n; i += s) { f4* p = d + i; asm volatile("global_store_dwordx4 %0, %1, off " bits :: "v"(p), "v"(v) : "memory"); } \
}
FILL_KERNEL(k_plain, "")
FILL_KERNEL(k_nt, "nt")
FILL_KERNEL(k_sc0, "sc0")
FILL_KERNEL(k_sc1, "sc1")
FILL_KERNEL(k_sc0sc1, "sc0 sc1")
FILL_KERNEL(k_sc1nt, "sc1 nt")
FILL_KERNEL(k_sc0nt, "sc0 nt")
FILL_KERNEL(k_all, "sc0 sc1 nt")

enum { PLAIN = 0, NT = 1, SC1 = 2 };
template <int POLICY> __device__ __forceinline__ void put(f4* p, f4 v)
{
    if (POLICY == NT) asm volatile("global_store_dwordx4 %0, %1, off nt" :: "v"(p), "v"(v) : "memory");
    else if (POLICY == SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off" :: "v"(p), "v"(v) : "memory");
}
template <int POLICY> __device__ __forceinline__ void put(f2* p, f2 v)
{
    if (POLICY == NT) asm volatile("global_store_dwordx2 %0, %1, off nt" :: "v"(p), "v"(v) : "memory");
    else if (POLICY == SC1) asm volatile("global_store_dwordx2 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(p), "v"(v) : "memory");
}
// n elements of type V (a power of two, a multiple of 128), each written exactly once in every shape; every index below is < n.
enum { ALIGNED = 0, SHIFTED = 1, MIRROR_WHOLE = 2, MIRROR_SHIFTED = 3 };
template <class V, int SHAPE, int POLICY>
__global__ void k_shape(V* __restrict__ d, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const size_t s = (size_t)gridDim.x * blockDim.x;
    V v; for (unsigned c = 0; c < sizeof(V) / 4; ++c) v[c] = 1.f + c;
    if (SHAPE == ALIGNED || SHAPE == SHIFTED) {
        for (; i < n; i += s) put<POLICY>(d + ((i + (SHAPE == SHIFTED)) & (n - 1)), v);
    } else {
        const size_t h = n / 2;
        for (; i < h; i += s) {
            put<POLICY>(d + i, v);
            put<POLICY>(d + h + (SHAPE == MIRROR_WHOLE ? h - 1 - i : (h - i) & (h - 1)), v);
        }
    }
}

static int shapes()
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (size_t mb : {128, 1024}) {
        const size_t bytes = mb << 20;
        void* d; if (hipMalloc(&d, bytes) != hipSuccess) return 1;
        (void)hipMemset(d, 0, bytes);
        auto time = [&](auto kern, auto* ptr) {
            const size_t n = bytes / sizeof(*ptr);
            const int reps = 20;
            for (int w = 0; w < 3; ++w) kern<<<4096, 256>>>(ptr, n);
            (void)hipEventRecord(e0); for (int r = 0; r < reps; ++r) kern<<<4096, 256>>>(ptr, n); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
            float ms; (void)hipEventElapsedTime(&ms, e0, e1);
            return bytes * 1e-9 * reps / (ms * 1e-3);
        };
        // one pair = the whole-piece shape and its shifted twin, measured alternately
        auto pair = [&](const char* name, auto whole, auto shifted, auto* ptr) {
            const int R = 7;
            std::vector<double> a, b;
            for (int r = 0; r < R; ++r) { a.push_back(time(whole, ptr)); b.push_back(time(shifted, ptr)); }
            printf("%5zu MiB  %-22s whole  ", mb, name); for (double x : a) printf(" %5.0f", x);
            printf("\n%5zu MiB  %-22s shifted", mb, name); for (double x : b) printf(" %5.0f", x);
            std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
            printf("\n%5zu MiB  %-22s median whole %5.0f  shifted %5.0f GB/s  shifted / whole = %.3f\n", mb, name, a[R / 2], b[R / 2], b[R / 2] / a[R / 2]);
        };
        f4* d4 = (f4*)d; f2* d2 = (f2*)d;
        pair("map linear plain", k_shape<f4, ALIGNED, PLAIN>, k_shape<f4, SHIFTED, PLAIN>, d4);
        pair("map linear nt", k_shape<f4, ALIGNED, NT>, k_shape<f4, SHIFTED, NT>, d4);
        pair("map mirror plain", k_shape<f4, MIRROR_WHOLE, PLAIN>, k_shape<f4, MIRROR_SHIFTED, PLAIN>, d4);
        pair("map mirror nt", k_shape<f4, MIRROR_WHOLE, NT>, k_shape<f4, MIRROR_SHIFTED, NT>, d4);
        pair("z 8 B/lane plain", k_shape<f2, ALIGNED, PLAIN>, k_shape<f2, SHIFTED, PLAIN>, d2);
        pair("z 8 B/lane nt", k_shape<f2, ALIGNED, NT>, k_shape<f2, SHIFTED, NT>, d2);
        pair("z 8 B/lane sc1", k_shape<f2, ALIGNED, SC1>, k_shape<f2, SHIFTED, SC1>, d2);
        if (hipDeviceSynchronize() != hipSuccess) return 1;
        (void)hipFree(d);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) return shapes();
    for (size_t mb : {128, 1024}) {
        const size_t bytes = mb << 20, n = bytes / 16;
        f4* d; if (hipMalloc(&d, bytes) != hipSuccess) return 1;
        hipMemset(d, 0, bytes);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        auto time = [&](auto kern, const char* name) {
            const int reps = 20;
            for (int w = 0; w < 3; ++w) kern<<<4096, 256>>>(d, n);
            hipEventRecord(e0); for (int r = 0; r < reps; ++r) kern<<<4096, 256>>>(d, n); hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            printf("%5zu MiB  %-12s %6.0f GB/s\n", mb, name, bytes * 1e-9 * reps / (ms * 1e-3));
        };
        time(k_plain, "plain"); time(k_nt, "nt"); time(k_sc0, "sc0"); time(k_sc1, "sc1"); time(k_sc0sc1, "sc0 sc1");
        time(k_sc1nt, "sc1 nt"); time(k_sc0nt, "sc0 nt"); time(k_all, "sc0 sc1 nt");
        hipFree(d);
    }
    return 0;
}
