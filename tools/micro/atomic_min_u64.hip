// Micro-benchmark: the rate of the 64-bit integer atomic minimum on a key plane, in the access shapes of tn_mesh_raster.hip — the
// guides and tools/micro/atomics_types.hip measured adds only.  A plane of 2048 x 2048 uint64 keys (32 MiB); every pass hits every key
// once with a key below what it holds (the minimum is written), PASSES passes per launch.
//   row      a wave's 64 lanes on 64 neighbouring keys of a row (512 contiguous bytes)
//   tile     the sweep's shape: a block of 256 on a 16 x 16 tile, a wave on 4 rows of 16 keys (four 128-byte segments)
//   boxes    the one-thread shape: every lane walks its own 2 x 2 box (neighbouring lanes, neighbouring boxes)
//   skipped  `tile` with keys that lose: the plain load alone, the atomic is never issued
//   hipcc --offload-arch=gfx950 -O3 tools/micro/atomic_min_u64.hip -o tools/micro/atomic_min_u64_bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kSide = 2048, kPasses = 8;
typedef unsigned long long u64;

// shape 0 row, 1 tile, 2 boxes; `lose`: the keys are above what the plane holds
__global__ void __launch_bounds__(256) hit(u64 *keys, int shape, int lose, int check) {
    const unsigned block = blockIdx.x, t = threadIdx.x;
    for (int pass = 0; pass < kPasses; ++pass) {
        unsigned i, j;
        if (shape == 0) {
            const unsigned p = block * 256 + t;
            i = p % kSide, j = p / kSide;
        } else if (shape == 1) {
            i = (block % (kSide / 16)) * 16 + t % 16, j = (block / (kSide / 16)) * 16 + t / 16;
        } else {
            const unsigned q = block * 64 + t / 4;  // a lane's box: four consecutive t walk it (as a loop would, one step per pass of the 4)
            i = (q % (kSide / 2)) * 2 + (t & 1), j = (q / (kSide / 2)) * 2 + ((t >> 1) & 1);
        }
        u64 *slot = keys + (size_t)j * kSide + i;
        const u64 key = lose ? ~0ull - 1 : ((u64)(1000 - pass) << 32) | t;
        if (!check || key < *slot) atomicMin(slot, key);
    }
}

static void run(const char *name, u64 *keys, int shape, int lose, int check) {
    const size_t bytes = (size_t)kSide * kSide * sizeof(u64);
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e30f, worst = 0.0f;
    for (int rep = 0; rep < 7; ++rep) {
        CK(hipMemset(keys, lose ? 0x00 : 0xff, bytes));
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(hit, dim3(kSide * kSide / 256), dim3(256), 0, 0, keys, shape, lose, check);
        CK(hipEventRecord(b));
        CK(hipDeviceSynchronize());
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (rep == 0) continue;  // warm-up
        best = ms < best ? ms : best, worst = ms > worst ? ms : worst;
    }
    const double n = (double)kSide * kSide * kPasses;
    printf("%-34s %8.4f .. %8.4f ms  %8.2f G keys/s  %8.1f GB/s of keys\n", name, best, worst, n / best / 1e6, n * 8 / best / 1e6);
}

int main() {
    u64 *keys;
    CK(hipMalloc(&keys, (size_t)kSide * kSide * sizeof(u64)));
    printf("64-bit atomic minimum on a %d x %d key plane, %d passes per launch, every key hit once per pass; 6 timed launches, min .. max\n",
           kSide, kSide, kPasses);
    run("row, atomic always", keys, 0, 0, 0);
    run("row, load then atomic", keys, 0, 0, 1);
    run("tile 16 x 16, atomic always", keys, 1, 0, 0);
    run("tile 16 x 16, load then atomic", keys, 1, 0, 1);
    run("boxes 2 x 2, atomic always", keys, 2, 0, 0);
    run("boxes 2 x 2, load then atomic", keys, 2, 0, 1);
    run("tile 16 x 16, skipped (load only)", keys, 1, 1, 1);
    CK(hipFree(keys));
    return 0;
}
