// Micro-measurement: the accuracy of the device library's expf and log10f against the host's fp64 exp / log10, over the argument
// ranges the per-ray training kernels and tn_image_losses use (tests/ray_losses_reference.py takes K_EXP and K_LOG10 from the
// output, with a margin of 2x; the record is profiles/micro/libm_accuracy.txt).  Built with the library's flags.
//   expf(-t):   t in [0, 87] (results normal), relative error in units of 2^-24; t in (87, 104] (results denormal or zero),
//               absolute error in units of 2^-126 (one smallest normal)
//   log10f(x):  x in [2^-24, 2^40], relative error in units of 2^-24
// Each range: N points on a regular grid plus N pseudo-random ones, and the powers of two inside it.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/micro/libm_accuracy.hip -o tools/micro/libm_accuracy_bin
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ void __launch_bounds__(256) apply(const float *x, float *y, int n, int fn) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = fn == 0 ? expf(-x[i]) : log10f(x[i]);
}

static std::vector<float> device(const std::vector<float> &x, int fn) {
    const int n = (int)x.size();
    float *dx, *dy;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&dy, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(apply, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, fn);
    CK(hipGetLastError());
    std::vector<float> y(n);
    CK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    CK(hipFree(dx));
    CK(hipFree(dy));
    return y;
}

static std::vector<float> points(double lo, double hi, int n, bool log_spaced) {
    std::vector<float> x;
    unsigned long long s = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < 2 * n; ++k) {
        double u;
        if (k < n) {
            u = (double)k / (n - 1);
        } else {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            u = (double)(s >> 11) / 9007199254740992.0;
        }
        x.push_back((float)(log_spaced ? lo * pow(hi / lo, u) : lo + (hi - lo) * u));
    }
    for (int e = -30; e <= 40; ++e) {
        const double p = ldexp(1.0, e);
        if (p >= lo && p <= hi) x.push_back((float)p);
    }
    return x;
}

int main() {
    const int N = 1 << 22;
    const double u24 = ldexp(1.0, -24), tiny = ldexp(1.0, -126);
    {
        const std::vector<float> x = points(0.0, 87.0, N, false), y = device(x, 0);
        double worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = exp(-(double)x[i]), e = fabs((double)y[i] - want) / (u24 * want);
            if (e > worst) worst = e, at = x[i];
        }
        printf("expf(-t)  t in [0, 87]     %zu points  worst relative error %.4f x 2^-24 at t = %.9g\n", x.size(), worst, at);
    }
    {
        const std::vector<float> x = points(87.0, 104.0, N / 4, false), y = device(x, 0);
        double worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double e = fabs((double)y[i] - exp(-(double)x[i])) / tiny;
            if (e > worst) worst = e, at = x[i];
        }
        printf("expf(-t)  t in (87, 104]   %zu points  worst absolute error %.4f x 2^-126 at t = %.9g\n", x.size(), worst, at);
    }
    {
        const std::vector<float> x = points(ldexp(1.0, -24), ldexp(1.0, 40), N, true), y = device(x, 1);
        double worst = 0.0, at = 0.0, worst_abs = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = log10((double)x[i]);
            worst_abs = fmax(worst_abs, fabs((double)y[i] - want) / (u24 * fmax(fabs(want), 1.0)));
            if (want == 0.0) {
                if (y[i] != 0.0f) worst = INFINITY, at = x[i];
                continue;
            }
            const double e = fabs((double)y[i] - want) / (u24 * fabs(want));
            if (e > worst) worst = e, at = x[i];
        }
        printf("log10f(x) x in [2^-24, 2^40] %zu points  worst relative error %.4f x 2^-24 at x = %.9g\n", x.size(), worst, at);
        printf("log10f(x) same points: worst |error| / (2^-24 max(|log10 x|, 1)) = %.4f\n", worst_abs);
    }
    return 0;
}
