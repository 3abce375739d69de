// Micro-measurement: the accuracy of the device library's expf and log10f against the host's fp64 exp / log10, over the argument
// ranges the per-ray training kernels and tn_image_losses use (tests/ray_losses_reference.py takes K_EXP and K_LOG10 from the
// output, with a margin of 2x; the record is profiles/micro/libm_accuracy.txt).  Built with the library's flags.
//   expf(-t):   t in [0, 87] (results normal), relative error in units of 2^-24; t in (87, 104] (results denormal or zero),
//               absolute error in units of 2^-126 (one smallest normal)
//   log10f(x):  x in [2^-24, 2^40], relative error in units of 2^-24
// and of the three fast operations of the eval field kernels, for which the platform documents no bound (tests/field_eval_reference.py
// takes K_FEXP_A / K_FEXP_B, K_FSIG and K_FSIG_PRE from the output, again with a margin of 2x):
//   __expf(x):  x in [-87, 0] and in [-30, 30], relative error in units of 2^-24 as a + b |x| (v_exp_f32 of the ROUNDED product
//               x log2(e) loses with |x|): a = the worst error over |x| <= 1, b = the largest (error - a) / |x| beyond;
//               x in [-104, -87): absolute error in units of 2^-126
//   fast_sigmoid(x) = v_rcp(1 + __expf(-x)) and fast_sigmoid_prescaled(a) = v_rcp(1 + v_exp(a)) (a = -log2(e) x, given as fp32):
//               x in [-100, 100] / a in [-144, 144], absolute error in units of 2^-24 against 1 / (1 + e^-x) and 1 / (1 + 2^a)
// and of powf(w, a), w in [0, 1], a in {0.5, 0.75}: the annealed PDF resampling of the fused proposal pass (tests/proposal_eval_reference.py
// takes K_POW from it the same way): relative error in units of 2^-24, 0 and 1 required exact
// Each range: N points on a regular grid plus N pseudo-random ones, and the powers of two inside it.
// The flags are the library's (thermo_nerf_amd/csrc/Makefile: -O3 -ffp-contract=off, no fast-math, default denormal mode), under which
// __expf(x) compiles to v_mul_f32 x, 0x3fb8aa3b + v_exp_f32 and the two sigmoids to that plus v_add_f32 and v_rcp_f32, in this tool
// as in the library's kernels: the constants describe the same instruction sequences.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/micro/libm_accuracy.hip -o tools/micro/libm_accuracy_bin
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ void __launch_bounds__(256) apply(const float *x, float *y, int n, int fn, float a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = fn == 0   ? expf(-v)
           : fn == 1 ? log10f(v)
           : fn == 2 ? __expf(v)
           : fn == 3 ? __builtin_amdgcn_rcpf(1.0f + __expf(-v))
           : fn == 4 ? __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v))
           : fn == 5 ? __builtin_amdgcn_rcpf(v)
                     : powf(v, a);  // a run-time exponent, as the kernels' pdf_anneal is: the library's general powf
}

static std::vector<float> device(const std::vector<float> &x, int fn, float a = 0.0f) {
    const int n = (int)x.size();
    float *dx, *dy;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&dy, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(apply, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, fn, a);
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
    const int M = 5000000;  // 10^7 arguments a range
    {
        std::vector<float> x = points(-87.0, 0.0, M, false);
        const std::vector<float> x2 = points(-30.0, 30.0, M, false);
        x.insert(x.end(), x2.begin(), x2.end());
        const std::vector<float> y = device(x, 2);
        double a = 0.0, b = 0.0, worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = exp((double)x[i]), e = fabs((double)y[i] - want) / (u24 * want);
            if (e > worst) worst = e, at = x[i];
            if (fabs(x[i]) <= 1.0f) a = fmax(a, e);
        }
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = exp((double)x[i]), e = fabs((double)y[i] - want) / (u24 * want);
            if (fabs(x[i]) > 1.0f) b = fmax(b, (e - a) / fabs((double)x[i]));
        }
        printf("__expf(x)  x in [-87, 0] and [-30, 30]  %zu points  worst relative error %.4f x 2^-24 at x = %.9g;  as a + b |x|: a = %.4f, b = %.4f\n",
               x.size(), worst, at, a, b);
    }
    {
        const std::vector<float> x = points(-104.0, -87.0, M / 4, false), y = device(x, 2);
        double worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            if (x[i] >= -87.0f) continue;
            const double e = fabs((double)y[i] - exp((double)x[i])) / tiny;
            if (e > worst) worst = e, at = x[i];
        }
        printf("__expf(x)  x in [-104, -87)  %zu points  worst absolute error %.4f x 2^-126 at x = %.9g\n", x.size(), worst, at);
    }
    for (int fn = 3; fn <= 4; ++fn) {
        const double span = fn == 3 ? 100.0 : 144.0;
        const std::vector<float> x = points(-span, span, M, false), y = device(x, fn);
        double worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = fn == 3 ? 1.0 / (1.0 + exp(-(double)x[i])) : 1.0 / (1.0 + exp2((double)x[i]));
            const double e = fabs((double)y[i] - want) / u24;
            if (!(e <= worst)) worst = e, at = x[i];
        }
        printf("%s in [-%g, %g]  %zu points  worst absolute error %.4f x 2^-24 at %.9g\n",
               fn == 3 ? "fast_sigmoid(x) = v_rcp(1 + __expf(-x))  x" : "fast_sigmoid_prescaled(a) = v_rcp(1 + v_exp(a))  a", span, span, x.size(), worst, at);
    }
    {   // v_rcp_f32 alone: the FAST kernels' 1 / x in spacing_fn_inv and in the scene contraction (K_RCP)
        const std::vector<float> x = points(ldexp(1.0, -20), ldexp(1.0, 20), M, true), y = device(x, 5);
        double worst = 0.0, at = 0.0;
        for (size_t i = 0; i < x.size(); ++i) {
            const double want = 1.0 / (double)x[i], e = fabs((double)y[i] - want) / (u24 * want);
            if (e > worst) worst = e, at = x[i];
        }
        printf("v_rcp_f32(x)  x in [2^-20, 2^20]  %zu points  worst relative error %.4f x 2^-24 at x = %.9g\n", x.size(), worst, at);
    }
    {   // powf(w, a): the PDF resampling of an annealed proposal pass (pdf_anneal != 1) raises a weight in [0, 1] to a in (0, 1)
        std::vector<float> x = points(0.0, 1.0, M / 2, false);
        const std::vector<float> x2 = points(ldexp(1.0, -60), 1.0, M / 2, true);
        x.insert(x.end(), x2.begin(), x2.end());
        x.push_back(0.0f);
        x.push_back(1.0f);
        double worst_all = 0.0;
        for (const double a : {0.5, 0.75}) {
            const std::vector<float> y = device(x, 6, (float)a);
            double worst = 0.0, at = 0.0;
            for (size_t i = 0; i < x.size(); ++i) {
                const double want = pow((double)x[i], a);
                const double e = want == 0.0 ? (y[i] == 0.0f ? 0.0 : INFINITY) : fabs((double)y[i] - want) / (u24 * want);
                if (!(e <= worst)) worst = e, at = x[i];
            }
            worst_all = fmax(worst_all, worst);
            printf("powf(w, %.2f)  w in [0, 1]  %zu points  worst relative error %.4f x 2^-24 at w = %.9g\n", a, x.size(), worst, at);
        }
        printf("powf(w, a)  a in {0.5, 0.75}: the worst of both %.4f x 2^-24\n", worst_all);
    }
    return 0;
}
