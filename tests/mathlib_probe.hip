// Worst observed error, in float32 ulps, of the device math functions the helper kernels call, each alone against the
// host's double-precision function over the range tests/helper_ref.py feeds it.  Not part of the library or of the
// suite: built and run by hand (hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics, the library's own
// flags); tests/helper_ref.py records what it printed on an MI355X and uses twice those figures.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

enum Fn { RSQRT = 0, ERF = 1, LOG = 2, SQRT = 3, RCP = 4, NFN = 5 };

__global__ void k_apply(int fn, const float* x, float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r;
  switch (fn) {
    case RSQRT: r = rsqrtf(v); break;
    case ERF: r = erff(v); break;
    case LOG: r = logf(v); break;
    case SQRT: r = sqrtf(v); break;
    default: r = 1.0f / v; break;
  }
  y[i] = r;
}

static double ref(int fn, double v) {
  switch (fn) {
    case RSQRT: return 1.0 / std::sqrt(v);
    case ERF: return std::erf(v);
    case LOG: return std::log(v);
    case SQRT: return std::sqrt(v);
    default: return 1.0 / v;
  }
}

#define CK(call)                                                       \
  do {                                                                 \
    hipError_t e_ = (call);                                            \
    if (e_ != hipSuccess) {                                            \
      std::printf("%s: %s\n", #call, hipGetErrorString(e_));           \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  const int n = 1 << 22;
  // (name, lo, hi, signed): log-spaced magnitudes in [lo, hi], both signs where the function takes them
  const struct { const char* name; double lo, hi; bool sgn; } R[NFN] = {
      {"rsqrtf", 1e-12, 1e8, false}, {"erff", 1e-6, 6.0, true}, {"logf", 1e-8, 1e16, false},
      {"sqrtf", 1e-12, 1e8, false},  {"1/x", 1e-12, 1e8, true}};
  std::vector<float> x(n), y(n);
  float *dx, *dy;
  CK(hipMalloc(&dx, n * sizeof(float)));
  CK(hipMalloc(&dy, n * sizeof(float)));
  for (int fn = 0; fn < NFN; ++fn) {
    for (int i = 0; i < n; ++i) {
      const double t = (i / 2) / (double)(n / 2 - 1);
      const double m = R[fn].lo * std::pow(R[fn].hi / R[fn].lo, t);
      x[i] = (float)((R[fn].sgn && (i & 1)) ? -m : m);
    }
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_apply, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, dy, n);
    CK(hipGetLastError());
    CK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0.0, at = 0.0;
    for (int i = 0; i < n; ++i) {
      const double r = ref(fn, (double)x[i]);
      if (r == 0.0 || !std::isfinite(r)) continue;
      int e;
      std::frexp(r, &e);                       // |r| in [2^(e-1), 2^e): one float32 ulp is 2^(e-24)
      const double ulp = std::ldexp(1.0, e - 24);
      const double err = std::fabs((double)y[i] - r) / ulp;
      if (err > worst) worst = err, at = x[i];
    }
    std::printf("%-7s [%g, %g]%s: worst %.3f ulp at x = %.9g\n", R[fn].name, R[fn].lo, R[fn].hi,
                R[fn].sgn ? " both signs" : "", worst, at);
  }
  CK(hipFree(dx));
  CK(hipFree(dy));
  return 0;
}
