// Evaluates the device math functions the layer kernels call (layers.hip) over the input ranges of the layer tests and
// writes float32 input / output arrays per function to <outdir>/probe_<name>.bin; tools/layer_math_ulp.py compares
// them with float64 and prints the budgets T of tests/test_layer_oracles.py (docs/LAYER_TEST_BOUNDS.md).
//   hipcc -O3 --offload-arch=gfx950 tools/layer_math_probe.hip -o build/layer_math_probe
//   build/layer_math_probe build/probe && python tools/layer_math_ulp.py build/probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <string>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__global__ void k_eval(int fn, const float* __restrict__ x, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r = 0.f;
  switch (fn) {
    case 0: r = erff(v); break;
    case 1: r = tanhf(v); break;
    case 2: r = expf(v); break;
    case 3: r = logf(v); break;
    case 4: r = log1pf(v); break;
    case 5: r = powf(0.9f, v); break;
    case 6: r = powf(0.999f, v); break;
    case 7: r = rsqrtf(v); break;
    case 8: r = __expf(v); break;
    case 9: r = sqrtf(v); break;
  }
  y[i] = r;
}

static void lin(std::vector<float>& v, double a, double b, int n) {
  for (int i = 0; i < n; ++i) v.push_back((float)(a + (b - a) * i / (n - 1)));
}
static void logsp(std::vector<float>& v, double a, double b, int n) {  // geometric grid a..b (> 0)
  for (int i = 0; i < n; ++i) v.push_back((float)(a * pow(b / a, (double)i / (n - 1))));
}

int main(int argc, char** argv) {
  const std::string outdir = argc > 1 ? argv[1] : ".";
  const char* names[10] = {"erff", "tanhf", "expf", "logf", "log1pf", "pow09", "pow0999", "rsqrtf", "fastexp", "sqrtf"};
  for (int fn = 0; fn < 10; ++fn) {
    std::vector<float> x;
    switch (fn) {
      case 0: lin(x, -8, 8, 400001); logsp(x, 1e-30, 1, 20001); break;                      // erf(g / sqrt 2)
      case 1: lin(x, -12, 12, 400001); lin(x, -130, 130, 2601); logsp(x, 1e-30, 1, 20001); break;
      case 2: lin(x, -20, 8.5, 400001); lin(x, -210, 0, 21001); x.push_back(50.f); x.push_back(200.f); break;
      case 3: logsp(x, 1e-37, 1, 200001); lin(x, 1, 8, 200001); logsp(x, 1e-4, 1e4, 100001); break;
      case 4: lin(x, -1, 0, 400001); logsp(x, 1e-37, 1, 100001); for (size_t i = x.size() - 100001; i < x.size(); ++i) x[i] = -x[i]; break;
      case 5: case 6: for (int t = 1; t <= 6000; ++t) x.push_back((float)t); break;
      case 7: logsp(x, 1e-5, 1e9, 400001); lin(x, 1e-5, 2e-5, 10001); break;
      case 8: lin(x, -100, 100, 400001); lin(x, -8, 8, 100001); break;
      case 9: logsp(x, 1e-30, 1e10, 400001); break;
    }
    const int n = (int)x.size();
    float *dx, *dy;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&dy, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, dy, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<float> y(n);
    CK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    CK(hipFree(dx));
    CK(hipFree(dy));
    std::string p = outdir + "/probe_" + names[fn] + ".bin";
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) { printf("cannot open %s\n", p.c_str()); return 1; }
    fwrite(x.data(), sizeof(float), n, f);
    fwrite(y.data(), sizeof(float), n, f);
    fclose(f);
    printf("%s: %d points\n", names[fn], n);
  }
  return 0;
}
