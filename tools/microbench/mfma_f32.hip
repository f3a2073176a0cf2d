// Micro-benchmark: v_mfma_f32_16x16x4_f32 on gfx950 -- operand / result layout (checked against a host product) and issue cost
// (independent accumulators back to back, and one dependent chain), one wave per SIMD.  What csrc/mcg_policy.hip builds on.
//   hipcc --offload-arch=gfx950 -O3 tools/microbench/mfma_f32.hip -o /tmp/mfma_f32 && /tmp/mfma_f32
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
typedef float vf4 __attribute__((ext_vector_type(4)));

__global__ void k_layout(const float* A, const float* B, float* D) {         // A[16][4], B[4][16] row-major; D raw: lane, element
  const int l = threadIdx.x;
  const float a = A[(l % 16) * 4 + l / 16];           // assumed: lane l holds A[i = l % 16][k = l / 16]
  const float b = B[(l / 16) * 16 + l % 16];          // assumed: lane l holds B[k = l / 16][j = l % 16]
  vf4 c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  for (int v = 0; v < 4; v++) D[l * 4 + v] = c[v];
}

// Two chained products without a transposition: the first product's registers are the second's B operands when the second's
// k-block r is the rows {4 g + r} of the first result.  out = W2 (W1 X) for W1[16][4], X[4][16], W2[16][16].
__global__ void k_chain(const float* W1, const float* X, const float* W2, float* D) {
  const int l = threadIdx.x, i = l % 16, g = l / 16;
  vf4 h = {0, 0, 0, 0};
  h = __builtin_amdgcn_mfma_f32_16x16x4f32(W1[i * 4 + g], X[g * 16 + i], h, 0, 0, 0);
  vf4 c = {0, 0, 0, 0};
  for (int r = 0; r < 4; r++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(W2[i * 16 + 4 * g + r], h[r], c, 0, 0, 0);
  for (int v = 0; v < 4; v++) D[l * 4 + v] = c[v];
}

__global__ void k_time(unsigned long long* out, float* sink, int iters, int dep) {
  const int l = threadIdx.x & 63;
  float a = 1.0f + l * 1e-3f, b = 1.0f - l * 1e-3f;
  vf4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0;
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < iters; it++) {
    if (dep) {
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0); c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0); c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0);
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0); c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0);
    } else {
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c0, 0, 0, 0); c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c1, 0, 0, 0);
      c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c2, 0, 0, 0); c3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c3, 0, 0, 0);
      c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c4, 0, 0, 0); c5 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c5, 0, 0, 0);
    }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (l == 0) out[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
  sink[blockIdx.x * blockDim.x + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3] + c4[0] + c5[1];
}

int main() {
  setvbuf(stdout, nullptr, _IONBF, 0);
  std::vector<float> A(64), B(64), W2(256), D(256), R(256), R2(256);
  for (int i = 0; i < 16; i++) for (int k = 0; k < 4; k++) A[i * 4 + k] = 1 + i + 0.25f * k;
  for (int k = 0; k < 4; k++) for (int j = 0; j < 16; j++) B[k * 16 + j] = 2 + 0.5f * j - k;
  for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++) W2[i * 16 + j] = (float)((i * 7 + j * 3) % 11) - 5;
  for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++) { float s = 0; for (int k = 0; k < 4; k++) s += A[i * 4 + k] * B[k * 16 + j]; R[i * 16 + j] = s; }
  for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++) { float s = 0; for (int k = 0; k < 16; k++) s += W2[i * 16 + k] * R[k * 16 + j]; R2[i * 16 + j] = s; }
  float *dA, *dB, *dW, *dD; hipMalloc(&dA, 256); hipMalloc(&dB, 256); hipMalloc(&dW, 1024); hipMalloc(&dD, 1024);
  hipMemcpy(dA, A.data(), 256, hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), 256, hipMemcpyHostToDevice);
  hipMemcpy(dW, W2.data(), 1024, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, dA, dB, dD); hipDeviceSynchronize();
  hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost);
  float e1 = 0, e2 = 0;                                // candidate result layouts (all values here are exact in float32)
  for (int l = 0; l < 64; l++) for (int v = 0; v < 4; v++) {
    e1 = fmaxf(e1, fabsf(D[l * 4 + v] - R[(4 * (l / 16) + v) * 16 + l % 16]));      // D[i = 4 (l / 16) + v][j = l % 16]
    e2 = fmaxf(e2, fabsf(D[l * 4 + v] - R[((l / 16) + 4 * v) * 16 + l % 16]));      // D[i = l / 16 + 4 v][j = l % 16]
  }
  printf("layout: A[l%%16][l/16], B[l/16][l%%16] assumed;  result = D[4(l/16)+v][l%%16]: max err %.3g;  result = D[l/16+4v][l%%16]: max err %.3g\n", e1, e2);
  hipLaunchKernelGGL(k_chain, dim3(1), dim3(64), 0, 0, dA, dB, dW, dD); hipDeviceSynchronize();
  hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost);
  float e3 = 0;
  for (int l = 0; l < 64; l++) for (int v = 0; v < 4; v++) e3 = fmaxf(e3, fabsf(D[l * 4 + v] - R2[(4 * (l / 16) + v) * 16 + l % 16]));
  printf("chain: W2 (W1 X) with the first result's registers as the second's B operands, k-block r = rows {4g + r}: max err %.3g\n", e3);
  for (int dep = 0; dep < 2; dep++) for (int w : {1, 4}) {
    const int wgs = 256, iters = 2000; unsigned long long* d; float* s;
    hipMalloc(&d, 8 * wgs * w); hipMalloc(&s, 4 * wgs * w * 64);
    hipLaunchKernelGGL(k_time, dim3(wgs), dim3(64 * w), 0, 0, d, s, 10, dep);
    hipLaunchKernelGGL(k_time, dim3(wgs), dim3(64 * w), 0, 0, d, s, iters, dep); hipDeviceSynchronize();
    std::vector<unsigned long long> h(wgs * w); hipMemcpy(h.data(), d, 8 * wgs * w, hipMemcpyDeviceToHost);
    double tot = 0; for (auto v : h) tot += (double)v;
    printf("%s v_mfma_f32_16x16x4_f32, %d wave(s) per workgroup: %.1f clocks per instruction per wave\n", dep ? "dependent  " : "independent", w, tot / h.size() / iters / 6);
    hipFree(d); hipFree(s);
  }
  return 0;
}
