// Micro-benchmark: the two operand arrangements of v_mfma_f32_16x16x4_f32 that csrc/mcg_policy_grad.hip adds to the forward's
// (mfma_f32.hip), each against a host product on a later layer of 32 units over 32 inputs packed as the policy's blob packs it:
// tile (T, 4 t + r), float 16 g + i = W[16 T + i][16 t + 4 g + r].  All values are small integers: every sum is exact in float32.
//   dX = W^T dZ   A operand gathered from the blob as it lies: for output tile T' and k-block (t, r), lane 16 g + i reads
//                 W[16 t + 4 g + r][16 T' + i] at tile (t, 4 T' + (i & 3)), float 16 (i >> 2) + 4 g + r
//   dW = dZ X^T   both operands from rows of 16 samples: instruction q sums the samples {4 g + q}; register r of the result is
//                 dW[16 T + 4 g + r][16 C + i], stored to tile (T, 4 C + (i & 3)), float 16 (i >> 2) + 4 g + r
//   hipcc --offload-arch=gfx950 -O3 tools/microbench/mfma_f32_grad.hip -o /tmp/mfma_f32_grad && /tmp/mfma_f32_grad
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
typedef float vf4 __attribute__((ext_vector_type(4)));
constexpr int OUT = 32, IN = 32, NKB = IN / 4;

__host__ __device__ inline int blob_at(int row, int col) {      // W[row][col] of the packed later layer
  const int T = row / 16, i = row % 16, t = col / 16, g = (col % 16) / 4, r = col % 4;
  return (T * NKB + 4 * t + r) * 64 + 16 * g + i;
}

// dZ rows [OUT][16 samples] -> dX rows [IN][16 samples]
__global__ void k_wt(const float* blob, const float* dZ, float* dX) {
  const int l = threadIdx.x, g = l / 16, i = l % 16;
  for (int Tp = 0; Tp < IN / 16; Tp++) {
    vf4 c = {0, 0, 0, 0};
    for (int t = 0; t < OUT / 16; t++) {
      const vf4 w = *reinterpret_cast<const vf4*>(blob + (t * NKB + 4 * Tp + (i & 3)) * 64 + 16 * (i >> 2) + 4 * g);
      for (int r = 0; r < 4; r++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r], dZ[(16 * t + 4 * g + r) * 16 + i], c, 0, 0, 0);
    }
    for (int r = 0; r < 4; r++) dX[(16 * Tp + 4 * g + r) * 16 + i] = c[r];
  }
}

// dZ rows [OUT][16], X rows [IN][16] -> dW in the blob's layout
__global__ void k_dw(const float* dZ, const float* X, float* grad) {
  const int l = threadIdx.x, g = l / 16, i = l % 16;
  for (int T = 0; T < OUT / 16; T++)
    for (int C = 0; C < IN / 16; C++) {
      const vf4 a = *reinterpret_cast<const vf4*>(dZ + (16 * T + i) * 16 + 4 * g), b = *reinterpret_cast<const vf4*>(X + (16 * C + i) * 16 + 4 * g);
      vf4 c = {0, 0, 0, 0};
      for (int q = 0; q < 4; q++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], c, 0, 0, 0);
      *reinterpret_cast<vf4*>(grad + (T * NKB + 4 * C + (i & 3)) * 64 + 16 * (i >> 2) + 4 * g) = c;
    }
}

int main() {
  setvbuf(stdout, nullptr, _IONBF, 0);
  std::vector<float> W(OUT * IN), blob(OUT * IN), dZ(OUT * 16), X(IN * 16), dX(IN * 16), grad(OUT * IN);
  for (int u = 0; u < OUT; u++) for (int k = 0; k < IN; k++) { W[u * IN + k] = (float)((u * 7 + k * 3) % 11) - 5; blob[blob_at(u, k)] = W[u * IN + k]; }
  for (int u = 0; u < OUT; u++) for (int s = 0; s < 16; s++) dZ[u * 16 + s] = (float)((u * 5 + s * 2) % 7) - 3;
  for (int k = 0; k < IN; k++) for (int s = 0; s < 16; s++) X[k * 16 + s] = (float)((k * 3 + s * 5) % 9) - 4;
  float *dB, *dD, *dXin, *dO, *dG;
  hipMalloc(&dB, 4 * OUT * IN); hipMalloc(&dD, 4 * OUT * 16); hipMalloc(&dXin, 4 * IN * 16); hipMalloc(&dO, 4 * IN * 16); hipMalloc(&dG, 4 * OUT * IN);
  hipMemcpy(dB, blob.data(), 4 * OUT * IN, hipMemcpyHostToDevice); hipMemcpy(dD, dZ.data(), 4 * OUT * 16, hipMemcpyHostToDevice);
  hipMemcpy(dXin, X.data(), 4 * IN * 16, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_wt, dim3(1), dim3(64), 0, 0, dB, dD, dO);
  hipLaunchKernelGGL(k_dw, dim3(1), dim3(64), 0, 0, dD, dXin, dG);
  hipDeviceSynchronize();
  hipMemcpy(dX.data(), dO, 4 * IN * 16, hipMemcpyDeviceToHost); hipMemcpy(grad.data(), dG, 4 * OUT * IN, hipMemcpyDeviceToHost);
  float e1 = 0, e2 = 0;
  for (int k = 0; k < IN; k++) for (int s = 0; s < 16; s++) { float r = 0; for (int u = 0; u < OUT; u++) r += W[u * IN + k] * dZ[u * 16 + s]; e1 = fmaxf(e1, fabsf(dX[k * 16 + s] - r)); }
  for (int u = 0; u < OUT; u++) for (int k = 0; k < IN; k++) { float r = 0; for (int s = 0; s < 16; s++) r += dZ[u * 16 + s] * X[k * 16 + s]; e2 = fmaxf(e2, fabsf(grad[blob_at(u, k)] - r)); }
  printf("dX = W^T dZ, A operand gathered from the packed blob: max err %.3g\n", e1);
  printf("dW = dZ X^T, operands from rows of 16 samples, result stored in the blob's layout: max err %.3g\n", e2);
  return e1 == 0 && e2 == 0 ? 0 : 1;
}
