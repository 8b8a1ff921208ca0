// Probe: operand / result lane mapping of v_mfma_f32_16x16x32_bf16 on gfx950, as csrc/gconv_bf16.hip assumes it:
//   lane l = (i = l % 16, kq = l / 16) supplies A[row i][k = 8 kq + e] and B[k = 8 kq + e][col i] in element e of its 8-wide fragment and
//   holds D[row 4 kq + v][col i] in accumulator element v.
// A and B hold small integers (exact in bf16, sums exact in fp32); the host forms D = A B and compares every (lane, v).
//   hipcc --offload-arch=gfx950 tools/mfma16x16x32_probe.hip -o mfma16x16x32_probe && ./mfma16x16x32_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ inline int a_val(int m, int k) { return (m * 7 + k * 3) % 11 - 5; }
__host__ __device__ inline int b_val(int k, int n) { return (k * 5 + n * 13) % 9 - 4; }

__global__ void probe(float* out) {
  const int l = threadIdx.x, i = l & 15, kq = l >> 4;
  bf16x8 a, b;
  for (int e = 0; e < 8; ++e) {
    a[e] = (__bf16)(float)a_val(i, 8 * kq + e);
    b[e] = (__bf16)(float)b_val(8 * kq + e, i);
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  for (int v = 0; v < 4; ++v) out[l * 4 + v] = c[v];
}

int main() {
  float* d;
  if (hipMalloc(&d, 256 * sizeof(float)) != hipSuccess) return 2;
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
  float h[256];
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
  int bad = 0;
  for (int l = 0; l < 64; ++l)
    for (int v = 0; v < 4; ++v) {
      const int m = 4 * (l >> 4) + v, n = l & 15;
      int ref = 0;
      for (int k = 0; k < 32; ++k) ref += a_val(m, k) * b_val(k, n);
      if (h[l * 4 + v] != (float)ref) {
        if (bad++ < 8) printf("lane %2d v %d: got %g, D[%d][%d] = %d\n", l, v, h[l * 4 + v], m, n, ref);
      }
    }
  printf(bad ? "mapping NOT as assumed: %d mismatches\n" : "mapping confirmed: A[i][8 kq + e], B[8 kq + e][i], D[4 kq + v][i] (%d mismatches)\n", bad);
  (void)hipFree(d);
  return bad ? 1 : 0;
}
