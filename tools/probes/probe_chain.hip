// Probe: do back-to-back DEPENDENT v_mfma_f32_32x32x2_f32 on ONE accumulator issue without a bubble on gfx950?
//
// mma_chunk_gather_f32 (njf_device.h) orders an exact-fp32 chunk by output block: 32 consecutive MFMAs accumulate into the
// same 16 registers.  That ordering is free only if the matrix pipe forwards the accumulator from one instruction to the
// next.  Per wave: `iters` x 32 MFMAs into 1 accumulator (the chain), 2 alternating, or 4 round-robin (the order
// mma_chunk<PREC_F32> issues them in); one wave per SIMD (256 threads) and two (512 threads), one workgroup per CU.
//
//   hipcc --offload-arch=gfx950 -O3 tools/probes/probe_chain.hip -o build/probe_chain && build/probe_chain
// Experiment tooling, not part of the product path.  Output recorded in profiles/gather_overlap.json.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)
#define MFMA(acc) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(fa), "v"(fb))
#define MFMA8(a0, a1, a2, a3) do { MFMA(a0); MFMA(a1); MFMA(a2); MFMA(a3); MFMA(a0); MFMA(a1); MFMA(a2); MFMA(a3); } while (0)

__global__ void __launch_bounds__(512) chain_kernel(int accs, int iters, unsigned long long* cycles, float* sink) {
  extern __shared__ char pad[];   // 96 KiB dynamic: one workgroup per CU
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0 && iters < 0) pad[wave] = 1;
  float fa = 0.001f * lane, fb = 0.002f * lane;
  f32x16 c0 = (f32x16)(0.f), c1 = (f32x16)(0.f), c2 = (f32x16)(0.f), c3 = (f32x16)(0.f);
  __syncthreads();
  unsigned long long t0 = __builtin_readcyclecounter();
  if (accs == 1) for (int it = 0; it < iters; ++it) { MFMA8(c0, c0, c0, c0); MFMA8(c0, c0, c0, c0); MFMA8(c0, c0, c0, c0); MFMA8(c0, c0, c0, c0); }
  else if (accs == 2) for (int it = 0; it < iters; ++it) { MFMA8(c0, c1, c0, c1); MFMA8(c0, c1, c0, c1); MFMA8(c0, c1, c0, c1); MFMA8(c0, c1, c0, c1); }
  else for (int it = 0; it < iters; ++it) { MFMA8(c0, c1, c2, c3); MFMA8(c0, c1, c2, c3); MFMA8(c0, c1, c2, c3); MFMA8(c0, c1, c2, c3); }
  unsigned long long t1 = __builtin_readcyclecounter();
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");   // MFMA results are read below: past every hazard window
  if (lane == 0) cycles[blockIdx.x * 8 + wave] = t1 - t0;
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += c0[i] + c1[i] + c2[i] + c3[i];
  if (s == 123.456f) sink[threadIdx.x] = s;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 1024;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int blocks = prop.multiProcessorCount;
  CK(hipFuncSetAttribute((const void*)chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  unsigned long long* d_cyc; float* d_sink;
  CK(hipMalloc(&d_cyc, blocks * 8 * 8)); CK(hipMalloc(&d_sink, 512 * 4));
  printf("# probe_chain on %s, %d CUs; %d x 32 v_mfma_f32_32x32x2_f32 per wave (64 clocks each at the pipe's rate)\n", prop.gcnArchName, blocks, iters);
  printf("%-14s %-12s %14s %18s\n", "waves/SIMD", "accumulators", "clk/MFMA(wave)", "clk/MFMA(SIMD)");
  for (int waves = 4; waves <= 8; waves += 4)
    for (int accs = 1; accs <= 4; accs *= 2) {
      for (int rep = 0; rep < 2; ++rep) {   // the second launch is the measured one
        hipLaunchKernelGGL(chain_kernel, dim3(blocks), dim3(waves * 64), 96 * 1024, 0, accs, iters, d_cyc, d_sink);
        CK(hipDeviceSynchronize());
      }
      std::vector<unsigned long long> cyc(blocks * 8);
      CK(hipMemcpy(cyc.data(), d_cyc, cyc.size() * 8, hipMemcpyDeviceToHost));
      double sum = 0;
      for (int i = 0; i < blocks; ++i) for (int w = 0; w < waves; ++w) sum += (double)cyc[i * 8 + w];
      const double per_wave = sum / (blocks * waves) / (iters * 32.0);
      printf("%-14d %-12d %14.1f %18.1f\n", waves / 4, accs, per_wave, per_wave / (waves / 4));
    }
  return 0;
}
