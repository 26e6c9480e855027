// LDS atomic-add rates on gfx950 for a byte histogram, the layouts the counting kernel (csrc/hip/count_kernels.hip)
// chose between: one 256-bin copy a wave ("per_wave") against 32 interleaved copies a workgroup, lane l on copy l mod 32
// ("lane32"); each for bytes spread over all bins and for one repeated byte.  No global memory in the loop: the bytes
// come from a hash of the lane and the step, so the numbers are the LDS's alone.
// Build: make -C profiles/tools/micro build/probe_counts   Run: build/probe_counts
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
typedef uint32_t u32;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr u32 kThreads = 512, kSteps = 4096;

template <int LAYOUT, int ONE_BYTE>
__global__ __launch_bounds__(kThreads) void lds_hist(u32 *out, u32 seed) {
    __shared__ __attribute__((aligned(16))) u32 tab[256 * 32];
    const u32 t = threadIdx.x;
    for (u32 i = t; i < 256 * 32; i += kThreads) tab[i] = 0;
    __syncthreads();
    u32 *base = LAYOUT == 0 ? tab + (t / 64) * 256 : tab + (t & 31);
    const u32 scale = LAYOUT == 0 ? 1 : 32;
    u32 x = seed ^ (t * 0x9E3779B9u) ^ (blockIdx.x * 0x85EBCA6Bu);
    for (u32 s = 0; s < kSteps; ++s) {
        x = x * 1664525u + 1013904223u;
        const u32 w = ONE_BYTE ? 0x41414141u : x;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) atomicAdd(&base[((w >> (8 * k)) & 0xFFu) * scale], 1u);
    }
    __syncthreads();
    if (t < 256) {
        u32 sum = 0;
        for (u32 c = 0; c < 32; ++c) sum += tab[t * 32 + c];
        atomicAdd(&out[t], sum);
    }
}

template <int LAYOUT, int ONE_BYTE>
static int run(const char *name, u32 *d_out, int grid) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    hipLaunchKernelGGL((lds_hist<LAYOUT, ONE_BYTE>), dim3(grid), dim3(kThreads), 0, 0, d_out, 1u);
    CK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 10; ++r) {
        CK(hipEventRecord(a, 0));
        hipLaunchKernelGGL((lds_hist<LAYOUT, ONE_BYTE>), dim3(grid), dim3(kThreads), 0, 0, d_out, (u32)r);
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        best = ms < best ? ms : best;
    }
    const double adds = (double)grid * kThreads * kSteps * 4; /* lane adds = bytes counted */
    const double wave_instr_per_cu = (double)grid / 256.0 * (kThreads / 64) * kSteps * 4;
    printf("%-22s %8.3f ms  %7.1f Gbytes/s counted  %5.2f ns per ds_add wave-instruction a CU (%.1f cycles at 2.4 GHz)\n",
           name, best, adds / best / 1e6, best * 1e6 / wave_instr_per_cu, best * 1e6 / wave_instr_per_cu * 2.4);
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return 0;
}

int main() {
    u32 *d_out;
    CK(hipMalloc(&d_out, 256 * 4));
    const int grid = 256 * 4; /* four workgroups (32 waves) a CU */
    if (run<0, 0>("per_wave  spread bytes", d_out, grid) || run<0, 1>("per_wave  one byte", d_out, grid) ||
        run<1, 0>("lane32    spread bytes", d_out, grid) || run<1, 1>("lane32    one byte", d_out, grid)) {
        return 1;
    }
    CK(hipFree(d_out));
    return 0;
}
