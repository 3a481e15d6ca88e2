// What the refine pass of an adaptive frame (lol_kernel_aa.h, render_aa_list) would pay for a worst-case grid instead of its
// grid-stride loop: one one-wave block per group of the whole frame, the blocks past the list's length (read from device memory)
// returning at once.  Times such launches with HIP events for a list of `n` entries, against the 8192-block grid of the loop.
//
//   hipcc -O3 --offload-arch=gfx950 -o tools/empty_grid_probe tools/empty_grid_probe.hip && tools/empty_grid_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// one group per block: the block writes one word per lane of its group (stands in for the work), or returns past the list
__global__ __launch_bounds__(64) void per_block(const unsigned* count, unsigned per_wave, unsigned* out) {
	const unsigned n = __builtin_amdgcn_readfirstlane(*count);
	if (blockIdx.x * per_wave >= n) return;
	out[blockIdx.x * 64u + threadIdx.x] = blockIdx.x;
}

// the grid-stride loop of render_aa_list, the same stand-in work
__global__ __launch_bounds__(64) void grid_stride(const unsigned* count, unsigned per_wave, unsigned* out) {
	const unsigned n = __builtin_amdgcn_readfirstlane(*count);
	for (unsigned g = blockIdx.x; g * per_wave < n; g += gridDim.x) out[g * 64u + threadIdx.x] = g;
}

int main() {
	const unsigned w = 3840, h = 2160, per_wave = 4;                 // 4K, s = 4: 4 pixels per wave
	const unsigned worst = (w * h + per_wave - 1) / per_wave;         // 2,073,600 blocks
	const unsigned lengths[] = { 0, 30700, 300000, w * h };          // no edge, scene4 at T = 16 (0.37 %), 3.6 %, every pixel
	unsigned *count, *out;
	CHECK(hipMalloc(&count, 4));
	CHECK(hipMalloc(&out, (size_t)worst * 64 * 4));
	hipEvent_t a, b;
	CHECK(hipEventCreate(&a));
	CHECK(hipEventCreate(&b));
	for (unsigned n : lengths) {
		CHECK(hipMemcpy(count, &n, 4, hipMemcpyHostToDevice));
		float best[2] = { 1e9f, 1e9f };
		for (int rep = 0; rep < 7; rep++) {
			for (int k = 0; k < 2; k++) {
				CHECK(hipEventRecord(a, 0));
				if (k == 0) hipLaunchKernelGGL(per_block, dim3(worst), dim3(64), 0, 0, count, per_wave, out);
				else        hipLaunchKernelGGL(grid_stride, dim3(8192), dim3(64), 0, 0, count, per_wave, out);
				CHECK(hipGetLastError());
				CHECK(hipEventRecord(b, 0));
				CHECK(hipEventSynchronize(b));
				float ms = 0;
				CHECK(hipEventElapsedTime(&ms, a, b));
				if (rep > 0 && ms < best[k]) best[k] = ms;
			}
		}
		printf("{\"list\": %u, \"worst_case_grid_blocks\": %u, \"worst_case_grid_ms\": %.4f, \"grid_stride_8192_ms\": %.4f}\n",
		       n, worst, best[0], best[1]);
	}
	CHECK(hipFree(count));
	CHECK(hipFree(out));
	return 0;
}
