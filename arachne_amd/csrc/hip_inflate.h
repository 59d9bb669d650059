// hip_inflate.h -- dev_inflate.h on the GPU: the inflate of BGZF input in front of the device feeder (device_feeder.h) and behind
// arx_selftest_inflate.  Included by arx_bgzf.hip, so that the kernel compiles there and not next to the pipeline's; other units start it
// through inflate_launch(), which arx_bgzf.hip defines and device_feeder.h declares as well.
//
//   k_bgzf_inflate   one wavefront (a workgroup of INF_LANES lanes) per BGZF block: the block's bytes and the decode tables in LDS (about 78 KB,
//                    two wavefronts a CU), the finished block copied to out + row.ooff.  status[b] is the block's status (dev_inflate.h: INF_*);
//                    counts[0] is raised by one per block that is not INF_OK, counts[1] by the DEFLATE blocks read.  A row that points outside
//                    src[0, src_bytes) or out[0, out_bytes) is INF_BAD_HEADER and touches nothing
#pragma once
#include <hip/hip_runtime.h>
#include "hip_launch.h"
#include "dev_inflate.h"

namespace arx {

struct InfHipDrv { // dev_inflate.h's driver on a wavefront
	int lane;
	template <class F> __device__ __forceinline__ void lanes(F f)
	{
		f(lane);
		// what a phase wrote (LDS) is read by other lanes of the same wavefront in the next one: dev_chain_group.h's hand-off
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
};

constexpr int INF_WORK_ALIGNED = (INF_WORK_BYTES + 15) & ~15;
constexpr int INF_LDS_BYTES = INF_WORK_ALIGNED + INF_MAX_OUT + 16; // the block's bytes start at the destination's alignment modulo 4

static __global__ void __launch_bounds__(INF_LANES) k_bgzf_inflate(const uint8_t *src, int64_t src_bytes, const InfRow *rows, int n_blocks, uint8_t *out, int64_t out_bytes,
                                                                   int32_t *status, int32_t *counts)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lds_inflate[];
	const int b = blockIdx.x;
	if (b >= n_blocks) return;
	const InfRow r = rows[b];
	int st = INF_BAD_HEADER, nd = 0;
	if (inf_row_in_range(r, src_bytes, out_bytes)) {
		uint8_t *dst = out + r.ooff;
		InfWork w;
		inf_carve(w, lds_inflate, lds_inflate + INF_WORK_ALIGNED + ((uintptr_t)dst & 3)); // whole words on the way out (inf_copy_out)
		InfHipDrv drv{(int)threadIdx.x};
		st = inf_block(drv, w, src + r.coff, r.clen, r.isize, r.crc, dst, &nd);
	}
	if (threadIdx.x == 0) {
		status[b] = st;
		if (st != INF_OK) atomicAdd(&counts[0], 1);
		if (nd) atomicAdd(&counts[1], nd);
	}
}

// enqueues the inflate of n_blocks rows on `stream`; everything is device memory.  counts is not cleared here.  Defined in arx_bgzf.hip
void inflate_launch(hipStream_t stream, const uint8_t *d_src, int64_t src_bytes, const InfRow *d_rows, int n_blocks, uint8_t *d_out, int64_t out_bytes, int32_t *d_status,
                    int32_t *d_counts);

} // namespace arx
