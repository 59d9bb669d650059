// arx_api.hip -- libarachne_amd.so: the C-ABI of include/arachne_amd.h on the HIP runtime (gfx950).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC arx_api.hip -o libarachne_amd.so
#ifdef ARX_RFA_STATS // diagnostics build (-DARX_RFA_STATS): clock ticks (100 MHz) per phase of rfa_barcode, summed over barcodes, printed per launch
#include <hip/hip_runtime.h>
__device__ unsigned long long g_rfa_t[8];
__shared__ unsigned long long rfa_t_prev;
#define ARX_RFA_T(k) do { if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); if ((k) > 0) atomicAdd(&g_rfa_t[k], t_ - rfa_t_prev); rfa_t_prev = t_; } } while (0)
#endif
#include "hip_rt.h"
#include "api_impl.h"

namespace arx { // register budgets of single thread-per-item kernels (hip_rt.h ItemsWpe), where a measurement backs them
#ifdef ARX_WPE_CHAIN
template <> struct ItemsWpe<KChain> { static constexpr int v = ARX_WPE_CHAIN; };
#endif
#ifdef ARX_WPE_EXTSTEP
template <> struct ItemsWpe<KExtStep> { static constexpr int v = ARX_WPE_EXTSTEP; };
#endif
#ifdef ARX_WPE_MAPQ
template <> struct ItemsWpe<KMapq> { static constexpr int v = ARX_WPE_MAPQ; };
#endif
#ifdef ARX_WPE_REG2ALN
template <> struct ItemsWpe<KReg2Aln> { static constexpr int v = ARX_WPE_REG2ALN; };
#endif
}

// When the library is loaded, in front of the registration of this library's device code and of every HIP call it makes: the hardware queues
// the batch handles' main and side streams need, and whether they will have them (switches.h sw_request_hw_queues)
__attribute__((constructor(101))) static void arx_request_hw_queues() { arx::sw_request_hw_queues(); }
extern "C" int32_t arx_side_streams_default(void) { return arx::sw_side_streams_have_queues() ? 1 : 0; }

ARX_DEFINE_C_API(arx::HipRT)

namespace arx { const IndexView *ctx_index_view(::arx_ctx *ctx) { return ctx ? &((Context<HipRT> *)ctx)->ix : nullptr; } }
