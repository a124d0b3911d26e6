// kernels_rebind.hip.cpp — batch_rebind_scatter: point a batch's descriptors at new pictures (chv_batch_rebind, chipvideo.cpp).
//
// One lane per {offset, address} pair, one 64-bit vector store each; the host made and checked the offsets (rebind.h).  No LDS, no scratch:
// the by-value twin reads its list from the kernarg segment through an address, never by indexing a private copy of the argument.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "rebind.h"

namespace chv {

#define CHV_GLOBAL __attribute__((address_space(1)))
#define CHV_CONSTANT __attribute__((address_space(4)))

static __device__ __forceinline__ void rebind_store(uint8_t *block, uint32_t off, uint64_t addr) {
    *(CHV_GLOBAL uint64_t *)(uintptr_t)(block + off) = addr;
}

// the list in memory the device can read (the batch's pinned staging)
__global__ __launch_bounds__(256) void batch_rebind_scatter(uint8_t *block, const RebindItem *__restrict__ items, int n) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const CHV_GLOBAL RebindItem *it = (const CHV_GLOBAL RebindItem *)(uintptr_t)(items + i);
    const uint32_t off = it->off;
    const uint64_t addr = it->addr;
    rebind_store(block, off, addr);
}

// the list as the launch's argument (RebindArgs is the first and only one: offset 0 of the kernarg segment)
__global__ __launch_bounds__(256) void batch_rebind_scatter_args(const RebindArgs a) {
    const int i = (int)threadIdx.x;
    const uint64_t ka = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    const CHV_CONSTANT RebindArgs *arg = (const CHV_CONSTANT RebindArgs *)(uintptr_t)ka;
    if (i >= arg->n) return;
    const CHV_CONSTANT RebindItem *it = (const CHV_CONSTANT RebindItem *)(uintptr_t)(ka + offsetof(RebindArgs, items) + (uint64_t)i * sizeof(RebindItem));
    const uint32_t off = it->off;
    const uint64_t addr = it->addr;
    rebind_store(arg->block, off, addr);
}

static hipError_t launch_batch_rebind(uint8_t *block, const RebindItem *items_host, const RebindItem *items_dev, int n, hipStream_t stream) {
    if (!block || n <= 0 || !items_host) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (n <= kRebindByValue) {
        RebindArgs a;
        a.block = block; a.n = n; a.pad = 0;
        memcpy(a.items, items_host, (size_t)n * sizeof(RebindItem));
        hipLaunchKernelGGL(batch_rebind_scatter_args, dim3(1), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    if (!items_dev) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_rebind_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, block, items_dev, n);
    return hipGetLastError();
}

// (the pointer in chipvideo.cpp is constant-initialised to null, so the order of the units' initialisers does not matter)
static const struct RebindRegistrar { RebindRegistrar() { register_rebind_launcher(launch_batch_rebind); } } g_rebind_registrar;

}  // namespace chv
