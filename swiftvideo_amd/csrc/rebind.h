// rebind.h — what chv_batch_rebind (chipvideo.cpp) and the scatter kernel's unit (kernels_rebind.hip.cpp) share.
//
// A rebind changes nothing but DPlane::ptr fields of a batch's descriptor block.  The host turns every rebound plane into one
// {byte offset inside the block, new address} pair — offsets are produced and bounds-checked there, the kernel only stores.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace chv {

struct RebindItem {
    uint32_t off;      // bytes from the block's base; a multiple of 8, off + 8 <= the block's used size
    uint32_t pad;
    uint64_t addr;     // the plane's new device address
};
static_assert(sizeof(RebindItem) == 16, "one 16-byte load per lane");

// Lists up to this length travel as kernel ARGUMENTS (the pattern of WaveOne, device_types.h: one stream operation, no staging, no copy):
// 220 * 16 = 3520 bytes beside the block's address and the count, inside the 4 KB kernarg segment.  8 headline ticks are 72 items.
constexpr int kRebindByValue = 220;
struct RebindArgs {
    uint8_t *block;
    int32_t n, pad;
    RebindItem items[kRebindByValue];
};
static_assert(sizeof(RebindArgs) <= 3584, "kernel arguments: 4 KB in all");

// n <= kRebindByValue: `items_host` is copied into the launch's arguments (items_dev is not used); longer lists are read by the kernel from
// `items_dev`, memory the device can read that stays unchanged until the launch has run.  Reports like every launcher, through its return value.
typedef hipError_t (*RebindLauncher)(uint8_t *block, const RebindItem *items_host, const RebindItem *items_dev, int n, hipStream_t stream);
// chipvideo.cpp owns the pointer (null: no kernel unit in this build — every rebind re-sends the whole block); the kernel unit registers its
// launcher when the library is loaded.  The host units therefore link without it (tests/stubhip).
void register_rebind_launcher(RebindLauncher fn);

}  // namespace chv
