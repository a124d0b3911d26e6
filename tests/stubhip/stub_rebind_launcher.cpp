// tests/stubhip/stub_rebind_launcher.cpp — the stand-in for kernels_rebind.hip.cpp in the sanitizer builds (tests/test_batch_rebind_sanitizers.py).
// TEST INFRASTRUCTURE.  The "scatter kernel" is a closure on the stream that writes the addresses into the stub's "device" block when the stream
// gets to it: a short list is copied at launch like kernel arguments, a long one is read from the batch's pinned area LATE — an area the host
// overwrote or freed too early is a wrong address (the stub tick kernels touch every plane: a sanitizer report) or a report of its own.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../swiftvideo_amd/csrc/rebind.h"

namespace chv {
static hipError_t stub_rebind(uint8_t *block, const RebindItem *items_host, const RebindItem *items_dev, int n, hipStream_t stream) {
    if (stubhip_launch_should_fail()) return hipErrorLaunchFailure;
    if (n <= kRebindByValue) {
        std::vector<RebindItem> v(items_host, items_host + n);
        stubhip_enqueue(stream, [block, v] { for (const RebindItem &r : v) memcpy(block + r.off, &r.addr, 8); });
    } else {
        stubhip_enqueue(stream, [block, items_dev, n] { for (int i = 0; i < n; i++) memcpy(block + items_dev[i].off, &items_dev[i].addr, 8); });
    }
    return hipSuccess;
}
static const struct Registrar { Registrar() { register_rebind_launcher(stub_rebind); } } g_registrar;
}  // namespace chv
