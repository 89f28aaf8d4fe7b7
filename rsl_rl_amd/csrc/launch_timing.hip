// The library's one launch-timing state and its C ABI (launch_timing.h; rslrl_launch_timing_* in include/rslrl_amd.h):
// host code around HIP events, used by every unit that launches through launch_timed.
#include "launch_timing.h"

#include "common.h"

namespace rslrl {
LaunchTiming& launch_timing() {
    static LaunchTiming t;
    return t;
}
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_launch_timing_enable(int32_t capacity) {
    if (capacity < 0) return RSLRL_E_INVALID_ARGUMENT;
    LaunchTiming& t = launch_timing();
    std::lock_guard<std::mutex> lk(t.mu);
    if (capacity == 0) {  // disarm; the recorded launches stay readable
        t.on.store(false);
        return RSLRL_OK;
    }
    t.on.store(false);
    while (t.pool.size() < static_cast<size_t>(capacity)) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t err = hipEventCreate(&e0);
        if (err == hipSuccess) err = hipEventCreate(&e1);
        if (err != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            return static_cast<int>(err);
        }
        t.pool.push_back({e0, e1, 0});
    }
    t.used = 0;
    t.cap = static_cast<size_t>(capacity);
    t.on.store(true);
    return RSLRL_OK;
}

extern "C" int rslrl_launch_timing_read_tag(int32_t tag, double* total_ms, int64_t* launches) {
    if (!total_ms || !launches || tag < 0 || tag >= kNumLaunchTags) return RSLRL_E_INVALID_ARGUMENT;
    LaunchTiming& t = launch_timing();
    // the used event pairs are copied under the lock and synchronised after it is released: a timed launch on
    // another thread (launch_timed takes the same lock) never waits for this read's event synchronisations
    std::vector<LaunchTiming::Slot> slots;
    {
        std::lock_guard<std::mutex> lk(t.mu);
        slots.assign(t.pool.begin(), t.pool.begin() + static_cast<std::ptrdiff_t>(t.used));
    }
    double sum = 0.0;
    int64_t n = 0;
    for (const auto& sl : slots) {
        if (sl.tag != tag) continue;
        hipError_t err = hipEventSynchronize(sl.stop);
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, sl.start, sl.stop);
        if (err != hipSuccess) return static_cast<int>(err);
        sum += static_cast<double>(ms);
        ++n;
    }
    *total_ms = sum;
    *launches = n;
    return RSLRL_OK;
}

extern "C" int rslrl_launch_timing_read(double* total_ms, int64_t* launches) {
    return rslrl_launch_timing_read_tag(kTagPpoLoss, total_ms, launches);
}
