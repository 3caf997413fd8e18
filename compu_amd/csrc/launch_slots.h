// The (device, stream) slot cache behind every persistent-grid launch ("Launch slots"): the scratch memory a
// launch needs is kept per stream between calls.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

namespace chip {

// What release_scratch() / release_scratch_of() (chip_internal.h) see of a codec's cache.
class SlotCacheBase {
  public:
    virtual void release(int dev, const hipStream_t *stream) = 0;  // every slot of `dev`, or only that of *stream

  protected:
    SlotCacheBase();  // joins the list those two walk (launch_slots.hip)
    ~SlotCacheBase() = default;
};

// One per codec, a global of its translation unit.  Slot: default-constructible, `void free()` releases its device memory;
// `size_t bytes() const` (device bytes held) where bytes_of() is used.  A launcher locks `mu` from at() to its last launch:
// a second host thread with a larger batch on the same stream may reallocate the slot, and the counter reset and the kernel
// have to reach the stream back to back.
template <class Slot>
class SlotCache final : public SlotCacheBase {
  public:
    std::mutex mu;

    // (caller holds mu) the slot of (current device, stream), empty when it is new
    hipError_t at(hipStream_t stream, Slot *&sl)
    {
        int dev = 0;
        const hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) sl = &slots_[{dev, stream}];
        return e;
    }

    size_t bytes_of(hipStream_t stream)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 0;
        std::lock_guard<std::mutex> lk(mu);
        const auto it = slots_.find({dev, stream});
        return it == slots_.end() ? 0 : it->second.bytes();
    }

    void release(int dev, const hipStream_t *stream) override
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto it = slots_.begin(); it != slots_.end();) {
            if (it->first.first == dev && (!stream || it->first.second == *stream)) {
                it->second.free();
                it = slots_.erase(it);
            } else {
                ++it;
            }
        }
    }

  private:
    std::map<std::pair<int, hipStream_t>, Slot> slots_;
};

// Waves of `kernel` (one 64-lane wave per block) that a full grid keeps resident on the current device: occupancy per CU
// (at most per_cu_cap when that is > 0) x CUs, asked once per device.  *asked_per_cu (optional) gets the per-CU figure in
// the call that asked, 0 afterwards.
struct ResidentWaves {
    int memo[64] = {0};
    hipError_t get(const void *kernel, int &waves, int per_cu_cap = 0, int *asked_per_cu = nullptr);
};

// Waves to allocate for a batch that wants `want` of at most `max`: a little headroom for batches that grow slowly,
// exactly one for the batches of one that streaming objects launch.
inline int grown_blocks(int want, int max) { return want <= 1 ? 1 : (want + want / 4 < max ? want + want / 4 : max); }

// The slot of four of the five codecs: `blocks` waves of scratch and, behind them in the same allocation (256 bytes of
// slack), the unit counter.
struct WaveScratch {
    uint8_t *scratch = nullptr;
    uint32_t *counter = nullptr;
    int blocks = 0;
    // room for min(n, max_blocks) waves of per_wave bytes each; a slot that is too small is replaced once the stream has drained
    hipError_t reserve(hipStream_t stream, uint32_t n, int max_blocks, size_t per_wave);
    void free() { (void)hipFree(scratch); }
};

}  // namespace chip
