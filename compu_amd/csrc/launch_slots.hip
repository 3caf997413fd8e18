// The shared half of the (device, stream) slot caches (launch_slots.h): the list of every codec's cache, the two release
// entry points of chip_internal.h, and the sizing rules the caches have in common.  Host code only.
#include "launch_slots.h"

#include <vector>

#include "chip_internal.h"

namespace chip {

namespace {
// Caches are globals of several translation units: a function-local list exists before the first of them registers,
// whatever order their initialisers run in.
std::vector<SlotCacheBase *> &caches()
{
    static std::vector<SlotCacheBase *> list;
    return list;
}
}  // namespace

SlotCacheBase::SlotCacheBase() { caches().push_back(this); }

hipError_t release_scratch()
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
    for (SlotCacheBase *c : caches()) c->release(dev, nullptr);
    return hipSuccess;
}

void release_scratch_of(hipStream_t stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    for (SlotCacheBase *c : caches()) c->release(dev, &stream);
}

hipError_t ResidentWaves::get(const void *kernel, int &waves, int per_cu_cap, int *asked_per_cu)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    int &m = memo[dev < 64 ? dev : 63];
    if (asked_per_cu) *asked_per_cu = 0;
    if (!m) {
        int per_cu = 0, cus = 0;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0)) != hipSuccess) return e;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        if (per_cu_cap > 0 && per_cu > per_cu_cap) per_cu = per_cu_cap;
        if (asked_per_cu) *asked_per_cu = per_cu;
        m = per_cu * cus;
    }
    waves = m;
    return hipSuccess;
}

hipError_t WaveScratch::reserve(hipStream_t stream, uint32_t n, int max_blocks, size_t per_wave)
{
    const int want = n < (uint32_t)max_blocks ? (int)n : max_blocks;
    if (blocks >= want) return hipSuccess;
    hipError_t e;
    if (scratch && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;  // launches on the stream still use it
    (void)hipFree(scratch);
    scratch = nullptr;
    blocks = 0;
    const int nb = grown_blocks(want, max_blocks);
    if ((e = hipMalloc((void **)&scratch, (size_t)nb * per_wave + 256)) != hipSuccess) return e;
    counter = (uint32_t *)(scratch + (size_t)nb * per_wave);
    blocks = nb;
    return hipSuccess;
}

}  // namespace chip
