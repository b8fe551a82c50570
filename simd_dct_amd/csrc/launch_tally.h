// launch_tally.h -- per-kernel-instantiation launch counter (diagnostics, mdct_kernel_counts in include/mdct.h).
// Every kernel launch of the library goes through MDCT_LAUNCH, which counts it and then launches as hipLaunchKernelGGL does.
// The key is the host-side kernel handle (&kernel, the exported symbol hipLaunchKernel resolves); names are resolved only at query
// time (dladdr + demangling, mdct_api.hip).  Launch path: an open-addressed table of fixed size, no lock, no allocation; one relaxed
// fetch_add per launch, plus one compare-and-swap the first time an instantiation is launched (it claims its slot).
#ifndef MDCT_LAUNCH_TALLY_H
#define MDCT_LAUNCH_TALLY_H

#include <atomic>
#include <stddef.h>
#include <stdint.h>

namespace mdct
{

constexpr int kTallyBits = 9; // 512 slots for the ~100 instantiations the library holds
constexpr size_t kTallySlots = size_t(1) << kTallyBits;

struct TallySlot
{
  std::atomic<const void *> key;
  std::atomic<uint64_t> count;
};

extern TallySlot g_tally[kTallySlots]; // zero-initialised (static storage), defined in mdct_api.hip

inline void tally_launch(const void *kernel)
{
  const size_t h = (size_t)(((uint64_t)(uintptr_t)kernel * 0x9E3779B97F4A7C15ull) >> (64 - kTallyBits));
  for (size_t i = 0; i < kTallySlots; i++)
  {
    TallySlot &s = g_tally[(h + i) & (kTallySlots - 1)];
    const void *cur = s.key.load(std::memory_order_relaxed);
    if (cur == nullptr && s.key.compare_exchange_strong(cur, kernel, std::memory_order_relaxed))
      cur = kernel;
    if (cur == kernel)
    {
      s.count.fetch_add(1, std::memory_order_relaxed);
      return;
    }
  }
}

} // namespace mdct

#define MDCT_LAUNCH(kernel, ...)                                          \
  do                                                                      \
  {                                                                       \
    ::mdct::tally_launch(reinterpret_cast<const void *>(&(kernel)));     \
    hipLaunchKernelGGL(kernel, __VA_ARGS__);                              \
  } while (0)

#endif
