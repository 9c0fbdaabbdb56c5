// TEST INFRASTRUCTURE: what csrc/render.hip needs from the host simulator beyond tests/hostsim/hip/hip_runtime.h: the 64-bit unsigned atomic minimum
// (global_atomic_umin_x2 on the GPU).  GPU threads are host threads here, so it is a real atomic.
#pragma once
#include <atomic>
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    std::atomic_ref<unsigned long long> a(*p);
    unsigned long long old = a.load(std::memory_order_relaxed);
    while (v < old && !a.compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
    return old;
}
