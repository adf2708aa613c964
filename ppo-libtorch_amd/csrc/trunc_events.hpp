// ppo-libtorch_amd/csrc/trunc_events.hpp -- the host side of the device event lists (ppo_host_truncations after a device-fed rollout, ppo_env_truncations):
// sorting what the fold kernels appended and handing it to the caller.  Plain C++, no HIP call, so it can be compiled and checked on its own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// The counter as copied back -> the entries the list holds: the fold kernels count every event and store only those below the capacity
inline int64_t clamp_event_count(int32_t raw, int64_t cap) { return std::min<int64_t>(std::max<int32_t>(raw, 0), cap); }

// (index, value) pairs in the order the workgroups got to the list -> ascending by index (indices are distinct: one event per sample)
inline void sort_events(const std::vector<int32_t>& ix, const std::vector<float>& va, std::vector<int32_t>& ix_out, std::vector<float>& va_out) {
    const size_t n = ix.size();
    std::vector<int32_t> order(n);
    for (size_t k = 0; k < n; k++) order[k] = (int32_t)k;
    std::sort(order.begin(), order.end(), [&ix](int32_t a, int32_t b) { return ix[(size_t)a] < ix[(size_t)b]; });
    ix_out.resize(n);
    va_out.resize(n);
    for (size_t k = 0; k < n; k++) { ix_out[k] = ix[(size_t)order[k]]; va_out[k] = va[(size_t)order[k]]; }
}

// The array rules of ppo_host_truncations: index_h / value_h may be null (count only); a non-null array needs cap >= the number of events.
// Returns false, writing nothing, when the room is short.
inline bool copy_events_out(const std::vector<int32_t>& ix, const std::vector<float>& va, int64_t* count, int32_t* index_h, float* value_h, int64_t cap) {
    const int64_t K = (int64_t)ix.size();
    if ((index_h || value_h) && cap < K) return false;
    if (K > 0 && index_h) std::memcpy(index_h, ix.data(), (size_t)K * 4);
    if (K > 0 && value_h) std::memcpy(value_h, va.data(), (size_t)K * 4);
    *count = K;
    return true;
}
