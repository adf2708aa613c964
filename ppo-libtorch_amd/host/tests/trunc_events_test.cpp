// ppo-libtorch_amd/host/tests/trunc_events_test.cpp -- the host half of the device event lists (csrc/trunc_events.hpp) as a program of its own: no HIP,
// no library.  tests/test_trunc_events_cpu.py builds it under the address and undefined-behaviour sanitizers and runs it.
#include "trunc_events.hpp"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static float value_of(int32_t index) { return 0.25f * (float)index - 3.0f; }

// sort_events on ix, with the value that belongs to each index: ascending indices, every value still beside its index
static bool sorts(const std::vector<int32_t>& ix) {
    std::vector<float> va;
    for (int32_t i : ix) va.push_back(value_of(i));
    std::vector<int32_t> ix_out(3, -1);   // stale contents of an earlier rollout
    std::vector<float> va_out(5, -1.0f);
    sort_events(ix, va, ix_out, va_out);
    if (ix_out.size() != ix.size() || va_out.size() != ix.size()) return false;
    std::vector<int32_t> want(ix);
    std::sort(want.begin(), want.end());
    for (size_t k = 0; k < ix.size(); k++)
        if (ix_out[k] != want[k] || va_out[k] != value_of(want[k])) return false;
    return true;
}

int main() {
    CHECK(sorts({}));
    CHECK(sorts({ 41 }));
    CHECK(sorts({ 0, 3, 4, 70, 1679 }));
    CHECK(sorts({ 1679, 70, 4, 3, 0 }));
    std::vector<int32_t> shuffled(1000);
    for (int32_t k = 0; k < 1000; k++) shuffled[(size_t)k] = 7 * k + 2;   // distinct
    uint32_t lcg = 12345u;
    for (size_t k = shuffled.size() - 1; k > 0; k--) {
        lcg = lcg * 1664525u + 1013904223u;
        std::swap(shuffled[k], shuffled[(lcg >> 8) % (k + 1)]);
    }
    CHECK(!std::is_sorted(shuffled.begin(), shuffled.end()));
    CHECK(sorts(shuffled));

    const std::vector<int32_t> ix = { 2, 5, 9 };
    const std::vector<float> va = { 0.5f, -1.5f, 2.25f };
    int64_t count = -7;
    CHECK(copy_events_out(ix, va, &count, nullptr, nullptr, 0) && count == 3);   // no arrays: the count only, whatever cap says
    count = -7;
    CHECK(copy_events_out(ix, va, &count, nullptr, nullptr, -1) && count == 3);
    int32_t ix_h[4] = { -7, -7, -7, -7 };
    float va_h[4] = { -7.0f, -7.0f, -7.0f, -7.0f };
    count = -7;
    CHECK(!copy_events_out(ix, va, &count, ix_h, va_h, 2));                       // short room: nothing is written
    CHECK(!copy_events_out(ix, va, &count, ix_h, nullptr, 2) && !copy_events_out(ix, va, &count, nullptr, va_h, 2));
    CHECK(count == -7);
    for (int k = 0; k < 4; k++) CHECK(ix_h[k] == -7 && va_h[k] == -7.0f);
    CHECK(copy_events_out(ix, va, &count, ix_h, va_h, 3) && count == 3);          // exact room
    for (int k = 0; k < 3; k++) CHECK(ix_h[k] == ix[(size_t)k] && va_h[k] == va[(size_t)k]);
    CHECK(ix_h[3] == -7 && va_h[3] == -7.0f);
    count = -7;
    CHECK(copy_events_out({}, {}, &count, ix_h, va_h, 0) && count == 0 && ix_h[0] == 2);   // an empty list fits anywhere

    CHECK(clamp_event_count(-1, 168) == 0 && clamp_event_count(INT32_MIN, 168) == 0);
    CHECK(clamp_event_count(0, 168) == 0 && clamp_event_count(5, 168) == 5 && clamp_event_count(168, 168) == 168);
    CHECK(clamp_event_count(169, 168) == 168 && clamp_event_count(INT32_MAX, 168) == 168);
    CHECK(clamp_event_count(3, 0) == 0);
    std::printf("trunc_events_test ok\n");
    return 0;
}
