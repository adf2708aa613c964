#include "Taxi.h"

#include <random>

namespace {
struct S { int r, c, p, d; };

int clampi(float v, int hi) { return v >= 0.0f ? (v >= static_cast<float>(hi) ? hi : static_cast<int>(v)) : 0; }   // a NaN becomes 0
S load(const float* st) { return S{ clampi(st[0], 4), clampi(st[1], 4), clampi(st[2], 4), clampi(st[3], 3) }; }
bool eastBlocked(int r, int c) { return c == 4 || (r <= 1 && c == 1) || (r >= 3 && (c == 0 || c == 2)); }
bool westBlocked(int r, int c) { return c == 0 || eastBlocked(r, c - 1); }
// R = (0,0), G = (0,4), Y = (4,0), B = (4,3) as (row, col); -1: not on a stand
int standAt(int r, int c) { return r == 0 ? (c == 0 ? 0 : (c == 4 ? 1 : -1)) : (r == 4 ? (c == 0 ? 2 : (c == 3 ? 3 : -1)) : -1); }
}  // namespace

float Taxi::transition(float* st, int action, bool& terminated) {
    S s = load(st);
    const int a = action < 0 ? 0 : (action > 5 ? 5 : action);
    const int on = standAt(s.r, s.c);
    float reward = -1.0f;
    terminated = false;
    if (a == 0) s.r = s.r < 4 ? s.r + 1 : 4;
    else if (a == 1) s.r = s.r > 0 ? s.r - 1 : 0;
    else if (a == 2) { if (!eastBlocked(s.r, s.c)) s.c += 1; }
    else if (a == 3) { if (!westBlocked(s.r, s.c)) s.c -= 1; }
    else if (a == 4) {
        if (s.p < 4 && on == s.p) s.p = 4;
        else reward = -10.0f;
    } else {
        if (s.p == 4 && on == s.d) { s.p = s.d; terminated = true; reward = 20.0f; }
        else if (s.p == 4 && on >= 0) s.p = on;
        else reward = -10.0f;
    }
    st[0] = static_cast<float>(s.r); st[1] = static_cast<float>(s.c); st[2] = static_cast<float>(s.p); st[3] = static_cast<float>(s.d);
    return reward;
}

void Taxi::observe(const float* st, float* obs) {
    const S s = load(st);
    for (int k = 0; k < 19; k++) obs[k] = 0.0f;
    obs[s.r] = 1.0f;
    obs[5 + s.c] = 1.0f;
    obs[10 + s.p] = 1.0f;
    obs[15 + s.d] = 1.0f;
}

std::array<uint8_t, 6> Taxi::mask(const float* st) {
    const S s = load(st);
    const int on = standAt(s.r, s.c);
    return { static_cast<uint8_t>(s.r < 4), static_cast<uint8_t>(s.r > 0), static_cast<uint8_t>(!eastBlocked(s.r, s.c)), static_cast<uint8_t>(!westBlocked(s.r, s.c)),
             static_cast<uint8_t>(s.p < 4 && on == s.p), static_cast<uint8_t>(s.p == 4 && on >= 0) };
}

void Taxi::stateOf(const float* obs, float* st) {
    static const int lo[4] = { 0, 5, 10, 15 }, n[4] = { 5, 5, 5, 4 };
    for (int g = 0; g < 4; g++) {
        int best = 0;
        for (int k = 1; k < n[g]; k++) if (obs[lo[g] + k] > obs[lo[g] + best]) best = k;
        st[g] = static_cast<float>(best);
    }
}

Taxi::Taxi(int64_t seed, int64_t env_index) : state(4, 0.0f), episode_length(0), episode_reward(0.0f), m_seed(seed), m_env_index(env_index) {
    state[3] = 1.0f;   // (0, 0, 0, 1): a start state
}

std::vector<float> Taxi::observation() const {
    std::vector<float> obs(19);
    observe(state.data(), obs.data());
    return obs;
}

std::array<uint8_t, 6> Taxi::actionMask() const { return mask(state.data()); }

std::tuple<std::vector<float>, float, bool, bool> Taxi::step(int64_t action) {
    bool terminated = false;
    const int a = action < 0 ? 0 : (action > 5 ? 5 : static_cast<int>(action));
    const float reward = transition(state.data(), a, terminated);
    episode_length += 1;
    episode_reward += reward;
    return { observation(), reward, terminated, false };
}

// As MountainCar::randomUniform: a deterministic function of (seed, env index, reset count); the device's map from three 32-bit words to the 300 start states
std::vector<float> Taxi::reset() {
    std::seed_seq seq{ static_cast<uint32_t>(m_seed), static_cast<uint32_t>(m_env_index), static_cast<uint32_t>(m_resets++) };
    std::mt19937 gen(seq);
    const uint64_t x = gen(), y = gen(), z = gen();
    const int cell = static_cast<int>((x * 25u) >> 32), pass = static_cast<int>((y * 4u) >> 32), d = static_cast<int>((z * 3u) >> 32);
    state = { static_cast<float>(cell / 5), static_cast<float>(cell % 5), static_cast<float>(pass), static_cast<float>(d + (d >= pass ? 1 : 0)) };
    episode_length = 0;
    episode_reward = 0.0f;
    return observation();
}
